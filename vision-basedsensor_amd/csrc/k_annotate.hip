// MarkerTracker._draw_tracking (marker_detection.py:398-427) for the annotated video: every tracked slot of every frame gets
// a filled red disc at its centre, a red arrow from its frame-0 position, its yellow major and blue minor axis.  The
// rasterisation is restated from OpenCV 4.x imgproc/src/drawing.cpp for 3-channel 8-bit images, LINE_8, shift 0:
//   circle(thickness -1)   -> Circle(fill = 1): the midpoint circle, horizontal spans
//   line(thickness 2)      -> ThickLine: FillConvexPoly of the 4-point band in XY_SHIFT = 16 fixed point (its outline drawn
//                             by Line2 after clipLine, its interior by the two-edge scanline walk) + radius-1 filled Circle caps
//   arrowedLine            -> line(pt1, pt2) and the two tip lines of length |pt1 - pt2| * tipLength
// All of these only SET pixels to a colour, so the frame the reference paints sequentially equals, pixel by pixel, the colour
// of the last primitive that covers it.  k_draw_slots: one thread per (frame, slot) rasterises the slot's primitives and
// leaves (primitive key + 1) in a per-pixel "last writer" map with atomicMax - keys increase in painting order (slot, then
// red / yellow / blue), so the result does not depend on the order the threads run in; k_draw_resolve copies the frame and
// paints the covered pixels.  tests/helpers/cv_draw.py is the sequential Python statement of the same functions.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vbs.h"

namespace {

constexpr int XY_SHIFT = 16;
constexpr int64_t XY_ONE = 1LL << XY_SHIFT;

__host__ __device__ inline int64_t lmax(int64_t a, int64_t b) { return a > b ? a : b; }
__host__ __device__ inline int64_t lmin(int64_t a, int64_t b) { return a < b ? a : b; }

// the device canvas: a frame's last-writer map
struct MapCanvas {
    int32_t* lastw;                                     // this frame's map [H][W]
    int W, H;
    int32_t key;                                        // key + 1 of the primitive being drawn
    __device__ void put(int x, int y) const {
        if (x >= 0 && x < W && y >= 0 && y < H) atomicMax(lastw + (int64_t)y * W + x, key);
    }
    __device__ void hline(int y, int x1, int x2) const {   // ICV_HLINE, clipped
        if (y < 0 || y >= H) return;
        x1 = x1 > 0 ? x1 : 0;
        x2 = x2 < W - 1 ? x2 : W - 1;
        for (int x = x1; x <= x2; ++x) atomicMax(lastw + (int64_t)y * W + x, key);
    }
};

__host__ __device__ inline int cv_round(double v) { return (int)rint(v); }   // cvRound: half to even

// Circle(img, center, radius, color, fill = 1)
template <class Canvas>
__host__ __device__ void circle_filled(const Canvas& c, int cx, int cy, int radius) {
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        c.hline(cy - dy, cx - dx, cx + dx);
        c.hline(cy + dy, cx - dx, cx + dx);
        c.hline(cy - dx, cx - dy, cx + dy);
        c.hline(cy + dx, cx - dy, cx + dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// clipLine(Size2l, Point2l&, Point2l&)
__host__ __device__ inline bool clip_line(int64_t w, int64_t h, int64_t& x1, int64_t& y1, int64_t& x2, int64_t& y2) {
    const int64_t right = w - 1, bottom = h - 1;
    if (w <= 0 || h <= 0) return false;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        int64_t a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// Line2: the fixed-point (XY_SHIFT) line FillConvexPoly draws its outline with
template <class Canvas>
__host__ __device__ void line2(const Canvas& c, int64_t x1, int64_t y1, int64_t x2, int64_t y2) {
    if (!clip_line((int64_t)c.W << XY_SHIFT, (int64_t)c.H << XY_SHIFT, x1, y1, x2, y2)) return;
    int64_t dx = x2 - x1, dy = y2 - y1;
    const int64_t j = dx < 0 ? -1 : 0, ax = (dx ^ j) - j;
    const int64_t i = dy < 0 ? -1 : 0, ay = (dy ^ i) - i;
    int64_t x_step, y_step;
    int ecount;
    if (ax > ay) {
        dy = (dy ^ j) - j;
        if (j) { int64_t t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        x_step = XY_ONE;
        y_step = (dy * XY_ONE) / (ax | 1);
        ecount = (int)((x2 - x1) >> XY_SHIFT);
    } else {
        dx = (dx ^ i) - i;
        if (i) { int64_t t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        x_step = (dx * XY_ONE) / (ay | 1);
        y_step = XY_ONE;
        ecount = (int)((y2 - y1) >> XY_SHIFT);
    }
    x1 += XY_ONE >> 1;
    y1 += XY_ONE >> 1;
    c.put((int)((x2 + (XY_ONE >> 1)) >> XY_SHIFT), (int)((y2 + (XY_ONE >> 1)) >> XY_SHIFT));
    if (ax > ay) {
        x1 >>= XY_SHIFT;
        for (; ecount >= 0; --ecount) { c.put((int)x1, (int)(y1 >> XY_SHIFT)); x1++; y1 += y_step; }
    } else {
        y1 >>= XY_SHIFT;
        for (; ecount >= 0; --ecount) { c.put((int)(x1 >> XY_SHIFT), (int)y1); x1 += x_step; y1++; }
    }
}

// FillConvexPoly(img, v, 4, color, LINE_8, shift = XY_SHIFT)
template <class Canvas>
__host__ __device__ void fill_convex4(const Canvas& c, const int64_t* vx, const int64_t* vy) {
    constexpr int npts = 4;
    constexpr int64_t delta = XY_ONE >> 1;
    int64_t xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    int64_t px = vx[npts - 1], py = vy[npts - 1];
    for (int k = 0; k < npts; ++k) {
        if (vy[k] < ymin) { ymin = vy[k]; imin = k; }
        ymax = lmax(ymax, vy[k]);
        xmax = lmax(xmax, vx[k]);
        xmin = lmin(xmin, vx[k]);
        line2(c, px, py, vx[k], vy[k]);
        px = vx[k];
        py = vy[k];
    }
    xmin = (xmin + delta) >> XY_SHIFT;
    xmax = (xmax + delta) >> XY_SHIFT;
    ymin = (ymin + delta) >> XY_SHIFT;
    ymax = (ymax + delta) >> XY_SHIFT;
    if ((int)xmax < 0 || (int)ymax < 0 || (int)xmin >= c.W || (int)ymin >= c.H) return;
    ymax = lmin(ymax, (int64_t)c.H - 1);
    int eidx[2] = {imin, imin}, edi[2] = {1, npts - 1}, eye[2];
    int64_t ex[2] = {-XY_ONE, -XY_ONE}, edx[2] = {0, 0};
    int y = (int)ymin;
    eye[0] = eye[1] = y;
    int edges = npts;
    do {
        for (int e = 0; e < 2; ++e) {
            if (y >= eye[e]) {
                int idx0 = eidx[e], di = edi[e];
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    const int ty = (int)((vy[idx] + delta) >> XY_SHIFT);
                    if (ty > y) {
                        const int64_t xs = vx[idx0], xe = vx[idx];
                        eye[e] = ty;
                        edx[e] = ((xe - xs) * 2 + (ty - y)) / (2 * (int64_t)(ty - y));
                        ex[e] = xs;
                        eidx[e] = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            const int l = ex[0] > ex[1] ? 1 : 0, r = 1 - l;
            const int xx1 = (int)((ex[l] + delta) >> XY_SHIFT), xx2 = (int)((ex[r] + delta) >> XY_SHIFT);
            if (xx2 >= 0 && xx1 < c.W) c.hline(y, xx1, xx2);
        }
        ex[0] += edx[0];
        ex[1] += edx[1];
    } while (++y <= (int)ymax);
}

// line(img, p0, p1, color, 2) = ThickLine(thickness 2, LINE_8, flags 3, shift 0)
template <class Canvas>
__host__ __device__ void thick_line2(const Canvas& c, int x0, int y0, int x1, int y1) {
    const int64_t p0x = (int64_t)x0 << XY_SHIFT, p0y = (int64_t)y0 << XY_SHIFT;
    const int64_t p1x = (int64_t)x1 << XY_SHIFT, p1y = (int64_t)y1 << XY_SHIFT;
    const double inv = 1.0 / (double)XY_ONE;
    const double dx = (double)(p0x - p1x) * inv, dy = (double)(p1y - p0y) * inv;
    double r = dx * dx + dy * dy;
    const int thickness = 2 << (XY_SHIFT - 1);
    if (fabs(r) > 2.220446049250313e-16) {               // DBL_EPSILON
        r = (double)thickness / sqrt(r);
        const int64_t dpx = cv_round(dy * r), dpy = cv_round(dx * r);
        const int64_t vx[4] = {p0x + dpx, p0x - dpx, p1x - dpx, p1x + dpx};
        const int64_t vy[4] = {p0y + dpy, p0y - dpy, p1y - dpy, p1y + dpy};
        fill_convex4(c, vx, vy);
    }
    const int rad = (int)((thickness + (XY_ONE >> 1)) >> XY_SHIFT);
    circle_filled(c, x0, y0, rad);                       // ((p0 + XY_ONE/2) >> XY_SHIFT) = the integer point itself
    circle_filled(c, x1, y1, rad);
}

// _draw_tracking(frame, ref, curr) of one slot: c.key on entry = 3 slot + 1 (the red disc and arrow); + 1 yellow, + 2 blue
template <class Canvas>
__host__ __device__ void draw_slot(Canvas& c, const double* d, double oxf, double oyf) {
    const double cx = d[0], cy = d[1], maj = d[2] / 2, mnr = d[3] / 2;
    const double a = d[4] * (3.141592653589793 / 180.0);                     // np.deg2rad
    const int icx = (int)cx, icy = (int)cy;                                  // int(): toward zero
    const int ox = (int)oxf, oy = (int)oyf;
    circle_filled(c, icx, icy, 4);
    // arrowedLine((ox, oy), (icx, icy), tipLength = 0.25)
    thick_line2(c, ox, oy, icx, icy);
    const double tip = sqrt((double)(ox - icx) * (ox - icx) + (double)(oy - icy) * (oy - icy)) * 0.25;
    const double ang = atan2((double)oy - icy, (double)ox - icx);
    const double pi4 = 3.141592653589793 / 4;
    thick_line2(c, cv_round(icx + tip * cos(ang + pi4)), cv_round(icy + tip * sin(ang + pi4)), icx, icy);
    thick_line2(c, cv_round(icx + tip * cos(ang - pi4)), cv_round(icy + tip * sin(ang - pi4)), icx, icy);
    c.key += 1;                                                              // major axis, yellow
    double cs = cos(a), sn = sin(a);
    thick_line2(c, (int)(cx - maj * cs), (int)(cy - maj * sn), (int)(cx + maj * cs), (int)(cy + maj * sn));
    c.key += 1;                                                              // minor axis, blue
    const double b = a + 3.141592653589793 / 2;
    cs = cos(b);
    sn = sin(b);
    thick_line2(c, (int)(cx - mnr * cs), (int)(cy - mnr * sn), (int)(cx + mnr * cs), (int)(cy + mnr * sn));
}

__global__ void __launch_bounds__(64) k_draw_slots(int n, int H, int W, const double* __restrict__ det, int max_markers,
                                                   const float* __restrict__ table, const double* __restrict__ ref_xy, int m_ref,
                                                   int32_t* __restrict__ lastw) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (slot >= m_ref || f >= n) return;
    const float* row = table + ((int64_t)f * m_ref + slot) * VBS_TABLE_COLS;
    if (!((int)row[0] & VBS_FLAG_TRACKED)) return;
    const int di = (int)row[9];
    if (di < 0 || di >= max_markers) return;
    MapCanvas c{lastw + (int64_t)f * H * W, W, H, 3 * slot + 1};
    draw_slot(c, det + ((int64_t)f * max_markers + di) * VBS_DET_COLS, ref_xy[2 * slot], ref_xy[2 * slot + 1]);
}

__global__ void __launch_bounds__(256) k_draw_resolve(const uint8_t* __restrict__ frames, int H, int W, int64_t sn, int64_t sr,
                                                      const int32_t* __restrict__ lastw, uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int f = blockIdx.y;
    const int y = (int)(p / W), x = (int)(p % W);
    const uint8_t* src = frames + f * sn + y * sr + 3 * x;
    uint8_t* dst = out + ((int64_t)f * H * W + p) * 3;
    const int k = lastw[(int64_t)f * H * W + p];
    if (k == 0) {
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    } else {
        const int sub = (k - 1) % 3;                     // BGR: red (0,0,255), yellow (0,255,255), blue (255,0,0)
        dst[0] = sub == 2 ? 255 : 0;
        dst[1] = sub == 1 ? 255 : 0;
        dst[2] = sub == 2 ? 0 : 255;
    }
}

}  // namespace

extern "C" int vbs_draw_tracking(const uint8_t* frames, int n, int height, int width, int64_t stride_n, int64_t stride_row,
                                 const double* det, int max_markers, const float* table, const double* ref_xy, int m_ref,
                                 int32_t* lastw, uint8_t* out, void* stream) {
    if (n < 0 || n > 65535 || height < 1 || width < 1 || m_ref < 0 || max_markers < 0 || stride_row < 3 * (int64_t)width ||
        (n > 1 && stride_n < stride_row * height) || (int64_t)m_ref * 3 + 1 > INT32_MAX)
        return VBS_EINVAL;
    if (n == 0) return VBS_OK;
    if (!frames || !lastw || !out || (m_ref > 0 && (!det || !table || !ref_xy))) return VBS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t px = (int64_t)height * width;
    if (hipMemsetAsync(lastw, 0, (size_t)(n * px * 4), s) != hipSuccess) return VBS_EHIP;
    if (m_ref > 0)
        hipLaunchKernelGGL(k_draw_slots, dim3((unsigned)((m_ref + 63) / 64), (unsigned)n), dim3(64), 0, s, n, height, width, det,
                           max_markers, table, ref_xy, m_ref, lastw);
    hipLaunchKernelGGL(k_draw_resolve, dim3((unsigned)((px + 255) / 256), (unsigned)n), dim3(256), 0, s, frames, height, width,
                       stride_n, stride_row, lastw, out);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}
