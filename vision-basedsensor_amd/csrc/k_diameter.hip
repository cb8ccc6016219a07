// Marker diameter validation (code/Precision_Validation/DiameterValidation.py: main :218, measure_markers :113-144, the
// statistics :169-170 / :233-234) on the device, per frame of a batch.
//
//   k_diam_threshold : GaussianBlur(gray, (5,5), 0) - OpenCV's fixed small kernel (1, 4, 6, 4, 1) / 16, here in the project's
//                      fixed-point model (taps 16, 64, 96, 64, 16 in 8 fractional bits, (sum + 2^15) >> 16, reflect-101) -
//                      fused with THRESH_BINARY_INV: bit = blur <= threshold.  One wave per 64-px word, the word is the
//                      wave's ballot; the blurred image never exists in memory.
//   (labelling)      : the general kernel k_label<0> labels the bits as its "opened" mask (8-connected, holes filled in
//                      place, component ids in raster order of the first pixel = findContours' order reversed); its band half
//                      gets an empty plane.  The instance is the one the tracker uses: nothing is generated anew for it.
//   k_diam_measure   : one work item per run: every border pixel's 8-neighbourhood -> its outgoing chain steps (step table,
//                      make_step_lut) -> per component the step counts and the shoelace sum x dy - y dx, pixel count and
//                      bounding box: integers, LDS integer atomics (order-free, exact).  Then the two filters (:123, :127,
//                      :130) in float64 and the survivors' rows in contour order (descending component id).
//   k_diam_circle    : one wave per survivor: minEnclosingCircle (:134) of the row extremes of the component (the hull's
//                      vertices are among them) by the incremental construction with 1, 2, 3 boundary points; every
//                      containment test is EXACT in 64-bit integers (coordinates relative to the bounding box), all lanes
//                      test, a ballot picks the first violator.  The box of a survivor is limited to VBS_DIAM_MAX_EXTENT: the
//                      candidates live in a 4 KB LDS array of 2 points per row, packed into 16 + 16 bits.
//   k_diam_stats     : one wave per frame: count, mean, np.std (ddof 0), min, max of diameter_mm in a fixed summation order.
#include <algorithm>

#include "ccl_common.h"

// Outgoing chain steps of a border pixel of hole-free foreground from its 8-neighbourhood (bit d = neighbour in chain
// direction d is foreground; 0 = E, 1 = NE, 2 = N, .. 7 = SE, y down): 4 bits per direction, the number of times the outer
// border leaves the pixel in that direction.  The arcs are those of make_contour_lut (k_morph.hip): one visit per maximal arc
// of background neighbours that holds a 4-neighbour, leaving to the foreground neighbour that follows the arc.  An isolated
// pixel (0) and an interior one (255) have no step.
void make_step_lut(u32 out[256]) {
    for (int p = 0; p < 256; ++p) {
        u32 v = 0;
        if (p != 0 && p != 255) {
            for (int a = 0; a < 8; ++a) {
                if (((p >> a) & 1) || !((p >> ((a + 7) & 7)) & 1)) continue;
                int b = a;
                bool has4 = false;
                while (!((p >> (b & 7)) & 1)) {
                    if (((b & 7) & 1) == 0) has4 = true;
                    ++b;
                }
                if (has4) v += 1u << (4 * (b & 7));
            }
        }
        out[p] = v;
    }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(256) void k_diam_threshold(const u8* __restrict__ gray, int64_t stride_n, int64_t stride_row,
                                                        u64* __restrict__ bits, u64* __restrict__ zero_plane, int nb, int H,
                                                        int W, int WW, int thr) {
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);           // one wave per word
    if (gw >= (int64_t)nb * H * WW) return;                                     // wave-uniform
    const int lane = threadIdx.x & 63;
    const int n = (int)(gw / ((int64_t)H * WW));
    const int r = (int)(gw - (int64_t)n * H * WW);
    const int y = r / WW, j = r - y * WW, x = 64 * j + lane;
    bool bit = false;
    if (x < W) {
        const u8* f = gray + (int64_t)n * stride_n;
        const int xs[5] = {reflect101(x - 2, W), reflect101(x - 1, W), x, reflect101(x + 1, W), reflect101(x + 2, W)};
        const u32 tap[5] = {16u, 64u, 96u, 64u, 16u};
        u32 sum = 0;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const u8* row = f + (int64_t)reflect101(y + dy - 2, H) * stride_row;
            u32 hs = 0;
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) hs += tap[dx] * row[xs[dx]];
            sum += tap[dy] * hs;                                                // <= 255 * 2^16
        }
        bit = (int)((sum + 32768u) >> 16) <= thr;
    }
    const u64 word = __ballot(bit);
    if (lane == 0) {
        bits[gw] = word;
        if (zero_plane) zero_plane[gw] = 0ull;
    }
}

void launch_diam_threshold(vbs_handle* h, const u8* gray, int64_t stride_n, int64_t stride_row, int nb, int thr, u64* bits,
                           u64* zero_plane, hipStream_t s) {
    const int64_t waves = (int64_t)nb * h->H * h->WW;
    VBS_LAUNCH(h, s, "k_diam_threshold", k_diam_threshold, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, gray, stride_n,
               stride_row, bits, zero_plane, nb, h->H, h->W, h->WW, thr);
}

// ------------------------------------------------------------------------------------------------
// node (run) index of the run that holds bit k of word j of a row (the tables k_label leaves in memory)
__device__ __forceinline__ u32 diam_node_of(const u64* __restrict__ row, const u32* __restrict__ wb, int j, int k) {
    int jj = j, kk = k, start;
    for (;;) {
        const u64 w = row[jj];
        const u64 below = (kk == 63) ? ~0ull : ((1ull << (kk + 1)) - 1ull);
        const u64 z = ~w & below;
        if (z) { start = 64 - __clzll(z); break; }
        if (jj == 0 || !(row[jj - 1] >> 63)) { start = 0; break; }
        --jj;
        kk = 63;
    }
    const u64 w = row[jj];
    const u64 prev = (jj > 0) ? (row[jj - 1] >> 63) : 0ull;
    const u64 starts = w & ~((w << 1) | prev);
    const u64 lowmask = start ? ((1ull << start) - 1ull) : 0ull;
    return wb[jj] + (u32)__popcll(starts & lowmask);
}

#define DIAM_SQRT2 1.4142135623730951
#define DIAM_PI 3.14159265358979323846

// frame n by one workgroup of CCL_NT threads; the tables are those of k_label's opened-mask half (slot 1)
__global__ __launch_bounds__(CCL_NT) void k_diam_measure(const u64* __restrict__ open_bits, const u32* __restrict__ wbase_all,
                                                         const u32* __restrict__ node_pos_all,
                                                         const u32* __restrict__ node_comp_all,
                                                         const u32* __restrict__ ncomp_all, const u32* __restrict__ area_first,
                                                         const u32* __restrict__ fstat, const u32* __restrict__ steps_g,
                                                         double* __restrict__ rec_all, int32_t* __restrict__ counts, int H,
                                                         int W, int WW, int maxm, double min_area, double min_circ) {
    __shared__ u64 s_a2[CCL_OPEN_COMPS];
    __shared__ u32 s_ax[CCL_OPEN_COMPS], s_dg[CCL_OPEN_COMPS], s_cnt[CCL_OPEN_COMPS];
    __shared__ u32 s_x0[CCL_OPEN_COMPS], s_y0[CCL_OPEN_COMPS], s_x1[CCL_OPEN_COMPS], s_y1[CCL_OPEN_COMPS];
    __shared__ short l_dx[256], l_dy[256];
    __shared__ u8 l_ax[256], l_dg[256];
    __shared__ u32 tmp[32];
    __shared__ u32 s_nruns;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int status = (int)fstat[n * 8 + 2];
    const u32 ncomp = ncomp_all[n * 2 + 1];
    if (status != 0 || ncomp > (u32)CCL_OPEN_COMPS || ncomp > (u32)maxm) {     // workgroup-uniform
        if (tid == 0) counts[n] = status != 0 ? status : VBS_ECAPACITY;
        return;
    }
    const int NW = H * WW;
    const u64* bits = open_bits + (int64_t)n * NW;
    const u32* wb = wbase_all + ((int64_t)n * 2 + 1) * NW;
    const u32* node_pos = node_pos_all + ((int64_t)n * 2 + 1) * VBS_RUN_CAP;
    const u32* node_comp = node_comp_all + ((int64_t)n * 2 + 1) * VBS_RUN_CAP;
    if (tid < 256) {                                    // the step table as sums: dx, dy, unit steps, diagonal steps
        const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
        const u32 v = steps_g[tid];
        int sx = 0, sy = 0, na = 0, nd = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int c = (int)((v >> (4 * d)) & 15u);
            sx += c * DX[d]; sy += c * DY[d];
            if (d & 1) nd += c; else na += c;
        }
        l_dx[tid] = (short)sx; l_dy[tid] = (short)sy; l_ax[tid] = (u8)na; l_dg[tid] = (u8)nd;
    }
    for (u32 c = tid; c < ncomp; c += CCL_NT) {
        s_a2[c] = 0; s_ax[c] = 0; s_dg[c] = 0; s_cnt[c] = 0;
        s_x0[c] = 0xFFFFFFFFu; s_y0[c] = 0xFFFFFFFFu; s_x1[c] = 0; s_y1[c] = 0;
    }
    if (tid == 0) {
        const u64 w = bits[NW - 1];
        const u64 prev = WW > 1 ? (bits[NW - 2] >> 63) : 0ull;
        s_nruns = min(wb[NW - 1] + (u32)__popcll(w & ~((w << 1) | prev)), (u32)VBS_RUN_CAP);
    }
    __syncthreads();
    const u32 nruns = s_nruns;
    for (u32 i = tid; i < nruns; i += CCL_NT) {
        const u32 cid = node_comp[i], pos = node_pos[i];
        if (cid >= ncomp) continue;                     // (never: the tables are this frame's)
        const int y = (int)(pos / (u32)W), x0 = (int)(pos - (u32)y * (u32)W);
        const u64* rowm = bits + (int64_t)y * WW;
        const bool hasu = y > 0, hasd = y + 1 < H;
        i64 a2 = 0;
        u32 na = 0, nd = 0, len_all = 0;
        bool more = true;
        for (int jw = x0 >> 6; more && jw < WW; ++jw) {          // word segments of the run
            const u64 w = rowm[jw];
            const int lo = jw == (x0 >> 6) ? (x0 & 63) : 0;
            const u64 t = ~(w >> lo);
            const int len = t ? __ffsll((long long)t) - 1 : 64;
            if (len == 0) break;                                 // (the run ended exactly at the previous word's last bit)
            const int hi = lo + len - 1;
            len_all += (u32)len;
            more = hi == 63;
            const u64 gg = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull)) & ~((1ull << lo) - 1ull);
            const bool contR = more && jw + 1 < WW && (rowm[jw + 1] & 1ull);
            const u64 up = hasu ? rowm[jw - WW] : 0ull, dn = hasd ? rowm[jw + WW] : 0ull;
            u64 upL = 0, upR = 0, dnL = 0, dnR = 0;
            if (lo == 0 && jw > 0) { upL = hasu ? rowm[jw - 1 - WW] >> 63 : 0ull; dnL = hasd ? rowm[jw - 1 + WW] >> 63 : 0ull; }
            if (hi == 63 && jw + 1 < WW) { upR = hasu ? rowm[jw + 1 - WW] & 1ull : 0ull; dnR = hasd ? rowm[jw + 1 + WW] & 1ull : 0ull; }
            const u64 E = (gg >> 1) | (contR ? 1ull << 63 : 0ull);
            const u64 Wd = (gg << 1) | (jw > (x0 >> 6) ? 1ull : 0ull);
            const u64 NE = (up >> 1) | (upR << 63), NWd = (up << 1) | upL;
            const u64 SE = (dn >> 1) | (dnR << 63), SW = (dn << 1) | dnL;
            u64 bg = gg & ~(up & dn & E & Wd);                   // pixels with a background 4-neighbour: the border
            while (bg) {
                const int k = __ffsll((long long)bg) - 1;
                bg &= bg - 1;
                const u32 pat = (u32)((E >> k) & 1ull) | ((u32)((NE >> k) & 1ull) << 1) |
                                ((u32)((up >> k) & 1ull) << 2) | ((u32)((NWd >> k) & 1ull) << 3) |
                                ((u32)((Wd >> k) & 1ull) << 4) | ((u32)((SW >> k) & 1ull) << 5) |
                                ((u32)((dn >> k) & 1ull) << 6) | ((u32)((SE >> k) & 1ull) << 7);
                const int x = 64 * jw + k;
                a2 += (i64)(x * (int)l_dy[pat] - y * (int)l_dx[pat]);       // sum over the steps of x dy - y dx
                na += l_ax[pat];
                nd += l_dg[pat];
            }
            if (!contR) break;
        }
        if (a2) atomicAdd(&s_a2[cid], (u64)a2);
        if (na) atomicAdd(&s_ax[cid], na);
        if (nd) atomicAdd(&s_dg[cid], nd);
        atomicAdd(&s_cnt[cid], len_all);
        atomicMin(&s_x0[cid], (u32)x0); atomicMax(&s_x1[cid], (u32)x0 + len_all - 1u);
        atomicMin(&s_y0[cid], (u32)y); atomicMax(&s_y1[cid], (u32)y);
    }
    __syncthreads();
    // the filters, one thread per component in contour order (descending id); survivors keep that order
    const int c = (int)ncomp - 1 - tid;
    bool pass = false;
    double area2 = 0, per = 0, circ = 0;
    if (c >= 0) {
        const i64 sa = (i64)s_a2[c];
        area2 = (double)(sa < 0 ? -sa : sa);
        per = (double)s_ax[c] + (double)s_dg[c] * DIAM_SQRT2;
        if (per > 0.0) circ = (4.0 * DIAM_PI * (area2 * 0.5)) / (per * per);
        pass = !(area2 * 0.5 < min_area) && per > 0.0 && !(circ < min_circ);
    }
    u32 total;
    const u32 rank = ccl_scan(pass ? 1u : 0u, tmp, &total);
    if (pass) {
        double* r = rec_all + ((int64_t)n * maxm + rank) * VBS_DIAM_COLS;
        r[0] = 0; r[1] = 0; r[2] = 0; r[3] = 0;
        r[4] = area2 * 0.5; r[5] = per; r[6] = circ;
        r[7] = (double)s_ax[c]; r[8] = (double)s_dg[c];
        r[9] = (double)area_first[(int64_t)n * maxm + c];
        r[10] = 0;
#pragma unroll
        for (int q = 11; q < 17; ++q) r[q] = 0;
        r[17] = (double)s_cnt[c];
        r[18] = (double)s_x0[c]; r[19] = (double)s_y0[c]; r[20] = (double)s_x1[c]; r[21] = (double)s_y1[c];
        r[22] = (double)(i64)s_a2[c];
        r[23] = (double)c;
    }
    if (tid == 0) counts[n] = (int32_t)total;
}

// ------------------------------------------------------------------------------------------------
struct DiamCircle {                                     // boundary points (relative to the bounding box) and, for three, the
    int ns, ax, ay, bx, by, cx, cy;                     // circumcentre a + (ux, uy) / D
    i64 D, ux, uy;
};

// p inside or on the circle: exact (|coordinates| < VBS_DIAM_MAX_EXTENT = 2^9: the products here stay below 2^41, the
// squared circumradius numerator ux^2 + uy^2 below 2^60; the extent's limit is the candidate array, not this range)
__device__ __forceinline__ bool diam_inside(const DiamCircle& c, int px, int py) {
    if (c.ns == 1) return px == c.ax && py == c.ay;
    if (c.ns == 2)                                       // Thales: the angle a p b is at least a right one
        return (i64)(px - c.ax) * (px - c.bx) + (i64)(py - c.ay) * (py - c.by) <= 0;
    const i64 qx = px - c.ax, qy = py - c.ay;            // |q D - u|^2 <= |u|^2  <=>  D (D |q|^2 - 2 q.u) <= 0
    const i64 t = c.D * (qx * qx + qy * qy) - 2 * (qx * c.ux + qy * c.uy);
    return (c.D > 0) ? t <= 0 : t >= 0;
}

// first index in [from, to) whose point lies outside the circle, -1 if none (wave-uniform result)
__device__ __forceinline__ int diam_first_out(const DiamCircle& c, const u32* pts, int from, int to) {
    const int lane = threadIdx.x & 63;
    for (int base = from & ~63; base < to; base += 64) {
        const int i = base + lane;
        bool out = false;
        if (i >= from && i < to) {
            const u32 p = pts[i];
            out = !diam_inside(c, (int)(p & 0xFFFFu), (int)(p >> 16));
        }
        const u64 m = __ballot(out);
        if (m) return base + __ffsll((long long)m) - 1;
    }
    return -1;
}

__global__ __launch_bounds__(64) void k_diam_circle(const u64* __restrict__ open_bits, const u32* __restrict__ wbase_all,
                                                    const u32* __restrict__ node_comp_all, u32* __restrict__ fstat,
                                                    double* __restrict__ rec_all, const int32_t* __restrict__ counts, int H, int W,
                                                    int WW, int maxm, double scale, double offset_mm) {
    __shared__ u32 pts[2 * VBS_DIAM_MAX_EXTENT];         // x | y << 16, relative to the bounding box
    const int n = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
    if (s >= counts[n]) return;                         // (also a negative status)
    double* r = rec_all + ((int64_t)n * maxm + s) * VBS_DIAM_COLS;
    const u32 cid = (u32)r[23];
    const int x0 = (int)r[18], y0 = (int)r[19], x1 = (int)r[20], y1 = (int)r[21];
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    if (bw > VBS_DIAM_MAX_EXTENT || bh > VBS_DIAM_MAX_EXTENT) {   // never truncated: the frame is reported instead
        if (lane == 0) atomicMin((int*)&fstat[n * 8 + 2], VBS_ECAPACITY);
        return;
    }
    const int NW = H * WW;
    const u64* bits = open_bits + (int64_t)n * NW;
    const u32* wb = wbase_all + ((int64_t)n * 2 + 1) * NW;
    const u32* node_comp = node_comp_all + ((int64_t)n * 2 + 1) * VBS_RUN_CAP;
    // candidates: the leftmost and rightmost pixel of the component in every row of its box (an 8-connected component has
    // a pixel in each of them)
    for (int rr = lane; rr < bh; rr += 64) {
        const int y = y0 + rr;
        const u64* row = bits + (int64_t)y * WW;
        int mn = 0x7FFFFFFF, mx = -1;
        for (int j = x0 >> 6; j <= (x1 >> 6); ++j) {
            u64 w = row[j];
            if (j == (x0 >> 6)) w &= ~0ull << (x0 & 63);
            if (j == (x1 >> 6) && (x1 & 63) != 63) w &= (1ull << ((x1 & 63) + 1)) - 1ull;
            while (w) {
                const u64 lowbit = w & (~w + 1ull);
                const u64 t = w + lowbit;
                const u64 g = w & ~t;
                w &= t;
                const int k0 = __ffsll((long long)g) - 1, k1 = 63 - __clzll(g);
                if (node_comp[diam_node_of(row, wb + (int64_t)y * WW, j, k0)] != cid) continue;
                mn = min(mn, 64 * j + k0);
                mx = max(mx, 64 * j + k1);
            }
        }
        if (mx < 0) { mn = mx = (int)r[9] % W; }         // (never: see above) - a point of the component all the same
        pts[2 * rr] = (u32)(mn - x0) | ((u32)rr << 16);
        pts[2 * rr + 1] = (u32)(mx - x0) | ((u32)rr << 16);
    }
    __syncthreads();
    const int N = 2 * bh;
    DiamCircle c;
    c.ns = 1; c.ax = (int)(pts[0] & 0xFFFFu); c.ay = (int)(pts[0] >> 16);
    c.bx = c.by = c.cx = c.cy = 0; c.D = 1; c.ux = c.uy = 0;
    for (int i = diam_first_out(c, pts, 1, N); i >= 0; i = diam_first_out(c, pts, i + 1, N)) {
        c.ns = 1; c.ax = (int)(pts[i] & 0xFFFFu); c.ay = (int)(pts[i] >> 16);
        for (int j = diam_first_out(c, pts, 0, i); j >= 0; j = diam_first_out(c, pts, j + 1, i)) {
            c.ns = 2; c.bx = (int)(pts[j] & 0xFFFFu); c.by = (int)(pts[j] >> 16);
            for (int k = diam_first_out(c, pts, 0, j); k >= 0; k = diam_first_out(c, pts, k + 1, j)) {
                const int kx = (int)(pts[k] & 0xFFFFu), ky = (int)(pts[k] >> 16);
                const i64 Bx = c.bx - c.ax, By = c.by - c.ay, Cx = kx - c.ax, Cy = ky - c.ay;
                const i64 D = 2 * (Bx * Cy - By * Cx);
                if (D == 0) continue;                    // (never: a = p_i and b = p_j lie ON the smallest circle around the prefix that
                                                         //  holds p_k, so a p_k on the line a b beyond either would put that one strictly inside)
                const i64 B2 = Bx * Bx + By * By, C2 = Cx * Cx + Cy * Cy;
                c.ns = 3; c.cx = kx; c.cy = ky; c.D = D;
                c.ux = Cy * B2 - By * C2; c.uy = Bx * C2 - Cx * B2;
            }
        }
    }
    if (lane == 0) {
        double cx, cy, rad;
        if (c.ns == 1) { cx = c.ax; cy = c.ay; rad = 0.0; }
        else if (c.ns == 2) {
            cx = (double)(c.ax + c.bx) * 0.5; cy = (double)(c.ay + c.by) * 0.5;
            const i64 dx = c.ax - c.bx, dy = c.ay - c.by;
            rad = sqrt((double)(dx * dx + dy * dy)) * 0.5;
        } else {
            cx = (double)c.ax + (double)c.ux / (double)c.D; cy = (double)c.ay + (double)c.uy / (double)c.D;
            rad = sqrt((double)(c.ux * c.ux + c.uy * c.uy)) / fabs((double)c.D);
        }
        r[0] = cx + (double)x0; r[1] = cy + (double)y0; r[2] = rad;
        r[3] = 2.0 * rad / scale + offset_mm;
        r[10] = (double)c.ns;
        r[11] = (double)(c.ax + x0); r[12] = (double)(c.ay + y0);
        if (c.ns >= 2) { r[13] = (double)(c.bx + x0); r[14] = (double)(c.by + y0); }
        if (c.ns >= 3) { r[15] = (double)(c.cx + x0); r[16] = (double)(c.cy + y0); }
    }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double diam_wave_sum(double v) {     // xor butterfly: the same order in every run and lane
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(64) void k_diam_stats(const double* __restrict__ rec_all, const u32* __restrict__ fstat,
                                                   int32_t* __restrict__ counts, double* __restrict__ stats, int maxm) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int status = (int)fstat[n * 8 + 2];
    int cnt = counts[n];
    if (status < 0) cnt = status;
    const double* rec = rec_all + (int64_t)n * maxm * VBS_DIAM_COLS;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double sum = 0, mn = 1e300, mx = -1e300;
    for (int i = lane; i < cnt; i += 64) {
        const double d = rec[(int64_t)i * VBS_DIAM_COLS + 3];
        sum += d; mn = fmin(mn, d); mx = fmax(mx, d);
    }
    sum = diam_wave_sum(sum);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { mn = fmin(mn, __shfl_xor(mn, off)); mx = fmax(mx, __shfl_xor(mx, off)); }
    const double mean = cnt > 0 ? sum / (double)cnt : nan;
    double ss = 0;
    for (int i = lane; i < cnt; i += 64) {
        const double d = rec[(int64_t)i * VBS_DIAM_COLS + 3] - mean;
        ss += d * d;
    }
    ss = diam_wave_sum(ss);
    if (lane == 0) {
        counts[n] = cnt;
        double* o = stats + (int64_t)n * VBS_DIAM_STATS_COLS;
        o[0] = (double)(cnt > 0 ? cnt : 0);
        o[1] = mean;
        o[2] = cnt > 0 ? sqrt(ss / (double)cnt) : nan;
        o[3] = cnt > 0 ? mn : nan;
        o[4] = cnt > 0 ? mx : nan;
    }
}

// label + measure + circle + statistics of the nb frames whose bits lie in w.open_bits (w.band_bits empty)
void launch_diam_measure(vbs_handle* h, Workspace& w, int nb, double min_area, double min_circ, double scale, double offset_mm,
                         double* rec, int32_t* counts, double* stats, hipStream_t s) {
    launch_label(h, w, nb, 1, nullptr, nullptr, s);      // k_label<0> over EVERY frame, planes as they lie in the workspace
    VBS_LAUNCH(h, s, "k_diam_measure", k_diam_measure, dim3(nb), dim3(CCL_NT), 0, s, w.open_bits, w.wbase, w.node_pos, w.node_comp,
               w.ncomp, w.area_first, w.fstat, h->step_lut, rec, counts, h->H, h->W, h->WW, h->maxm, min_area, min_circ);
    VBS_LAUNCH(h, s, "k_diam_circle", k_diam_circle, dim3(std::min(h->maxm, CCL_OPEN_COMPS), nb), dim3(64), 0, s, w.open_bits,
               w.wbase, w.node_comp, w.fstat, rec, counts, h->H, h->W, h->WW, h->maxm, scale, offset_mm);
    VBS_LAUNCH(h, s, "k_diam_stats", k_diam_stats, dim3(nb), dim3(64), 0, s, rec, w.fstat, counts, stats, h->maxm);
}
