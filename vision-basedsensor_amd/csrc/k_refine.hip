// f23: grey-level refinement of tracked markers - levels, area, centre, axes (the rule: include/vbs.h, vbs_refine_markers).
//   k_refine   one wave per table row, VBS_REFINE_WAVES rows a workgroup.  A lane owns the window's columns `lane` and `lane + 64`
//              (the window is at most 127 wide) and walks the rows in order.
//              pass 1  the levels of the core and of the ring into two 256-bin histograms of the wave in LDS (LDS atomics);
//                      the quartiles and the trimmed sums come from a wave scan over the bins, four bins a lane.
//              pass 2  the disc is read a SECOND time for the weights: keeping up to 2 x 127 levels a lane between the passes
//                      would need an array indexed by the row counter, which the compiler puts into scratch; a wave touches at
//                      most 127 x 127 bytes, which the second pass finds in the vector L1.  A lane's dx is fixed, so it adds
//                      sum w, sum w dy and sum w dy dy per column in int32 and multiplies by dx, dx dx once; the six int64 sums are
//                      folded over the wave (wave_fold.h) - integers, exact whatever the order.
//              Both passes take the rows RF_ROWS at a time and load a batch before they use it, unconditionally (every pixel of
//              the window is inside the frame; a batch that runs past the last row re-reads that row and drops it): one
//              load latency per batch, not per row.  With a load behind each row's own test the kernel ran at one latency a row.
//              Lane 0 does the float64 tail and writes the row of every output.
// A row whose status is decided from the table row alone (1 .. 4) loads no pixel.  The waves of a workgroup meet at two
// barriers (around pass 1) and nowhere else; no wait between workgroups.  Float64 without contraction, as the restatement in the
// tests computes.
#include <cmath>
#include "common.h"
#include "wave_fold.h"

#pragma clang fp contract(off)

#define RF_WAVES VBS_REFINE_WAVES
#define RF_BINS 256
#define RF_ROWS 8                               // window rows whose loads a lane has in flight together

struct RefineParams {
    double core_f, disc_f, ring_f, min_contrast, max_shift_f;
    int polarity, keep_unrefined;
};

static __device__ __forceinline__ int rf_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

static __device__ __forceinline__ int rf_wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

// T8 of the set whose histogram is `hist` (at least one pixel): lane l holds the bins 4 l .. 4 l + 3
static __device__ int rf_trimmed8(const u32* hist, int lane) {
    const uint4 b4 = *reinterpret_cast<const uint4*>(hist + 4 * lane);
    const int b[4] = {(int)b4.x, (int)b4.y, (int)b4.z, (int)b4.w};
    const int mine = (b[0] + b[1]) + (b[2] + b[3]);
    const int incl = rf_scan_inclusive(mine, lane);
    const int total = __shfl(incl, 63);
    int first1 = RF_BINS, first3 = RF_BINS, cum = incl - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cum += b[k];
        if (first1 == RF_BINS && cum * 4 >= total) first1 = 4 * lane + k;
        if (first3 == RF_BINS && cum * 4 >= total * 3) first3 = 4 * lane + k;
    }
    const int q1 = rf_wave_min(first1), q3 = rf_wave_min(first3);
    int cnt = 0, sv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = 4 * lane + k;
        if (v >= q1 && v <= q3) { cnt += b[k]; sv += v * b[k]; }
    }
    cnt = wave_sum(cnt);
    sv = wave_sum(sv);
    return (8 * sv) / cnt;
}

__global__ __launch_bounds__(64 * RF_WAVES) void k_refine(const u8* __restrict__ gray, int h, int w, int64_t stride_n,
                                                          int64_t stride_row, const float* __restrict__ table, int m_ref,
                                                          int64_t rows, RefineParams p, double* __restrict__ rec,
                                                          i64* __restrict__ sums, float* __restrict__ table_out) {
    __shared__ __attribute__((aligned(16))) u32 hist[RF_WAVES][2 * RF_BINS];        // core, ring
    const double PI = 3.14159265358979323846;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t id = (int64_t)blockIdx.x * RF_WAVES + wave;
    const bool have = id < rows;
    u32* hc = hist[wave];
    u32* hr = hc + RF_BINS;

    // ---- the table row: everything here is the same in every lane of the wave --------------------------------------------------
    float in[VBS_TABLE_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int status = VBS_REFINE_NOT_TRACKED, flags = 0, x0 = 0, y0 = 0, R = 0, c2 = 0, g2 = 0;
    double Cx = 0.0, Cy = 0.0, r = 0.0;
    if (have) {
        const float* row = table + id * VBS_TABLE_COLS;
#pragma unroll
        for (int c = 0; c < VBS_TABLE_COLS; ++c) in[c] = row[c];
        flags = (in[0] >= 0.f && in[0] < 16777216.f) ? (int)in[0] : 0;
        Cx = (double)in[1];
        Cy = (double)in[2];
        const double major = (double)in[3];
        r = 0.5 * major;
        if (!(flags & VBS_FLAG_TRACKED)) status = VBS_REFINE_NOT_TRACKED;
        else if (!isfinite(Cx) || !isfinite(Cy) || !isfinite(major) || major < 2.0 || fabs(Cx) >= 1073741824.0 ||
                 fabs(Cy) >= 1073741824.0)
            status = VBS_REFINE_BAD_ROW;
        else if (ceil(p.ring_f * r) + 1.0 > (double)VBS_REFINE_MAX_R) status = VBS_REFINE_TOO_LARGE;
        else {
            x0 = (int)floor(Cx + 0.5);
            y0 = (int)floor(Cy + 0.5);
            R = (int)ceil(p.ring_f * r) + 1;
            const double cr = p.core_f * r, gr = p.disc_f * r;
            c2 = (int)floor(cr * cr);
            g2 = (int)floor(gr * gr);
            status = (x0 - R < 0 || x0 + R > w - 1 || y0 - R < 0 || y0 + R > h - 1) ? VBS_REFINE_AT_BORDER : 0;
        }
    }
    const int R2 = R * R;
    const u8* src = gray + (have ? (id / m_ref) * stride_n : 0);

    // ---- pass 1: the levels of the core and of the ring ------------------------------------------------------------------------
    for (int i = lane; i < 2 * RF_BINS; i += 64) hc[i] = 0;
    __syncthreads();
    if (status == 0) {
        const u8* win = src + (int64_t)y0 * stride_row + (x0 - R);
        for (int dy0 = -R; dy0 <= R; dy0 += RF_ROWS) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int col = lane + 64 * k;
                if (col <= 2 * R) {
                    const int dx2 = (col - R) * (col - R);
                    int v[RF_ROWS];
#pragma unroll
                    for (int j = 0; j < RF_ROWS; ++j) v[j] = win[(int64_t)min(dy0 + j, R) * stride_row + col];
#pragma unroll
                    for (int j = 0; j < RF_ROWS; ++j) {
                        const int dy = dy0 + j, d2 = dx2 + dy * dy;
                        const bool core = d2 <= c2;
                        if (dy <= R && (core || (d2 > g2 && d2 <= R2)))
                            atomicAdd(&(core ? hc : hr)[p.polarity ? 255 - v[j] : v[j]], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    int B8 = 0, D8 = 0, C8 = 0;
    if (status == 0) {
        B8 = rf_trimmed8(hr, lane);
        D8 = rf_trimmed8(hc, lane);
        C8 = B8 - D8;
        if ((double)C8 < 8.0 * p.min_contrast) status = VBS_REFINE_LOW_CONTRAST;
    }

    // ---- pass 2: the six sums over the disc ------------------------------------------------------------------------------------
    i64 S[6] = {0, 0, 0, 0, 0, 0};                       // S0, Sx, Sy, Sxx, Sxy, Syy
    const bool summed = status == 0;
    if (summed) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int col = lane + 64 * k, dx = col - R;
            int a0 = 0, a1 = 0, a2 = 0;                  // sum w, sum w dy, sum w dy dy of this column: below 2^29 at R = 63
            if (col <= 2 * R) {
                const u8* colp = src + (int64_t)y0 * stride_row + (x0 - R) + col;
                for (int dy0 = -R; dy0 <= R; dy0 += RF_ROWS) {
                    const int near = dy0 > 0 ? dy0 : (dy0 + RF_ROWS - 1 < 0 ? -(dy0 + RF_ROWS - 1) : 0);
                    if (near * near > g2) continue;      // (the same in every lane) no row of the batch meets the disc
                    int v[RF_ROWS];
#pragma unroll
                    for (int j = 0; j < RF_ROWS; ++j) v[j] = colp[(int64_t)min(dy0 + j, R) * stride_row];
#pragma unroll
                    for (int j = 0; j < RF_ROWS; ++j) {
                        const int dy = dy0 + j, dy2 = dy * dy;
                        const int lv = p.polarity ? 255 - v[j] : v[j];
                        const int wgt = (dy <= R && dx * dx + dy2 <= g2) ? min(max(B8 - 8 * lv, 0), C8) : 0;
                        a0 += wgt;
                        a1 += wgt * dy;
                        a2 += wgt * dy2;
                    }
                }
            }
            S[0] += a0;
            S[1] += (i64)a0 * dx;
            S[2] += a1;
            S[3] += (i64)a0 * (dx * dx);
            S[4] += (i64)a1 * dx;
            S[5] += a2;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) S[q] = wave_fold_down(S[q]);
    }
    if (!have || lane != 0) return;

    // ---- lane 0: the float64 tail and the row of every output ------------------------------------------------------------------
    double o[VBS_REFINE_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (status == 0 || status == VBS_REFINE_LOW_CONTRAST) {
        o[8] = (double)B8 / 8.0;
        o[9] = (double)D8 / 8.0;
    }
    if (summed) {
        const double A = (double)S[0] / (double)C8;
        const double d_area = 2.0 * sqrt(A / PI);
        o[6] = d_area;
        o[7] = A;
        if (S[0] <= 0) status = VBS_REFINE_DEGENERATE;
        else {
            const double s0 = (double)S[0];
            const double cx = (double)x0 + (double)S[1] / s0, cy = (double)y0 + (double)S[2] / s0;
            const double ex = cx - Cx, ey = cy - Cy;
            const double shift = hypot(ex, ey);
            o[1] = cx;
            o[2] = cy;
            o[11] = shift;
            const double den = s0 * s0;
            const double mxx = (double)(S[3] * S[0] - S[1] * S[1]) / den;
            const double mxy = (double)(S[4] * S[0] - S[1] * S[2]) / den;
            const double myy = (double)(S[5] * S[0] - S[2] * S[2]) / den;
            const double t = 0.5 * (mxx + myy), hd = 0.5 * (mxx - myy);
            const double q = sqrt(hd * hd + mxy * mxy);
            const double l1 = t + q, l2 = t - q;
            if (!(l2 > 0.0)) status = VBS_REFINE_DEGENERATE;
            else {
                const double k = sqrt(sqrt(l1 / l2));
                o[3] = d_area * k;
                o[4] = d_area / k;
                o[5] = (0.5 * atan2(2.0 * mxy, mxx - myy)) * 180.0 / PI + 180.0;
                o[10] = sqrt(l1 * l2) - A / (4.0 * PI);
                if (shift > p.max_shift_f * r) status = VBS_REFINE_MOVED;
            }
        }
    }
    o[0] = (double)status;
    if (rec) {
        double* dst = rec + id * VBS_REFINE_COLS;
#pragma unroll
        for (int c = 0; c < VBS_REFINE_COLS; ++c) dst[c] = o[c];
    }
    if (sums) {
        i64* dst = sums + id * VBS_REFINE_SUM_COLS;
        const bool lv = status == 0 || status >= VBS_REFINE_LOW_CONTRAST;
        dst[0] = lv ? B8 : 0;
        dst[1] = lv ? D8 : 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) dst[2 + q] = S[q];
    }
    if (table_out) {
        float t[VBS_TABLE_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, in[9]};
        if (status == 0) {
            t[0] = (float)VBS_FLAG_TRACKED;
#pragma unroll
            for (int c = 1; c <= 5; ++c) t[c] = (float)o[c];
        } else if (p.keep_unrefined && status >= VBS_REFINE_BAD_ROW) {
            t[0] = (float)(flags & ~VBS_FLAG_XYZ);
#pragma unroll
            for (int c = 1; c <= 5; ++c) t[c] = in[c];
        }
        float* dst = table_out + id * VBS_TABLE_COLS;
#pragma unroll
        for (int c = 0; c < VBS_TABLE_COLS; ++c) dst[c] = t[c];
    }
}

void launch_refine(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, const float* table, int m_ref,
                   double core_f, double disc_f, double ring_f, double min_contrast, double max_shift_f, int polarity,
                   int keep_unrefined, double* rec, i64* sums, float* table_out, hipStream_t s) {
    // vbs_refine_markers bounds n * m_ref below 2^30, a grid's x extent
    const int64_t rows = (int64_t)n * m_ref;
    const RefineParams p = {core_f, disc_f, ring_f, min_contrast, max_shift_f, polarity, keep_unrefined};
    hipLaunchKernelGGL(k_refine, dim3((unsigned)((rows + RF_WAVES - 1) / RF_WAVES)), dim3(64 * RF_WAVES), 0, s, gray, h, w, stride_n,
                       stride_row, table, m_ref, rows, p, rec, sums, table_out);
}
