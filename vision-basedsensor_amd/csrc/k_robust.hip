// Despiking a tracked series: a gap-aware rolling median and median absolute deviation along time for many series
// at once, and the Hampel rule on them.  An order statistic has no order of summation: every correct selection gives the same bits,
// so only the definitions of include/vbs.h bind, and a result depends on its window only, never on the launch shape.
//   k_median_mad    one wave = 64 series (the lanes) x VBS_ROBUST_TILE frames of ONE value column (blockIdx.z).  A lane walks the
//                   rows [first - h, last + h] of its tile in ascending order and keeps the valid values of the current window
//                   SORTED in its own LDS column win[k][lane] (no lane reads another's: no barrier; a wave's access to one k is
//                   512 contiguous bytes, free of bank conflicts whatever k each lane is at).  The row that enters is inserted
//                   by shifting, BEHIND the values equal to it; the row that leaves is the oldest of the window, so among values
//                   equal to it it is the FIRST: the column is in (x, g) order by construction, -0.0 and +0.0 tie.  Both places
//                   are COUNTED (values <= x, values < x) in a pass of independent reads, not searched.  The median is
//                   read at its index; the MAD comes from a two-pointer walk outward from the median over the sorted column
//                   (|x - med| does not decrease away from med on either side, rounding is monotone): c/2 + 1 reads per output
//                   where rank counting would take c^2.  Lanes differ in c because of gaps; their loops are predicated.
//   k_hampel_flags  one thread per emitted entry: the spike test on the stored med and mad, the flag, and the clean record
// The data is time-major, series on the fast axis: a wave's accesses to one frame row are contiguous.
#include "common.h"
#pragma clang fp contract(off)

#define ROBUST_WIN (2 * VBS_ROBUST_MAX_HALF + 1)
static_assert(ROBUST_WIN * 64 * sizeof(double) * 2 <= 160 * 1024, "two workgroups fit the LDS of a CU");

// out [fe - fb][s][2 + 2 nv]: this launch writes c (the instance of value 0), med_v and mad_v; k_hampel_flags writes the flag
__global__ __launch_bounds__(64) void k_median_mad(const double* __restrict__ rec, int n, int s, int cols, int nv, int h,
                                                   int min_count, int frame_begin, int frame_end, double* __restrict__ out) {
    __shared__ double win[ROBUST_WIN][64];
    const int lane = threadIdx.x;
    const int v = blockIdx.z;
    const int64_t series = (int64_t)blockIdx.y * 64 + lane;
    if (series >= s) return;                                     // (no barrier below: a lane owns its column)
    const int64_t tile0 = (int64_t)frame_begin + (int64_t)blockIdx.x * VBS_ROBUST_TILE;       // first output frame of the tile
    const int64_t tile1 = tile0 + VBS_ROBUST_TILE < frame_end ? tile0 + VBS_ROBUST_TILE : frame_end;   // one past its last
    const int64_t row_step = (int64_t)s * cols;
    const double* base = rec + series * cols;
    const int oc = 2 + 2 * nv;

    // The row that enters at step t and the row that leaves after it are loaded one step ahead, so their latency hides behind
    // the step's LDS work.  A row's value is loaded whatever its flag (the row exists) and selected out when invalid.
    auto load = [&](int64_t r, bool& ok, double& x) {
        ok = false;
        x = 0.0;
        if (r >= 0 && r < n) {
            const double* p = base + r * row_step;
            const double y = p[1 + v];
            ok = p[0] != 0.0;
            x = y != y ? 0.0 : y;                                // a valid NaN (refused by the interface) must not break the order
        }
    };
    bool in_ok, out_ok;
    double in_x, out_x;
    load(tile0 - h, in_ok, in_x);
    load(tile0 - h, out_ok, out_x);                              // the first row to leave is the first that entered

    int c = 0;                                                   // the population of the window, win[0 .. c-1][lane] sorted
    for (int64_t t = tile0 - h; t < tile1 + h; ++t) {            // row t enters; rows outside [0, n) are never read
        const int64_t f = t - h;                                 // the frame whose window [f - h, f + h] is complete after it
        bool nin_ok, nout_ok;
        double nin_x, nout_x;
        load(t + 1 < tile1 + h ? t + 1 : -1, nin_ok, nin_x);
        load(f >= tile0 ? f + 1 - h : -1, nout_ok, nout_x);
        if (in_ok) {
            // behind every value <= x.  The count is a full pass whose reads do not depend on each other (a search that stops
            // at the place would wait for every read in turn), and so is the shift
            const double x = in_x;
            int pos = 0;
#pragma unroll 8
            for (int k = 0; k < c; ++k) pos += win[k][lane] <= x ? 1 : 0;
#pragma unroll 8
            for (int k = c - 1; k >= pos; --k) win[k + 1][lane] = win[k][lane];
            win[pos][lane] = x;
            ++c;
        }
        if (f >= tile0) {
            double med = 0.0, mad = 0.0;
            if (c >= min_count) {
                const int mi = (c - 1) >> 1;
                med = win[mi][lane];
                if (!(c & 1)) med = 0.5 * med + 0.5 * win[mi + 1][lane];
                // the split: rows below p are <= med, rows from p on are >= med.  c / 2 is that split unless the halving of a
                // subnormal rounded med out of [q_mi, q_mi+1]; the two loops cost one read each otherwise
                int p = c >> 1;
                while (p > 0 && win[p - 1][lane] > med) --p;
                while (p < c && win[p][lane] < med) ++p;
                int li = p - 1, ri = p;
                double dl = li >= 0 ? fabs(win[li][lane] - med) : 0.0;
                double dr = ri < c ? fabs(win[ri][lane] - med) : 0.0;
                double prev = 0.0, cur = 0.0;                    // the deviations of rank step - 1 and step
                for (int step = 0; step <= (c >> 1); ++step) {   // at most c steps: one side always has a candidate
                    const bool left = li >= 0 && (ri >= c || dl <= dr);
                    prev = cur;
                    cur = left ? dl : dr;
                    li -= left ? 1 : 0;
                    ri += left ? 0 : 1;
                    const int idx = left ? li : ri;
                    const double d = (idx >= 0 && idx < c) ? fabs(win[idx][lane] - med) : 0.0;
                    dl = left ? d : dl;
                    dr = left ? dr : d;
                }
                mad = (c & 1) ? cur : 0.5 * prev + 0.5 * cur;
            }
            double* o = out + ((f - frame_begin) * s + series) * oc;
            if (v == 0) o[1] = (double)c;
            o[2 + v] = med;
            o[2 + nv + v] = mad;

            if (out_ok) {                                        // row f - h leaves (it is >= tile0 - h: it did enter)
                // the oldest row of the window: the FIRST of the values equal to it, which as many values are below
                const double x = out_x;
                int pos = 0;
#pragma unroll 8
                for (int k = 0; k < c; ++k) pos += win[k][lane] < x ? 1 : 0;
#pragma unroll 8
                for (int k = pos; k < c - 1; ++k) win[k][lane] = win[k + 1][lane];
                --c;
            }
        }
        in_ok = nin_ok; in_x = nin_x;
        if (f >= tile0) { out_ok = nout_ok; out_x = nout_x; }
    }
}

// One thread per emitted entry, 4 frames x 64 series a workgroup; at most ROBUST_FLAG_BLOCKS workgroups along the frames, which
// stride over the rest, so the launch stays inside the grid limits whatever the frame count.  clean [fe - fb][s][cols] may be null.
#define ROBUST_FLAG_BLOCKS 65535
__global__ __launch_bounds__(256) void k_hampel_flags(const double* __restrict__ rec, int s, int cols, int nv, int min_count,
                                                      double thr, double min_scale, int frame_begin, int frame_end,
                                                      double* __restrict__ out, double* __restrict__ clean) {
    const int64_t series = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (series >= s) return;
    for (int64_t f = (int64_t)frame_begin + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < frame_end;
         f += (int64_t)gridDim.x * 4) {
        const double* in = rec + (f * s + series) * cols;
        double* o = out + ((f - frame_begin) * s + series) * (2 + 2 * nv);
        const bool valid = in[0] != 0.0;
        const bool judged = o[1] >= (double)min_count;
        bool spike = false;
        if (valid && judged) {
            for (int v = 0; v < nv; ++v) {
                const double dev = fabs(in[1 + v] - o[2 + v]);
                spike = spike || (dev > thr * o[2 + nv + v] && dev > min_scale);
            }
        }
        o[0] = (valid ? 1.0 : 0.0) + (judged ? 2.0 : 0.0) + (spike ? 4.0 : 0.0);
        if (!clean) continue;
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(in);     // bit for bit: NaN payloads survive
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(clean + ((f - frame_begin) * s + series) * cols);
        dst[0] = spike ? 0ull : src[0];
        for (int c = 1; c < cols; ++c) dst[c] = src[c];
    }
}

// thr = k_sigma * 1.4826, formed by the caller
void launch_hampel_series(const double* rec, int n, int s, int cols, int n_values, int half_window, int min_count, double thr,
                          double min_scale, int frame_begin, int frame_end, double* out, double* clean, hipStream_t st) {
    const int64_t frames = (int64_t)frame_end - frame_begin;
    const unsigned groups = (unsigned)((s + 63) / 64);
    hipLaunchKernelGGL(k_median_mad, dim3((unsigned)((frames + VBS_ROBUST_TILE - 1) / VBS_ROBUST_TILE), groups, (unsigned)n_values),
                       dim3(64), 0, st, rec, n, s, cols, n_values, half_window, min_count, frame_begin, frame_end, out);
    const int64_t quads = (frames + 3) / 4;
    hipLaunchKernelGGL(k_hampel_flags, dim3((unsigned)(quads < ROBUST_FLAG_BLOCKS ? quads : ROBUST_FLAG_BLOCKS), groups), dim3(256), 0,
                       st, rec, s, cols, n_values, min_count, thr, min_scale, frame_begin, frame_end, out, clean);
}
