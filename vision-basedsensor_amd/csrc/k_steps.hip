// The probe-indentation analysis: a step detector along time with gaps for many series at once, the peak search
// on its response, and the statistics of the dwells between the steps.  Float64 without contraction, no atomics, a stated order
// of every sum: a result depends on its inputs only, never on the launch shape (the rule of k_series.hip and k_filter.hip).
//   k_step_response<NV>   k_fir's orientation: tile = 64 series (the lanes) x STEP_WAVES * P frames, P outputs a lane with BOTH
//                         one-sided sums of each in registers; the input rows [first - w, last + w) of the tile stream ONCE, in
//                         ascending order, through a stage of STEP_ROWS rows in LDS, every wave adding a row to the left or the
//                         right window of those of its outputs that reach it.  One output therefore adds each of its windows in
//                         ascending g from 0.0 whatever the tile or s.
//   k_find_steps          one workgroup per 64 series walks the time tiles IN ASCENDING ORDER, so the list is ascending by
//                         construction: the scores of [first - w, last + w] stream through the same kind of stage (a row that is
//                         not ok is staged as NaN: it compares false, so it neither is a step nor suppresses one), every lane
//                         keeps its P candidates in registers, the marks of a tile go through LDS to wave 0, which appends.
//   k_dwell_stats<NV>     one wave per (series, dwell): lane sums in ascending order, the fold of k_axis_displacement, two passes.
// The data is time-major, series on the fast axis: a wave's accesses to one frame row are contiguous.
#include "common.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define STEP_WAVES 8
#define STEP_ROWS  16                    // input rows staged in LDS at a time: 16 x 64 x (NV + 1) doubles, 32 KB at NV = 3
#define FIND_P     8                     // candidates (consecutive frames) a lane keeps in registers
#define FIND_TILE  (STEP_WAVES * FIND_P)
#define FIND_ROWS  64                    // score rows staged at a time: 64 x 64 doubles, 32 KB
static_assert(FIND_P <= 8, "a wave's marks of a tile travel as one byte a lane");

// outputs (consecutive frames) a lane keeps in registers: 2 NV + 2 accumulators each, so fewer of them for the wide records
template <int NV> struct StepP { static constexpr int value = NV <= 3 ? 8 : 4; };

template <int NV>
__global__ __launch_bounds__(STEP_WAVES * 64) void k_step_response(const double* __restrict__ rec, int n, int s, int cols, int w,
                                                                   int min_count, double* __restrict__ out) {
    constexpr int P = StepP<NV>::value, TILE = STEP_WAVES * P;
    __shared__ double stage[STEP_ROWS][NV + 1][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t series = (int64_t)blockIdx.y * 64 + lane;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE;                          // first output frame of the tile
    const int64_t tile1 = tile0 + TILE < n ? tile0 + TILE : n;                 // one past its last
    const int64_t f0 = tile0 + wave * P;                                       // first output of this wave
    // output f reaches rows [f - w, f + w); rows outside [0, n) are in no window: they are not visited at all
    const int64_t row_lo = tile0 - w > 0 ? tile0 - w : 0;
    const int64_t row_hi = tile1 - 1 + w - 1 < n - 1 ? tile1 - 1 + w - 1 : n - 1;
    const int64_t row_step = (int64_t)s * cols;

    double sl[P][NV], sr[P][NV];
    int cl[P], cr[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        cl[p] = 0; cr[p] = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) { sl[p][v] = 0.0; sr[p][v] = 0.0; }
    }

    for (int64_t c0 = row_lo; c0 <= row_hi; c0 += STEP_ROWS) {
        const int rows = (int)(row_hi - c0 + 1 < STEP_ROWS ? row_hi - c0 + 1 : STEP_ROWS);
        __syncthreads();                                         // the stage's previous rows have been used by every wave
        for (int e = threadIdx.x; e < rows * 64 * (NV + 1); e += STEP_WAVES * 64) {
            const int r = e / (64 * (NV + 1)), q = e % (64 * (NV + 1)), sn = q / (NV + 1), c = q % (NV + 1);
            const int64_t sg = (int64_t)blockIdx.y * 64 + sn;
            stage[r][c][sn] = sg < s ? rec[(c0 + r) * row_step + sg * cols + c] : 0.0;       // (a series past s: flag 0)
        }
        __syncthreads();
        // this wave's outputs f0 .. f0 + P - 1 reach rows [f0 - w, f0 + P - 1 + w)
        const int r_a = (int)(f0 - w - c0 > 0 ? f0 - w - c0 : 0);
        const int r_b = (int)(f0 + P - 1 + w - 1 - c0 < rows - 1 ? f0 + P - 1 + w - 1 - c0 : rows - 1);
        for (int r = r_a; r <= r_b; ++r) {
            const bool valid = stage[r][0][lane] != 0.0;
            double x[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = stage[r][1 + v][lane];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int d = (int)(c0 + r - f0) - p;            // g - f, wave-uniform
                if (d < -w || d >= w) continue;
                if (valid) {                                     // selected out, never multiplied by zero
                    if (d < 0) {
                        ++cl[p];
#pragma unroll
                        for (int v = 0; v < NV; ++v) sl[p][v] = sl[p][v] + x[v];
                    } else {
                        ++cr[p];
#pragma unroll
                        for (int v = 0; v < NV; ++v) sr[p][v] = sr[p][v] + x[v];
                    }
                }
            }
        }
    }

    if (series >= s) return;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int64_t f = f0 + p;
        if (f >= tile1) break;
        double* o = out + (f * s + series) * (2 + NV);
        const bool ok = cl[p] >= min_count && cr[p] >= min_count;
        double r[NV], score = 0.0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            r[v] = 0.0;
            if (ok) {
                r[v] = sr[p][v] / (double)cr[p] - sl[p][v] / (double)cl[p];
                score = score + r[v] * r[v];
            }
        }
        o[0] = ok ? 1.0 : 0.0;
        o[1] = score;
#pragma unroll
        for (int v = 0; v < NV; ++v) o[2 + v] = r[v];
    }
}

void launch_step_response(const double* rec, int n, int s, int cols, int n_values, int w, int min_count, double* out,
                          hipStream_t st) {
    const dim3 block(STEP_WAVES * 64);
#define STEP_CASE(NV)                                                                                                         \
    case NV: {                                                                                                                \
        constexpr int TILE = STEP_WAVES * StepP<NV>::value;                                                                   \
        const dim3 grid((unsigned)(((int64_t)n + TILE - 1) / TILE), (unsigned)((s + 63) / 64));                               \
        hipLaunchKernelGGL(k_step_response<NV>, grid, block, 0, st, rec, n, s, cols, w, min_count, out);                      \
    } break
    switch (n_values) {
        STEP_CASE(1); STEP_CASE(2); STEP_CASE(3); STEP_CASE(4); STEP_CASE(5); STEP_CASE(6); STEP_CASE(7);
    }
#undef STEP_CASE
}

// steps [s][1 + max_steps]: the count, the first min(count, max_steps) step frames in ascending order, then -1
__global__ __launch_bounds__(STEP_WAVES * 64) void k_find_steps(const double* __restrict__ resp, int n, int s, int resp_cols,
                                                                int w, double thr2, int max_steps, int32_t* __restrict__ steps) {
    __shared__ double stage[FIND_ROWS][64];
    __shared__ u8 marks[STEP_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t series = (int64_t)blockIdx.x * 64 + lane;
    const int64_t row_step = (int64_t)s * resp_cols;
    const double nan = __builtin_nan("");
    int count = 0;                                               // of this lane's series so far (wave 0 alone keeps it)

    for (int64_t tile0 = 0; tile0 < n; tile0 += FIND_TILE) {
        const int64_t tile1 = tile0 + FIND_TILE < n ? tile0 + FIND_TILE : n;
        const int64_t f0 = tile0 + wave * FIND_P;
        const int64_t row_lo = tile0 - w > 0 ? tile0 - w : 0;
        const int64_t row_hi = tile1 - 1 + w < n - 1 ? tile1 - 1 + w : n - 1;
        double own[FIND_P];
        bool alive[FIND_P];
        bool any = false;
#pragma unroll
        for (int p = 0; p < FIND_P; ++p) {
            const int64_t f = f0 + p;
            own[p] = nan;
            if (f < tile1 && series < s) {
                const double* in = resp + f * row_step + series * resp_cols;
                const double flag = in[0], score = in[1];        // both loads at once: neither waits for the other
                if (flag != 0.0) own[p] = score;
            }
            alive[p] = own[p] >= thr2;                           // false for NaN
            any = any || alive[p];
        }
        const bool wave_any = __builtin_amdgcn_readfirstlane(__any(any) ? 1 : 0) != 0;
        // no candidate in the whole tile: nothing to stage, nothing to append (and every wave has passed wave 0's last append)
        if (!__syncthreads_or(wave_any ? 1 : 0)) continue;

        for (int64_t c0 = row_lo; c0 <= row_hi; c0 += FIND_ROWS) {
            const int rows = (int)(row_hi - c0 + 1 < FIND_ROWS ? row_hi - c0 + 1 : FIND_ROWS);
            __syncthreads();                                     // the previous rows have been used by every wave
#pragma unroll 4
            for (int e = threadIdx.x; e < rows * 64; e += STEP_WAVES * 64) {
                const int r = e >> 6, sn = e & 63;
                const int64_t sg = (int64_t)blockIdx.x * 64 + sn;
                double x = nan;                                  // a series past s, a row that is not ok
                if (sg < s) {
                    const double* in = resp + (c0 + r) * row_step + sg * resp_cols;
                    const double flag = in[0], score = in[1];
                    if (flag != 0.0) x = score;
                }
                stage[r][sn] = x;
            }
            __syncthreads();
            if (!wave_any) continue;                             // wave-uniform: no candidate among this wave's 64 x P outputs
            // this wave's candidates f0 .. f0 + FIND_P - 1 reach rows [f0 - w, f0 + FIND_P - 1 + w]
            const int r_a = (int)(f0 - w - c0 > 0 ? f0 - w - c0 : 0);
            const int r_b = (int)(f0 + FIND_P - 1 + w - c0 < rows - 1 ? f0 + FIND_P - 1 + w - c0 : rows - 1);
            for (int r = r_a; r <= r_b; ++r) {
                const double x = stage[r][lane];
#pragma unroll
                for (int p = 0; p < FIND_P; ++p) {
                    const int d = (int)(c0 + r - f0) - p;        // g - f, wave-uniform
                    if (d < -w || d > w || d == 0) continue;
                    // an earlier frame wins a tie, a later one does not; NaN on either side compares false
                    if (d < 0 ? x >= own[p] : x > own[p]) alive[p] = false;
                }
            }
        }

        unsigned m = 0;
#pragma unroll
        for (int p = 0; p < FIND_P; ++p) m |= alive[p] ? 1u << p : 0u;
        marks[wave][lane] = (u8)m;
        __syncthreads();
        if (wave == 0 && series < s) {
            int32_t* row = steps + series * (1 + (int64_t)max_steps);
            for (int k = 0; k < STEP_WAVES; ++k) {
                unsigned bits = marks[k][lane];
                while (bits) {
                    const int p = __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (count < max_steps) row[1 + count] = (int32_t)(tile0 + k * FIND_P + p);
                    ++count;
                }
            }
        }
    }
    if (wave == 0 && series < s) {
        int32_t* row = steps + series * (1 + (int64_t)max_steps);
        row[0] = count;
        for (int k = count; k < max_steps; ++k) row[1 + k] = -1;
    }
}

void launch_find_steps(const double* resp, int n, int s, int resp_cols, int w, double thr2, int max_steps, int32_t* steps,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_find_steps, dim3((unsigned)((s + 63) / 64)), dim3(STEP_WAVES * 64), 0, st, resp, n, s, resp_cols, w, thr2,
                       max_steps, steps);
}

// out [s][max_steps + 1][3 + 2 NV] = begin, end, count, mean[NV], M2[NV].  Whatever `steps` holds, begin and end are clipped to
// [0, n] before a frame is read.
template <int NV>
__global__ __launch_bounds__(64) void k_dwell_stats(const double* __restrict__ rec, int n, int s, int cols,
                                                    const int32_t* __restrict__ steps, int steps_rows, int max_steps, int guard,
                                                    double* __restrict__ out) {
    const int lane = threadIdx.x;
    const int64_t series = blockIdx.x;
    const int j = blockIdx.y;
    const int32_t* row = steps + (steps_rows == 1 ? 0 : series) * (1 + (int64_t)max_steps);
    double* o = out + (series * (max_steps + 1) + j) * (3 + 2 * NV);
    const double nan = __builtin_nan("");
    int k = row[0];
    k = k < 0 ? 0 : (k > max_steps ? max_steps : k);
    if (j > k) {
        if (lane == 0) {
            o[0] = -1.0; o[1] = -1.0; o[2] = 0.0;
#pragma unroll
            for (int v = 0; v < 2 * NV; ++v) o[3 + v] = nan;
        }
        return;
    }
    int64_t begin = j == 0 ? 0 : (int64_t)row[j] + guard;        // row[j] = c_{j-1}
    int64_t end = j == k ? n : (int64_t)row[1 + j] - guard;
    begin = begin < 0 ? 0 : (begin > n ? n : begin);
    end = end < 0 ? 0 : (end > n ? n : end);
    end = end > begin ? end : begin;
    const int64_t row_step = (int64_t)s * cols;
    const double* base = rec + series * cols;

    double sum[NV];
    int cnt = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) sum[v] = 0.0;
    for (int64_t f = begin + lane; f < end; f += 64) {
        const double* in = base + f * row_step;
        if (in[0] != 0.0) {                                      // selected out, never multiplied by zero
            ++cnt;
#pragma unroll
            for (int v = 0; v < NV; ++v) sum[v] = sum[v] + in[1 + v];
        }
    }
    cnt = wave_sum(cnt);
    double mean[NV], m2[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double t = wave_sum(sum[v]);
        mean[v] = cnt > 0 ? t / (double)cnt : nan;
        m2[v] = 0.0;
    }
    for (int64_t f = begin + lane; f < end; f += 64) {
        const double* in = base + f * row_step;
        if (in[0] != 0.0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const double d = in[1 + v] - mean[v];
                m2[v] = m2[v] + d * d;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) m2[v] = wave_sum(m2[v]);
    if (lane == 0) {
        o[0] = (double)begin; o[1] = (double)end; o[2] = (double)cnt;
#pragma unroll
        for (int v = 0; v < NV; ++v) { o[3 + v] = mean[v]; o[3 + NV + v] = m2[v]; }
    }
}

void launch_dwell_stats(const double* rec, int n, int s, int cols, int n_values, const int32_t* steps, int steps_rows,
                        int max_steps, int guard, double* out, hipStream_t st) {
    const dim3 grid((unsigned)s, (unsigned)(max_steps + 1));
#define DWELL_CASE(NV)                                                                                                        \
    case NV: hipLaunchKernelGGL(k_dwell_stats<NV>, grid, dim3(64), 0, st, rec, n, s, cols, steps, steps_rows, max_steps, guard, out); break
    switch (n_values) {
        DWELL_CASE(1); DWELL_CASE(2); DWELL_CASE(3); DWELL_CASE(4); DWELL_CASE(5); DWELL_CASE(6); DWELL_CASE(7);
    }
#undef DWELL_CASE
}
