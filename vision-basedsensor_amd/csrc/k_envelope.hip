// Time-resolved amplitude and phase along a recording: the weighted sums of a sliding window at one known frequency
// for every frame and series, and the floating-mean fit of those sums.  Float64, no atomics; a result depends on its inputs only.
//   k_window_moments  a banded (Toeplitz) product [16 output frames x K input frames] . [K x 16 columns] on the float64 matrix
//            instruction (mfma_f64.h states its lane map).  The columns are the FLATTENED axis
//            i * M + m of the output (slot i, sum m of M = 5 + 4 n_values), so a tile row is 16 contiguous doubles of `mom` and a
//            tile may straddle slots.  A workgroup owns VBS_ENV_TILE output frames (one 16-frame tile a wave), aligned to multiples
//            of VBS_ENV_TILE of the GLOBAL frame index whatever the range asked for, x ENV_CT column tiles: a frame meets the same
//            instructions in the same order in every range, on every n and among any s.  Wave w multiplies the input frames
//            f0 - h .. f0 + 15 + h of its tile (f0 = tile frame 16 w), 4 a step, one A fragment feeding ENV_CT products.
//            A[r][k] = w[k - r - h] inside the band, else 0.0: the same for every tile, read from a zero-padded copy of the taps in
//            LDS (`wp`).  B = the SELECTED terms phi_m(j) of the workgroup's columns, each computed once per (input frame, column)
//            when it is staged: 1, c, s, c2, s2, then x, x c, x s, x x per value, products rounded (no contraction); an invalid
//            entry, a frame outside [0, n) and a column >= s M is the constant 0.0, selected by its flag and never multiplied by
//            zero; nothing past n or s or beyond n_values is read.  The staged rows walk the workgroup's input frames in chunks of
//            ENV_CHUNK, double-buffered as k_project's: the next chunk's entries are fetched before this chunk's products and
//            stored after them, one barrier a chunk.  A product outside the band is 0.0 * (a finite staged term) = 0.0 exactly.
//   k_window_fit  one thread per (frame, slot), no barrier, nothing shared; every expression is the one include/vbs.h states,
//            without contraction.
#include "common.h"
#include "mfma_f64.h"
#pragma clang fp contract(off)

#define ENV_WAVES   (VBS_ENV_TILE / 16)              // one 16-frame tile a wave
#define ENV_THREADS (ENV_WAVES * 64)
#define ENV_CT      4                                // column tiles of a workgroup
#define ENV_COLS    (ENV_CT * 16)                    // flattened columns of a workgroup
#define ENV_CHUNK   32                               // input frames staged at a time
#define ENV_BUF     (ENV_CHUNK * ENV_COLS)           // doubles of one staged chunk
#define ENV_ENTRIES (ENV_BUF / ENV_THREADS)          // entries a thread stages per chunk
static_assert(VBS_ENV_TILE % 16 == 0 && ENV_WAVES >= 1 && ENV_THREADS <= 1024, "a workgroup is a whole number of 16-frame tiles");
static_assert(ENV_COLS == 64, "a thread stages one column: its lane");
static_assert(ENV_CHUNK % 16 == 0 && ENV_BUF % ENV_THREADS == 0, "a wave's steps never straddle a chunk; equal staging shares");
static_assert(ENV_WAVES * 32 == VBS_HALF_TAPS, "the taps travel 32 a wave");
static_assert((2 * ENV_BUF + BAND_ROW) * 8 <= 64 * 1024, "two staged chunks and the taps fit the LDS a workgroup gets without asking");

__global__ __launch_bounds__(ENV_THREADS) void k_window_moments(const double* __restrict__ rec, int n, int s, int cols, int nv,
                                                                const double* __restrict__ carrier, HalfTaps taps, int h,
                                                                int frame_begin, int frame_end, int tile_first,
                                                                double* __restrict__ mom) {
    __shared__ __attribute__((aligned(16))) double stage[2 * ENV_BUF];   // [buffer][column tile][input row][16]
    __shared__ double wp[BAND_ROW];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int M = 5 + 4 * nv;
    const int64_t C = (int64_t)s * M;                                    // the flattened column axis
    const int64_t F0 = ((int64_t)tile_first + blockIdx.x) * VBS_ENV_TILE;  // the first output frame of this workgroup, global
    const int64_t c0 = (int64_t)blockIdx.y * ENV_COLS;
    const int steps = (2 * h + 16 + 3) >> 2;                             // steps of 4 input frames a wave takes
    const int rows = 16 * (ENV_WAVES - 1) + 4 * steps;                   // input rows of the workgroup: row p is frame F0 - h + p
    const int chunks = (rows + ENV_CHUNK - 1) / ENV_CHUNK;

    // the padded taps: wp[BAND_PAD + h + d] = w[d], |d| <= h; 0.0 elsewhere.  Wave w holds half[32 w + lane] (uniform loads, one
    // select a lane) and writes both of its places
    for (int i = tid; i < BAND_ROW; i += ENV_THREADS) {
        const int d = i - BAND_PAD - h;
        if (d < -h || d > h) wp[i] = 0.0;
    }
    {
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const double t = taps.half[wave * 32 + k];
            mine = lane == k ? t : mine;
        }
        const int d = wave * 32 + lane;
        if (lane < 32 && d <= h) { wp[BAND_PAD + h + d] = mine; wp[BAND_PAD + h - d] = mine; }
    }

    // this thread's column of the workgroup: slot, sum, and what its term is made of.  kind 0: 1; 1: the carrier row `crow`;
    // 2: x; 3: x * carrier row `crow`; 4: x * x
    const int64_t cg = c0 + lane;
    const bool col_live = cg < C;
    const int slot = (int)((col_live ? cg : C - 1) / M);
    const int m = (int)((col_live ? cg : C - 1) - (int64_t)slot * M);
    const int t4 = (m - 5) & 3;
    const int kind = m == 0 ? 0 : m < 5 ? 1 : t4 == 0 ? 2 : t4 == 3 ? 4 : 3;
    const int crow = m < 5 ? (m == 0 ? 0 : m - 1) : (t4 == 2 ? 1 : 0);
    const int xcol = m < 5 ? 0 : 1 + ((m - 5) >> 2);                     // (the flag again where no value is needed)
    const double* car = carrier + (int64_t)crow * n;
    const double* col = rec + (int64_t)slot * cols;
    const int64_t row_step = (int64_t)s * cols;
    const int prow = tid >> 6;                                           // this thread stages rows prow, prow + ENV_WAVES, ..

    // the entries of chunk `ch` this thread stages.  No branch: a frame outside [0, n) fetches frame 0 or n - 1 instead
    auto gather = [&](int ch, double (&v)[ENV_ENTRIES][3]) {
#pragma unroll
        for (int j = 0; j < ENV_ENTRIES; ++j) {
            const int64_t f = F0 - h + ch * ENV_CHUNK + prow + j * ENV_WAVES;
            const int64_t fc = f < 0 ? 0 : f < n ? f : n - 1;
            const double* e = col + fc * row_step;
            v[j][0] = e[0]; v[j][1] = e[xcol]; v[j][2] = car[fc];
        }
    };
    // ... SELECTED by the flag when they are staged: the value of an invalid entry never reaches a sum
    auto store = [&](int ch, double* buf, const double (&v)[ENV_ENTRIES][3]) {
#pragma unroll
        for (int j = 0; j < ENV_ENTRIES; ++j) {
            const int lrow = prow + j * ENV_WAVES;
            const int64_t f = F0 - h + ch * ENV_CHUNK + lrow;
            const bool valid = col_live & (f >= 0) & (f < n) & (v[j][0] != 0.0);     // (& not &&: selects, no control flow)
            const double x = v[j][1], cv = v[j][2];
            const double xc = x * cv, xx = x * x;
            const double term = kind == 0 ? 1.0 : kind == 1 ? cv : kind == 2 ? x : kind == 3 ? xc : xx;
            buf[((lane >> 4) * ENV_CHUNK + lrow) * 16 + (lane & 15)] = valid ? term : 0.0;
        }
    };

    const int64_t f0 = F0 + 16 * wave;                                   // this wave's first output frame
    const bool live = f0 < frame_end && f0 + 16 > frame_begin;           // it emits something (it stages and waits either way)
    const int w_lo = 16 * wave, w_hi = 16 * wave + 4 * steps;            // its input rows, of the workgroup's

    f64x4 acc[ENV_CT];
#pragma unroll
    for (int ct = 0; ct < ENV_CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    double v[ENV_ENTRIES][3];
    gather(0, v);
    store(0, stage, v);
    __syncthreads();
    for (int ch = 0; ch < chunks; ++ch) {
        const bool more = ch + 1 < chunks;
        if (more) gather(ch + 1, v);
        if (live) {
            const double* buf = stage + (ch & 1) * ENV_BUF;
            const int lo = w_lo > ch * ENV_CHUNK ? w_lo : ch * ENV_CHUNK;
            const int hi = w_hi < (ch + 1) * ENV_CHUNK ? w_hi : (ch + 1) * ENV_CHUNK;
            for (int p = lo; p < hi; p += 4) {
                const double av = wp[p - w_lo + q - r + BAND_PAD];       // A[r][k], k = p - w_lo + q
                const int lrow = p - ch * ENV_CHUNK + q;
#pragma unroll
                for (int ct = 0; ct < ENV_CT; ++ct) {
                    const double b = buf[(ct * ENV_CHUNK + lrow) * 16 + r];
                    acc[ct] = mfma_f64(av, b, acc[ct]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                               // the staging waits for its entries AFTER the products
        if (more) store(ch + 1, stage + ((ch + 1) & 1) * ENV_BUF, v);
        __syncthreads();
    }
    if (!live) return;

#pragma unroll
    for (int ct = 0; ct < ENV_CT; ++ct) {
        const int64_t oc = c0 + ct * 16 + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t f = f0 + q + 4 * g;
            if (oc < C && f >= frame_begin && f < frame_end) mom[(f - frame_begin) * C + oc] = acc[ct][g];
        }
    }
}

void launch_window_moments(const double* rec, int n, int s, int cols, int n_values, const double* carrier, const double* half,
                           int n_half, int frame_begin, int frame_end, double* mom, hipStream_t st) {
    int first;
    const int64_t C = (int64_t)s * (5 + 4 * n_values);
    const dim3 grid((unsigned)band_tiles(frame_begin, frame_end, VBS_ENV_TILE, &first), (unsigned)((C + ENV_COLS - 1) / ENV_COLS));
    hipLaunchKernelGGL(k_window_moments, grid, dim3(ENV_THREADS), 0, st, rec, n, s, cols, n_values, carrier,
                       half_taps_arg(half, n_half), n_half - 1, frame_begin, frame_end, first, mom);
}

__global__ __launch_bounds__(256) void k_window_fit(const double* __restrict__ mom, int64_t count, int nv, double need,
                                                    double det_min, double* __restrict__ fit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;           // (frame, slot), flattened
    if (i >= count) return;
    const int M = 5 + 4 * nv, fc = 1 + 5 * nv;
    const double* P = mom + i * M;
    double* o = fit + i * fc;
    const double W = P[0], C1 = P[1], S1 = P[2], C2 = P[3], S2 = P[4];
    const double CC = 0.5 * (W + C2) - (C1 * C1) / W;
    const double SS = 0.5 * (W - C2) - (S1 * S1) / W;
    const double CS = 0.5 * S2 - (C1 * S1) / W;
    const double det = CC * SS - CS * CS;
    const bool ok = W > 0.0 && W >= need && det > det_min * (W * W);
    o[0] = ok ? 1.0 : 0.0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (v >= nv) continue;
        double a = 0.0, b = 0.0, p = 0.0, c = 0.0, m2 = 0.0;
        if (ok) {
            const double X = P[5 + 4 * v], XC = P[6 + 4 * v], XS = P[7 + 4 * v], XX = P[8 + 4 * v];
            const double m = X / W;
            const double pc = XC - m * C1;
            const double ps = XS - m * S1;
            a = (pc * SS - ps * CS) / det;
            b = (ps * CC - pc * CS) / det;
            p = a * pc + b * ps;
            c = m - (a * C1 + b * S1) / W;
            m2 = XX - m * X;
        }
        o[1 + 5 * v] = a; o[2 + 5 * v] = b; o[3 + 5 * v] = p; o[4 + 5 * v] = c; o[5 + 5 * v] = m2;
    }
}

// need = min_coverage * sw, one IEEE product on the host
void launch_window_fit(const double* mom, int F, int s, int n_values, double need, double det_min, double* fit, hipStream_t st) {
    const int64_t count = (int64_t)F * s;
    hipLaunchKernelGGL(k_window_fit, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, mom, count, n_values, need, det_min, fit);
}
