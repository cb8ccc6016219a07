// Marker velocity, acceleration and gap filling along a recording: the moments of a gap-aware weighted local
// polynomial fit (Savitzky-Golay with the gaps selected out) for every frame and series, and the fit of every window with its
// fallback in degree.  Float64, no atomics; a result depends on its inputs only.
//   k_poly_moments<D>  a banded (Toeplitz) product on the float64 matrix instruction (mfma_f64.h states its lane map) in a shape
//            of its own: SEVERAL bands over ONE staged operand.  The 2D + 1 tap rows
//            t_k[delta] = w[delta] u^k (u = delta / H, H a power of two, u^k exact, so one rounding a tap) each make their own A
//            fragment, A_k[r][j] = t_k[j - r - h] inside the band and 0.0 outside, read from a zero-padded copy of the row in LDS
//            (`wp`) as k_window_moments reads its one row.  B, staged ONCE per (input frame, slot) and chunk, is the SELECTED
//            terms of KIN_SLOTS = 16 slots in 9 tiles of 16 columns:
//              tiles 0-3  (valid, x1, x2, x3) of 4 slots each, k_project's tile:   x A_0 .. A_D      -> S_k, X_k   (k <= D)
//              tiles 4-7  (0, x1 x1, x2 x2, x3 x3) of 4 slots each:               x A_0             -> XX
//              tile  8    the flags of all 16 slots:                              x A_(D+1) .. A_2D -> S_k        (k > D)
//            so a step of 4 input frames costs 4 (D + 1) + 4 + D products for 16 slots, each into its own accumulator
//            (23 at D = 3; carrying the orders k > D on the idle column of tiles 4-7 instead would cost 4 (D + 1) + 4 + 4 D = 32).
//            A workgroup owns VBS_KIN_TILE output frames (one 16-frame tile a wave), aligned to multiples of VBS_KIN_TILE of the
//            GLOBAL frame index whatever the range asked for, x 16 slots: a frame meets the same instructions in the same order
//            in every range, on every n and among any s.  Wave w multiplies the input frames f0 - h .. f0 + 15 + h of its tile, 4
//            a step.  An invalid entry, a frame outside [0, n), a slot >= s and a value beyond n_values is the constant 0.0,
//            selected by its flag BEFORE anything is computed from it and never multiplied by zero; a frame outside [0, n) fetches
//            frame 0 or n - 1 instead, a slot past the end the last one; nothing past n or s or beyond n_values is read.  The
//            staged rows walk the workgroup's input frames in chunks of KIN_CHUNK, double-buffered: the next chunk's entries are
//            fetched before this chunk's products and stored after them, one barrier a chunk.  A product outside the band is
//            0.0 * (a finite staged term) = 0.0 exactly.
//            LDS: a B fragment is 64 consecutive doubles (4 rows x 16 columns), an A fragment 19 consecutive doubles read with
//            repeats, both free of bank conflicts; the staging writes of a wave fall on 4 of the 16 double-wide write banks, which
//            costs about 150 cycles a chunk beside the chunk's 4 x 23 products.
//   k_poly_fit<D>  one thread per (frame, slot), no barrier, nothing shared; every expression is the one include/vbs.h states,
//            without contraction.
#include "common.h"
#include "mfma_f64.h"
#include <type_traits>
#pragma clang fp contract(off)

#define KIN_WAVES   (VBS_KIN_TILE / 16)              // one 16-frame tile a wave
#define KIN_THREADS (KIN_WAVES * 64)
#define KIN_SLOTS   16                               // slots of a workgroup
#define KIN_TILES   9                                // staged tiles: 4 of values, 4 of squares, 1 of flags
#define KIN_CHUNK   16                               // input frames staged at a time
#define KIN_BUF     (KIN_TILES * KIN_CHUNK * 16)     // doubles of one staged chunk
#define KIN_ROWS    (2 * VBS_KIN_MAX_DEGREE + 1)     // tap rows at most
static_assert(VBS_KIN_TILE % 16 == 0 && KIN_WAVES >= 1 && KIN_THREADS <= 1024, "a workgroup is a whole number of 16-frame tiles");
static_assert(KIN_THREADS == KIN_CHUNK * KIN_SLOTS, "a thread stages one (input frame, slot) a chunk");
static_assert(KIN_CHUNK % 16 == 0, "a wave's steps never straddle a chunk");
static_assert(KIN_WAVES * 32 == VBS_HALF_TAPS, "the weights travel 32 a wave");
static_assert((2 * KIN_BUF + KIN_ROWS * BAND_ROW + VBS_HALF_TAPS) * 8 <= 64 * 1024,
              "two staged chunks, the tap rows and the weights fit the LDS a workgroup gets without asking");

struct KinThr { double t[VBS_KIN_MAX_DEGREE + 1]; };

template <int D>
__global__ __launch_bounds__(KIN_THREADS) void k_poly_moments(const double* __restrict__ rec, int n, int s, int cols, int nv,
                                                              HalfTaps taps, int h, double inv_H, int frame_begin, int frame_end,
                                                              int tile_first, double* __restrict__ mom) {
    constexpr int R = 2 * D + 1;                                         // tap rows
    __shared__ __attribute__((aligned(32))) double stage[2 * KIN_BUF];   // [buffer][tile][input row][16]
    __shared__ double wp[R * BAND_ROW];
    __shared__ double wh[VBS_HALF_TAPS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int M = R + (D + 2) * nv;
    const int64_t F0 = ((int64_t)tile_first + blockIdx.x) * VBS_KIN_TILE;  // the first output frame of this workgroup, global
    const int S0 = (int)blockIdx.y * KIN_SLOTS;
    const int steps = (2 * h + 16 + 3) >> 2;                             // steps of 4 input frames a wave takes
    const int rows = 16 * (KIN_WAVES - 1) + 4 * steps;                   // input rows of the workgroup: row p is frame F0 - h + p
    const int chunks = (rows + KIN_CHUNK - 1) / KIN_CHUNK;

    // the weights: wave w holds half[32 w + lane] (uniform loads, one select a lane)
    {
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const double t = taps.half[wave * 32 + k];
            mine = lane == k ? t : mine;
        }
        if (lane < 32) wh[wave * 32 + lane] = mine;
    }
    __syncthreads();
    // the padded tap rows: wp[k][BAND_PAD + h + d] = w[|d|] * u^k, u = d / H, |d| <= h; 0.0 elsewhere.  u^k by repeated
    // multiplication, every product exact (|d|^k < 2^42), so the tap is rounded once
    for (int i = tid; i < R * BAND_ROW; i += KIN_THREADS) {
        const int k = i / BAND_ROW;
        const int d = i - k * BAND_ROW - BAND_PAD - h;
        double t = 0.0;
        if (d >= -h && d <= h) {
            const double u = (double)d * inv_H;
            double p = 1.0;
            for (int j = 0; j < k; ++j) p = p * u;
            t = wh[d < 0 ? -d : d] * p;
        }
        wp[i] = t;
    }

    // this thread's (input row, slot) of a chunk
    const int prow = tid >> 4, sl = tid & 15;
    const bool slot_live = S0 + sl < s;
    const int sc = slot_live ? S0 + sl : s - 1;
    const double* col = rec + (int64_t)sc * cols;
    const int64_t row_step = (int64_t)s * cols;
    const int c2 = nv >= 2 ? 2 : 1, c3 = nv >= 3 ? 3 : 1;               // (the first value again where there is no such value)

    // the entry of chunk `ch` this thread stages.  No branch: a frame outside [0, n) fetches frame 0 or n - 1 instead
    auto gather = [&](int ch, double (&v)[4]) {
        const int64_t f = F0 - h + ch * KIN_CHUNK + prow;
        const int64_t fc = f < 0 ? 0 : f < n ? f : n - 1;
        const double* e = col + fc * row_step;
        v[0] = e[0]; v[1] = e[1]; v[2] = e[c2]; v[3] = e[c3];
    };
    // ... SELECTED by the flag before anything is computed from it: the value of an invalid entry never enters an operation
    auto store = [&](int ch, double* buf, const double (&v)[4]) {
        const int64_t f = F0 - h + ch * KIN_CHUNK + prow;
        const bool valid = slot_live & (f >= 0) & (f < n) & (v[0] != 0.0);       // (& not &&: selects, no control flow)
        const double x1 = valid ? v[1] : 0.0;
        const double x2 = (valid & (nv >= 2)) ? v[2] : 0.0;
        const double x3 = (valid & (nv >= 3)) ? v[3] : 0.0;
        double* pv = buf + (((sl >> 2) * KIN_CHUNK + prow) * 16 + (sl & 3) * 4);
        double* ps = pv + 4 * KIN_CHUNK * 16;
        pv[0] = valid ? 1.0 : 0.0; pv[1] = x1; pv[2] = x2; pv[3] = x3;
        ps[0] = 0.0; ps[1] = x1 * x1; ps[2] = x2 * x2; ps[3] = x3 * x3;
        buf[(8 * KIN_CHUNK + prow) * 16 + sl] = valid ? 1.0 : 0.0;
    };

    const int64_t f0 = F0 + 16 * wave;                                   // this wave's first output frame
    const bool live = f0 < frame_end && f0 + 16 > frame_begin;           // it emits something (it stages and waits either way)
    const int w_lo = 16 * wave, w_hi = 16 * wave + 4 * steps;            // its input rows, of the workgroup's

    f64x4 accv[4][D + 1], accs[4], accf[D > 0 ? D : 1];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        accs[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k <= D; ++k) accv[t][k] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll
    for (int k = 0; k < (D > 0 ? D : 1); ++k) accf[k] = f64x4{0.0, 0.0, 0.0, 0.0};

    double v[4];
    gather(0, v);
    store(0, stage, v);
    __syncthreads();
    for (int ch = 0; ch < chunks; ++ch) {
        const bool more = ch + 1 < chunks;
        if (more) gather(ch + 1, v);
        if (live) {
            const double* buf = stage + (ch & 1) * KIN_BUF;
            const int lo = w_lo > ch * KIN_CHUNK ? w_lo : ch * KIN_CHUNK;
            const int hi = w_hi < (ch + 1) * KIN_CHUNK ? w_hi : (ch + 1) * KIN_CHUNK;
            for (int p = lo; p < hi; p += 4) {
                const int ai = p - w_lo + q - r + BAND_PAD;              // A_k[r][j], j = p - w_lo + q
                double av[R];
#pragma unroll
                for (int k = 0; k < R; ++k) av[k] = wp[k * BAND_ROW + ai];
                const int lrow = p - ch * KIN_CHUNK + q;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double b = buf[(t * KIN_CHUNK + lrow) * 16 + r];
#pragma unroll
                    for (int k = 0; k <= D; ++k) accv[t][k] = mfma_f64(av[k], b, accv[t][k]);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double b = buf[((4 + t) * KIN_CHUNK + lrow) * 16 + r];
                    accs[t] = mfma_f64(av[0], b, accs[t]);
                }
                if constexpr (D > 0) {
                    const double b = buf[(8 * KIN_CHUNK + lrow) * 16 + r];
#pragma unroll
                    for (int k = 0; k < D; ++k) accf[k] = mfma_f64(av[D + 1 + k], b, accf[k]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                               // the staging waits for its entry AFTER the products
        if (more) store(ch + 1, stage + ((ch + 1) & 1) * KIN_BUF, v);
        __syncthreads();
    }
    if (!live) return;

    // the scatter into mom [F, s, M]: S_0 .. S_2D, then X_0 .. X_D, XX per value
    const int comp = r & 3;                                              // of tiles 0-7: 0 the flag, 1..3 the values
    const int vcol = R + (comp - 1) * (D + 2);                           // where this value's sums begin
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int64_t f = f0 + q + 4 * g;
        if (f < frame_begin || f >= frame_end) continue;
        double* row = mom + (f - frame_begin) * (int64_t)s * M;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int slot = S0 + 4 * t + (r >> 2);
            if (slot >= s || comp > nv) continue;
            double* o = row + (int64_t)slot * M;
#pragma unroll
            for (int k = 0; k <= D; ++k) o[comp == 0 ? k : vcol + k] = accv[t][k][g];
            if (comp > 0) o[vcol + D + 1] = accs[t][g];
        }
        if constexpr (D > 0) {
            const int slot = S0 + r;
            if (slot < s) {
                double* o = row + (int64_t)slot * M;
#pragma unroll
                for (int k = 0; k < D; ++k) o[D + 1 + k] = accf[k][g];
            }
        }
    }
}

// the smallest power of two >= max(h, 1): u = delta / H is an exact scaling
static int kin_scale(int h) {
    int H = 1;
    while (H < h) H *= 2;
    return H;
}

// launch(D) with the degree as a constant: the kernels are compiled per degree
template <class Launch> static void kin_by_degree(int degree, Launch launch) {
    switch (degree) {
        case 0: launch(std::integral_constant<int, 0>{}); break;
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        default: launch(std::integral_constant<int, 3>{}); break;
    }
}

void launch_poly_moments(const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half, int degree,
                         int frame_begin, int frame_end, double* mom, hipStream_t st) {
    const int h = n_half - 1;
    const double inv_H = 1.0 / (double)kin_scale(h);
    int first;
    const dim3 grid((unsigned)band_tiles(frame_begin, frame_end, VBS_KIN_TILE, &first), (unsigned)((s + KIN_SLOTS - 1) / KIN_SLOTS));
    kin_by_degree(degree, [&](auto D) {
        hipLaunchKernelGGL(k_poly_moments<decltype(D)::value>, grid, dim3(KIN_THREADS), 0, st, rec, n, s, cols, n_values,
                           half_taps_arg(half, n_half), h, inv_H, frame_begin, frame_end, first, mom);
    });
}

template <int D>
__global__ __launch_bounds__(256) void k_poly_fit(const double* __restrict__ mom, const double* __restrict__ rec, int s, int cols,
                                                  int nv, int frame_begin, int64_t count, KinThr thr, double inv_H, int fill_degree,
                                                  double* __restrict__ fit, double* __restrict__ filled) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;           // (frame - frame_begin, slot), flattened
    if (i >= count) return;
    constexpr int R = 2 * D + 1;
    const int M = R + (D + 2) * nv, fc = 2 + (D + 2) * nv;
    const double* P = mom + i * M;
    double* o = fit + i * fc;
    double S[R];
#pragma unroll
    for (int k = 0; k < R; ++k) S[k] = P[k];
    // G[a][b] = S[a + b] = L diag(Dv) L^T, column by column; V[i][j] = L[i][j] Dv[j]
    double Lm[D + 1][D + 1], V[D + 1][D + 1], Dv[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) {
        double t = S[2 * j];
#pragma unroll
        for (int m = 0; m < j; ++m) t = t - V[j][m] * Lm[j][m];
        Dv[j] = t;
#pragma unroll
        for (int a = j + 1; a <= D; ++a) {
            double w = S[a + j];
#pragma unroll
            for (int m = 0; m < j; ++m) w = w - V[a][m] * Lm[j][m];
            V[a][j] = w;
            Lm[a][j] = w / t;
        }
    }
    int q = -1;
    bool ok = true;
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        ok = ok && Dv[k] > thr.t[k];
        q = ok ? k : q;
    }
    const double* e = rec + (i + (int64_t)frame_begin * s) * cols;
    const bool valid = e[0] != 0.0;
    o[0] = (valid ? 1.0 : 0.0) + (q >= 0 ? 2.0 : 0.0) + (q == D ? 4.0 : 0.0);
    o[1] = (double)q;
    const double inv_H2 = inv_H * inv_H, inv_H3 = inv_H2 * inv_H;
    double y0s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (v >= nv) continue;
        const double* X = P + R + v * (D + 2);
        double z[D + 1], g[D + 1], c[D + 1];
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            double t = X[k];
#pragma unroll
            for (int m = 0; m < k; ++m) t = t - Lm[k][m] * z[m];
            z[k] = t;
            g[k] = t / Dv[k];
        }
#pragma unroll
        for (int k = D; k >= 0; --k) {
            double t = 0.0;
            if (k <= q) {
                t = g[k];
#pragma unroll
                for (int m = k + 1; m <= D; ++m)
                    if (m <= q) t = t - Lm[m][k] * c[m];
            }
            c[k] = t;
        }
        double rss = X[D + 1];
#pragma unroll
        for (int k = 0; k <= D; ++k)
            if (k <= q) rss = rss - z[k] * g[k];
        double* ov = o + 2 + v * (D + 2);
        ov[0] = c[0];
        if constexpr (D >= 1) ov[1] = c[1] * inv_H;
        if constexpr (D >= 2) ov[2] = (2.0 * c[2]) * inv_H2;
        if constexpr (D >= 3) ov[3] = (6.0 * c[3]) * inv_H3;
        ov[D + 1] = rss;
        y0s[v] = c[0];
    }
    if (filled) {
        double* fo = filled + i * cols;
        if (valid) {
            for (int k = 0; k < cols; ++k) fo[k] = e[k];
        } else {
            const bool fill = q >= fill_degree;
            fo[0] = fill ? 2.0 : 0.0;
            for (int k = 1; k < cols; ++k) fo[k] = 0.0;
#pragma unroll
            for (int v = 0; v < 3; ++v)
                if (v < nv) fo[1 + v] = fill ? y0s[v] : 0.0;
        }
    }
}

// thr [degree + 1] HOST, checked by the caller; rec [n, s, cols], mom and fit (and filled) the frames [frame_begin, frame_end)
void launch_poly_fit(const double* mom, const double* rec, int s, int cols, int n_values, int degree, int half_window,
                     const double* thr, int fill_degree, int frame_begin, int frame_end, double* fit, double* filled,
                     hipStream_t st) {
    KinThr t{};
    for (int k = 0; k <= degree; ++k) t.t[k] = thr[k];
    const double inv_H = 1.0 / (double)kin_scale(half_window);
    const int64_t count = (int64_t)(frame_end - frame_begin) * s;
    const dim3 grid((unsigned)((count + 255) / 256));
    kin_by_degree(degree, [&](auto D) {
        hipLaunchKernelGGL(k_poly_fit<decltype(D)::value>, grid, dim3(256), 0, st, mom, rec, s, cols, n_values, frame_begin, count,
                           t, inv_H, fill_degree, fit, filled);
    });
}
