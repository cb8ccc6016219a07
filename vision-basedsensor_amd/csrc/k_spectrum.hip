// Displacement spectra along a recording: the gap-aware projection of every series onto a basis the caller gives, and
// the floating-mean harmonic fit of those projections.  Float64, no atomics; a result depends on its inputs only.
//   k_project  [R basis rows x n frames] . [n x 16 columns] by mfma_f64 of mfma_f64.h, the second user of the lane map and of the
//            fragment scheme of k_field_map (k_field.hip), with the LONG axis as K.  The 16 columns of a tile are
//            VBS_PROJ_SLOTS = 4 slots x (x1, x2, x3, flag as 1.0 / 0.0), so the flag column's product IS den.  A workgroup owns
//            VBS_PROJ_ROWS rows x VBS_PROJ_WG_SLOTS slots: wave w takes row tile w against all PROJ_CT column tiles, and keeps its
//            PROJ_CT accumulators in registers across the whole K loop - K is never split across workgroups, every output is one
//            accumulator chain over the chunks in ascending order from frame 0.  A chunk is VBS_PROJ_CHUNK frames of SELECTED
//            values in LDS (an invalid entry, a column beyond n_values, a slot >= s or a frame >= n is the constant 0.0: selected
//            by its flag, never multiplied by zero; nothing past n, R or s is read), double-buffered: the next chunk's entries
//            and the next chunk's A fragment are fetched into registers before this chunk's products, the entries selected and
//            stored after them, one barrier a chunk.
//            K is taken 16 frames at a time and PERMUTED inside those 16 exactly as k_field_map permutes slots: lane (row r,
//            quarter q) loads basis[r][k0 + 4q .. 4q + 3], a contiguous 32-byte run, and uses element e in step e, so step e
//            multiplies frames k0 + 4q + e, q = 0..3.  The staged rows are stored in that order (frame k0 + 4q + e at row
//            k0 + 4e + q) and column tile by column tile ([tile][row][16]): a step reads 64 consecutive doubles of LDS.
//            The order of summation is not part of the interface (include/vbs.h); every output meets the same order.
//   k_harmonic_fit  one wave per slot, VBS_FIT_GROUP slots (waves) a workgroup, no barrier, nothing shared.  Lane l takes bins l,
//            l + 64, .. ascending; every expression is the one include/vbs.h states, without contraction; the peak folds 32, 16,
//            8, 4, 2, 1 with the tie rule of k_patch_stats.
#include "common.h"
#include "mfma_f64.h"
#include <type_traits>
#pragma clang fp contract(off)

#define PROJ_WAVES   (VBS_PROJ_ROWS / 16)            // one row tile a wave
#define PROJ_THREADS (PROJ_WAVES * 64)
#define PROJ_CT      (VBS_PROJ_WG_SLOTS / VBS_PROJ_SLOTS)   // column tiles of a workgroup
#define PROJ_COLS    (VBS_PROJ_SLOTS * 4)            // columns of a tile
#define PROJ_BUF     (VBS_PROJ_CHUNK * PROJ_CT * PROJ_COLS) // doubles of one staged chunk
#define PROJ_ENTRIES (VBS_PROJ_CHUNK * VBS_PROJ_WG_SLOTS / PROJ_THREADS)   // (frame, slot) entries a thread stages per chunk
#define PROJ_KB      (VBS_PROJ_CHUNK / 16)           // blocks of 16 frames in a chunk
static_assert(PROJ_COLS == 16, "a tile is 16 columns: 4 slots x (3 values, flag)");
static_assert(VBS_PROJ_CHUNK % 16 == 0 && VBS_PROJ_ROWS % 16 == 0 && VBS_PROJ_WG_SLOTS % VBS_PROJ_SLOTS == 0, "tile multiples");
static_assert(VBS_PROJ_WG_SLOTS == 16, "the staging index splits an entry into (frame, slot of 16)");
static_assert((VBS_PROJ_CHUNK * VBS_PROJ_WG_SLOTS) % PROJ_THREADS == 0, "every thread stages the same number of entries");
static_assert(2 * PROJ_BUF * 8 <= 64 * 1024, "two staged chunks fit the LDS a workgroup gets without asking");
static_assert(PROJ_THREADS <= 1024, "a workgroup");

__global__ __launch_bounds__(PROJ_THREADS) void k_project(const double* __restrict__ rec, int n, int s, int cols, int nv,
                                                          const double* __restrict__ basis, int R, double* __restrict__ proj) {
    __shared__ __attribute__((aligned(16))) double stage[2 * PROJ_BUF];  // [buffer][column tile][frame row, permuted][16]
    const int row0 = blockIdx.x * VBS_PROJ_ROWS;
    const int s0 = blockIdx.y * VBS_PROJ_WG_SLOTS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;

    // the entries of chunk `f0` this thread stages, fetched as quad_gather says
    auto gather = [&](int f0, double (&v)[PROJ_ENTRIES][4]) { quad_gather<PROJ_THREADS>(rec, n, s, cols, nv, f0, s0, tid, v); };
    // ... SELECTED by the flag when they are staged (after the products that ran while they were in flight): the value of an
    // invalid entry never reaches an operation
    auto store = [&](int f0, double* buf, const double (&v)[PROJ_ENTRIES][4]) {
#pragma unroll
        for (int j = 0; j < PROJ_ENTRIES; ++j) {
            const int i = tid + j * PROJ_THREADS;
            const int sl = i & 15, fr = i >> 4;
            const bool valid = (s0 + sl < s) & (f0 + fr < n) & (v[j][3] != 0.0);     // (& not &&: selects, no control flow)
            const int row = (fr & ~15) | ((fr & 3) << 2) | ((fr >> 2) & 3);
            double* d = buf + ((sl >> 2) * VBS_PROJ_CHUNK + row) * PROJ_COLS + (sl & 3) * 4;
            d[0] = valid ? v[j][0] : 0.0;
            d[1] = (valid & (nv > 1)) ? v[j][1] : 0.0;
            d[2] = (valid & (nv > 2)) ? v[j][2] : 0.0;
            d[3] = valid ? 1.0 : 0.0;
        }
    };

    const int row = row0 + wave * 16 + r;
    const bool prow = row < R;                                           // (a row >= R is selected to 0.0)
    const bool live = row0 + wave * 16 < R;                              // this wave has a row tile (it stages and waits either way)
    const double* br = basis + (int64_t)(prow ? row : R - 1) * n + 4 * q;
    // this lane's A values of chunk `f0`: element kb * 4 + e is frame f0 + 16 kb + 4 q + e
    auto fetch_full = [&](int f0, double (&a)[4 * PROJ_KB]) {
#pragma unroll
        for (int k = 0; k < 4 * PROJ_KB; ++k) a[k] = br[f0 + (k >> 2) * 16 + (k & 3)];
    };
    auto fetch = [&](int f0, double (&a)[4 * PROJ_KB]) {
        if (f0 + VBS_PROJ_CHUNK <= n) fetch_full(f0, a);
        else {                                                           // the last, partial chunk: frames >= n are the constant 0.0
#pragma unroll
            for (int k = 0; k < 4 * PROJ_KB; ++k) {
                const int f = f0 + (k >> 2) * 16 + 4 * q + (k & 3);
                const double w = br[(f < n ? f : n - 1) - 4 * q];        // (the row's last frame instead: never a read past n)
                a[k] = f < n ? w : 0.0;
            }
        }
    };

    f64x4 acc[PROJ_CT];
#pragma unroll
    for (int ct = 0; ct < PROJ_CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    double v[PROJ_ENTRIES][4], a0[4 * PROJ_KB], a1[4 * PROJ_KB];
    // one chunk: the next chunk's entries and A values are asked for, this chunk's products run on `a` and stage buffer `cur`, the
    // next chunk is staged into the other buffer.  STEADY: a complete next chunk is known to exist, so the body has no branch and
    // the fetches stay in flight under the products; LIVE: this wave has a row tile.  (`more` is uniform over the workgroup.)
    auto chunk = [&](auto steady, auto has_rows, int f0, int cur, const double (&a)[4 * PROJ_KB], double (&an)[4 * PROJ_KB])
                     __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady)::value, LIVE = decltype(has_rows)::value;
        const bool more = STEADY || f0 + VBS_PROJ_CHUNK < n;
        if (more) {
            gather(f0 + VBS_PROJ_CHUNK, v);
            if constexpr (LIVE) {
                if constexpr (STEADY) fetch_full(f0 + VBS_PROJ_CHUNK, an);
                else fetch(f0 + VBS_PROJ_CHUNK, an);
            }
        }
        if constexpr (LIVE) {
            const double* buf = stage + cur * PROJ_BUF;
#pragma unroll
            for (int kb = 0; kb < PROJ_KB; ++kb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double av = prow ? a[kb * 4 + e] : 0.0;
#pragma unroll
                    for (int ct = 0; ct < PROJ_CT; ++ct) {
                        const double b = buf[(ct * VBS_PROJ_CHUNK + kb * 16 + 4 * e + q) * PROJ_COLS + r];
                        acc[ct] = mfma_f64(av, b, acc[ct]);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                               // the staging waits for its entries AFTER the products
        if (more) store(f0 + VBS_PROJ_CHUNK, stage + (cur ^ 1) * PROJ_BUF, v);
        __syncthreads();
    };
    // two chunks a turn, so that the A values alternate between a0 and a1 without a copy: steady turns while the chunk after the
    // second one is complete, then the last few chunks with their tests
    auto walk = [&](auto has_rows) __attribute__((always_inline)) {
        const std::true_type yes;
        const std::false_type no;
        int f0 = 0;
        for (; f0 + 3 * VBS_PROJ_CHUNK <= n; f0 += 2 * VBS_PROJ_CHUNK) {
            chunk(yes, has_rows, f0, 0, a0, a1);
            chunk(yes, has_rows, f0 + VBS_PROJ_CHUNK, 1, a1, a0);
        }
        for (; f0 < n; f0 += 2 * VBS_PROJ_CHUNK) {
            chunk(no, has_rows, f0, 0, a0, a1);
            if (f0 + VBS_PROJ_CHUNK < n) chunk(no, has_rows, f0 + VBS_PROJ_CHUNK, 1, a1, a0);
        }
    };
    gather(0, v);
    store(0, stage, v);
    if (live) fetch(0, a0);
    __syncthreads();
    if (live) walk(std::true_type{});
    else walk(std::false_type{});
    if (!live) return;

    const int c = r & 3;                                                 // this lane's column: slot r >> 2 of the tile, x_c or (c == 3) den
    const int oc = 1 + nv;
#pragma unroll
    for (int ct = 0; ct < PROJ_CT; ++ct) {
        const int m = s0 + ct * VBS_PROJ_SLOTS + (r >> 2);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rr = row0 + wave * 16 + q + 4 * g;
            if (m < s && rr < R) {
                double* o = proj + ((int64_t)m * R + rr) * oc;
                if (c == 3) o[0] = acc[ct][g];
                else if (c < nv) o[1 + c] = acc[ct][g];
            }
        }
    }
}

void launch_project_series(const double* rec, int n, int s, int cols, int n_values, const double* basis, int R, double* proj,
                           hipStream_t st) {
    const dim3 grid((unsigned)((R + VBS_PROJ_ROWS - 1) / VBS_PROJ_ROWS), (unsigned)((s + VBS_PROJ_WG_SLOTS - 1) / VBS_PROJ_WG_SLOTS));
    hipLaunchKernelGGL(k_project, grid, dim3(PROJ_THREADS), 0, st, rec, n, s, cols, n_values, basis, R, proj);
}

__global__ __launch_bounds__(VBS_FIT_GROUP * 64) void k_harmonic_fit(const double* __restrict__ proj, int s, int R, int nv, int Q,
                                                                    double min_count, double det_min, double* __restrict__ fit,
                                                                    double* __restrict__ peak) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VBS_FIT_GROUP + (threadIdx.x >> 6);
    if (i >= s) return;                                                  // (a whole wave; the kernel has no barrier)
    const int oc = 1 + nv, fc = 1 + 3 * nv;
    const double* P = proj + i * R * oc;
    const double N = P[0];
    const bool enough = N >= min_count;
    double m[3] = {0.0, 0.0, 0.0};
    if (enough) {
#pragma unroll
        for (int v = 0; v < 3; ++v)
            if (v < nv) m[v] = P[1 + v] / N;
    }
    int bi[3] = {-1, -1, -1};
    double bp[3] = {0.0, 0.0, 0.0}, ba[3] = {0.0, 0.0, 0.0}, bb[3] = {0.0, 0.0, 0.0};
    for (int qq = lane; qq < Q; qq += 64) {
        const double* rc = P + (int64_t)(1 + 2 * qq) * oc;
        const double* rs = P + (int64_t)(2 + 2 * qq) * oc;
        const double c1 = rc[0], s1 = rs[0];
        const double c2 = P[(int64_t)(1 + 2 * Q + 2 * qq) * oc], s2 = P[(int64_t)(2 + 2 * Q + 2 * qq) * oc];
        const double CC = 0.5 * (N + c2) - (c1 * c1) / N;
        const double SS = 0.5 * (N - c2) - (s1 * s1) / N;
        const double CS = 0.5 * s2 - (c1 * s1) / N;
        const double det = CC * SS - CS * CS;
        const bool ok = enough && det > det_min * (N * N);
        double* f = fit ? fit + (i * Q + qq) * fc : nullptr;
        if (f) f[0] = ok ? 1.0 : 0.0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            if (v >= nv) continue;
            double av = 0.0, bv = 0.0, pv = 0.0;
            if (ok) {
                const double pc = rc[1 + v] - m[v] * c1;
                const double ps = rs[1 + v] - m[v] * s1;
                av = (pc * SS - ps * CS) / det;
                bv = (ps * CC - pc * CS) / det;
                pv = av * pc + bv * ps;
                if (pv == pv && (bi[v] < 0 || pv > bp[v])) {             // ascending q: the earliest of equal maxima stays; a NaN
                    bi[v] = qq; bp[v] = pv; ba[v] = av; bb[v] = bv;      // power never wins and never suppresses
                }
            }
            if (f) { f[1 + 3 * v] = av; f[2 + 3 * v] = bv; f[3 + 3 * v] = pv; }
        }
    }
    if (!peak) return;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (v >= nv) continue;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double op = __shfl_down(bp[v], off), oa = __shfl_down(ba[v], off), ob = __shfl_down(bb[v], off);
            const int oi = __shfl_down(bi[v], off);
            if (oi >= 0 && (bi[v] < 0 || op > bp[v] || (op == bp[v] && oi < bi[v]))) { bp[v] = op; bi[v] = oi; ba[v] = oa; bb[v] = ob; }
        }
        if (lane == 0) {
            double* o = peak + (i * nv + v) * VBS_PEAK_COLS;
            const bool has = enough && bi[v] >= 0;
            o[0] = !enough ? 0.0 : has ? 2.0 : 1.0;
            o[1] = N;
            o[2] = enough ? m[v] : 0.0;
            o[3] = has ? (double)bi[v] : -1.0;
            o[4] = has ? ba[v] : 0.0; o[5] = has ? bb[v] : 0.0; o[6] = has ? bp[v] : 0.0;
        }
    }
}

void launch_harmonic_fit(const double* proj, int s, int R, int n_values, int Q, int min_count, double det_min, double* fit,
                         double* peak, hipStream_t st) {
    hipLaunchKernelGGL(k_harmonic_fit, dim3((unsigned)(((int64_t)s + VBS_FIT_GROUP - 1) / VBS_FIT_GROUP)), dim3(VBS_FIT_GROUP * 64), 0,
                       st, proj, s, R, n_values, Q, (double)min_count, det_min, fit, peak);
}
