// Principal modes of the displacement field along a recording: the cross moments of all pairs of series, the
// covariance they give, its leading eigenpairs by orthogonal iteration, and the score of every mode in every frame.  Float64, no
// atomics, no wait across workgroups; a result depends on its inputs only.
//   k_cross_moments  the symmetric product [4 s x n] . [n x 4 s] by mfma_f64 of mfma_f64.h, the next user of the lane map and of the
//            fragment scheme of k_project (k_spectrum.hip), with the frame axis as K.  Per slot the staged columns are
//            (z1, z2, z3, flag as 1.0 / 0.0), z = x - shift rounded once when a valid entry is staged: k_project's tile column set, so
//            a 16-column tile is 4 slots.  A workgroup owns one PAIR of slot tiles (ti <= tj) of VBS_MOM_WG_SLOTS slots each: both
//            operands are staged from the record into LDS in the same layout ([tile of 4 slots][frame row, permuted][16]), wave w
//            takes the 4 slots w of tile ti as A against all MOM_CT column tiles of tj as B, and keeps its MOM_CT accumulators in
//            registers across the whole K loop - K is never split across workgroups, every output is one accumulator chain over the
//            chunks of VBS_MOM_CHUNK frames in ascending order from frame 0.  An invalid entry, a column beyond n_values, a slot >= s
//            and a frame >= n are the constant 0.0, selected by the flag and never multiplied by zero; nothing past n or s or beyond
//            n_values is read.  Double-buffered as k_project: the next chunk's entries are fetched before this chunk's products and
//            stored after them, one barrier a chunk.  The frame rows are stored in k_project's in-16 permutation (frame k0 + 4q + e
//            at row k0 + 4e + q); both operands read the same rows, so any permutation serves and a step reads 64 consecutive
//            doubles of LDS per operand.  On the diagonal (ti == tj) one staged tile is both operands.
//            The workgroup writes its block and the mirror block: mom[j, i, w, v] is a copy of mom[i, j, v, w], and on the diagonal
//            only the entries with 4 i + v <= 4 j + w are taken from the accumulators, so every cell has one writer and one value.
//   k_covariance  one thread per slot pair i <= j; every expression is the one include/vbs.h states, without contraction.
//   k_modes_apply  Y = A Q, one wave per row of A, lane l adds columns l, l + 64, .. ascending for all r vectors, the fold is 32,
//            16, 8, 4, 2, 1: the kernel is bound by reading A and has no matrix instruction.
//   k_modes_orth, k_modes_ritz  one workgroup of MODES_THREADS; thread t owns rows t, t + MODES_THREADS, .. of the block, so a row
//            is read and written by one thread and only the sums need a barrier (one each, the LDS slot alternates).
//   k_mode_scores  one wave per frame, VBS_SCORE_GROUP frames a workgroup, no barrier, nothing shared.
#include "common.h"
#include "mfma_f64.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define MOM_WAVES   (VBS_MOM_WG_SLOTS / 4)              // one 16-row tile (4 slots) a wave
#define MOM_THREADS (MOM_WAVES * 64)
#define MOM_CT      (VBS_MOM_WG_SLOTS / 4)              // column tiles of a slot tile
#define MOM_TILE    (VBS_MOM_CHUNK * VBS_MOM_WG_SLOTS * 4)       // doubles of one staged slot tile of one chunk
#define MOM_ENTRIES (VBS_MOM_CHUNK * VBS_MOM_WG_SLOTS / MOM_THREADS)   // (frame, slot) entries a thread stages per chunk and tile
#define MOM_KB      (VBS_MOM_CHUNK / 16)                // blocks of 16 frames in a chunk
static_assert(VBS_MOM_WG_SLOTS == 16, "the staging index splits an entry into (frame, slot of 16)");
static_assert(VBS_MOM_CHUNK % 16 == 0 && (VBS_MOM_CHUNK * VBS_MOM_WG_SLOTS) % MOM_THREADS == 0, "tile multiples; equal staging shares");
static_assert(4 * MOM_TILE * 8 <= 64 * 1024, "two staged chunks of two slot tiles fit the LDS a workgroup gets without asking");
static_assert(MOM_THREADS <= 1024, "a workgroup");

__global__ __launch_bounds__(MOM_THREADS) void k_cross_moments(const double* __restrict__ rec, int n, int s, int cols, int nv,
                                                               const double* __restrict__ shift, int tiles,
                                                               double* __restrict__ mom) {
    __shared__ __attribute__((aligned(16))) double stage[4 * MOM_TILE];  // [buffer][operand][column tile][frame row, permuted][16]
    // the tile pair of this workgroup: pairs are numbered row by row of the upper triangle
    int ti = 0, p = (int)blockIdx.x;
    while (p >= tiles - ti) { p -= tiles - ti; ++ti; }
    const int tj = ti + p;
    const bool diag = ti == tj;
    const int i0 = ti * VBS_MOM_WG_SLOTS, j0 = tj * VBS_MOM_WG_SLOTS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int sl = tid & 15;                                             // the slot of a tile this thread stages, in every entry

    // the shift of the two slots this thread stages (0.0 without one); a slot >= s reads slot s - 1 and is never used
    double sh[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (shift) {
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int m = (o ? j0 : i0) + sl;
            const double* e = shift + (int64_t)(m < s ? m : s - 1) * nv;
            sh[o][0] = e[0]; sh[o][1] = e[nv > 1 ? 1 : 0]; sh[o][2] = e[nv > 2 ? 2 : 0];
        }
    }
    // the entries of chunk `f0` this thread stages, fetched as quad_gather says
    auto gather = [&](int f0, int m0, double (&v)[MOM_ENTRIES][4]) { quad_gather<MOM_THREADS>(rec, n, s, cols, nv, f0, m0, tid, v); };
    // ... SELECTED by the flag when they are staged (after the products that ran while they were in flight), the shift subtracted
    // once: the value of an invalid entry never reaches an operation
    auto store = [&](int f0, int m0, const double (&sft)[3], double* buf, const double (&v)[MOM_ENTRIES][4]) {
#pragma unroll
        for (int j = 0; j < MOM_ENTRIES; ++j) {
            const int fr = (tid + j * MOM_THREADS) >> 4;
            const bool valid = (m0 + sl < s) & (f0 + fr < n) & (v[j][3] != 0.0);     // (& not &&: selects, no control flow)
            const int row = (fr & ~15) | ((fr & 3) << 2) | ((fr >> 2) & 3);
            double* d = buf + ((sl >> 2) * VBS_MOM_CHUNK + row) * 16 + (sl & 3) * 4;
            d[0] = valid ? v[j][0] - sft[0] : 0.0;
            d[1] = (valid & (nv > 1)) ? v[j][1] - sft[1] : 0.0;
            d[2] = (valid & (nv > 2)) ? v[j][2] - sft[2] : 0.0;
            d[3] = valid ? 1.0 : 0.0;
        }
    };

    const bool live = i0 + wave * 4 < s;                                 // this wave has a row tile (it stages and waits either way)
    f64x4 acc[MOM_CT];
#pragma unroll
    for (int ct = 0; ct < MOM_CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    double vi[MOM_ENTRIES][4], vj[MOM_ENTRIES][4];
    gather(0, i0, vi);
    if (!diag) gather(0, j0, vj);
    store(0, i0, sh[0], stage, vi);
    if (!diag) store(0, j0, sh[1], stage + MOM_TILE, vj);
    __syncthreads();
    int cur = 0;
    for (int f0 = 0; f0 < n; f0 += VBS_MOM_CHUNK, cur ^= 1) {
        const bool more = f0 + VBS_MOM_CHUNK < n;                        // (uniform over the workgroup)
        if (more) {
            gather(f0 + VBS_MOM_CHUNK, i0, vi);
            if (!diag) gather(f0 + VBS_MOM_CHUNK, j0, vj);
        }
        if (live) {
            const double* ba = stage + cur * 2 * MOM_TILE + wave * VBS_MOM_CHUNK * 16;
            const double* bb = stage + cur * 2 * MOM_TILE + (diag ? 0 : MOM_TILE);
#pragma unroll
            for (int kb = 0; kb < MOM_KB; ++kb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = kb * 16 + 4 * e + q;
                    const double av = ba[row * 16 + r];
#pragma unroll
                    for (int ct = 0; ct < MOM_CT; ++ct) {
                        const double b = bb[(ct * VBS_MOM_CHUNK + row) * 16 + r];
                        acc[ct] = mfma_f64(av, b, acc[ct]);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                               // the staging waits for its entries AFTER the products
        if (more) {
            double* nb = stage + (cur ^ 1) * 2 * MOM_TILE;
            store(f0 + VBS_MOM_CHUNK, i0, sh[0], nb, vi);
            if (!diag) store(f0 + VBS_MOM_CHUNK, j0, sh[1], nb + MOM_TILE, vj);
        }
        __syncthreads();
    }
    if (!live) return;

    const int w = r & 3;                                                 // this lane's column: slot r >> 2 of the column tile, value w
#pragma unroll
    for (int ct = 0; ct < MOM_CT; ++ct) {
        const int j = j0 + ct * 4 + (r >> 2);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = q + 4 * g;                                   // of this wave's 16: slot row >> 2, value row & 3
            const int i = i0 + wave * 4 + (row >> 2), v = row & 3;
            if (i < s && j < s && (!diag || 4 * i + v <= 4 * j + w)) {
                mom[(((int64_t)i * s + j) * 4 + v) * 4 + w] = acc[ct][g];
                mom[(((int64_t)j * s + i) * 4 + w) * 4 + v] = acc[ct][g];
            }
        }
    }
}

void launch_cross_moments(const double* rec, int n, int s, int cols, int n_values, const double* shift, double* mom, hipStream_t st) {
    const int tiles = (s + VBS_MOM_WG_SLOTS - 1) / VBS_MOM_WG_SLOTS;
    hipLaunchKernelGGL(k_cross_moments, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(MOM_THREADS), 0, st, rec, n, s, cols, n_values,
                       shift, tiles, mom);
}

__global__ __launch_bounds__(256) void k_covariance(const double* __restrict__ mom, int s, int nv, int mode, double need, double denom,
                                                    const u8* __restrict__ slot_mask, double* __restrict__ cov, u8* __restrict__ ok) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (i, j), flattened
    if (t >= (int64_t)s * s) return;
    const int i = (int)(t / s), j = (int)(t - (int64_t)i * s);
    if (i > j) return;                                                   // the pair (j, i) writes this cell
    const double* P = mom + ((int64_t)i * s + j) * 16;
    const double N = P[15];
    const bool good = N >= need && (!slot_mask || (slot_mask[i] != 0 && slot_mask[j] != 0));
    if (ok) { ok[(int64_t)i * s + j] = good ? 1 : 0; ok[(int64_t)j * s + i] = good ? 1 : 0; }
    const int64_t C = (int64_t)s * nv;
    const double* Pi = mom + ((int64_t)i * s + i) * 16;
    const double* Pj = mom + ((int64_t)j * s + j) * 16;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            if (v >= nv || w >= nv || (i == j && v > w)) continue;
            double c = 0.0;
            if (good) {
                const double S = P[4 * v + w], a = P[4 * v + 3], b = P[12 + w];
                if (mode == 0) c = (S - (a * b) / N) / (N - 1.0);
                else {
                    const double mi = Pi[4 * v + 3] / Pi[15], mj = Pj[4 * w + 3] / Pj[15];
                    c = (S - mi * b - mj * a + N * (mi * mj)) / denom;
                }
            }
            cov[((int64_t)i * nv + v) * C + (int64_t)j * nv + w] = c;
            cov[((int64_t)j * nv + w) * C + (int64_t)i * nv + v] = c;
        }
    }
}

void launch_covariance(const double* mom, int s, int n_values, int mode, int min_count, double denom, const u8* slot_mask, double* cov,
                       u8* ok, hipStream_t st) {
    const int64_t count = (int64_t)s * s;
    hipLaunchKernelGGL(k_covariance, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, mom, s, n_values, mode, (double)min_count,
                       denom, slot_mask, cov, ok);
}

// ---- the leading eigenpairs: blocks are [C][VBS_MODES_MAX] row-major, columns >= r never read ----------------------------------------
#define MODES_THREADS 256
#define MODES_WAVES   (MODES_THREADS / 64)
#define MR            VBS_MODES_MAX
static_assert(MR == 16 && MODES_WAVES == 4, "the sums below are written for 16 columns and 4 waves");

__global__ __launch_bounds__(MODES_THREADS) void k_modes_apply(const double* __restrict__ A, int C, int r, const double* __restrict__ Q,
                                                               double* __restrict__ Y) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * MODES_WAVES + (threadIdx.x >> 6);
    if (row >= C) return;                                                // (a whole wave; the kernel has no barrier)
    const double* a = A + (int64_t)row * C;
    double acc[MR];
#pragma unroll
    for (int k = 0; k < MR; ++k) acc[k] = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double av = a[c];
        const double* qr = Q + (int64_t)c * MR;
#pragma unroll
        for (int k = 0; k < MR; ++k)
            if (k < r) acc[k] = acc[k] + av * qr[k];
    }
#pragma unroll
    for (int k = 0; k < MR; ++k) {
        if (k >= r) continue;
        acc[k] = wave_fold_down(acc[k]);
        if (lane == 0) Y[(int64_t)row * MR + k] = acc[k];
    }
}

// S[k] = sum over the rows c of X[c][j] * Z[c][k] for lo <= k < hi, by the rule of the one-workgroup kernels: thread t adds rows t,
// t + MODES_THREADS, .. ascending, every wave folds its 64 sums 32, 16, 8, 4, 2, 1, the four wave sums are added ((W0 + W1) + W2) + W3.
// Every thread gets every sum.  `slot` alternates so that one barrier a call is enough.
__device__ __forceinline__ void modes_sums(const double* X, int j, const double* Z, int lo, int hi, int C, double (*red)[MODES_WAVES][MR],
                                           int& slot, double (&S)[MR]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[MR];
#pragma unroll
    for (int k = 0; k < MR; ++k) acc[k] = 0.0;
    for (int c = tid; c < C; c += MODES_THREADS) {
        const double x = X[(int64_t)c * MR + j];
        const double* z = Z + (int64_t)c * MR;
#pragma unroll
        for (int k = 0; k < MR; ++k)
            if (k >= lo && k < hi) acc[k] = acc[k] + x * z[k];
    }
#pragma unroll
    for (int k = 0; k < MR; ++k) {
        if (k < lo || k >= hi) continue;
        acc[k] = wave_fold_down(acc[k]);
        if (lane == 0) red[slot][wave][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MR; ++k) S[k] = (k >= lo && k < hi) ? ((red[slot][0][k] + red[slot][1][k]) + red[slot][2][k]) + red[slot][3][k] : 0.0;
    slot ^= 1;
}

// the start block of include/vbs.h: an integer hash of (c, k), exact in float64
__device__ __forceinline__ double modes_start(int c, int k) {
    u32 x = (u32)c * (u32)MR + (u32)k + 1u;
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return (double)(int32_t)x * 4.656612873077393e-10;                  // 2^-31
}

__global__ __launch_bounds__(MODES_THREADS) void k_modes_orth(double* __restrict__ X, int C, int r, double tiny, int start,
                                                              int32_t* __restrict__ info) {
    __shared__ double red[2][MODES_WAVES][MR];
    const int tid = threadIdx.x;
    int slot = 0, dropped = 0;
    double S[MR];
    if (start)
        for (int c = tid; c < C; c += MODES_THREADS)
#pragma unroll
            for (int k = 0; k < MR; ++k)
                if (k < r) X[(int64_t)c * MR + k] = modes_start(c, k);
    // the largest squared norm of the columns as they came in
    double big = 0.0;
    for (int j = 0; j < r; ++j) {
        modes_sums(X, j, X, j, j + 1, C, red, slot, S);
        big = S[j] > big ? S[j] : big;
    }
    for (int pass = 0; pass < 2; ++pass) {
        for (int j = 0; j < r; ++j) {
            modes_sums(X, j, X, j, r, C, red, slot, S);                  // the squared norm of column j and its products with the later ones
            const double nn = S[j];
            const bool keep = pass == 0 ? nn > tiny * big : nn > 0.0;    // (a NaN is dropped)
            if (!keep && pass == 0) ++dropped;
            const double nrm = sqrt(nn);
            for (int c = tid; c < C; c += MODES_THREADS) {
                double* x = X + (int64_t)c * MR;
                if (!keep) { x[j] = 0.0; continue; }
                const double qj = x[j] / nrm;
                x[j] = qj;
#pragma unroll
                for (int k = 0; k < MR; ++k)
                    if (k > j && k < r) x[k] = x[k] - (S[k] / nrm) * qj;
            }
        }
    }
    if (tid == 0 && info) { info[0] = r - dropped; info[1] = dropped; }
}

__global__ __launch_bounds__(MODES_THREADS) void k_modes_ritz(const double* __restrict__ Q, const double* __restrict__ Y, int C, int r,
                                                              double* __restrict__ values, double* __restrict__ modes,
                                                              double* __restrict__ resid) {
    __shared__ double red[2][MODES_WAVES][MR];
    __shared__ double T[MR][MR], V[MR][MR], lam[MR];
    __shared__ int perm[MR];
    __shared__ double bestv[MODES_WAVES][MR];
    __shared__ int besti[MODES_WAVES][MR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int slot = 0;
    double S[MR];
    // T = Q^T (A Q): the upper triangle from the sums, mirrored
    for (int k = 0; k < r; ++k) {
        modes_sums(Q, k, Y, k, r, C, red, slot, S);
        if (tid == 0)
#pragma unroll
            for (int l = 0; l < MR; ++l)
                if (l >= k && l < r) { T[k][l] = S[l]; T[l][k] = S[l]; }
    }
    if (tid == 0) {
        for (int k = 0; k < r; ++k)
            for (int l = 0; l < r; ++l) V[k][l] = k == l ? 1.0 : 0.0;
        // cyclic Jacobi: pairs (p, q), p < q, row by row, VBS_MODES_SWEEPS sweeps; both sides applied to the full matrix.  The
        // expressions of a pair are those fit_math.h states (jacobi_pair), here on a run-time r x r in LDS by one thread
        for (int sweep = 0; sweep < VBS_MODES_SWEEPS; ++sweep)
            for (int p = 0; p + 1 < r; ++p)
                for (int qq = p + 1; qq < r; ++qq) {
                    const double apq = T[p][qq];
                    if (apq == 0.0) continue;
                    const double theta = (T[qq][qq] - T[p][p]) / (2.0 * apq);
                    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
                    for (int k = 0; k < r; ++k) {
                        const double x = T[k][p], y = T[k][qq];
                        T[k][p] = cs * x - sn * y; T[k][qq] = sn * x + cs * y;
                    }
                    for (int k = 0; k < r; ++k) {
                        const double x = T[p][k], y = T[qq][k];
                        T[p][k] = cs * x - sn * y; T[qq][k] = sn * x + cs * y;
                    }
                    for (int k = 0; k < r; ++k) {
                        const double x = V[k][p], y = V[k][qq];
                        V[k][p] = cs * x - sn * y; V[k][qq] = sn * x + cs * y;
                    }
                    T[p][qq] = 0.0; T[qq][p] = 0.0;
                }
        // descending, the smaller index first among equals (a stable insertion)
        for (int k = 0; k < r; ++k) {
            int at = k;
            while (at > 0 && T[perm[at - 1]][perm[at - 1]] < T[k][k]) { perm[at] = perm[at - 1]; --at; }
            perm[at] = k;
        }
        for (int k = 0; k < r; ++k) { lam[k] = T[perm[k]][perm[k]]; values[k] = lam[k]; }
    }
    __syncthreads();
    // U = Q V and A U = Y V, l ascending from 0.0; the residual rows; the entry of largest magnitude of this thread's rows
    double acc[MR], bv[MR];
    int bi[MR];
#pragma unroll
    for (int k = 0; k < MR; ++k) { acc[k] = 0.0; bv[k] = -1.0; bi[k] = 0; }
    for (int c = tid; c < C; c += MODES_THREADS) {
        const double* qr = Q + (int64_t)c * MR;
        const double* yr = Y + (int64_t)c * MR;
#pragma unroll
        for (int k = 0; k < MR; ++k) {
            if (k >= r) continue;
            double u = 0.0, au = 0.0;
            for (int l = 0; l < r; ++l) {
                const double vv = V[l][perm[k]];
                u = u + qr[l] * vv;
                au = au + yr[l] * vv;
            }
            modes[(int64_t)k * C + c] = u;
            const double d = au - lam[k] * u;
            acc[k] = acc[k] + d * d;
            const double m = fabs(u);
            if (m > bv[k]) { bv[k] = m; bi[k] = c; }
        }
    }
#pragma unroll
    for (int k = 0; k < MR; ++k) {
        if (k >= r) continue;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            acc[k] = acc[k] + __shfl_down(acc[k], off);
            const double ov = __shfl_down(bv[k], off);
            const int oi = __shfl_down(bi[k], off);
            if (ov > bv[k] || (ov == bv[k] && oi < bi[k])) { bv[k] = ov; bi[k] = oi; }
        }
        if (lane == 0) { red[slot][wave][k] = acc[k]; bestv[wave][k] = bv[k]; besti[wave][k] = bi[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MR; ++k) {
        if (k >= r) continue;
        double m = bestv[0][k];
        int at = besti[0][k];
        for (int w = 1; w < MODES_WAVES; ++w)
            if (bestv[w][k] > m || (bestv[w][k] == m && besti[w][k] < at)) { m = bestv[w][k]; at = besti[w][k]; }
        // the entry of largest magnitude is made positive: `at` is a row of one thread, whose write above this thread may not see,
        // so the sign is recomputed from Q and V as it was there
        double u = 0.0;
        for (int l = 0; l < r; ++l) u = u + Q[(int64_t)at * MR + l] * V[l][perm[k]];
        if (u < 0.0)
            for (int c = tid; c < C; c += MODES_THREADS) modes[(int64_t)k * C + c] = -modes[(int64_t)k * C + c];
        if (tid == 0) resid[k] = sqrt(((red[slot][0][k] + red[slot][1][k]) + red[slot][2][k]) + red[slot][3][k]);
    }
}

void launch_leading_modes(const double* A, int C, int r, int iters, double tiny, double* work, double* values, double* modes,
                          double* resid, int32_t* info, hipStream_t st) {
    double* Q = work;
    double* Y = work + (int64_t)C * MR;
    const dim3 rows((unsigned)((C + MODES_WAVES - 1) / MODES_WAVES)), one(1), th(MODES_THREADS);
    hipLaunchKernelGGL(k_modes_orth, one, th, 0, st, Q, C, r, tiny, 1, info);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(k_modes_apply, rows, th, 0, st, A, C, r, Q, Y);
        hipLaunchKernelGGL(k_modes_orth, one, th, 0, st, Y, C, r, tiny, 0, info);
        double* t = Q; Q = Y; Y = t;
    }
    hipLaunchKernelGGL(k_modes_apply, rows, th, 0, st, A, C, r, Q, Y);
    hipLaunchKernelGGL(k_modes_ritz, one, th, 0, st, Q, Y, C, r, values, modes, resid);
}

__global__ __launch_bounds__(VBS_SCORE_GROUP * 64) void k_mode_scores(const double* __restrict__ rec, int s, int cols, int nv,
                                                                      const double* __restrict__ center,
                                                                      const double* __restrict__ modes, int r, double min_coverage,
                                                                      int frame_begin, int frame_end, double* __restrict__ scores,
                                                                      double* __restrict__ energy) {
    const int lane = threadIdx.x & 63;
    const int64_t f = frame_begin + (int64_t)blockIdx.x * VBS_SCORE_GROUP + (threadIdx.x >> 6);
    if (f >= frame_end) return;                                          // (a whole wave; the kernel has no barrier)
    const int C = s * nv;
    const double* row = rec + f * s * cols;
    double num[MR], den[MR], e = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < MR; ++k) { num[k] = 0.0; den[k] = 0.0; }
    for (int c = lane; c < C; c += 64) {
        const int i = c / nv, v = c - i * nv;
        const double* en = row + (int64_t)i * cols;
        if (en[0] == 0.0) continue;                                      // selected out: nothing of an invalid entry is read
        const double d = en[1 + v] - center[c];
        e = e + d * d;
        cnt = cnt + 1.0;
#pragma unroll
        for (int k = 0; k < MR; ++k) {
            if (k >= r) continue;
            const double u = modes[(int64_t)k * C + c];
            num[k] = num[k] + d * u;
            den[k] = den[k] + u * u;
        }
    }
    // the fold of wave_fold_down for two sums, a step of each in turn (written out here and below: one whole fold after the
    // other is the same arithmetic but other device code, profiles/analysis_fold_text_equal.txt)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { e = e + __shfl_down(e, off); cnt = cnt + __shfl_down(cnt, off); }
    const int64_t o = f - frame_begin;
    if (lane == 0 && energy) { energy[o * 2] = cnt; energy[o * 2 + 1] = e; }
#pragma unroll
    for (int k = 0; k < MR; ++k) {
        if (k >= r) continue;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { num[k] = num[k] + __shfl_down(num[k], off); den[k] = den[k] + __shfl_down(den[k], off); }
        if (lane == 0) {
            double* sc = scores + (o * r + k) * 3;
            const bool seen = den[k] >= min_coverage;
            sc[0] = seen ? 1.0 : 0.0; sc[1] = seen ? num[k] / den[k] : 0.0; sc[2] = den[k];
        }
    }
}

void launch_mode_scores(const double* rec, int s, int cols, int n_values, const double* center, const double* modes, int r,
                        double min_coverage, int frame_begin, int frame_end, double* scores, double* energy, hipStream_t st) {
    const int F = frame_end - frame_begin;
    hipLaunchKernelGGL(k_mode_scores, dim3((unsigned)((F + VBS_SCORE_GROUP - 1) / VBS_SCORE_GROUP)), dim3(VBS_SCORE_GROUP * 64), 0, st,
                       rec, s, cols, n_values, center, modes, r, min_coverage, frame_begin, frame_end, scores, energy);
}
