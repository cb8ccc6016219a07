// Contact maps along a recording: a gap-aware normalised kernel smoother in space, the spatial counterpart of
// k_fir, and the contact patch of every map.  Float64, no atomics; a result depends on its inputs only, never on the launch shape.
//   k_field_map<NT>  [P grid points x s slots] . [s x 16 columns] by mfma_f64 of mfma_f64.h.  The 16 columns of a tile are
//            VBS_FIELD_FRAMES = 4 frames x (x1, x2, x3, flag as 1.0 / 0.0), so the flag column's product IS den.  A workgroup takes
//            NT frame tiles (4, 2 or 1 by s, so that the staged values fit FIELD_LDS_MAX), stages their SELECTED values once in LDS
//            - an invalid entry, a column beyond n_values, a slot >= s or a frame past the range is the constant 0.0 and is never
//            read - and its waves walk the grid tiles against them: one A fragment (W, from global memory: every workgroup
//            re-reads it, it is cache-resident) feeds NT matrix instructions.
//            K is taken 16 slots at a time and PERMUTED inside those 16: lane (row r, quarter q) loads W[r][k0 + 4q .. 4q + 3], a
//            contiguous 32-byte run, and uses element e in step e, so step e multiplies slots k0 + 4q + e, q = 0..3.  The staged
//            rows are stored in that order (slot k0 + 4q + e at row k0 + 4e + q): a step reads 64 consecutive doubles of LDS.
//            The order of summation is not part of the interface (include/vbs.h); every frame tile meets the same order.
//   k_patch_stats   one wave per frame, VBS_PATCH_GROUP frames (waves) a workgroup, nothing shared; every sum follows the rule of
//            k_axis_displacement (lane l adds points l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1), without contraction.
#include "common.h"
#include "mfma_f64.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define FIELD_WAVES   8
#define FIELD_THREADS (FIELD_WAVES * 64)
#define FIELD_LDS_MAX (128 * 1024)               // bytes of staged values a workgroup may hold (of 160 KB)
#define FIELD_COLS    (VBS_FIELD_FRAMES * 4)     // columns of a tile
static_assert(FIELD_COLS == 16, "a tile is 16 columns: 4 frames x (3 values, flag)");
static_assert(((VBS_FIELD_MAX_SLOTS + 15) & ~15) * FIELD_COLS * 8 <= FIELD_LDS_MAX, "one frame tile of the longest record fits");

template <int NT>
__global__ __launch_bounds__(FIELD_THREADS) void k_field_map(const double* __restrict__ rec, int s, int cols, int nv,
                                                             const double* __restrict__ W, const double* __restrict__ wsum, int P,
                                                             double min_coverage, int frame_begin, int n_frames,
                                                             double* __restrict__ map) {
    extern __shared__ __attribute__((aligned(16))) double stage[];       // [NT][s16][FIELD_COLS], rows permuted as stated above
    const int s16 = (s + 15) & ~15;
    const int64_t f0 = (int64_t)blockIdx.x * (NT * VBS_FIELD_FRAMES);    // this workgroup's first frame among those emitted

    for (int i = threadIdx.x; i < NT * VBS_FIELD_FRAMES * s16; i += FIELD_THREADS) {
        const int fj = i / s16, m = i - fj * s16;                        // frame of the workgroup, slot
        const int64_t fi = f0 + fj;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (m < s && fi < n_frames) {
            const double* r = rec + (((int64_t)frame_begin + fi) * s + m) * cols;
            if (r[0] != 0.0) {                                           // what is not selected is never read into a value
                v[3] = 1.0;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c < nv) v[c] = r[1 + c];
            }
        }
        const int row = (m & ~15) | ((m & 3) << 2) | ((m >> 2) & 3);
        double* d = stage + ((int64_t)((fj >> 2) * s16 + row) * FIELD_COLS + (fj & 3) * 4);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int tiles = (P + 15) >> 4;
    const int oc = 1 + nv;
    const int sfull = s & ~15;
    for (int t = wave; t < tiles; t += FIELD_WAVES) {
        const int p = t * 16 + r;
        const bool prow = p < P;
        const double* wr = W + (int64_t)(prow ? p : P - 1) * s + 4 * q;  // (a row of W in every lane; a row >= P is selected to 0.0)
        f64x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f64x4{0.0, 0.0, 0.0, 0.0};
        auto products = [&](int k0, const double* a) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const double b = stage[(int64_t)(nt * s16 + k0 + 4 * e + q) * FIELD_COLS + r];
                    acc[nt] = mfma_f64(prow ? a[e] : 0.0, b, acc[nt]);
                }
            }
        };
        // whole blocks of 16 slots: this lane's four of the next block are in flight while this block's products run (the last
        // block is fetched twice rather than branched around)
        double a[4], an[4];
        if (sfull > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = wr[e];
        }
        for (int k0 = 0; k0 < sfull; k0 += 16) {
            const int kn = k0 + 16 < sfull ? k0 + 16 : k0;
#pragma unroll
            for (int e = 0; e < 4; ++e) an[e] = wr[kn + e];
            products(k0, a);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = an[e];
        }
        if (sfull < s) {                                                 // the last, partial block: slots >= s are the constant 0.0
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = sfull + 4 * q + e;
                const double w = wr[(m < s ? m : s - 1) - 4 * q];        // (the row's last slot instead: never a read past s)
                a[e] = m < s ? w : 0.0;
            }
            products(sfull, a);
        }
        const int j = r >> 2, c = r & 3;                                 // this lane's column: frame j of the tile, x_c or (c == 3) den
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t fi = f0 + nt * VBS_FIELD_FRAMES + j;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int pp = t * 16 + q + 4 * g;
                const double val = acc[nt][g];
                const double den = __shfl(val, lane | 3);                // the flag column of the same frame and row
                if (pp < P && fi < n_frames) {
                    const bool ok = den > 0.0 && den >= min_coverage * wsum[pp];
                    double* o = map + (fi * P + pp) * oc;
                    if (c == 3) o[0] = ok ? 1.0 : 0.0;
                    else if (c < nv) o[1 + c] = ok ? val / den : 0.0;
                }
            }
        }
    }
}

int launch_field_map(const double* rec, int s, int cols, int n_values, const double* W, const double* wsum, int P,
                     double min_coverage, int frame_begin, int frame_end, double* map, hipStream_t st) {
    const int nf = frame_end - frame_begin;
    const int s16 = (s + 15) & ~15;
    const size_t tile_bytes = (size_t)s16 * FIELD_COLS * sizeof(double);
    int nt = 4 * tile_bytes <= FIELD_LDS_MAX ? 4 : 2 * tile_bytes <= FIELD_LDS_MAX ? 2 : 1;
    while (nt > 1 && (nt / 2) * VBS_FIELD_FRAMES >= nf) nt /= 2;         // (no result depends on it)
    const size_t lds = nt * tile_bytes;
    const dim3 grid((unsigned)(((int64_t)nf + nt * VBS_FIELD_FRAMES - 1) / (nt * VBS_FIELD_FRAMES)));
#define FIELD_GO(NT)                                                                                                              \
    do {                                                                                                                          \
        if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_field_map<NT>),                                \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)           \
            return VBS_EHIP;                                                                                                      \
        hipLaunchKernelGGL(k_field_map<NT>, grid, dim3(FIELD_THREADS), lds, st, rec, s, cols, n_values, W, wsum, P, min_coverage, \
                           frame_begin, nf, map);                                                                                 \
    } while (0)
    if (nt == 4) FIELD_GO(4);
    else if (nt == 2) FIELD_GO(2);
    else FIELD_GO(1);
#undef FIELD_GO
    return VBS_OK;
}

__global__ __launch_bounds__(VBS_PATCH_GROUP * 64) void k_patch_stats(const double* __restrict__ map, int F, int P, int nv,
                                                                      const double* __restrict__ grid_xy, int component, double sign,
                                                                      double thr, double* __restrict__ patch) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * VBS_PATCH_GROUP + (threadIdx.x >> 6);
    if (fi >= F) return;                                                 // (a whole wave; the kernel has no barrier)
    const int oc = 1 + nv;
    const double* mp = map + fi * P * oc;
    int covered = 0, count = 0, pi = -1;
    double S = 0.0, Sx = 0.0, Sy = 0.0, pk = 0.0;
    for (int p = lane; p < P; p += 64) {
        const double* e = mp + (int64_t)p * oc;
        if (e[0] == 0.0) continue;
        ++covered;
        double sc;
        if (component >= 0) sc = sign * e[1 + component];
        else {
            sc = e[1] * e[1];
            if (nv > 1) sc = sc + e[2] * e[2];
            if (nv > 2) sc = sc + e[3] * e[3];
        }
        if (!(sc >= thr)) continue;                                      // (a NaN score is never in the patch)
        ++count;
        S = S + sc;
        Sx = Sx + sc * grid_xy[2 * p];
        Sy = Sy + sc * grid_xy[2 * p + 1];
        if (pi < 0 || sc > pk) { pk = sc; pi = p; }                      // ascending p: the earliest of equal maxima stays
    }
    // wave_argmax_down(pk, pi), written out: through the function's references this kernel compiles to other device code
    // (profiles/analysis_fold_text_equal.txt)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ok = __shfl_down(pk, off);
        const int oi = __shfl_down(pi, off);
        if (oi >= 0 && (pi < 0 || ok > pk || (ok == pk && oi < pi))) { pk = ok; pi = oi; }
    }
    covered = wave_sum(covered); count = wave_sum(count);
    S = wave_sum(S); Sx = wave_sum(Sx); Sy = wave_sum(Sy);
    if (lane == 0) {
        double* o = patch + fi * VBS_PATCH_COLS;
        const bool centre = covered > 0 && count > 0 && S > 0.0;
        o[0] = covered == 0 ? 0.0 : centre ? 2.0 : 1.0;
        o[1] = (double)covered; o[2] = (double)count; o[3] = S;
        o[4] = centre ? Sx / S : 0.0; o[5] = centre ? Sy / S : 0.0;
        o[6] = centre ? pk : 0.0;
        o[7] = centre ? (double)pi : covered == 0 ? 0.0 : -1.0;
    }
}

void launch_patch_stats(const double* map, int F, int P, int n_values, const double* grid_xy, int component, double sign, double thr,
                        double* patch, hipStream_t st) {
    hipLaunchKernelGGL(k_patch_stats, dim3((unsigned)(((int64_t)F + VBS_PATCH_GROUP - 1) / VBS_PATCH_GROUP)),
                       dim3(VBS_PATCH_GROUP * 64), 0, st, map, F, P, n_values, grid_xy, component, sign, thr, patch);
}
