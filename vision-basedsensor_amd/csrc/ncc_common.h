// What the NCC kernels share (k_ncc_mfma.hip, k_ncc_map.hip): the exact float64 evaluation straight from the mask bits, the
// threshold on G, and the constants of the float16 filter.  The algebra is at the top of k_ncc_mfma.hip.
#pragma once
#include "common.h"

__device__ __forceinline__ u64 load_bits(const u64* __restrict__ row, int WW, int start) {
    int wi = start >> 6, sh = start & 63;
    u64 a = (wi >= 0 && wi < WW) ? row[wi] : 0ull;
    u64 b = (wi + 1 >= 0 && wi + 1 < WW) ? row[wi + 1] : 0ull;
    return sh ? ((a >> sh) | (b << (64 - sh))) : a;
}

// Horizontal Gaussian sum of one pixel from the runs of 1-bits in its window (float64): a run [b, e) in
// window coordinates contributes CG[e] - CG[b], CG the cumulative template factor.
template <int L, int LO>
__device__ __forceinline__ double ncc_row_exact(const u64* __restrict__ row, int WW, int x, const double* cg,
                                                u32* cnt) {
    u64 w0 = load_bits(row, WW, x + LO), w1 = 0;
    if (L > 64) w1 = load_bits(row, WW, x + LO + 64) & ((1ull << (L > 64 ? L - 64 : 1)) - 1ull);
    else w0 &= (1ull << (L < 64 ? L : 0)) - 1ull;
    *cnt += __popcll(w0) + __popcll(w1);
    double h = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        u64 w = half ? w1 : w0;
        while (w) {
            int b0 = __ffsll((long long)w) - 1;
            u64 t = ~(w >> b0);
            int len = t ? __ffsll((long long)t) - 1 : 64 - b0;
            w &= (len >= 64) ? 0ull : ~(((1ull << len) - 1ull) << b0);
            h += cg[half * 64 + b0 + len] - cg[half * 64 + b0];
        }
    }
    return h;
}

// Exact float64 G(y, x) = sum_i g[i] H(y + LO + i, x), products added in ascending i.  Rare path (pixels the float32
// filter cannot decide, or the diagnostic map): kept out of line so that its loops are not replicated 8x.
template <int L, int LO>
__device__ __attribute__((noinline)) double ncc_exact_G(const u64* fbits, int H, int WW, int y, int x, const double* cg,
                                                        const double* gsh) {
    u32 dummy = 0;
    double Ge = 0.0;
    for (int i = 0; i < L; ++i) {
        int yy = y + LO + i;
        double hrow = (yy >= 0 && yy < H) ? ncc_row_exact<L, LO>(fbits + (int64_t)yy * WW, WW, x, cg, &dummy) : 0.0;
        Ge = __builtin_fma(gsh[i], hrow, Ge);
    }
    return Ge;
}

#define NCC_WSCALE 1024.0                               // weights are scaled so that every wlo is a normal float16
#define NCC_REL 2e-5f
#define NCC_NEVER 3e38                                  // "no G reaches this" (finite, so G - theta stays ordered)
#define NCC_TRIM_BIT 0x100                              // of k_ncc_mfma's dbg_arg: skip strips and rows whose windows are empty
#define NCC_ABS 1e-3f                                   // in units of G * 2^20: far below any theta with c >= 1

// theta on 2^20 G for a window with c foreground and nn in-image samples (+inf where var <= 0)
__device__ __forceinline__ double ncc_theta(double c, double nn, double sum_t, double mu, const NccConst& nc) {
    double sum_I = 255.0 * c;
    double rest = -nc.tbar * sum_I - mu * (sum_t - nn * nc.tbar);
    double s1 = sum_I - nn * mu;
    double s2 = 255.0 * sum_I - 2.0 * mu * sum_I + nn * mu * mu;
    double var = s2 - s1 * s1 * nc.inv_l2;
    double rhs = nc.thr2 * var * nc.T2;
    if (!(var > 0.0)) return NCC_NEVER;
    // an empty window has G = 0 exactly on both paths: decide it here
    if (c == 0.0) return (rest > 0.0 && rest * rest > rhs) ? -NCC_NEVER : NCC_NEVER;
    return (sqrt(rhs) - rest) * (NCC_WSCALE * NCC_WSCALE / 255.0);
}
