// The fold of the 64 values a wave holds, one a lane: the one statement of its order.
//
// Every fold here goes DOWN: step `off` = 32, 16, 8, 4, 2, 1 gives lane i the combination of its own value (left operand) and
// lane i + off's (right operand), and a lane >= off is not read again.  For a sum that is
//     b[i] = a[i] + a[i + 32]  (i < 32),   c[i] = b[i] + b[i + 16]  (i < 16),   ...   total = g[0] + g[1],
// in IEEE float64 without contraction.  This order is part of the contract of the float64 entries (include/vbs.h): the oracles
// under tests/helpers restate exactly this tree, so a result depends on its inputs only and never on the launch shape.  The
// __shfl_xor butterflies of k_solve, k_calib, k_chess and k_diameter add in another order and are not this fold.
#pragma once
#include <hip/hip_runtime.h>

// lane 0 holds the sum (the other lanes hold partial sums nobody reads)
__device__ __forceinline__ double wave_fold_down(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ int wave_fold_down(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__device__ __forceinline__ long long wave_fold_down(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// every lane gets lane 0's sum
__device__ __forceinline__ double wave_sum(double v) { return __shfl(wave_fold_down(v), 0); }
__device__ __forceinline__ int wave_sum(int v) { return __shfl(wave_fold_down(v), 0); }

// The largest value with the smallest index among equals; a lane without a candidate holds i = -1 and never wins.  Lane 0 holds
// the result (v is meaningful only where i >= 0).
__device__ __forceinline__ void wave_argmax_down(double& v, int& i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int oi = __shfl_down(i, off);
        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
    }
}
