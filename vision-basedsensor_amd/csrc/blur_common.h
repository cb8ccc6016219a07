// What the two blur kernels share (k_blur_mfma.hip, k_blur16.hip).
// a4-a5: two uint8 GaussianBlurs (OpenCV fixed-point model), DoG + 15 (mod 256), inRange.
// Reference: marker_detection.py:114-129.  Integer arithmetic throughout, so results are
// independent of summation order and bit-exact against oracle/stages.py:gaussian_blur_u8.
//
//   out(y,x) = ( sum_i ky[i] * ( sum_j kx[j] * p(y+i-c, x+j-c) ) + 2^15 ) >> 16,  taps in 1/256
#pragma once
#include "common.h"

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// a horizontal result tile as the vertical product's operand: its signed high bytes and its low bytes (offset by 128),
// four rows to a dword - 32 x 32 tiles (k_blur_mfma) and 16 x 16 tiles (k_blur16)
__device__ __forceinline__ void pack_tile(const v16i& acc, v4i& hi, v4i& lo) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        u32 t01 = __builtin_amdgcn_perm((u32)acc[4 * q + 1], (u32)acc[4 * q + 0], 0x05010400u);
        u32 t23 = __builtin_amdgcn_perm((u32)acc[4 * q + 3], (u32)acc[4 * q + 2], 0x05010400u);
        lo[q] = (int)(__builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u);
        hi[q] = (int)__builtin_amdgcn_perm(t23, t01, 0x07060302u);
    }
}

__device__ __forceinline__ void pack16(const v4i& acc, int& hi, int& lo) {
    const u32 t01 = __builtin_amdgcn_perm((u32)acc[1], (u32)acc[0], 0x05010400u);
    const u32 t23 = __builtin_amdgcn_perm((u32)acc[3], (u32)acc[2], 0x05010400u);
    lo = (int)(__builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u);
    hi = (int)__builtin_amdgcn_perm(t23, t01, 0x07060302u);
}
