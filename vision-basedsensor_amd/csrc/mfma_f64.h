// What the float64 matrix-core kernels of the recording analyses (k_field_map, k_project, k_window_moments, k_poly_moments,
// k_cross_moments) share: the instruction and its lane map, the padded tap row and tile arithmetic of the banded products, the fetch
// of (x1, x2, x3, flag) entries.  Walks, stores, band geometry and the row permutation stay in the kernels: shared, they compile to
// other device code, slower in two of them (profiles/mfma_f64_text_equal.txt).  The contract(off) below is the header's own.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

// v_mfma_f64_16x16x4_f64, D = A . B + C over one wave.  Lane map: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// one double a lane; D[row = (lane >> 4) + 4 reg][col = lane & 15], reg 0..3.
typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }

// The banded (Toeplitz) products along time (k_window_moments, k_poly_moments) read A from a zero-padded copy of a tap row in LDS:
// BAND_PAD zeros, t[-h .. h], zeros up to the last step's reach, BAND_ROW doubles in all.  Their workgroups own TILE output frames
// aligned to multiples of TILE of the GLOBAL frame index: the tiles [first, first + count) hold the frames [frame_begin, frame_end)
#define BAND_PAD 15
#define BAND_ROW (2 * (VBS_HALF_TAPS - 1) + 40)
static inline int band_tiles(int frame_begin, int frame_end, int tile, int* first) {
    *first = frame_begin / tile;
    return (frame_end - 1) / tile - *first + 1;
}

// The (x1, x2, x3, flag) entries k_project and k_cross_moments stage, ENTRIES a thread: entry j of thread tid is slot m0 + (tid & 15)
// of frame f0 + ((tid + j THREADS) >> 4), fetched as it lies in the record.  No branch and no load that waits for another: a slot >= s
// or a frame >= n fetches the last slot or frame instead, a column beyond n_values the flag again; nothing beyond them is read.
template <int THREADS, int ENTRIES>
__device__ __forceinline__ void quad_gather(const double* rec, int n, int s, int cols, int nv, int f0, int m0, int tid,
                                            double (&v)[ENTRIES][4]) {
    static_assert(THREADS % 16 == 0, "a thread stages one slot of the 16 in every entry");
#pragma unroll
    for (int j = 0; j < ENTRIES; ++j) {
        const int m = m0 + (tid & 15), f = f0 + ((tid + j * THREADS) >> 4);
        const double* e = rec + ((int64_t)(f < n ? f : n - 1) * s + (m < s ? m : s - 1)) * cols;
        v[j][3] = e[0]; v[j][0] = e[1]; v[j][1] = e[nv > 1 ? 2 : 0]; v[j][2] = e[nv > 2 ? 3 : 0];
    }
}
