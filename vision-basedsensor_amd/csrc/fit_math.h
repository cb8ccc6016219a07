// What the one-wave-per-frame float64 fits (k_posecov, k_shape, k_rigid, k_sphere) share around their sums: the point rules of a
// table slot, one pair of the cyclic Jacobi and the LDL' without pivoting.  Every expression here is part of the bit-for-bit
// contract of include/vbs.h and is stated ONCE, here; the oracles under tests/helpers restate it per entry.  Float64 without
// contraction: the pragma below is this header's own, because an including file sets its own only after its includes.  Every
// function runs in every lane alike over constant indices (the loops unroll), so the small matrices live in registers.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

// ---- the point rules -----------------------------------------------------------------------------------------------------------------
// a table row carries a 3-D point where it has VBS_FLAG_XYZ; the point is columns 6, 7, 8 as doubles
__device__ __forceinline__ bool row_has_point(const float* r) { return ((int)r[0] & VBS_FLAG_XYZ) != 0; }
__device__ __forceinline__ void row_xyz(const float* r, double* p) { p[0] = (double)r[6]; p[1] = (double)r[7]; p[2] = (double)r[8]; }
__device__ __forceinline__ bool row_point(const float* r, double* p) {
    if (!row_has_point(r)) return false;
    row_xyz(r, p);
    return true;
}

// The end point of a slot as vbs_pose_series forms it, or false: the slot is selected, its ref_disp row is flagged and both the
// start frame's row (in srow) and this frame's (in frow) carry a point.  p = ref + scale * ((X_f - X_start) - ref_disp), with
// ref_z taken as 0.0 unless `shell`.  k_pose computes the same expressions from its LDS stage.
__device__ __forceinline__ bool end_point(const float* frow, const float* srow, const double* ref_disp, const double* ref_xyz,
                                          const u8* slot_mask, int shell, double scale, int slot, double* p) {
    const double* d = ref_disp + (int64_t)slot * 4;
    const float* r0 = srow + (int64_t)slot * VBS_TABLE_COLS;
    const float* r = frow + (int64_t)slot * VBS_TABLE_COLS;
    if (!((!slot_mask || slot_mask[slot]) && d[0] != 0.0 && row_has_point(r0) && row_has_point(r))) return false;
    const double* rp = ref_xyz + (int64_t)slot * 3;
    const double dx = ((double)r[6] - (double)r0[6]) - d[1];
    const double dy = ((double)r[7] - (double)r0[7]) - d[2];
    const double dz = ((double)r[8] - (double)r0[8]) - d[3];
    const double sx = scale * dx, sy = scale * dy, sz = scale * dz;
    p[0] = rp[0] + sx; p[1] = rp[1] + sy; p[2] = (shell ? rp[2] : 0.0) + sz;
    return true;
}

// ---- the cyclic Jacobi ---------------------------------------------------------------------------------------------------------------
// One pair (P, Q) of a sweep over the symmetric T, V accumulating the rotations: columns, rows, V, then both off-diagonal entries
// are set to 0.  The caller lists the pairs over constant indices and keeps its sweep loop rolled (`#pragma unroll 1`).
// k_modes_ritz applies the same expressions to a run-time r x r in LDS.
// theta * theta may overflow to +inf: then tt = +-0, cs = 1, sn = +-0 and the rotation is the identity.
template <int N, int P, int Q>
__device__ __forceinline__ void jacobi_pair(double (&T)[N][N], double (&V)[N][N]) {
    const double apq = T[P][Q];
    if (apq == 0.0) return;                                      // (the same for every lane: the sums are broadcast)
    const double theta = (T[Q][Q] - T[P][P]) / (2.0 * apq);
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double x = T[k][P], y = T[k][Q];
        T[k][P] = cs * x - sn * y; T[k][Q] = sn * x + cs * y;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double x = T[P][k], y = T[Q][k];
        T[P][k] = cs * x - sn * y; T[Q][k] = sn * x + cs * y;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double x = V[k][P], y = V[k][Q];
        V[k][P] = cs * x - sn * y; V[k][Q] = sn * x + cs * y;
    }
    T[P][Q] = 0.0; T[Q][P] = 0.0;
}

// ---- LDL' of a symmetric N x N in basis order without pivoting -----------------------------------------------------------------------
// A = L D L' column by column, left at the first pivot that fails d_j > piv_rel * A[j][j]; returns the number of leading pivots
// that passed (the same for every lane: the sums are broadcast).  Lm (below the diagonal) and d are written for those columns
// only, so the substitutions below take that number or a smaller one.
template <int N>
__device__ __forceinline__ int ldl_factor(const double (&A)[N][N], double piv_rel, double (&Lm)[N][N], double (&d)[N]) {
    double c[N][N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - Lm[j][k] * c[j][k];
        if (!(dj > piv_rel * A[j][j])) return j;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double cij = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) cij = cij - Lm[j][k] * c[i][k];
            c[i][j] = cij; Lm[i][j] = cij / dj;
        }
    }
    return N;
}

// y = D^-1 L^-1 g over the leading npass rows (the others are left as they are)
template <int N>
__device__ __forceinline__ void ldl_forward(const double (&Lm)[N][N], const double (&d)[N], const double* g, int npass, double (&y)[N]) {
    double z[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i >= npass) return;
        double zi = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) zi = zi - Lm[i][k] * z[k];
        z[i] = zi; y[i] = zi / d[i];
    }
}

// x = L'^-1 y of the leading M x M alone, from the last row up
template <int M, int N>
__device__ __forceinline__ void ldl_back(const double (&Lm)[N][N], const double (&y)[N], double* x) {
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        double b = y[i];
#pragma unroll
        for (int k = i + 1; k < M; ++k) b = b - Lm[k][i] * x[k];
        x[i] = b;
    }
}
