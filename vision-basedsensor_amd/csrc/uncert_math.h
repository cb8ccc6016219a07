// The forward mode through the 3-D solve that k_uncert.hip and k_posecov.hip (4.23) share: the primal as executed,
// the push of ONE direction through it, the observation Jacobian and covariance, the usable rule.  Every expression here is
// restated in tests/helpers/uncert_oracle.py and held bit for bit; the including file sets `#pragma clang fp contract(off)`.
#pragma once
#include "track_common.h"
#pragma clang fp contract(off)

#define UNC_CAM   VBS_UNCERT_CAM
#define UNC_SEED  (UNC_CAM + 3)
#define UNC_REF   VBS_UNCERT_REF_COLS            // usable, the six entries of J_obs Sigma_o J_obs', G [q][3]
static_assert(UNC_CAM == 16 && UNC_REF == 7 + 3 * UNC_CAM, "the layout of a reference row");

struct UncFactor { double v[UNC_CAM * UNC_CAM]; };               // column c of L at v[c * 16 .. c * 16 + 15]

// what the solve leaves behind for its tangents: the iterates BEFORE each of the five steps, the last one, and solve_marker's values
struct UncPrimal {
    double xi[5], yi[5], xe, ye;
    double du, dv, Rr, fa, kk, S, q, h, a0, a1, pc[3];
};

// undistort_point followed by solve_marker, statement for statement (the same bits), keeping the intermediates
static __device__ __forceinline__ bool unc_primal(const CamD& c, double u0, double v0, double d, UncPrimal& P, double* X) {
    const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
    const double x0 = (u0 - cx) / fx, y0 = (v0 - cy) / fy;
    double x = x0, y = y0;
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        P.xi[it] = x; P.yi[it] = y;
        if (c.has_dist) {
            const double r2 = x * x + y * y;
            const double icd = 1.0 / (1.0 + ((c.k[4] * r2 + c.k[1]) * r2 + c.k[0]) * r2);
            const double dxx = 2.0 * c.k[2] * x * y + c.k[3] * (r2 + 2.0 * x * x);
            const double dyy = c.k[2] * (r2 + 2.0 * y * y) + 2.0 * c.k[3] * x * y;
            x = (x0 - dxx) * icd;
            y = (y0 - dyy) * icd;
        }
    }
    P.xe = x; P.ye = y;
    const double u = x * fx + cx, v = y * fy + cy;
    const float f_avg = (c.fx + c.fy) / 2.0f;
    P.du = u - cx; P.dv = v - cy;
    P.Rr = sqrt(P.du * P.du + P.dv * P.dv);
    X[0] = X[1] = X[2] = 0.0;
    if (P.Rr < 1e-6) return false;
    const float k32 = c.dmm / f_avg;
    const float f2 = f_avg * f_avg;
    P.fa = (double)f_avg; P.kk = (double)k32;
    P.S = sqrt(P.Rr * P.Rr + (double)f2);
    const double d_eff = P.kk * P.S;
    P.q = d_eff / d;
    P.h = P.fa * P.q;
    P.a0 = P.h * P.du / fx; P.a1 = P.h * P.dv / fy;
    P.pc[0] = P.a0 - c.T[0]; P.pc[1] = P.a1 - c.T[1]; P.pc[2] = P.h - c.T[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = c.R[0 * 3 + i] * P.pc[0] + c.R[1 * 3 + i] * P.pc[1] + c.R[2 * 3 + i] * P.pc[2];
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

// The directional derivative of X along the seed s [19].  f_avg, dmm / f_avg and f_avg^2 are differentiated as the smooth float64
// expressions; the primal values the tangents multiply are the solve's own.  du = (x fx + cx) - cx: the two seeds of cx
// cancel and are left out.  The rotation is perturbed on the camera side, R_wc' = exp([w]x) R_wc at w = 0: dX = R_wc' (pc x w).
static __device__ __forceinline__ void unc_push(const CamD& c, const UncPrimal& P, double d, const double* s, double* t) {
    const double fx = c.fx, fy = c.fy;
    const double x0 = P.xi[0], y0 = P.yi[0];
    const double tx0 = ((s[16] - s[2]) - x0 * s[0]) / fx, ty0 = ((s[17] - s[3]) - y0 * s[1]) / fy;
    double tx = tx0, ty = ty0;
    if (c.has_dist) {
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const double x = P.xi[it], y = P.yi[it];
            const double r2 = x * x + y * y, tr2 = 2.0 * (x * tx + y * ty);
            const double a = c.k[4] * r2 + c.k[1], b = a * r2 + c.k[0];
            const double icd = 1.0 / (1.0 + b * r2);
            const double ta = (s[8] * r2 + c.k[4] * tr2) + s[5];
            const double tb = (ta * r2 + a * tr2) + s[4];
            const double tc = tb * r2 + b * tr2;
            const double ticd = -((tc * icd) * icd);
            const double xy = x * y, txy = tx * y + x * ty;
            const double ax = r2 + 2.0 * x * x, ay = r2 + 2.0 * y * y;
            const double tax = tr2 + 4.0 * (x * tx), tay = tr2 + 4.0 * (y * ty);
            const double dxx = 2.0 * c.k[2] * x * y + c.k[3] * ax;
            const double dyy = c.k[2] * ay + 2.0 * c.k[3] * x * y;
            const double tdxx = 2.0 * (s[6] * xy + c.k[2] * txy) + (s[7] * ax + c.k[3] * tax);
            const double tdyy = (s[6] * ay + c.k[2] * tay) + 2.0 * (s[7] * xy + c.k[3] * txy);
            tx = (tx0 - tdxx) * icd + (x0 - dxx) * ticd;
            ty = (ty0 - tdyy) * icd + (y0 - dyy) * ticd;
        }
    }
    const double tdu = tx * fx + P.xe * s[0], tdv = ty * fy + P.ye * s[1];
    const double tRr = (P.du * tdu + P.dv * tdv) / P.Rr;
    const double tfa = 0.5 * (s[0] + s[1]);
    const double tkk = (s[15] - P.kk * tfa) / P.fa;
    const double tS = (P.Rr * tRr + P.fa * tfa) / P.S;
    const double tde = tkk * P.S + P.kk * tS;
    const double tq = (tde - P.q * s[18]) / d;
    const double th = tfa * P.q + P.fa * tq;
    const double ta0 = ((th * P.du + P.h * tdu) - P.a0 * s[0]) / fx;
    const double ta1 = ((th * P.dv + P.h * tdv) - P.a1 * s[1]) / fy;
    const double p0 = (ta0 - s[12]) + (P.pc[1] * s[11] - P.pc[2] * s[10]);
    const double p1 = (ta1 - s[13]) + (P.pc[2] * s[9] - P.pc[0] * s[11]);
    const double p2 = (th - s[14]) + (P.pc[0] * s[10] - P.pc[1] * s[9]);
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = c.R[0 * 3 + i] * p0 + c.R[1 * 3 + i] * p1 + c.R[2 * 3 + i] * p2;
}

// the three observation directions: A[r][k] = dX_r / d(Cx, Cy, major)_k
static __device__ __forceinline__ void unc_obs_jac(const CamD& c, const UncPrimal& P, double d, double A[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s[UNC_SEED], t[3];
#pragma unroll
        for (int j = 0; j < UNC_SEED; ++j) s[j] = j == UNC_CAM + k ? 1.0 : 0.0;
        unc_push(c, P, d, s, t);
        A[0][k] = t[0]; A[1][k] = t[1]; A[2][k] = t[2];
    }
}

// column c of the camera factor pushed as one direction: g = J_cam L[:, c]
static __device__ __forceinline__ void unc_cam_push(const CamD& c, const UncPrimal& P, double d, const UncFactor& L, int col, double* g) {
    double s[UNC_SEED];
#pragma unroll
    for (int j = 0; j < UNC_CAM; ++j) s[j] = L.v[col * UNC_CAM + j];
    s[16] = s[17] = s[18] = 0.0;
    unc_push(c, P, d, s, g);
}

// o = xx, xy, xz, yy, yz, zz of A S A', S = (uu, uv, ud, vv, vd, dd): M = A S row by row, then M A', each a sum of three products
// from the left
static __device__ __forceinline__ void unc_obs_cov(const double A[3][3], const double* S6, double* o) {
    const double S[3][3] = {{S6[0], S6[1], S6[2]}, {S6[1], S6[3], S6[4]}, {S6[2], S6[4], S6[5]}};
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[i][k] = A[i][0] * S[0][k] + A[i][1] * S[1][k] + A[i][2] * S[2][k];
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) o[e++] = M[i][0] * A[j][0] + M[i][1] * A[j][1] + M[i][2] * A[j][2];
}

// a table row is usable where it carries VBS_FLAG_XYZ, major >= min_size and the recomputed solve succeeds
static __device__ __forceinline__ bool unc_row(const CamD& c, const float* __restrict__ row, double min_size, UncPrimal& P, double& d) {
    if (!((int)row[0] & VBS_FLAG_XYZ)) return false;
    d = (double)row[3];
    if (!(d >= min_size)) return false;
    double X[3];
    return unc_primal(c, (double)row[1], (double)row[2], d, P, X);
}

// host [16, q] row-major -> columns
static inline UncFactor unc_factor(const double* cam_factor, int q) {
    UncFactor L{};
    for (int c = 0; c < q; ++c)
        for (int k = 0; k < UNC_CAM; ++k) L.v[c * UNC_CAM + k] = cam_factor[k * q + c];
    return L;
}
