// f9: the arithmetic of the planar camera calibration (k_calib.hip), float64 without contraction, next to pnp_math.h whose
// projection, pose Jacobian, pose update, elimination and polar iteration it uses.  Plain C++ on scalars and small fixed arrays;
// tests/helpers/calib_oracle.py repeats every function in NumPy.
#pragma once
#include "pnp_math.h"

#define CALIB_H_SUMS 44            // upper triangle of an 8 x 8 normal matrix (36) and its right-hand side (8)
#define CALIB_H_GN_STEPS 5         // Gauss-Newton steps on the transfer error after the linear homography
#define CALIB_NI 9                 // intrinsic parameters: fx fy cx cy k1 k2 p1 p2 k3
#define CALIB_NA 54                // intrinsic block: upper triangle of 9 x 9 (45) and its gradient (9)
#define CALIB_NB 54                // B_v: 9 x 6, row-major
#define CALIB_NV 81                // per view: B_v (54), upper triangle of C_v (21), g_v (6)
#define CALIB_LAMBDA0 1e-3
#define CALIB_LAMBDA_FAIL 1e10     // a system that no damping up to this factorises is degenerate

#pragma clang fp contract(off)

// index of (p, q), p <= q, in the row-major upper triangle of an n x n matrix
PNP_HD constexpr int calib_tri(int n, int p, int q) { return p * n - (p * (p - 1)) / 2 + (q - p); }

// normal equations of two rows (ju, jv) with right-hand sides (bu, bv): acc = upper triangle (36) then J^T b (8)
PNP_HD void calib_h_accumulate(const double ju[8], const double jv[8], double bu, double bv, double acc[CALIB_H_SUMS]) {
    int q = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = i; j < 8; ++j) { acc[q] = acc[q] + (ju[i] * ju[j] + jv[i] * jv[j]); ++q; }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[36 + i] = acc[36 + i] + (ju[i] * bu + jv[i] * bv);
}

// the two rows of the linear system of one correspondence (X, Y) -> (x, y) with h33 = 1
PNP_HD void calib_h_linear(double X, double Y, double x, double y, double acc[CALIB_H_SUMS]) {
    const double ju[8] = {X, Y, 1.0, 0.0, 0.0, 0.0, -(x * X), -(x * Y)};
    const double jv[8] = {0.0, 0.0, 0.0, X, Y, 1.0, -(y * X), -(y * Y)};
    calib_h_accumulate(ju, jv, x, y, acc);
}

// one correspondence of a Gauss-Newton step on the transfer error of h (h33 = 1)
PNP_HD void calib_h_gauss_newton(const double h[8], double X, double Y, double x, double y, double acc[CALIB_H_SUMS]) {
    const double w = (h[6] * X + h[7] * Y) + 1.0;
    const double iw = 1.0 / w;
    const double u = ((h[0] * X + h[1] * Y) + h[2]) * iw, v = ((h[3] * X + h[4] * Y) + h[5]) * iw;
    const double ju[8] = {X * iw, Y * iw, iw, 0.0, 0.0, 0.0, -(u * X) * iw, -(u * Y) * iw};
    const double jv[8] = {0.0, 0.0, 0.0, X * iw, Y * iw, iw, -(v * X) * iw, -(v * Y) * iw};
    calib_h_accumulate(ju, jv, x - u, y - v, acc);
}

// the summed normal equations -> h (the solution, or the step); false = void (pnp_eliminate8's pivot test)
PNP_HD bool calib_h_solve(const double acc[CALIB_H_SUMS], double h[8]) {
    double A[8][9];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = i; j < 8; ++j) { A[i][j] = acc[q]; A[j][i] = acc[q]; ++q; }
        A[i][8] = acc[36 + i];
    }
    return pnp_eliminate8(A, h, nullptr);
}

// Hartley normalisation from the sums: centre m = sum / n; scale s = sqrt 2 / mean distance from it
PNP_HD double calib_hartley_scale(double dist_sum, double n) { return sqrt(2.0) / (dist_sum / n); }

// Corners that all lie on one line (or coincide) carry no homography although the linear system of a board in general position
// still has its pivots: the scatter (sxx sxy ; sxy syy) of the centred corners must not be singular, to the pivot test's 1e-9
PNP_HD bool calib_scatter_ok(double sxx, double sxy, double syy) { return sxx * syy - sxy * sxy > 1e-9 * (sxx * syy); }

// H = Ti^-1 Hn To with x_n = s (x - m) on both sides, scaled to H[8] = 1.  False when H[8] is not positive (the origin of the
// board behind the camera) or an entry is not finite.
PNP_HD bool calib_h_denormalise(const double hn[8], double mxo, double myo, double so, double mxi, double myi, double si, double H[9]) {
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a = r < 2 ? hn[3 * r] : hn[6], b = r < 2 ? hn[3 * r + 1] : hn[7], c = r < 2 ? hn[3 * r + 2] : 1.0;
        G[3 * r] = a * so; G[3 * r + 1] = b * so; G[3 * r + 2] = c - (a * (so * mxo) + b * (so * myo));
    }
    const double isi = 1.0 / si;
    double F[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        F[j] = G[j] * isi + mxi * G[6 + j];
        F[3 + j] = G[3 + j] * isi + myi * G[6 + j];
        F[6 + j] = G[6 + j];
    }
    bool ok = F[8] > 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { H[i] = F[i] / F[8]; ok = ok && isfinite(H[i]); }
    return ok;
}

// cv2's initial focal lengths of a planar target (cvInitIntrinsicParams2D, recalled): the two rows one view adds to the
// least-squares system in (a, b) = (1 / fx^2, 1 / fy^2), summed as 2 x 2 normal equations m = (m00 m01 m11 r0 r1)
PNP_HD void calib_init_rows(const double H[9], double cx, double cy, double m[5]) {
    double h[3], v[3], d1[3], d2[3];
    h[0] = H[0] - cx * H[6]; h[1] = H[3] - cy * H[6]; h[2] = H[6];
    v[0] = H[1] - cx * H[7]; v[1] = H[4] - cy * H[7]; v[2] = H[7];
    double nh = 0.0, nv = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d1[j] = (h[j] + v[j]) * 0.5; d2[j] = (h[j] - v[j]) * 0.5;
        nh = nh + h[j] * h[j]; nv = nv + v[j] * v[j]; n1 = n1 + d1[j] * d1[j]; n2 = n2 + d2[j] * d2[j];
    }
    nh = 1.0 / sqrt(nh); nv = 1.0 / sqrt(nv); n1 = 1.0 / sqrt(n1); n2 = 1.0 / sqrt(n2);
#pragma unroll
    for (int j = 0; j < 3; ++j) { h[j] = h[j] * nh; v[j] = v[j] * nv; d1[j] = d1[j] * n1; d2[j] = d2[j] * n2; }
    const double a0 = h[0] * v[0], b0 = h[1] * v[1], c0 = -(h[2] * v[2]);
    const double a1 = d1[0] * d2[0], b1 = d1[1] * d2[1], c1 = -(d1[2] * d2[2]);
    m[0] = m[0] + (a0 * a0 + a1 * a1); m[1] = m[1] + (a0 * b0 + a1 * b1); m[2] = m[2] + (b0 * b0 + b1 * b1);
    m[3] = m[3] + (a0 * c0 + a1 * c1); m[4] = m[4] + (b0 * c0 + b1 * c1);
}

// (fx, fy) from the summed rows; false when the 2 x 2 system is singular (determinant below 1e-9 of m00 m11: every view
// fronto-parallel) or a or b is not positive and finite
PNP_HD bool calib_init_focal(const double m[5], double* fx, double* fy) {
    const double det = m[0] * m[2] - m[1] * m[1];
    if (!(det > 1e-9 * (m[0] * m[2]))) return false;
    const double a = (m[3] * m[2] - m[1] * m[4]) / det, b = (m[0] * m[4] - m[1] * m[3]) / det;
    if (!(a > 0.0) || !(b > 0.0) || !isfinite(a) || !isfinite(b)) return false;
    *fx = sqrt(fabs(1.0 / a)); *fy = sqrt(fabs(1.0 / b));
    return isfinite(*fx) && isfinite(*fy);
}

// the pose of one view from its homography: K^-1 H scaled by the mean norm of its first two columns, (r1 r2 r1 x r2) to the
// nearest rotation.  False when the polar iteration fails or the board is not in front (t_z <= 0).
PNP_HD bool calib_init_pose(const double H[9], double fx, double fy, double cx, double cy, double R[9], double t[3]) {
    double M[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        M[j] = (H[j] - cx * H[6 + j]) / fx;
        M[3 + j] = (H[3 + j] - cy * H[6 + j]) / fy;
        M[6 + j] = H[6 + j];
    }
    const double n1 = sqrt((M[0] * M[0] + M[3] * M[3]) + M[6] * M[6]);
    const double n2 = sqrt((M[1] * M[1] + M[4] * M[4]) + M[7] * M[7]);
    double sc = 0.5 * (n1 + n2);
    if (!(sc > 0.0)) return false;
    sc = 1.0 / sc;
    t[0] = M[2] * sc; t[1] = M[5] * sc; t[2] = M[8] * sc;
    M[0] = M[0] * sc; M[3] = M[3] * sc; M[6] = M[6] * sc;
    M[1] = M[1] * sc; M[4] = M[4] * sc; M[7] = M[7] * sc;
    M[2] = M[3] * M[7] - M[6] * M[4];
    M[5] = M[6] * M[1] - M[0] * M[7];
    M[8] = M[0] * M[4] - M[3] * M[1];
    if (!pnp_polar(M)) return false;
    bool ok = t[2] > 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = M[i]; ok = ok && isfinite(M[i]); }
    return ok && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
}

// d(u, v) / d(fx, fy, cx, cy, k1, k2, p1, p2, k3) of one board point (Z = 0), analytic; the pose columns are pnp_pixel_jacobian's
PNP_HD void calib_intrinsic_columns(const PnpCam& c, const double R[9], const double t[3], double X, double Y, double Iu[CALIB_NI],
                                    double Iv[CALIB_NI]) {
    double Pc[3];
    pnp_to_camera(R, t, X, Y, 0.0, Pc);
    const double x = Pc[0] / Pc[2], y = Pc[1] / Pc[2];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
    const double rad = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xd = (x * rad + 2.0 * c.p1 * xy) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * rad + c.p1 * (r2 + 2.0 * y2)) + 2.0 * c.p2 * xy;
    const double r4 = r2 * r2, r6 = r4 * r2;
    Iu[0] = xd; Iu[1] = 0.0; Iu[2] = 1.0; Iu[3] = 0.0;
    Iu[4] = c.fx * (x * r2); Iu[5] = c.fx * (x * r4); Iu[6] = c.fx * (2.0 * xy); Iu[7] = c.fx * (r2 + 2.0 * x2); Iu[8] = c.fx * (x * r6);
    Iv[0] = 0.0; Iv[1] = yd; Iv[2] = 0.0; Iv[3] = 1.0;
    Iv[4] = c.fy * (y * r2); Iv[5] = c.fy * (y * r4); Iv[6] = c.fy * (r2 + 2.0 * y2); Iv[7] = c.fy * (2.0 * xy); Iv[8] = c.fy * (y * r6);
}

// one point's share of the block-arrow normal equations, in two parts so that their sums need not be live together:
// accA = the intrinsic block (45 + 9); accV = the view's B_v (54), C_v (21), g_v (6)
PNP_HD void calib_accumulate_intrinsic(const double Iu[CALIB_NI], const double Iv[CALIB_NI], double ru, double rv, double accA[CALIB_NA]) {
    int q = 0;
#pragma unroll
    for (int i = 0; i < CALIB_NI; ++i)
#pragma unroll
        for (int j = i; j < CALIB_NI; ++j) { accA[q] = accA[q] + (Iu[i] * Iu[j] + Iv[i] * Iv[j]); ++q; }
#pragma unroll
    for (int i = 0; i < CALIB_NI; ++i) accA[45 + i] = accA[45 + i] + (Iu[i] * ru + Iv[i] * rv);
}

PNP_HD void calib_accumulate_view(const double Iu[CALIB_NI], const double Iv[CALIB_NI], const double Pu[6], const double Pv[6], double ru,
                                  double rv, double accV[CALIB_NV]) {
#pragma unroll
    for (int i = 0; i < CALIB_NI; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) accV[6 * i + j] = accV[6 * i + j] + (Iu[i] * Pu[j] + Iv[i] * Pv[j]);
    pnp_accumulate(Pu, Pv, ru, rv, accV + CALIB_NB, accV + CALIB_NB + 21);
}

// (C + lambda diag C)^-1 of a view's 6 x 6 block (upper triangles, 21) by Cholesky; false when a pivot is not positive
PNP_HD bool calib_inverse6(const double C[21], double lambda, double Ci[21]) {
    double M[6][6], Lm[6][6], Li[6][6];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { M[i][j] = C[q]; M[j][i] = C[q]; ++q; }
#pragma unroll
    for (int i = 0; i < 6; ++i) M[i][i] = M[i][i] + lambda * M[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - Lm[j][k] * Lm[j][k];
        if (!(s > 0.0)) { ok = false; s = 1.0; }
        const double ljj = sqrt(s);
        Lm[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - Lm[i][k] * Lm[j][k];
            Lm[i][j] = v / ljj;
        }
    }
    // Li = L^-1 (lower), column by column
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        Li[j][j] = 1.0 / Lm[j][j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) v = v - Lm[i][k] * Li[k][j];
            Li[i][j] = v / Lm[i][i];
        }
    }
    q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < 6; ++k) v = v + Li[k][i] * Li[k][j];
            Ci[q] = v; ++q;
        }
    return ok;
}

// b^T Ci c for a symmetric 6 x 6 Ci given by its upper triangle
PNP_HD double calib_quad6(const double* b, const double* Ci, const double* c) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) w = w + Ci[p <= q ? calib_tri(6, p, q) : calib_tri(6, q, p)] * c[q];
        s = s + b[p] * w;
    }
    return s;
}

// Entry e of the Schur complement of the pose blocks over `nact` views, summed in view order.  e < 45: entry (i, j) of
// S = A_lambda - sum B_v Ci_v B_v^T (upper triangle); e >= 45: component e - 45 of gA - sum B_v Ci_v g_v.
// blk = per view B (54), C (21), g (6); ci = per view Ci (21).
PNP_HD double calib_schur_entry(int e, const double* A, double lambda, const double* blk, const double* ci, int nact) {
    int i = 0, j = 0;
    if (e < 45) {
        int rest = e;
        while (rest >= CALIB_NI - i) { rest -= CALIB_NI - i; ++i; }
        j = i + rest;
    } else {
        i = e - 45;
    }
    double s = A[e];
    if (e < 45 && i == j) s = s + lambda * s;
    for (int a = 0; a < nact; ++a) {
        const double* B = blk + a * CALIB_NV;
        const double* c = e < 45 ? B + 6 * j : B + CALIB_NB + 21;
        s = s - calib_quad6(B + 6 * i, ci + a * 21, c);
    }
    return s;
}

// S dA = -rhs by Cholesky for the 9 x 9 Schur system; S = upper triangle (45) then rhs (9); inv_diag (may be null) = diag S^-1.
// False when a pivot is not positive.  Loops over memory, not registers: the factors live in the caller's work array W[CALIB_SOLVE9_WORK] (LDS on the device), so that nothing goes to scratch.
#define CALIB_SOLVE9_WORK (2 * CALIB_NI * CALIB_NI + CALIB_NI)
PNP_HD bool calib_solve9(const double* S, double* dA, double* inv_diag, double* W) {
    double (*Lm)[CALIB_NI] = (double (*)[CALIB_NI])W;
    double (*Li)[CALIB_NI] = (double (*)[CALIB_NI])(W + CALIB_NI * CALIB_NI);
    double* y = W + 2 * CALIB_NI * CALIB_NI;
    bool ok = true;
    for (int j = 0; j < CALIB_NI; ++j) {
        double s = S[calib_tri(CALIB_NI, j, j)];
        for (int k = 0; k < j; ++k) s = s - Lm[j][k] * Lm[j][k];
        if (!(s > 0.0)) { ok = false; s = 1.0; }
        const double ljj = sqrt(s);
        Lm[j][j] = ljj;
        for (int i = j + 1; i < CALIB_NI; ++i) {
            double v = S[calib_tri(CALIB_NI, j, i)];
            for (int k = 0; k < j; ++k) v = v - Lm[i][k] * Lm[j][k];
            Lm[i][j] = v / ljj;
        }
    }
    for (int i = 0; i < CALIB_NI; ++i) {
        double v = -S[45 + i];
        for (int k = 0; k < i; ++k) v = v - Lm[i][k] * y[k];
        y[i] = v / Lm[i][i];
    }
    for (int i = CALIB_NI - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < CALIB_NI; ++k) v = v - Lm[k][i] * dA[k];
        dA[i] = v / Lm[i][i];
    }
    if (inv_diag) {
        for (int j = 0; j < CALIB_NI; ++j) {
            Li[j][j] = 1.0 / Lm[j][j];
            for (int i = j + 1; i < CALIB_NI; ++i) {
                double v = 0.0;
                for (int k = j; k < i; ++k) v = v - Lm[i][k] * Li[k][j];
                Li[i][j] = v / Lm[i][i];
            }
        }
        for (int i = 0; i < CALIB_NI; ++i) {
            double v = 0.0;
            for (int k = i; k < CALIB_NI; ++k) v = v + Li[k][i] * Li[k][i];
            inv_diag[i] = v;
        }
    }
    return ok;
}

// pnp_apply_step with the Rodrigues coefficients a = sin th / th, b = (1 - cos th) / th^2 from their series in th^2, in plain
// arithmetic (12 terms by Horner: below 1e-21 at th = 1): the maths library's sin / cos differ between host and device in the
// last place, and with them would the whole path of the fit - the helper could not follow it step for step.  A step beyond
// 1 rad, which a converging fit does not take, uses the library.
PNP_HD void calib_apply_step(const double d[6], double R[9], double t[3]) {
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double a, b;
    if (th2 <= 1.0) {
        double sa = 1.0, sb = 1.0;
#pragma unroll
        for (int k = 12; k >= 1; --k) {
            sa = 1.0 - th2 / (double)((2 * k) * (2 * k + 1)) * sa;
            sb = 1.0 - th2 / (double)((2 * k + 1) * (2 * k + 2)) * sb;
        }
        a = sa; b = 0.5 * sb;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th; b = (1.0 - cos(th)) / th2;
    }
    pnp_apply_rotation(d, th2, a, b, R, t);
}

// the pose step of one view after the intrinsic step: d = -Ci (g + B^T dA)
PNP_HD void calib_back_substitute(const double* B, const double* g, const double* Ci, const double* dA, double d[6]) {
    double r[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double v = g[p];
#pragma unroll
        for (int i = 0; i < CALIB_NI; ++i) v = v + B[6 * i + p] * dA[i];
        r[p] = v;
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) w = w + Ci[p <= q ? calib_tri(6, p, q) : calib_tri(6, q, p)] * r[q];
        d[p] = -w;
    }
}

#pragma clang fp contract(fast)
