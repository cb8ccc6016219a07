// f7: the per-hypothesis and per-point arithmetic of the PnP RANSAC (k_pnp.hip), float64 without contraction.  Every function is
// plain C++ on scalars and small fixed arrays whose indices are compile-time constants after unrolling, so that they live in
// registers on the device; tests/helpers/pnp_oracle.py repeats them operation for operation in NumPy.
#pragma once
#include <math.h>

#ifndef PNP_HD
#define PNP_HD __host__ __device__ __forceinline__
#endif

#define PNP_SAMPLE 6               // correspondences per hypothesis: 4 for the homography, all 6 for the Gauss-Newton steps
#define PNP_GN_STEPS 10
#define PNP_POLAR_STEPS 8
#define PNP_LM_STEPS 20            // as SOLVEPNP_ITERATIVE
#define PNP_LM_EPS 1e-11           // largest |component| of a step (rad, mm) below which the refit stops

#pragma clang fp contract(off)

struct PnpCam { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };

// E = I + a [w]x + b [w]x^2 left-multiplied onto (R, t): R <- E R, t <- E t + dt.  th2 = |w|^2; a, b = the Rodrigues coefficients
PNP_HD void pnp_apply_rotation(const double d[6], double th2, double a, double b, double R[9], double t[3]) {
    const double wx = d[0], wy = d[1], wz = d[2];
    // E = I + a [w]x + b [w]x^2,   [w]x^2 = w w^T - th2 I
    double E[9];
    E[0] = 1.0 + b * (wx * wx - th2); E[1] = b * (wx * wy) - a * wz;    E[2] = b * (wx * wz) + a * wy;
    E[3] = b * (wx * wy) + a * wz;    E[4] = 1.0 + b * (wy * wy - th2); E[5] = b * (wy * wz) - a * wx;
    E[6] = b * (wx * wz) - a * wy;    E[7] = b * (wy * wz) + a * wx;    E[8] = 1.0 + b * (wz * wz - th2);
    double Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
        tn[i] = ((E[3 * i] * t[0] + E[3 * i + 1] * t[1]) + E[3 * i + 2] * t[2]) + d[3 + i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tn[i];
}

// Rodrigues matrix of w, left-multiplied onto (R, t): R <- E R, t <- E t + dt
PNP_HD void pnp_apply_step(const double d[6], double R[9], double t[3]) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th2 = wx * wx + wy * wy + wz * wz;
    const double th = sqrt(th2);
    double a = 1.0, b = 0.5;
    if (th > 1e-12) { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    pnp_apply_rotation(d, th2, a, b, R, t);
}

PNP_HD void pnp_to_camera(const double R[9], const double t[3], double X, double Y, double Z, double Pc[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) Pc[i] = ((R[3 * i] * X + R[3 * i + 1] * Y) + R[3 * i + 2] * Z) + t[i];
}

// forward Brown-Conrady model to pixels (k1, k2, p1, p2, k3); false behind the camera
PNP_HD bool pnp_project(const PnpCam& c, const double R[9], const double t[3], double X, double Y, double Z, double* u, double* v) {
    double Pc[3];
    pnp_to_camera(R, t, X, Y, Z, Pc);
    if (!(Pc[2] > 0.0)) return false;
    const double x = Pc[0] / Pc[2], y = Pc[1] / Pc[2];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
    const double rad = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xd = (x * rad + 2.0 * c.p1 * xy) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * rad + c.p1 * (r2 + 2.0 * y2)) + 2.0 * c.p2 * xy;
    *u = c.fx * xd + c.cx;
    *v = c.fy * yd + c.cy;
    return true;
}

// squared pixel error of one correspondence; a point behind the camera is infinitely far off
PNP_HD double pnp_err2(const PnpCam& c, const double R[9], const double t[3], double X, double Y, double Z, double uo, double vo) {
    double u, v;
    if (!pnp_project(c, R, t, X, Y, Z, &u, &v)) return INFINITY;
    const double du = u - uo, dv = v - vo;
    return du * du + dv * dv;
}

// Upper triangle (row-major, 21) of a 6 x 6 normal matrix and its right-hand side from one 2 x 6 Jacobian block
PNP_HD void pnp_accumulate(const double Ju[6], const double Jv[6], double ru, double rv, double A[21], double g[6]) {
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) { A[q] = A[q] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]); ++q; }
        g[i] = g[i] + (Ju[i] * ru + Jv[i] * rv);
    }
}

// (A + lambda diag A) d = -g by Cholesky; false when a pivot is not positive
PNP_HD bool pnp_solve6(const double A[21], const double g[6], double lambda, double d[6]) {
    double M[6][6], Lm[6][6];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { M[i][j] = A[q]; M[j][i] = A[q]; ++q; }
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
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - Lm[i][k] * y[k];
        y[i] = v / Lm[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - Lm[k][i] * d[k];
        d[i] = v / Lm[i][i];
    }
    return ok;
}

// d(Pc)/d(step) = [ -[Pc]x | I ] behind a 2 x 3 block (ax ay az ; bx by bz): the two Jacobian rows
PNP_HD void pnp_chain(const double Pc[3], double ax, double ay, double az, double bx, double by, double bz, double Ju[6], double Jv[6]) {
    Ju[0] = ay * -Pc[2] + az * Pc[1];  Ju[1] = ax * Pc[2] + az * -Pc[0];  Ju[2] = ax * -Pc[1] + ay * Pc[0];
    Ju[3] = ax; Ju[4] = ay; Ju[5] = az;
    Jv[0] = by * -Pc[2] + bz * Pc[1];  Jv[1] = bx * Pc[2] + bz * -Pc[0];  Jv[2] = bx * -Pc[1] + by * Pc[0];
    Jv[3] = bx; Jv[4] = by; Jv[5] = bz;
}

// One correspondence of the pixel-error refit: residual and analytic Jacobian through the distortion model.  False behind the camera.
PNP_HD bool pnp_pixel_jacobian(const PnpCam& c, const double R[9], const double t[3], double X, double Y, double Z, double uo, double vo,
                               double Ju[6], double Jv[6], double* ru, double* rv) {
    double Pc[3];
    pnp_to_camera(R, t, X, Y, Z, Pc);
    if (!(Pc[2] > 0.0)) return false;
    const double iz = 1.0 / Pc[2];
    const double x = Pc[0] / Pc[2], y = Pc[1] / Pc[2];
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
    const double rad = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double drad = (3.0 * c.k3 * r2 + 2.0 * c.k2) * r2 + c.k1;
    const double xd = (x * rad + 2.0 * c.p1 * xy) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * rad + c.p1 * (r2 + 2.0 * y2)) + 2.0 * c.p2 * xy;
    *ru = (c.fx * xd + c.cx) - uo;
    *rv = (c.fy * yd + c.cy) - vo;
    // d(xd, yd) / d(x, y), scaled to pixels
    const double dxx = c.fx * (((rad + 2.0 * x2 * drad) + 2.0 * c.p1 * y) + 6.0 * c.p2 * x);
    const double dxy = c.fx * ((2.0 * xy * drad + 2.0 * c.p1 * x) + 2.0 * c.p2 * y);
    const double dyx = c.fy * ((2.0 * xy * drad + 2.0 * c.p1 * x) + 2.0 * c.p2 * y);
    const double dyy = c.fy * (((rad + 2.0 * y2 * drad) + 6.0 * c.p1 * y) + 2.0 * c.p2 * x);
    // d(x, y) / d(Pc) = (iz 0 -x iz ; 0 iz -y iz)
    const double ax = dxx * iz, ay = dxy * iz, az = -(dxx * x + dxy * y) * iz;
    const double bx = dyx * iz, by = dyy * iz, bz = -(dyx * x + dyy * y) * iz;
    pnp_chain(Pc, ax, ay, az, bx, by, bz, Ju, Jv);
    return true;
}

// A h = A[.][8] for the 8 x 9 augmented system A (destroyed): Gaussian elimination with partial pivoting.  False = void: a pivot
// below 1e-9 of the largest |entry|.  *cond (may be null) = smallest |pivot| over the largest |entry|.
PNP_HD bool pnp_eliminate8(double A[8][9], double h[8], double* cond) {
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fabs(A[i][j]) > amax ? fabs(A[i][j]) : amax;
    double pmin = INFINITY;
    // Gaussian elimination with partial pivoting; the row exchange is a chain of predicated swaps so that no index is dynamic
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int piv = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int r = k + 1; r < 8; ++r)
            if (fabs(A[r][k]) > best) { best = fabs(A[r][k]); piv = r; }
#pragma unroll
        for (int r = k + 1; r < 8; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int j = k; j < 9; ++j) {
                const double a = A[k][j], b = A[r][j];
                A[k][j] = sw ? b : a;
                A[r][j] = sw ? a : b;
            }
        }
        pmin = best < pmin ? best : pmin;
        const double pv = best > 0.0 ? A[k][k] : 1.0;
#pragma unroll
        for (int r = k + 1; r < 8; ++r) {
            const double f = A[r][k] / pv;
#pragma unroll
            for (int j = k + 1; j < 9; ++j) A[r][j] = A[r][j] - f * A[k][j];
        }
    }
    if (cond) *cond = pmin / amax;
    if (!(pmin > 1e-9 * amax)) return false;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double v = A[i][8];
#pragma unroll
        for (int j = i + 1; j < 8; ++j) v = v - A[i][j] * h[j];
        h[i] = v / A[i][i];
    }
    return true;
}

// M <- the nearest rotation = its polar factor, by Newton's iteration M <- (M + M^-T) / 2; false when M loses its orientation
PNP_HD bool pnp_polar(double M[9]) {
    bool ok = true;
#pragma unroll 1
    for (int it = 0; it < PNP_POLAR_STEPS; ++it) {
        double C[9];
        C[0] = M[4] * M[8] - M[5] * M[7]; C[1] = M[5] * M[6] - M[3] * M[8]; C[2] = M[3] * M[7] - M[4] * M[6];
        C[3] = M[2] * M[7] - M[1] * M[8]; C[4] = M[0] * M[8] - M[2] * M[6]; C[5] = M[1] * M[6] - M[0] * M[7];
        C[6] = M[1] * M[5] - M[2] * M[4]; C[7] = M[2] * M[3] - M[0] * M[5]; C[8] = M[0] * M[4] - M[1] * M[3];
        const double det = (M[0] * C[0] + M[1] * C[1]) + M[2] * C[2];
        if (!(det > 1e-12)) { ok = false; break; }
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = 0.5 * (M[i] + C[i] / det);
    }
    return ok;
}

// The minimal solver of one hypothesis.  W = world [n][3], (xn, yn) = normalised image points, s = the 6 sample indices
// (distinct, valid).  Planar homography of the first four (Z ignored) -> pose -> PNP_GN_STEPS Gauss-Newton steps on all six with
// their true Z, residuals in normalised coordinates.  False = void.  *cond (may be null) = smallest |pivot| of the 8 x 8
// elimination over the largest |entry| of the system: what the test helper rates the conditioning by.
PNP_HD bool pnp_minimal(const double* W, const double* xn, const double* yn, const int s[PNP_SAMPLE], double R[9], double t[3],
                        double* cond) {
    double A[8][9];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double X = W[3 * s[p]], Y = W[3 * s[p] + 1], x = xn[s[p]], y = yn[s[p]];
        A[2 * p][0] = X; A[2 * p][1] = Y; A[2 * p][2] = 1.0; A[2 * p][3] = 0.0; A[2 * p][4] = 0.0; A[2 * p][5] = 0.0;
        A[2 * p][6] = -(x * X); A[2 * p][7] = -(x * Y); A[2 * p][8] = x;
        A[2 * p + 1][0] = 0.0; A[2 * p + 1][1] = 0.0; A[2 * p + 1][2] = 0.0; A[2 * p + 1][3] = X; A[2 * p + 1][4] = Y; A[2 * p + 1][5] = 1.0;
        A[2 * p + 1][6] = -(y * X); A[2 * p + 1][7] = -(y * Y); A[2 * p + 1][8] = y;
    }
    double h[8];
    if (!pnp_eliminate8(A, h, cond)) return false;
    // H = (h0 h1 h2 ; h3 h4 h5 ; h6 h7 1) ~ (r1 r2 t)
    const double n1 = sqrt((h[0] * h[0] + h[3] * h[3]) + h[6] * h[6]);
    const double n2 = sqrt((h[1] * h[1] + h[4] * h[4]) + h[7] * h[7]);
    double sc = 0.5 * (n1 + n2);
    if (!(sc > 0.0)) return false;
    sc = 1.0 / sc;                                       // t_z = sc: positive, the board is in front (h33 = +1)
    double M[9];
    M[0] = h[0] * sc; M[3] = h[3] * sc; M[6] = h[6] * sc;
    M[1] = h[1] * sc; M[4] = h[4] * sc; M[7] = h[7] * sc;
    t[0] = h[2] * sc; t[1] = h[5] * sc; t[2] = sc;
    M[2] = M[3] * M[7] - M[6] * M[4];
    M[5] = M[6] * M[1] - M[0] * M[7];
    M[8] = M[0] * M[4] - M[3] * M[1];
    if (!pnp_polar(M)) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = M[i];
#pragma unroll 1
    for (int it = 0; it < PNP_GN_STEPS; ++it) {
        double N[21], g[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) N[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = 0.0;
#pragma unroll
        for (int p = 0; p < PNP_SAMPLE; ++p) {
            double Pc[3], Ju[6], Jv[6];
            pnp_to_camera(R, t, W[3 * s[p]], W[3 * s[p] + 1], W[3 * s[p] + 2], Pc);
            if (!(Pc[2] > 0.0)) { ok = false; break; }
            const double iz = 1.0 / Pc[2];
            const double x = Pc[0] / Pc[2], y = Pc[1] / Pc[2];
            pnp_chain(Pc, iz, 0.0, -(x * iz), 0.0, iz, -(y * iz), Ju, Jv);
            pnp_accumulate(Ju, Jv, x - xn[s[p]], y - yn[s[p]], N, g);
        }
        if (!ok) break;
        double d[6];
        if (!pnp_solve6(N, g, 0.0, d)) { ok = false; break; }
        pnp_apply_step(d, R, t);
    }
    if (!ok) return false;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fin = fin && isfinite(t[i]);
    return fin;
}

#pragma clang fp contract(fast)
