// Noise-weighted rigid motion along a recording: for every frame the maximum-likelihood pose of
//     P_i ~ R (Q_i - qm) + c        under        S_i = Sigma_P,i + R Sigma_Q,i R',
// started at the pose vbs_rigid_series left, by a fixed number of Gauss-Newton steps on (omega, c) with R <- exp([omega]x) R taken
// through the quaternion (1, omega / 2) / |.| - no sine or cosine anywhere -, the covariance (J' W J)^-1 of that pose, chi^2 and the
// Mahalanobis distance of every marker.  Float64 without contraction, + - * / and sqrt only (but the four angle columns), no
// atomics, no LDS, no barrier; the operand order of every expression is stated in include/vbs.h and restated in
// tests/helpers/rigid_ml_oracle.py.
//   k_rigid_ml   one wave per frame, VBS_RIGID_ML_GROUP frames a workgroup.  A wave reads its inputs directly and meets no barrier,
//                so a frame's result cannot depend on the frames next to it.  ONE sweep over the slots serves every iteration, the
//                sweep at the final pose and the sweep at the start of a frame that stops early (the loop around it stays rolled): a
//                lane keeps 28 running sums - the 21 upper entries of A = sum J' W J as N [6], M [9], W [6], the 6 of g and chi^2 -
//                which fold through wave_sum.  The 3 x 3 of a slot and the 6 x 6 of a frame are the LDL' of fit_math.h, every lane
//                alike over constant indices, so they live in registers (profiles/rigid_ml_resource_usage.txt).
#include "common.h"
#include "fit_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define RML_WAVES VBS_RIGID_ML_GROUP
static_assert(RML_WAVES >= 1 && RML_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_RIGID_ML_COLS == 40, "flag, n_start, n_used, iters, w x y z, R [9], t [3], c [3], qm [3], chi2, dof, chi2_start, "
                                       "step_rot, step_c, four angles, Sigma_n [3], t2_tilt, var_twist");
static_assert(VBS_RIGID_COLS == 33, "the start record is a row of vbs_rigid_series");

// R row-major from the unit quaternion: the expressions of vbs_rigid_series, so the start's R is the record's to the bit
static __device__ __forceinline__ void rml_rotation(const double* qt, double* R) {
    const double w = qt[0], x = qt[1], y = qt[2], z = qt[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// the largest of |a|, |b|, |c| by comparisons (a NaN never wins)
static __device__ __forceinline__ double rml_maxabs(double a, double b, double c) {
    double s = fabs(a);
    if (fabs(b) > s) s = fabs(b);
    if (fabs(c) > s) s = fabs(c);
    return s;
}

// x = S^-1 v from the factors of S: the forward and the back substitution of fit_math.h
static __device__ __forceinline__ void rml_solve3(const double (&Lm)[3][3], const double (&d)[3], const double* v, double* x) {
    double y[3];
    ldl_forward<3>(Lm, d, v, 3, y);
    ldl_back<3, 3>(Lm, y, x);
}

__global__ __launch_bounds__(RML_WAVES * 64) void k_rigid_ml(const float* __restrict__ table, int m, const double* __restrict__ source,
                                                             const double* __restrict__ cov, const double* __restrict__ start,
                                                             const double* __restrict__ residual,
                                                             const double* __restrict__ source_cov, int iters, double piv_rel,
                                                             int frame_begin, int n_frames, double* __restrict__ ml,
                                                             double* __restrict__ pcov, double* __restrict__ coef,
                                                             double* __restrict__ mahal) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * RML_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                  // (a whole wave: no barrier follows)
    const float* frow = table + ((int64_t)frame_begin + fi) * ((int64_t)m * VBS_TABLE_COLS);
    const double* crow = cov + fi * ((int64_t)m * VBS_UNCERT_COV_COLS);
    const double* rrow = residual + fi * ((int64_t)m * 4);
    const double* st = start + fi * VBS_RIGID_COLS;
    double* mrow = mahal ? mahal + fi * ((int64_t)m * 3) : nullptr;

    const bool have = st[0] != 0.0;                              // (nothing else of a row without a fit is read)
    double q0[4] = {0.0, 0.0, 0.0, 0.0}, qm[3] = {0.0, 0.0, 0.0}, c0[3] = {0.0, 0.0, 0.0};
    double quat[4] = {0.0, 0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    if (have) {
#pragma unroll
        for (int k = 0; k < 4; ++k) quat[k] = q0[k] = st[9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) qm[k] = st[3 + k];
        rml_rotation(quat, R);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = c0[i] = ((R[i * 3] * qm[0] + R[i * 3 + 1] * qm[1]) + R[i * 3 + 2] * qm[2]) + st[22 + i];
    }

    int flag = have ? 2 : 0, n_start = 0, n_used = 0, it = 0;
    bool stopped = !have;                                        // the sweep runs at the start and is the last
    double A[6][6], Lm[6][6], dg[6], chi2 = 0.0, chi2_start = 0.0, step_rot = 0.0, step_c = 0.0;
    double C[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) C[k] = 0.0;

#pragma unroll 1
    for (;;) {                                                   // (every test below is wave-uniform: the sums are broadcast)
        const bool last = stopped || it == iters;
        const bool first = it == 0 && !stopped;
        // ---- the sweep at (R, c) ------------------------------------------------------------------------------------------------
        double aN[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, aM[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double aW[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ag[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ac = 0.0;
        int cs = 0, cu = 0;
        for (int slot = lane; slot < m; slot += 64) {
            double dist = 0.0;
            bool in = false;
            const bool begun = have && rrow[(int64_t)slot * 4] != 0.0;
            if (begun) ++cs;
            const double* cp = crow + (int64_t)slot * VBS_UNCERT_COV_COLS;
            const double* cq = source_cov ? source_cov + (int64_t)slot * VBS_UNCERT_COV_COLS : nullptr;
            if (begun && cp[0] != 0.0 && (!cq || cq[0] != 0.0)) {
                double S[3][3];
                S[0][0] = cp[1]; S[0][1] = S[1][0] = cp[2]; S[0][2] = S[2][0] = cp[3];
                S[1][1] = cp[4]; S[1][2] = S[2][1] = cp[5]; S[2][2] = cp[6];
                if (cq) {                                        // S = Sigma_P + (R Sigma_Q) R'
                    const double G[3][3] = {{cq[1], cq[2], cq[3]}, {cq[2], cq[4], cq[5]}, {cq[3], cq[5], cq[6]}};
                    double T[3][3];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) T[i][j] = (R[i * 3] * G[0][j] + R[i * 3 + 1] * G[1][j]) + R[i * 3 + 2] * G[2][j];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = i; j < 3; ++j) {
                            const double rs = (T[i][0] * R[j * 3] + T[i][1] * R[j * 3 + 1]) + T[i][2] * R[j * 3 + 2];
                            S[i][j] = S[i][j] + rs;
                            S[j][i] = S[i][j];
                        }
                }
                double L3[3][3], d3[3];
                if (ldl_factor<3>(S, piv_rel, L3, d3) == 3) {
                    in = true;
                    ++cu;
                    const double* sr = source + (int64_t)slot * 4;
                    const float* tr = frow + (int64_t)slot * VBS_TABLE_COLS;
                    const double dq[3] = {sr[1] - qm[0], sr[2] - qm[1], sr[3] - qm[2]};
                    double y[3], e[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        y[i] = (R[i * 3] * dq[0] + R[i * 3 + 1] * dq[1]) + R[i * 3 + 2] * dq[2];
                        e[i] = (double)tr[6 + i] - (y[i] + c[i]);
                    }
                    // W = S^-1 column by column; the upper triangle is read, W[i][j] with i <= j from column j
                    double W[3][3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double unit[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
                        double x[3];
                        rml_solve3(L3, d3, unit, x);
#pragma unroll
                        for (int i = 0; i <= j; ++i) { W[i][j] = x[i]; W[j][i] = x[i]; }
                    }
                    double u[3], M[3][3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        u[i] = (W[i][0] * e[0] + W[i][1] * e[1]) + W[i][2] * e[2];
                        M[i][0] = W[i][2] * y[1] - W[i][1] * y[2];   // M = W B, B = -[y]x
                        M[i][1] = W[i][0] * y[2] - W[i][2] * y[0];
                        M[i][2] = W[i][1] * y[0] - W[i][0] * y[1];
                    }
                    dist = (e[0] * u[0] + e[1] * u[1]) + e[2] * u[2];
                    ac = ac + dist;
                    // N = B' M, upper
                    aN[0] = aN[0] + (M[2][0] * y[1] - M[1][0] * y[2]);
                    aN[1] = aN[1] + (M[2][1] * y[1] - M[1][1] * y[2]);
                    aN[2] = aN[2] + (M[2][2] * y[1] - M[1][2] * y[2]);
                    aN[3] = aN[3] + (M[0][1] * y[2] - M[2][1] * y[0]);
                    aN[4] = aN[4] + (M[0][2] * y[2] - M[2][2] * y[0]);
                    aN[5] = aN[5] + (M[1][2] * y[0] - M[0][2] * y[1]);
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) aM[i * 3 + j] = aM[i * 3 + j] + M[i][j];
                    aW[0] = aW[0] + W[0][0]; aW[1] = aW[1] + W[0][1]; aW[2] = aW[2] + W[0][2];
                    aW[3] = aW[3] + W[1][1]; aW[4] = aW[4] + W[1][2]; aW[5] = aW[5] + W[2][2];
                    ag[0] = ag[0] + (u[2] * y[1] - u[1] * y[2]);
                    ag[1] = ag[1] + (u[0] * y[2] - u[2] * y[0]);
                    ag[2] = ag[2] + (u[1] * y[0] - u[0] * y[1]);
                    ag[3] = ag[3] + u[0]; ag[4] = ag[4] + u[1]; ag[5] = ag[5] + u[2];
                }
            }
            if (mrow) {
                double* o = mrow + (int64_t)slot * 3;
                if (first) o[2] = dist;                          // (the same lane rewrites the row in the last sweep)
                if (last) {
                    o[0] = in ? 1.0 : 0.0; o[1] = dist;
                    if (stopped || !in) o[2] = dist;
                }
            }
        }
        if (!have) break;
        cs = wave_sum(cs); cu = wave_sum(cu);
#pragma unroll
        for (int k = 0; k < 6; ++k) { aN[k] = wave_sum(aN[k]); aW[k] = wave_sum(aW[k]); ag[k] = wave_sum(ag[k]); }
#pragma unroll
        for (int k = 0; k < 9; ++k) aM[k] = wave_sum(aM[k]);
        chi2 = wave_sum(ac);
        n_start = cs; n_used = cu;
        if (first || stopped) chi2_start = chi2;
        if (stopped) break;

        // A = [N M'; M W], the 6 x 6 of (omega, c)
        A[0][0] = aN[0]; A[0][1] = A[1][0] = aN[1]; A[0][2] = A[2][0] = aN[2];
        A[1][1] = aN[3]; A[1][2] = A[2][1] = aN[4]; A[2][2] = aN[5];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { A[j][3 + i] = aM[i * 3 + j]; A[3 + i][j] = aM[i * 3 + j]; }
        A[3][3] = aW[0]; A[3][4] = A[4][3] = aW[1]; A[3][5] = A[5][3] = aW[2];
        A[4][4] = aW[3]; A[4][5] = A[5][4] = aW[4]; A[5][5] = aW[5];
        if (!(cu >= 3 && ldl_factor<6>(A, piv_rel, Lm, dg) == 6)) {  // the start stands: one sweep at it, and that is the last
            flag = 1; stopped = true; step_rot = 0.0; step_c = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) quat[k] = q0[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = c0[k];
            rml_rotation(quat, R);
            continue;
        }
        if (last) {                                              // the covariance A^-1, column by column, the upper triangle
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double unit[6], yv[6], x[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) unit[k] = k == j ? 1.0 : 0.0;
                ldl_forward<6>(Lm, dg, unit, 6, yv);
                ldl_back<6, 6>(Lm, yv, x);
#pragma unroll
                for (int i = 0; i <= j; ++i) C[i * 6 - (i * (i - 1)) / 2 + (j - i)] = x[i];
            }
            break;
        }
        // ---- the step: A x = g, q <- dq (x) q, c <- c + dc -----------------------------------------------------------------------
        double yv[6], x[6];
        ldl_forward<6>(Lm, dg, ag, 6, yv);
        ldl_back<6, 6>(Lm, yv, x);
        const double h0 = 0.5 * x[0], h1 = 0.5 * x[1], h2 = 0.5 * x[2];
        const double hn = sqrt(((1.0 + h0 * h0) + h1 * h1) + h2 * h2);
        const double aw = 1.0 / hn, ax = h0 / hn, ay = h1 / hn, az = h2 / hn;
        const double bw = quat[0], bx = quat[1], by = quat[2], bz = quat[3];
        double w = ((aw * bw - ax * bx) - ay * by) - az * bz;
        double xq = ((aw * bx + ax * bw) + ay * bz) - az * by;
        double yq = ((aw * by - ax * bz) + ay * bw) + az * bx;
        double zq = ((aw * bz + ax * by) - ay * bx) + az * bw;
        const double nr = sqrt(((w * w + xq * xq) + yq * yq) + zq * zq);
        w = w / nr; xq = xq / nr; yq = yq / nr; zq = zq / nr;
        const double lead = xq != 0.0 ? xq : (yq != 0.0 ? yq : zq);
        if (w < 0.0 || (w == 0.0 && lead < 0.0)) { w = -w; xq = -xq; yq = -yq; zq = -zq; }
        quat[0] = w; quat[1] = xq; quat[2] = yq; quat[3] = zq;
        rml_rotation(quat, R);
        c[0] = c[0] + x[3]; c[1] = c[1] + x[4]; c[2] = c[2] + x[5];
        step_rot = rml_maxabs(x[0], x[1], x[2]);
        step_c = rml_maxabs(x[3], x[4], x[5]);
        ++it;
    }
    if (lane != 0) return;

    // ---- the columns (every lane holds the same values; lane 0 writes) ---------------------------------------------------------------
    const double fl = (double)flag;
    double t[3] = {0.0, 0.0, 0.0};
    if (have) {
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = c[i] - ((R[i * 3] * qm[0] + R[i * 3 + 1] * qm[1]) + R[i * 3 + 2] * qm[2]);
    }
    if (ml) {
        double* o = ml + fi * VBS_RIGID_ML_COLS;
        const double w = quat[0], x = quat[1], y = quat[2], z = quat[3];
        o[0] = fl; o[1] = (double)n_start; o[2] = (double)n_used; o[3] = (double)it;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[4 + k] = quat[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) o[8 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[17 + k] = t[k]; o[20 + k] = c[k]; o[23 + k] = qm[k]; }
        o[26] = chi2;
        o[27] = have ? (double)(3 * n_used - 6) : 0.0;
        o[28] = chi2_start; o[29] = step_rot; o[30] = step_c;
        o[31] = have ? (2.0 * atan2(sqrt((x * x + y * y) + z * z), w)) * VBS_DEG : 0.0;
        o[32] = have ? atan2(sqrt(R[2] * R[2] + R[5] * R[5]), R[8]) * VBS_DEG : 0.0;
        o[33] = have ? atan2(R[5], R[2]) * VBS_DEG : 0.0;
        o[34] = have ? (2.0 * atan2(z, w)) * VBS_DEG : 0.0;
        // Sigma_n = G Sigma_ww G' with G the x, y rows of -[n]x, n = R z; t2_tilt; var_twist = n' Sigma_ww n
        double nxx = 0.0, nxy = 0.0, nyy = 0.0, t2 = 0.0, vtw = 0.0;
        if (flag == 2) {
            const double n0 = R[2], n1 = R[5], n2 = R[8];
            const double s00 = C[0], s01 = C[1], s02 = C[2], s11 = C[6], s12 = C[7], s22 = C[11];
            const double a0 = n2 * s01 - n1 * s02, a1 = n2 * s11 - n1 * s12, a2 = n2 * s12 - n1 * s22;
            const double b0 = n0 * s02 - n2 * s00, b2 = n0 * s22 - n2 * s02;
            nxx = a1 * n2 - a2 * n1; nxy = a2 * n0 - a0 * n2; nyy = b2 * n0 - b0 * n2;
            const double l = nxy / nxx, d2 = nyy - l * nxy, z2 = n1 - l * n0;
            if (nxx > 0.0 && d2 > piv_rel * nyy) t2 = (n0 * n0) / nxx + (z2 * z2) / d2;
            const double v0 = (s00 * n0 + s01 * n1) + s02 * n2, v1 = (s01 * n0 + s11 * n1) + s12 * n2;
            const double v2 = (s02 * n0 + s12 * n1) + s22 * n2;
            vtw = (n0 * v0 + n1 * v1) + n2 * v2;
        }
        o[35] = nxx; o[36] = nxy; o[37] = nyy; o[38] = t2; o[39] = vtw;
    }
    if (pcov) {
        double* o = pcov + fi * VBS_RIGID_ML_PCOV_COLS;
        o[0] = flag == 2 ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k) o[1 + k] = C[k];
    }
    if (coef) {
        double* o = coef + fi * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[i * 4] = fl; o[i * 4 + 1] = R[i * 3]; o[i * 4 + 2] = R[i * 3 + 1]; o[i * 4 + 3] = R[i * 3 + 2]; }
        o[12] = fl; o[13] = t[0]; o[14] = t[1]; o[15] = t[2];
    }
}

void launch_rigid_ml_series(const float* table, int m, const double* source, const double* cov, const double* start,
                            const double* residual, const double* source_cov, int iters, double piv_rel, int frame_begin,
                            int frame_end, double* ml, double* pcov, double* coef, double* mahal, hipStream_t s) {
    const int nf = frame_end - frame_begin;
    hipLaunchKernelGGL(k_rigid_ml, dim3((unsigned)(((int64_t)nf + RML_WAVES - 1) / RML_WAVES)), dim3(RML_WAVES * 64), 0, s, table, m,
                       source, cov, start, residual, source_cov, iters, piv_rel, frame_begin, nf, ml, pcov, coef, mahal);
}
