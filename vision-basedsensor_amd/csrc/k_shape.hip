// Indentation shape along a recording: for every frame the quadric
//     z ~ c0 + a x + b y + (p x x + 2 q x y + r y y) / 2
// through the end points vbs_pose_series fits its plane to, its apex, depth and curvatures, what it leaves per marker, and the plane
// of the same factorisation.  Float64 without contraction, + - * / only (but the columns rms_plane, rms, k1, k2, dir_deg), no atomics;
// the operand order of every expression is stated in include/vbs.h and restated in tests/helpers/shape_oracle.py.
//   k_shape   one wave per frame, VBS_SHAPE_GROUP frames a workgroup.  A wave reads the table directly (as k_posecov: no LDS) and
//             meets no barrier, so a frame's result cannot depend on the frames next to it.  A fit is three sweeps - count and
//             means, the 20 sums, the residuals - and the kept set of the one round of rejection takes the same three through
//             the same code (the round loop stays rolled); a last sweep writes the residual record.  A lane keeps its partial
//             sums in registers and the 6 x 6 factorisation is unrolled over constant indices: no scratch
//             (profiles/shape_resource_usage.txt).
#include "common.h"
#include "fit_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define SHP_WAVES VBS_SHAPE_GROUP
#define SHP_SUMS  20             // u, v, u2, uv, v2, u3, u2v, uv2, v3, u4, u3v, u2v2, uv3, v4, then w, uw, vw, u2w, uvw, v2w
static_assert(SHP_WAVES >= 1 && SHP_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_SHAPE_COLS == 24, "degree, count, n_used, means [3], c0, a, b, p, q, r, two rms, H, K, k1, k2, dir, apex [4], depth");

// The 6 x 6 normal equations in basis order (1, u, v, u2, uv, v2) by fit_math.h's LDL'; returns the number of leading pivots that
// passed.  gam [3] (from the leading 3 x 3 alone) is written where 3 passed, beta [6] where all 6 did.
static __device__ __forceinline__ int shp_solve(double n, const double* S, double piv_rel, double* beta, double* gam) {
    const double N[6][6] = {{n, S[0], S[1], S[2], S[3], S[4]},      {S[0], S[2], S[3], S[5], S[6], S[7]},
                            {S[1], S[3], S[4], S[6], S[7], S[8]},   {S[2], S[5], S[6], S[9], S[10], S[11]},
                            {S[3], S[6], S[7], S[10], S[11], S[12]}, {S[4], S[7], S[8], S[11], S[12], S[13]}};
    double Lm[6][6], d[6], y[6];
    const int npass = ldl_factor(N, piv_rel, Lm, d);
    ldl_forward(Lm, d, S + 14, npass, y);
    if (npass >= 3) ldl_back<3>(Lm, y, gam);
    if (npass == 6) ldl_back<6>(Lm, y, beta);
    return npass;
}

__global__ __launch_bounds__(SHP_WAVES * 64) void k_shape(const float* __restrict__ table, int m, int start_frame,
                                                          const double* __restrict__ ref_disp, const double* __restrict__ ref_xyz,
                                                          const u8* __restrict__ slot_mask, int shell, double scale, double length,
                                                          double reject_k, int min_count, double piv_rel, double apex_rel,
                                                          double max_apex, int frame_begin, int n_frames, double* __restrict__ shape,
                                                          double* __restrict__ coef, double* __restrict__ residual) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * SHP_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                  // (a whole wave: no barrier follows)
    const int64_t row_step = (int64_t)m * VBS_TABLE_COLS;
    const float* frow = table + ((int64_t)frame_begin + fi) * row_step;
    const float* srow = table + (int64_t)start_frame * row_step;

    // the end point of a slot, or false: the common rule (fit_math.h)
    auto point = [&](int slot, double* p) -> bool {
        return end_point(frow, srow, ref_disp, ref_xyz, slot_mask, shell, scale, slot, p);
    };
    // the residual of a point against a fit of `degree` (1: g, 2: b) around the means mn
    auto resid = [&](const double* p, const double* mn, int degree, const double* b, const double* g) -> double {
        const double u = (p[0] - mn[0]) / length, v = (p[1] - mn[1]) / length, w = p[2] - mn[2];
        if (degree == 2) {
            const double u2 = u * u, uv = u * v, v2 = v * v;
            return w - (((((b[0] + b[1] * u) + b[2] * v) + b[3] * u2) + b[4] * uv) + b[5] * v2);
        }
        return w - ((g[0] + g[1] * u) + g[2] * v);
    };

    // the fit that stands (mean, beta, gam, ...) and the first fit (f_*), which decides the kept set in every later sweep
    double mean[3] = {0.0, 0.0, 0.0}, beta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gam[3] = {0.0, 0.0, 0.0};
    double f_mean[3] = {0.0, 0.0, 0.0}, f_beta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, f_gam[3] = {0.0, 0.0, 0.0};
    double ssr1 = 0.0, ssr2 = 0.0, thr = 0.0;
    int degree = 0, cnt = 0, n_used = 0;
    bool two = false;
    auto kept = [&](const double* p) -> bool {
        const double r = resid(p, f_mean, degree, f_beta, f_gam);    // (the degree never changes after the first fit)
        return r * r <= thr;
    };

#pragma unroll 1
    for (int round = 0; round < 2; ++round) {                    // 0: the common set, 1: its kept slots (every test below is wave-uniform)
        const bool second = round == 1;
        double sp[3] = {0.0, 0.0, 0.0};
        int c = 0;
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot, p) || (second && !kept(p))) continue;
            ++c;
            sp[0] = sp[0] + p[0]; sp[1] = sp[1] + p[1]; sp[2] = sp[2] + p[2];
        }
        c = wave_sum(c);
#pragma unroll
        for (int k = 0; k < 3; ++k) sp[k] = wave_sum(sp[k]);
        const double n = (double)c;
        if (!second) {
            cnt = n_used = c;
#pragma unroll
            for (int k = 0; k < 3; ++k) mean[k] = c > 0 ? sp[k] / n : 0.0;
        } else if (c >= cnt) {
            break;                                               // nothing was rejected
        }
        if (c < 3) break;
        const double mn[3] = {sp[0] / n, sp[1] / n, sp[2] / n};

        double S[SHP_SUMS];
#pragma unroll
        for (int k = 0; k < SHP_SUMS; ++k) S[k] = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot, p) || (second && !kept(p))) continue;
            const double u = (p[0] - mn[0]) / length, v = (p[1] - mn[1]) / length, w = p[2] - mn[2];
            const double u2 = u * u, uv = u * v, v2 = v * v;
            const double u3 = u2 * u, u2v = u2 * v, uv2 = u * v2, v3 = v2 * v;
            const double u4 = u2 * u2, u3v = u3 * v, u2v2 = u2 * v2, uv3 = u * v3, v4 = v2 * v2;
            S[0] = S[0] + u; S[1] = S[1] + v; S[2] = S[2] + u2; S[3] = S[3] + uv; S[4] = S[4] + v2;
            S[5] = S[5] + u3; S[6] = S[6] + u2v; S[7] = S[7] + uv2; S[8] = S[8] + v3;
            S[9] = S[9] + u4; S[10] = S[10] + u3v; S[11] = S[11] + u2v2; S[12] = S[12] + uv3; S[13] = S[13] + v4;
            S[14] = S[14] + w; S[15] = S[15] + u * w; S[16] = S[16] + v * w;
            S[17] = S[17] + u2 * w; S[18] = S[18] + uv * w; S[19] = S[19] + v2 * w;
        }
#pragma unroll
        for (int k = 0; k < SHP_SUMS; ++k) S[k] = wave_sum(S[k]);
        double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        const int npass = shp_solve(n, S, piv_rel, b, g);
        const int deg = (c >= min_count && npass == 6) ? 2 : (npass >= 3 ? 1 : 0);
        if (second ? deg < degree : deg == 0) break;             // the kept set must reach the first fit's degree
        const int dsel = second ? degree : deg;

        double s1 = 0.0, s2 = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot, p) || (second && !kept(p))) continue;
            const double r1 = resid(p, mn, 1, b, g);
            s1 = s1 + r1 * r1;
            if (dsel == 2) {
                const double r2 = resid(p, mn, 2, b, g);
                s2 = s2 + r2 * r2;
            }
        }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        const double sel = dsel == 2 ? s2 : s1;
        const bool again = !second && reject_k > 0.0 && sel > 0.0;
        if (again) {                                             // before the fit that stands is replaced: kept() reads f_* and degree
            thr = (reject_k * reject_k) * (sel / n);
#pragma unroll
            for (int k = 0; k < 3; ++k) { f_mean[k] = mn[k]; f_gam[k] = g[k]; }
#pragma unroll
            for (int k = 0; k < 6; ++k) f_beta[k] = b[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { mean[k] = mn[k]; gam[k] = g[k]; }
#pragma unroll
        for (int k = 0; k < 6; ++k) beta[k] = dsel == 2 ? b[k] : 0.0;
        ssr1 = s1; ssr2 = dsel == 2 ? s2 : 0.0;
        degree = dsel; n_used = c; two = second;
        if (!again) break;
    }

    // ---- the residual record: (1, r) of the fit that stands for every used slot -----------------------------------------------------
    if (residual) {
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            const bool in = degree >= 1 && point(slot, p) && (!two || kept(p));
            double* o = residual + (fi * m + slot) * 2;
            o[0] = in ? 1.0 : 0.0;
            o[1] = in ? resid(p, mean, degree, beta, gam) : 0.0;
        }
    }
    if (lane != 0) return;

    // ---- the columns (every lane holds the same values; lane 0 writes) ---------------------------------------------------------------
    const double nu = (double)n_used;
    double c0 = 0.0, a = 0.0, b = 0.0, p = 0.0, q = 0.0, r = 0.0;
    if (degree == 2) { c0 = mean[2] + beta[0]; a = beta[1] / length; b = beta[2] / length; }
    if (degree == 1) { c0 = mean[2] + gam[0]; a = gam[1] / length; b = gam[2] / length; }
    double H = 0.0, K = 0.0, k1 = 0.0, k2 = 0.0, dir = 0.0, rms = 0.0;
    double apex = 0.0, ax = 0.0, ay = 0.0, az = 0.0, depth = 0.0;
    if (degree == 2) {
        p = ((2.0 * beta[3]) / length) / length; q = (beta[4] / length) / length; r = ((2.0 * beta[5]) / length) / length;
        H = (p + r) / 2.0; K = p * r - q * q;
        const double hd = (p - r) / 2.0;
        const double s = sqrt(hd * hd + q * q);
        k1 = H + s; k2 = H - s;
        dir = (0.5 * atan2(2.0 * q, p - r)) * VBS_DEG;
        rms = sqrt(ssr2 / nu);
        if (fabs(K) > apex_rel * ((p * p + 2.0 * (q * q)) + r * r)) {
            const double xi = (q * b - r * a) / K, eta = (q * a - p * b) / K;
            const double reach = max_apex * length;
            if (xi * xi + eta * eta <= reach * reach) {
                apex = 1.0; ax = mean[0] + xi; ay = mean[1] + eta; az = c0 + (a * xi + b * eta) / 2.0;
                depth = az - (mean[2] + ((gam[0] + (gam[1] * xi) / length) + (gam[2] * eta) / length));
            }
        }
    }
    if (shape) {
        double* o = shape + fi * VBS_SHAPE_COLS;
        o[0] = (double)degree; o[1] = (double)cnt; o[2] = nu; o[3] = mean[0]; o[4] = mean[1]; o[5] = mean[2];
        o[6] = c0; o[7] = a; o[8] = b; o[9] = p; o[10] = q; o[11] = r;
        o[12] = degree >= 1 ? sqrt(ssr1 / nu) : 0.0; o[13] = rms;
        o[14] = H; o[15] = K; o[16] = k1; o[17] = k2; o[18] = dir;
        o[19] = apex; o[20] = ax; o[21] = ay; o[22] = az; o[23] = depth;
    }
    if (coef) {
        double* o = coef + fi * 8;
        o[0] = (double)degree; o[1] = c0; o[2] = a; o[3] = b;
        o[4] = degree == 2 ? 1.0 : 0.0; o[5] = p; o[6] = q; o[7] = r;
    }
}

void launch_shape_series(const float* table, int m, int start_frame, const double* ref_disp, const double* ref_xyz, const u8* slot_mask,
                         int shell, double scale, double length, double reject_k, int min_count, double piv_rel, double apex_rel,
                         double max_apex, int frame_begin, int frame_end, double* shape, double* coef, double* residual, hipStream_t s) {
    const int nf = frame_end - frame_begin;
    hipLaunchKernelGGL(k_shape, dim3((unsigned)(((int64_t)nf + SHP_WAVES - 1) / SHP_WAVES)), dim3(SHP_WAVES * 64), 0, s, table, m,
                       start_frame, ref_disp, ref_xyz, slot_mask, shell, scale, length, reject_k, min_count, piv_rel, apex_rel, max_apex,
                       frame_begin, nf, shape, coef, residual);
}
