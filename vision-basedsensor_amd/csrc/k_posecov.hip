// Uncertainty of the pose misalignment: the first-order covariance of the plane (a, b, c) that
// vbs_pose_series fits to the deviation field, of its tilt and azimuth, and the test "is the plane tilted at all".  Float64 without
// contraction, + - * / only (but the optional `pose` columns tilt, azimuth, rms), no atomics; the operand order of every expression
// is stated in include/vbs.h and restated in tests/helpers/posecov_oracle.py, so every output is held bit for bit.
//   k_posecov_fix   thread per slot: what does not depend on the frame - the start row and, when given, the two rows of the
//                   reference session: usable, the summed observation parts, the summed camera directions.  Once per slot.
//   k_posecov       one wave per frame, VBS_POSECOV_GROUP frames a workgroup.  The plane's sweeps first, in k_pose's arithmetic and
//                   order (so flag, a, b, c, n_used are k_pose's bits), then ONE sweep for Sigma_obs, then one sweep per camera
//                   column.  A wave reads the table directly (no LDS: the forward mode, not the 40-byte rows, is what a sweep costs)
//                   and meets no barrier, so a frame's result cannot depend on the frames next to it.
// A deviation is d = (X_f - X_start) - (X_re - X_rs): up to four solves with ONE camera.  The camera's error enters every marker
// coherently and partly cancels in d, so the direction of column c is s (g_c,f - g_fix,c) and is summed over the markers BEFORE it
// is squared; pixel noise is independent per row and adds in quadrature.  Per column the primal is RECOMPUTED (as k_uncert_total
// does) instead of keeping 3 q = 48 accumulators next to it: the loop over c stays rolled, no register array is indexed with a
// runtime value, and the kernel needs no scratch (profiles/posecov_resource_usage.txt).
#include "fit_math.h"
#include "uncert_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define PCV_WAVES VBS_POSECOV_GROUP
static_assert(PCV_WAVES >= 1 && PCV_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_POSECOV_COLS == 17, "flag, n_unusable, Sigma [6], Sigma_cam [6], var_tilt, var_azimuth, t2");

// fix [m][UNC_REF] = fixed_usable, S_fix [6], g_fix [q][3].  ref_rows [2][m][10] (ref_start, ref_end) or null.
__global__ __launch_bounds__(64) void k_posecov_fix(const float* __restrict__ start_row, const float* __restrict__ ref_rows, int m,
                                                    CamD cam, double min_size, const double* __restrict__ obs, int obs_stride,
                                                    UncFactor L, int q, double* __restrict__ fix) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= m) return;
    double* o = fix + (int64_t)slot * UNC_REF;
    UncPrimal P0, P1, P2;                                        // start, ref_end, ref_start
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    bool ok = unc_row(cam, start_row + (int64_t)slot * VBS_TABLE_COLS, min_size, P0, d0);
    if (ref_rows) {
        const bool ok2 = unc_row(cam, ref_rows + (int64_t)slot * VBS_TABLE_COLS, min_size, P2, d2);
        const bool ok1 = unc_row(cam, ref_rows + ((int64_t)m + slot) * VBS_TABLE_COLS, min_size, P1, d1);
        ok = ok && ok1 && ok2;
    }
    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
        const double* S6 = obs + (int64_t)slot * obs_stride;
        double A[3][3];
        unc_obs_jac(cam, P0, d0, A);
        unc_obs_cov(A, S6, p);
        if (ref_rows) {
            double p1[6], p2[6];
            unc_obs_jac(cam, P1, d1, A);
            unc_obs_cov(A, S6, p1);
            unc_obs_jac(cam, P2, d2, A);
            unc_obs_cov(A, S6, p2);
#pragma unroll
            for (int e = 0; e < 6; ++e) p[e] = (p[e] + p1[e]) + p2[e];
        }
    }
    o[0] = ok ? 1.0 : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) o[1 + e] = p[e];
#pragma unroll 1
    for (int c = 0; c < q; ++c) {
        double g[3] = {0.0, 0.0, 0.0};
        if (ok) {
            unc_cam_push(cam, P0, d0, L, c, g);
            if (ref_rows) {
                double g1[3], g2[3];
                unc_cam_push(cam, P1, d1, L, c, g1);
                unc_cam_push(cam, P2, d2, L, c, g2);
#pragma unroll
                for (int k = 0; k < 3; ++k) g[k] = (g[k] + g1[k]) - g2[k];
            }
        }
        o[7 + 3 * c] = g[0]; o[8 + 3 * c] = g[1]; o[9 + 3 * c] = g[2];
    }
}

// the used set's plane, as the linearisation needs it
struct PcvPlane { double a, b, mx, my, mz, xx, xy, yy, det, n_used; };

// K [3][3]: column k = what the unit perturbation e_k of ONE used slot does to (a, b, c); x, y, r = the slot's centred
// coordinates and residual
static __device__ __forceinline__ void pcv_influence(const PcvPlane& f, double x, double y, double r, double K[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dx = k == 0 ? 1.0 : 0.0, dy = k == 1 ? 1.0 : 0.0, dz = k == 2 ? 1.0 : 0.0;
        const double e = (dz - f.a * dx) - f.b * dy;
        const double h1 = x * e + r * dx, h2 = y * e + r * dy;
        const double da = (h1 * f.yy - h2 * f.xy) / f.det, db = (h2 * f.xx - h1 * f.xy) / f.det;
        K[0][k] = da; K[1][k] = db; K[2][k] = (e / f.n_used - da * f.mx) - db * f.my;
    }
}

__global__ __launch_bounds__(PCV_WAVES * 64) void k_posecov(const float* __restrict__ table, int m, int start_frame,
                                                            const double* __restrict__ ref_disp, const double* __restrict__ ref_xyz,
                                                            const u8* __restrict__ slot_mask, int shell, double scale, double reject_k,
                                                            int frame_begin, int n_frames, CamD cam, double min_size,
                                                            const double* __restrict__ obs, int obs_stride, UncFactor L, int q,
                                                            double piv_rel, const double* __restrict__ fix, double* __restrict__ pose,
                                                            double* __restrict__ pcov) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * PCV_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                  // (a whole wave: no barrier follows)
    const int64_t row_step = (int64_t)m * VBS_TABLE_COLS;
    const float* frow = table + ((int64_t)frame_begin + fi) * row_step;
    const float* srow = table + (int64_t)start_frame * row_step;

    // the end point of a slot, or false: the common rule (fit_math.h)
    auto point = [&](int slot, double* p) -> bool {
        return end_point(frow, srow, ref_disp, ref_xyz, slot_mask, shell, scale, slot, p);
    };

    // ---- the plane of vbs_pose_series and its one round of rejection ------------------------------------------------------------------
    // A fit is three sweeps - count and means, centred sums, SSR - and the kept set takes the same three through the same code (the
    // round loop stays rolled).  The plane that stands (a, b, cc, ssr, f) and the first plane (f_*), which decides the kept set in
    // every later sweep.
    double a = 0.0, b = 0.0, cc = 0.0, ssr = 0.0, flag = 0.0, thr = 0.0, f_a = 0.0, f_b = 0.0, f_m[3] = {0.0, 0.0, 0.0};
    PcvPlane f = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    bool two = false;
    auto kept = [&](const double* p) -> bool {
        const double x = p[0] - f_m[0], y = p[1] - f_m[1], z = p[2] - f_m[2];
        const double r = z - (f_a * x + f_b * y);
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
            cnt = c;
            f.n_used = n;                                        // (the `pose` column n_used, with or without a plane)
        } else if (c >= cnt) {
            break;                                               // nothing was rejected
        }
        if (c < 3) break;
        const double mn[3] = {sp[0] / n, sp[1] / n, sp[2] / n};

        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                 // xx, xy, yy, xz, yz
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot, p) || (second && !kept(p))) continue;
            const double x = p[0] - mn[0], y = p[1] - mn[1], z = p[2] - mn[2];
            e[0] = e[0] + x * x; e[1] = e[1] + x * y; e[2] = e[2] + y * y; e[3] = e[3] + x * z; e[4] = e[4] + y * z;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) e[k] = wave_sum(e[k]);
        const double det = e[0] * e[2] - e[1] * e[1];
        if (!(fabs(det) > 1e-300)) break;                        // the set does not fix a plane
        const double an = (e[3] * e[2] - e[4] * e[1]) / det, bn = (e[4] * e[0] - e[3] * e[1]) / det;

        double s1 = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot, p) || (second && !kept(p))) continue;
            const double x = p[0] - mn[0], y = p[1] - mn[1], z = p[2] - mn[2];
            const double r = z - (an * x + bn * y);
            s1 = s1 + r * r;
        }
        s1 = wave_sum(s1);
        const bool again = !second && reject_k > 0.0 && s1 > 0.0;
        if (again) {                                             // kept() reads thr and f_*
            thr = (reject_k * reject_k) * (s1 / n);
            f_a = an; f_b = bn; f_m[0] = mn[0]; f_m[1] = mn[1]; f_m[2] = mn[2];
        }
        a = an; b = bn; cc = mn[2] - an * mn[0] - bn * mn[1]; ssr = s1;
        f = {an, bn, mn[0], mn[1], mn[2], e[0], e[1], e[2], det, n};
        flag = second ? 2.0 : 1.0; two = second;
        if (!again) break;
    }
    const bool plane = flag != 0.0;
    if (pose && lane == 0) {
        double* o = pose + fi * VBS_POSE_COLS;
        o[0] = flag; o[1] = a; o[2] = b; o[3] = cc;
        o[4] = plane ? atan(sqrt(a * a + b * b)) * VBS_DEG : 0.0;
        o[5] = plane ? atan2(b, a) * VBS_DEG : 0.0;
        o[6] = plane ? sqrt(ssr / f.n_used) : 0.0;
        o[7] = f.n_used;
    }
    if (!pcov) return;                                           // (the same for every thread of the grid)

    // ---- Sigma_obs: one sweep over the used slots --------------------------------------------------------------------------------------
    const double ss = scale * scale;
    double so[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int slot = lane; slot < m; slot += 64) {
        double p[3];
        if (!point(slot, p) || (two && !kept(p))) continue;
        const double* fx = fix + (int64_t)slot * UNC_REF;
        UncPrimal P;
        double d = 0.0;
        if (!(fx[0] != 0.0 && unc_row(cam, frow + (int64_t)slot * VBS_TABLE_COLS, min_size, P, d))) { ++bad; continue; }
        if (!plane) continue;
        double A[3][3], K[3][3], pf[6], C[6], o[6];
        unc_obs_jac(cam, P, d, A);
        unc_obs_cov(A, obs + (int64_t)slot * obs_stride, pf);
#pragma unroll
        for (int e = 0; e < 6; ++e) C[e] = ss * (pf[e] + fx[1 + e]);
        const double x = p[0] - f.mx, y = p[1] - f.my, z = p[2] - f.mz;
        pcv_influence(f, x, y, z - (f.a * x + f.b * y), K);
        unc_obs_cov(K, C, o);
#pragma unroll
        for (int e = 0; e < 6; ++e) so[e] = so[e] + o[e];
    }
    bad = wave_sum(bad);
#pragma unroll
    for (int e = 0; e < 6; ++e) so[e] = wave_fold_down(so[e]);
    const bool good = plane && bad == 0;

    // ---- Sigma_cam: column c of the factor summed over the used slots, then squared -----------------------------------------------------
    double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (good) {
#pragma unroll 1
        for (int col = 0; col < q; ++col) {
            double v[3] = {0.0, 0.0, 0.0};
            for (int slot = lane; slot < m; slot += 64) {
                double p[3];
                if (!point(slot, p) || (two && !kept(p))) continue;
                const double* fx = fix + (int64_t)slot * UNC_REF;
                UncPrimal P;
                double d = 0.0, g[3], K[3][3];
                if (!unc_row(cam, frow + (int64_t)slot * VBS_TABLE_COLS, min_size, P, d)) continue;   // (none: bad == 0)
                unc_cam_push(cam, P, d, L, col, g);
                const double u0 = scale * (g[0] - fx[7 + 3 * col]), u1 = scale * (g[1] - fx[8 + 3 * col]),
                             u2 = scale * (g[2] - fx[9 + 3 * col]);
                const double x = p[0] - f.mx, y = p[1] - f.my, z = p[2] - f.mz;
                pcv_influence(f, x, y, z - (f.a * x + f.b * y), K);
#pragma unroll
                for (int i = 0; i < 3; ++i) v[i] = v[i] + ((K[i][0] * u0 + K[i][1] * u1) + K[i][2] * u2);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) v[i] = wave_fold_down(v[i]);
            sc[0] = sc[0] + v[0] * v[0]; sc[1] = sc[1] + v[0] * v[1]; sc[2] = sc[2] + v[0] * v[2];
            sc[3] = sc[3] + v[1] * v[1]; sc[4] = sc[4] + v[1] * v[2]; sc[5] = sc[5] + v[2] * v[2];
        }
    }
    if (lane != 0) return;

    // ---- Sigma, the angle variances, t2 (lane 0 holds the sums) --------------------------------------------------------------------------
    double* o = pcov + fi * VBS_POSECOV_COLS;
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double vt = 0.0, va = 0.0, t2 = 0.0;
    bool valid = false, angles = false;
    if (good) {
#pragma unroll
        for (int e = 0; e < 6; ++e) S[e] = so[e] + sc[e];
        const double aa = f.a * f.a, bb = f.b * f.b, ab2 = (2.0 * f.a) * f.b;
        const double rho2 = aa + bb;
        const double k2 = VBS_DEG * VBS_DEG;
        if (rho2 > 0.0) {
            angles = true;
            const double w = 1.0 + rho2;
            vt = (k2 * ((aa * S[0] + ab2 * S[1]) + bb * S[3])) / (rho2 * (w * w));
            va = (k2 * ((bb * S[0] - ab2 * S[1]) + aa * S[3])) / (rho2 * rho2);
        }
        const double piv = piv_rel * (S[0] + S[3]);
        const double d1 = S[0];
        if (d1 > piv) {
            const double l = S[1] / d1;
            const double d2 = S[3] - l * S[1];
            if (d2 > piv) {
                const double z1 = f.a, z2 = f.b - l * f.a;
                t2 = z1 * z1 / d1 + z2 * z2 / d2;
                valid = true;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) sc[e] = 0.0;
    }
    o[0] = good ? (1.0 + (valid ? 2.0 : 0.0)) + (angles ? 4.0 : 0.0) : 0.0;
    o[1] = (double)bad;
#pragma unroll
    for (int e = 0; e < 6; ++e) { o[2 + e] = S[e]; o[8 + e] = sc[e]; }
    o[14] = vt; o[15] = va; o[16] = t2;
}

// obs [dev] [obs_rows (1 or m), 6]; fix [dev] [m, UNC_REF], written here when pcov is asked for and read by the kernel that follows
void launch_pose_cov(const float* table, int m, int start_frame, const double* ref_disp, const double* ref_xyz, const u8* slot_mask,
                     int shell, double scale, double reject_k, const vbs_camera& cam, const double* obs, int obs_rows,
                     const double* cam_factor, int q, double min_size, double piv_rel, const float* ref_rows, int frame_begin,
                     int frame_end, double* fix, double* pose, double* pcov, hipStream_t s) {
    const UncFactor L = unc_factor(cam_factor, q);
    const CamD c = make_cam(cam);
    const int stride = obs_rows == 1 ? 0 : 6;
    const int nf = frame_end - frame_begin;
    if (pcov)
        hipLaunchKernelGGL(k_posecov_fix, dim3((m + 63) / 64), dim3(64), 0, s, table + (int64_t)start_frame * m * VBS_TABLE_COLS, ref_rows,
                           m, c, min_size, obs, stride, L, q, fix);
    hipLaunchKernelGGL(k_posecov, dim3((unsigned)(((int64_t)nf + PCV_WAVES - 1) / PCV_WAVES)), dim3(PCV_WAVES * 64), 0, s, table, m,
                       start_frame, ref_disp, ref_xyz, slot_mask, shell, scale, reject_k, frame_begin, nf, c, min_size, obs, stride, L, q,
                       piv_rel, (const double*)fix, pose, pcov);
}
