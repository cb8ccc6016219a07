// Uncertainty of the 3-D solve: the Jacobians of undistort_point + solve_marker (track_common.h) by forward
// mode THROUGH THE FIVE ITERATIONS AS EXECUTED, and the covariances they give.  Float64 without contraction, + - * / sqrt only, no
// atomics; every expression below is restated in tests/helpers/uncert_oracle.py, so every output is held bit for bit.
//   k_uncert_points   thread per point: xyz, ok as k_points gives them, J_obs [3,3], J_cam [3,16]
//   k_uncert_ref      thread per slot: what the reference frame contributes (usable, its observation part, its G) - once per slot
//   k_uncert_cov      thread per table row: Sigma_X, and with a reference frame Sigma_D and t2 = D' Sigma_D^-1 D (LDL', no roots)
//   k_uncert_total    one wave per frame, VBS_UNCERT_GROUP frames a workgroup: the variance of the total displacement and the
//                     coherent camera share of it, summed in k_axis_displacement's order (lane l adds slots l, l + 64, ..; the
//                     fold of wave_fold.h)
//   k_pixel_noise     thread per slot: count, mean and covariance of (Cx, Cy, major) over a frame range, two passes, frames in order
// A direction is a seed of 19 numbers: the 16 entries of the camera vector (fx, fy, cx, cy, k1, k2, p1, p2, k3, w0, w1, w2, T0,
// T1, T2, dmm), then the observation (Cx, Cy, major).  A thread keeps the ten primal iterates and pushes ONE direction at a time
// through them; a column of the camera factor is pushed as it is, so G = J_cam L is formed column by column and J_cam never
// exists for a table.  Nothing here indexes a register array with a runtime value: no scratch.  The primal, the push and the
// products live in uncert_math.h, which k_posecov.hip shares.
#include "uncert_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define UNC_WAVES VBS_UNCERT_GROUP
static_assert(UNC_WAVES >= 1 && UNC_WAVES <= 16, "a workgroup is at most 1024 threads");

__global__ __launch_bounds__(256) void k_uncert_points(const double* __restrict__ uvd, int n, CamD cam, double* __restrict__ xyz,
                                                       double* __restrict__ j_obs, double* __restrict__ j_cam,
                                                       int32_t* __restrict__ ok) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    UncPrimal P;
    double X[3];
    const double d = uvd[3 * i + 2];
    const bool good = unc_primal(cam, uvd[3 * i], uvd[3 * i + 1], d, P, X);
    xyz[3 * i] = X[0]; xyz[3 * i + 1] = X[1]; xyz[3 * i + 2] = X[2];
    ok[i] = good ? 1 : 0;
#pragma unroll 1
    for (int k = 0; k < UNC_SEED; ++k) {
        double s[UNC_SEED], t[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < UNC_SEED; ++j) s[j] = j == k ? 1.0 : 0.0;
        if (good) unc_push(cam, P, d, s, t);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (k < UNC_CAM) j_cam[((int64_t)i * 3 + r) * UNC_CAM + k] = t[r];
            else j_obs[((int64_t)i * 3 + r) * 3 + (k - UNC_CAM)] = t[r];
        }
    }
}

// ref [m][UNC_REF] of the reference frame's rows
__global__ __launch_bounds__(64) void k_uncert_ref(const float* __restrict__ table, int m, int ref_frame, CamD cam, double min_size,
                                                   const double* __restrict__ obs, int obs_stride, UncFactor L, int q,
                                                   double* __restrict__ ref) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= m) return;
    double* o = ref + (int64_t)slot * UNC_REF;
    UncPrimal P;
    double d = 0.0;
    const bool ok = unc_row(cam, table + ((int64_t)ref_frame * m + slot) * VBS_TABLE_COLS, min_size, P, d);
    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
        double A[3][3];
        unc_obs_jac(cam, P, d, A);
        unc_obs_cov(A, obs + (int64_t)slot * obs_stride, p);
    }
    o[0] = ok ? 1.0 : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) o[1 + e] = p[e];
#pragma unroll 1
    for (int c = 0; c < q; ++c) {
        double g[3] = {0.0, 0.0, 0.0};
        if (ok) unc_cam_push(cam, P, d, L, c, g);
        o[7 + 3 * c] = g[0]; o[8 + 3 * c] = g[1]; o[9 + 3 * c] = g[2];
    }
}

// cov [rows][7] = flag, xx, xy, xz, yy, yz, zz (may be null); dcov [rows][8] = flag (1 both usable, + 2 t2 valid), the six
// entries of Sigma_D, t2 (may be null; ref is read only then)
__global__ __launch_bounds__(256) void k_uncert_cov(const float* __restrict__ table, int m, int64_t rows, int frame_begin,
                                                    int ref_frame, CamD cam, double min_size, const double* __restrict__ obs,
                                                    int obs_stride, UncFactor L, int q, double piv_rel,
                                                    const double* __restrict__ ref, double* __restrict__ cov,
                                                    double* __restrict__ dcov) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int slot = (int)(i % m);
    const float* row = table + ((int64_t)frame_begin * m + i) * VBS_TABLE_COLS;
    UncPrimal P;
    double d = 0.0;
    const bool ok = unc_row(cam, row, min_size, P, d);
    const double* r0 = ref + (int64_t)slot * UNC_REF;
    const bool both = dcov && ok && r0[0] != 0.0;
    double sx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sd[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
        double A[3][3];
        unc_obs_jac(cam, P, d, A);
        unc_obs_cov(A, obs + (int64_t)slot * obs_stride, sx);
        if (both) {
#pragma unroll
            for (int e = 0; e < 6; ++e) sd[e] = sx[e] + r0[1 + e];
        }
#pragma unroll 1
        for (int c = 0; c < q; ++c) {
            double g[3];
            unc_cam_push(cam, P, d, L, c, g);
            sx[0] = sx[0] + g[0] * g[0]; sx[1] = sx[1] + g[0] * g[1]; sx[2] = sx[2] + g[0] * g[2];
            sx[3] = sx[3] + g[1] * g[1]; sx[4] = sx[4] + g[1] * g[2]; sx[5] = sx[5] + g[2] * g[2];
            if (both) {
                const double e0 = g[0] - r0[7 + 3 * c], e1 = g[1] - r0[8 + 3 * c], e2 = g[2] - r0[9 + 3 * c];
                sd[0] = sd[0] + e0 * e0; sd[1] = sd[1] + e0 * e1; sd[2] = sd[2] + e0 * e2;
                sd[3] = sd[3] + e1 * e1; sd[4] = sd[4] + e1 * e2; sd[5] = sd[5] + e2 * e2;
            }
        }
    }
    if (cov) {
        double* o = cov + i * VBS_UNCERT_COV_COLS;
        o[0] = ok ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < 6; ++e) o[1 + e] = sx[e];
    }
    if (!dcov) return;
    double t2 = 0.0;
    bool valid = false;
    if (both) {
        // D as k_axis_displacement forms it; Sigma_D = L diag(d1, d2, d3) L' without square roots
        const float* rr = table + ((int64_t)ref_frame * m + slot) * VBS_TABLE_COLS;
        const double D0 = (double)row[6] - (double)rr[6], D1 = (double)row[7] - (double)rr[7], D2 = (double)row[8] - (double)rr[8];
        const double thr = piv_rel * ((sd[0] + sd[3]) + sd[5]);
        const double d1 = sd[0];
        if (d1 > thr) {
            const double l21 = sd[1] / d1, l31 = sd[2] / d1;
            const double d2 = sd[3] - l21 * sd[1];
            if (d2 > thr) {
                const double w = sd[4] - l21 * sd[2];
                const double l32 = w / d2;
                const double d3 = (sd[5] - l31 * sd[2]) - l32 * w;
                if (d3 > thr) {
                    const double z1 = D0, z2 = D1 - l21 * z1, z3 = (D2 - l31 * z1) - l32 * z2;
                    t2 = (z1 * z1 / d1 + z2 * z2 / d2) + z3 * z3 / d3;
                    valid = true;
                }
            }
        }
    }
    double* o = dcov + i * VBS_UNCERT_DCOV_COLS;
    o[0] = both ? (valid ? 3.0 : 1.0) : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) o[1 + e] = sd[e];
    o[7] = t2;
}

// total [frames][8] = count, complete, var_x, var_y, var_z, cam_x, cam_y, cam_z.  A slot counts where the mask selects it, the
// reference row is usable (`want`) and this frame's row is.  Sweep 0 adds the observation parts of both frames in quadrature;
// sweep 1 + c adds column c of G_f - G_0 over the slots, and the square of that sum is the column's coherent share.
__global__ __launch_bounds__(UNC_WAVES * 64) void k_uncert_total(const float* __restrict__ table, int m, int frame_begin, int n_frames,
                                                                 CamD cam, double min_size, const double* __restrict__ obs,
                                                                 int obs_stride, UncFactor L, int q, const u8* __restrict__ slot_mask,
                                                                 const double* __restrict__ ref, double* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * UNC_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                   // (a whole wave: no barrier follows)
    const float* frow = table + ((int64_t)frame_begin + fi) * m * VBS_TABLE_COLS;
    double so[3] = {0.0, 0.0, 0.0};
    int cnt = 0, want = 0;
    for (int slot = lane; slot < m; slot += 64) {
        const double* r0 = ref + (int64_t)slot * UNC_REF;
        if (!((!slot_mask || slot_mask[slot]) && r0[0] != 0.0)) continue;
        ++want;
        UncPrimal P;
        double d = 0.0;
        if (!unc_row(cam, frow + (int64_t)slot * VBS_TABLE_COLS, min_size, P, d)) continue;
        ++cnt;
        double A[3][3], p[6];
        unc_obs_jac(cam, P, d, A);
        unc_obs_cov(A, obs + (int64_t)slot * obs_stride, p);
        so[0] = so[0] + (p[0] + r0[1]); so[1] = so[1] + (p[3] + r0[4]); so[2] = so[2] + (p[5] + r0[6]);
    }
    cnt = wave_fold_down(cnt); want = wave_fold_down(want);
#pragma unroll
    for (int k = 0; k < 3; ++k) so[k] = wave_fold_down(so[k]);
    double camv[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int c = 0; c < q; ++c) {
        double b[3] = {0.0, 0.0, 0.0};
        for (int slot = lane; slot < m; slot += 64) {
            const double* r0 = ref + (int64_t)slot * UNC_REF;
            if (!((!slot_mask || slot_mask[slot]) && r0[0] != 0.0)) continue;
            UncPrimal P;
            double d = 0.0, g[3];
            if (!unc_row(cam, frow + (int64_t)slot * VBS_TABLE_COLS, min_size, P, d)) continue;
            unc_cam_push(cam, P, d, L, c, g);
            b[0] = b[0] + (g[0] - r0[7 + 3 * c]); b[1] = b[1] + (g[1] - r0[8 + 3 * c]); b[2] = b[2] + (g[2] - r0[9 + 3 * c]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[k] = wave_fold_down(b[k]);
            camv[k] = camv[k] + b[k] * b[k];
        }
    }
    if (lane == 0) {
        double* o = total + fi * VBS_UNCERT_TOTAL_COLS;
        o[0] = (double)cnt; o[1] = (want >= 1 && cnt == want) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[2 + k] = so[k] + camv[k]; o[5 + k] = camv[k]; }
    }
}

// out [m][10] = count, mean Cx, Cy, major, then uu, uv, ud, vv, vd, dd (sample covariance, ddof 1) over the rows of
// [frame_begin, frame_end) with VBS_FLAG_TRACKED; count 0: zeros, count 1: the mean and zeros
__global__ __launch_bounds__(64) void k_pixel_noise(const float* __restrict__ table, int m, int frame_begin, int frame_end,
                                                    double* __restrict__ out) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= m) return;
    const int64_t step = (int64_t)m * VBS_TABLE_COLS;
    const float* p0 = table + (int64_t)frame_begin * step + (int64_t)slot * VBS_TABLE_COLS;
    double s[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    const float* p = p0;
    for (int f = frame_begin; f < frame_end; ++f, p += step) {
        if ((int)p[0] & VBS_FLAG_TRACKED) {
            s[0] = s[0] + (double)p[1]; s[1] = s[1] + (double)p[2]; s[2] = s[2] + (double)p[3];
            ++cnt;
        }
    }
    const double nn = (double)cnt;
    double mu[3] = {0.0, 0.0, 0.0}, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (cnt > 0) { mu[0] = s[0] / nn; mu[1] = s[1] / nn; mu[2] = s[2] / nn; }
    p = p0;
    for (int f = frame_begin; f < frame_end; ++f, p += step) {
        if ((int)p[0] & VBS_FLAG_TRACKED) {
            const double a = (double)p[1] - mu[0], b = (double)p[2] - mu[1], e = (double)p[3] - mu[2];
            c[0] = c[0] + a * a; c[1] = c[1] + a * b; c[2] = c[2] + a * e;
            c[3] = c[3] + b * b; c[4] = c[4] + b * e; c[5] = c[5] + e * e;
        }
    }
    double* o = out + (int64_t)slot * VBS_NOISE_COLS;
    o[0] = nn; o[1] = mu[0]; o[2] = mu[1]; o[3] = mu[2];
#pragma unroll
    for (int e = 0; e < 6; ++e) o[4 + e] = cnt > 1 ? c[e] / (nn - 1.0) : 0.0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------

void launch_uncert_points(const double* uvd, int n, const vbs_camera& cam, double* xyz, double* j_obs, double* j_cam, int32_t* ok,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_uncert_points, dim3((n + 255) / 256), dim3(256), 0, s, uvd, n, make_cam(cam), xyz, j_obs, j_cam, ok);
}

// obs [dev] [obs_rows (1 or m), 6]; ref [dev] [m, UNC_REF], written here when ref_frame >= 0 and read by the kernel that follows
void launch_uncert_cov(const float* table, int m, const vbs_camera& cam, const double* obs, int obs_rows, const double* cam_factor,
                       int q, int ref_frame, double min_size, double piv_rel, int frame_begin, int frame_end, double* ref, double* cov,
                       double* dcov, hipStream_t s) {
    const UncFactor L = unc_factor(cam_factor, q);
    const CamD c = make_cam(cam);
    const int stride = obs_rows == 1 ? 0 : 6;
    if (dcov)
        hipLaunchKernelGGL(k_uncert_ref, dim3((m + 63) / 64), dim3(64), 0, s, table, m, ref_frame, c, min_size, obs, stride, L, q, ref);
    const int64_t rows = ((int64_t)frame_end - frame_begin) * m;
    hipLaunchKernelGGL(k_uncert_cov, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, table, m, rows, frame_begin, ref_frame, c,
                       min_size, obs, stride, L, q, piv_rel, (const double*)ref, cov, dcov);
}

void launch_uncert_total(const float* table, int m, const vbs_camera& cam, const double* obs, int obs_rows, const double* cam_factor,
                         int q, int ref_frame, const u8* slot_mask, double min_size, int frame_begin, int frame_end, double* ref,
                         double* total, hipStream_t s) {
    const UncFactor L = unc_factor(cam_factor, q);
    const CamD c = make_cam(cam);
    const int stride = obs_rows == 1 ? 0 : 6;
    const int nf = frame_end - frame_begin;
    hipLaunchKernelGGL(k_uncert_ref, dim3((m + 63) / 64), dim3(64), 0, s, table, m, ref_frame, c, min_size, obs, stride, L, q, ref);
    hipLaunchKernelGGL(k_uncert_total, dim3((unsigned)(((int64_t)nf + UNC_WAVES - 1) / UNC_WAVES)), dim3(UNC_WAVES * 64), 0, s, table, m,
                       frame_begin, nf, c, min_size, obs, stride, L, q, slot_mask, (const double*)ref, total);
}

void launch_pixel_noise(const float* table, int m, int frame_begin, int frame_end, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_pixel_noise, dim3((m + 63) / 64), dim3(64), 0, s, table, m, frame_begin, frame_end, out);
}
