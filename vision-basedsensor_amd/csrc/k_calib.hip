// f9: intrinsic calibration - cv2.calibrateCamera(obj_points, img_points, img_size, None, None) (intrinsic_calibration.py:97-98)
// for one planar board seen in V views, as a batch of problems that each use a subset of the views (leave-one-out, random
// subsets) and share the corners.
//   k_calib_homography   one wave per view: Hartley-normalised linear homography (normal equations with h33 = 1), then
//                        CALIB_H_GN_STEPS Gauss-Newton steps on the transfer error; H does not depend on the subset
//   k_calib_refine       one workgroup per problem: cv2's closed-form focal lengths over the active views, a pose per view,
//                        then Levenberg-Marquardt on the pixel error over 9 + 6 V_active parameters in block-arrow form
//                        (9 x 9 Schur complement of the 6 x 6 pose blocks), and the standard deviations of the intrinsics
// Float64 without contraction, no atomics, every sum in a fixed order that depends on the position in the active list only: two
// runs give the same bits, and a masked problem equals the same views passed alone.  Nothing waits on another workgroup; every
// loop has a fixed bound.  gfx950, wave64.
#include "common.h"
#include "calib_math.h"

#pragma clang fp contract(off)

#define CALIB_THREADS 256
#define CALIB_WAVES (CALIB_THREADS / 64)
#define CALIB_PER (VBS_CHESS_MAX_PATTERN / 64)          // board points of one lane: lane + 64 k
#define CALIB_MAXV VBS_CALIB_MAX_VIEWS

static_assert(VBS_CALIB_MAX_VIEWS == 64, "thread a of wave 0 owns active view a");

static __device__ __forceinline__ double calib_wave_sum(double v) {     // fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_calib_homography(const double* __restrict__ obj, int n, const double* __restrict__ img,
                                                         double* __restrict__ H, int32_t* __restrict__ view_void) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const double* ip = img + (int64_t)v * n * 2;
    double X[CALIB_PER], Y[CALIB_PER], x[CALIB_PER], y[CALIB_PER];
    bool in[CALIB_PER];
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k) {
        const int i = lane + 64 * k;
        in[k] = i < n;
        X[k] = Y[k] = x[k] = y[k] = 0.0;
        if (in[k]) {
            X[k] = obj[2 * i]; Y[k] = obj[2 * i + 1]; x[k] = ip[2 * i]; y[k] = ip[2 * i + 1];
            s4[0] = s4[0] + X[k]; s4[1] = s4[1] + Y[k]; s4[2] = s4[2] + x[k]; s4[3] = s4[3] + y[k];
        }
    }
    const double dn = (double)n;
    const double mxo = calib_wave_sum(s4[0]) / dn, myo = calib_wave_sum(s4[1]) / dn;
    const double mxi = calib_wave_sum(s4[2]) / dn, myi = calib_wave_sum(s4[3]) / dn;
    double d2[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k) {
        if (in[k]) {
            const double a = X[k] - mxo, b = Y[k] - myo, c = x[k] - mxi, d = y[k] - myi;
            d2[0] = d2[0] + sqrt(a * a + b * b); d2[1] = d2[1] + sqrt(c * c + d * d);
        }
    }
    const double so = calib_hartley_scale(calib_wave_sum(d2[0]), dn), si = calib_hartley_scale(calib_wave_sum(d2[1]), dn);
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k) {
        X[k] = so * (X[k] - mxo); Y[k] = so * (Y[k] - myo); x[k] = si * (x[k] - mxi); y[k] = si * (y[k] - myi);
    }
    double acc[CALIB_H_SUMS], h[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < CALIB_H_SUMS; ++q) acc[q] = 0.0;
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k)
        if (in[k]) calib_h_linear(X[k], Y[k], x[k], y[k], acc);
#pragma unroll
    for (int q = 0; q < CALIB_H_SUMS; ++q) acc[q] = calib_wave_sum(acc[q]);
    double sc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k)
        if (in[k]) { sc[0] = sc[0] + x[k] * x[k]; sc[1] = sc[1] + x[k] * y[k]; sc[2] = sc[2] + y[k] * y[k]; }
    bool ok = isfinite(so) && isfinite(si) && calib_scatter_ok(calib_wave_sum(sc[0]), calib_wave_sum(sc[1]), calib_wave_sum(sc[2]));
    ok = calib_h_solve(acc, h) && ok;                                        // (every lane holds the same sums: uniform)
#pragma unroll 1
    for (int it = 0; it < CALIB_H_GN_STEPS; ++it) {
#pragma unroll
        for (int q = 0; q < CALIB_H_SUMS; ++q) acc[q] = 0.0;
#pragma unroll
        for (int k = 0; k < CALIB_PER; ++k)
            if (in[k]) calib_h_gauss_newton(h, X[k], Y[k], x[k], y[k], acc);
#pragma unroll
        for (int q = 0; q < CALIB_H_SUMS; ++q) acc[q] = calib_wave_sum(acc[q]);
        double d[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        ok = calib_h_solve(acc, d) && ok;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = h[i] + d[i];
    }
    double Hd[9];
    ok = calib_h_denormalise(h, mxo, myo, so, mxi, myi, si, Hd) && ok;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) H[(int64_t)v * 9 + i] = ok ? Hd[i] : NAN;
        view_void[v] = ok ? 0 : 1;
    }
}

struct CalibOut {
    int32_t* status; double* K4; double* dist; double* R; double* T; double* rms; double* view_rms; double* std_intrinsics;
    int32_t* iterations;
};

// One pass over the active views with the trial parameters (cam, pose).  Wave w takes the views at positions w, w + 4, ... of
// the active list, its lanes the points lane + 64 k.  Always: the squared error of every view -> vcost.  JAC: also the view's
// B, C, g -> blk, and then its share of the intrinsic block (the Jacobian is computed a second time, so that the 81 and the 54
// sums are never live together), added to the wave's running sum in `part`; the waves are summed in wave order -> A.
template <bool JAC>
static __device__ __forceinline__ void calib_pass(int n, int nact, const int* act, const double* __restrict__ img, const double* cam,
                                                  const double* pose, const double X[CALIB_PER], const double Y[CALIB_PER],
                                                  double* blk, double* vcost, double (*part)[CALIB_NA], double* A) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PnpCam c = PnpCam{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7], cam[8]};
    if (JAC && lane == 0)                                 // (lane 0 alone touches its wave's running sums)
        for (int q = 0; q < CALIB_NA; ++q) part[wave][q] = 0.0;
#pragma unroll 1
    for (int a = wave; a < nact; a += CALIB_WAVES) {
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = pose[a * 12 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = pose[a * 12 + 9 + i];
        const double* ip = img + (int64_t)act[a] * n * 2;
        double cost = 0.0;
        if (JAC) {
            double accV[CALIB_NV];
#pragma unroll
            for (int q = 0; q < CALIB_NV; ++q) accV[q] = 0.0;
#pragma unroll 1
            for (int k = 0; k < CALIB_PER; ++k) {
                const int i = lane + 64 * k;
                if (i < n) {
                    double Pu[6], Pv[6], Iu[CALIB_NI], Iv[CALIB_NI], ru, rv;
                    if (pnp_pixel_jacobian(c, R, t, X[k], Y[k], 0.0, ip[2 * i], ip[2 * i + 1], Pu, Pv, &ru, &rv)) {
                        calib_intrinsic_columns(c, R, t, X[k], Y[k], Iu, Iv);
                        calib_accumulate_view(Iu, Iv, Pu, Pv, ru, rv, accV);
                        cost = cost + (ru * ru + rv * rv);
                    } else {
                        cost = INFINITY;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < CALIB_NV; ++q) {
                const double s = calib_wave_sum(accV[q]);
                if (lane == 0) blk[a * CALIB_NV + q] = s;
            }
            double accA[CALIB_NA];
#pragma unroll
            for (int q = 0; q < CALIB_NA; ++q) accA[q] = 0.0;
#pragma unroll 1
            for (int k = 0; k < CALIB_PER; ++k) {
                const int i = lane + 64 * k;
                if (i < n) {
                    double Pu[6], Pv[6], Iu[CALIB_NI], Iv[CALIB_NI], ru, rv;
                    if (pnp_pixel_jacobian(c, R, t, X[k], Y[k], 0.0, ip[2 * i], ip[2 * i + 1], Pu, Pv, &ru, &rv)) {
                        calib_intrinsic_columns(c, R, t, X[k], Y[k], Iu, Iv);
                        calib_accumulate_intrinsic(Iu, Iv, ru, rv, accA);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < CALIB_NA; ++q) {
                const double s = calib_wave_sum(accA[q]);
                if (lane == 0) part[wave][q] = part[wave][q] + s;
            }
        } else {
#pragma unroll
            for (int k = 0; k < CALIB_PER; ++k) {
                const int i = lane + 64 * k;
                if (i < n) cost = cost + pnp_err2(c, R, t, X[k], Y[k], 0.0, ip[2 * i], ip[2 * i + 1]);   // (behind the camera: infinity)
            }
        }
        cost = calib_wave_sum(cost);
        if (lane == 0) vcost[a] = cost;
    }
    __syncthreads();
    if (JAC) {
        if (tid < CALIB_NA) {
            double s = part[0][tid];
            for (int w = 1; w < CALIB_WAVES; ++w) s = s + part[w][tid];
            A[tid] = s;
        }
        __syncthreads();
    }
}

// Factor and solve the block-arrow system at damping lambda: thread a inverts its view's damped C, threads 0..53 sum the Schur
// complement in view order, thread 0 solves it.  Returns (uniform) whether every factorisation succeeded.  dA = the intrinsic
// step; ci = the inverses, for the back-substitution; inv_diag (may be null) = diag S^-1.
static __device__ __forceinline__ bool calib_factor(int nact, double lambda, const double* A, const double* blk, double* ci, double* S,
                                                    double* dA, double* inv_diag, double* work, int* flag) {
    const int tid = threadIdx.x;
    bool bad = false;
    if (tid < nact) {
        double C[21], Ci[21];
#pragma unroll
        for (int q = 0; q < 21; ++q) C[q] = blk[tid * CALIB_NV + CALIB_NB + q];
        bad = !calib_inverse6(C, lambda, Ci);
#pragma unroll
        for (int q = 0; q < 21; ++q) ci[tid * 21 + q] = Ci[q];
    }
    if (__syncthreads_or(bad)) return false;
    if (tid < CALIB_NA) S[tid] = calib_schur_entry(tid, A, lambda, blk, ci, nact);
    __syncthreads();
    if (tid == 0) {
        bool ok = calib_solve9(S, dA, inv_diag, work);
        for (int i = 0; i < CALIB_NI; ++i) ok = ok && isfinite(dA[i]);
        *flag = ok ? 1 : 0;
    }
    __syncthreads();
    return *flag != 0;
}

__global__ __launch_bounds__(CALIB_THREADS) void k_calib_refine(const double* __restrict__ obj, int n, const double* __restrict__ img,
                                                                int nv, const u8* __restrict__ view_mask, int w, int h, int max_iter,
                                                                const double* __restrict__ H, const int32_t* __restrict__ view_void,
                                                                CalibOut out) {
    __shared__ double blk[CALIB_MAXV * CALIB_NV];          // per active view: B (54), C (21), g (6) at the accepted parameters
    __shared__ double ci[CALIB_MAXV * 21];                 // per active view: (C + lambda diag C)^-1
    __shared__ double pose[CALIB_MAXV * 12];               // per active view: the trial pose, R then t
    __shared__ double vcost[CALIB_MAXV], vstep[CALIB_MAXV];
    __shared__ double A[CALIB_NA], S[CALIB_NA], part[CALIB_WAVES][CALIB_NA], work[CALIB_SOLVE9_WORK];
    __shared__ double cam_c[CALIB_NI], cam_t[CALIB_NI], dA[CALIB_NI], inv_diag[CALIB_NI];
    __shared__ int act[CALIB_MAXV], slot[CALIB_MAXV];
    __shared__ int s_nact, s_fail, s_flag;
    const int b = blockIdx.x, tid = threadIdx.x;
    // the board: a lane sees the same points in every view, so they stay in registers
    double X[CALIB_PER], Y[CALIB_PER];
#pragma unroll
    for (int k = 0; k < CALIB_PER; ++k) {
        const int i = (tid & 63) + 64 * k;
        X[k] = i < n ? obj[2 * i] : 0.0;
        Y[k] = i < n ? obj[2 * i + 1] : 0.0;
    }
    if (tid == 0) {
        // the active views in index order, then cv2's closed form over them
        int na = 0, fail = 0;
        for (int v = 0; v < nv; ++v) {
            const bool on = view_mask ? view_mask[(int64_t)b * nv + v] != 0 : true;
            slot[v] = on ? na : -1;
            if (on) { act[na] = v; ++na; if (view_void[v]) fail = VBS_CALIB_DEGENERATE; }
        }
        if (na < 3) fail = VBS_CALIB_FEW_VIEWS;
        if (!fail) {
            const double cx = ((double)w - 1.0) * 0.5, cy = ((double)h - 1.0) * 0.5;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, fx = 0.0, fy = 0.0;
            for (int a = 0; a < na; ++a) {
                double Hv[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) Hv[i] = H[(int64_t)act[a] * 9 + i];
                calib_init_rows(Hv, cx, cy, m);
            }
            if (!calib_init_focal(m, &fx, &fy)) fail = VBS_CALIB_DEGENERATE;
            cam_c[0] = fx; cam_c[1] = fy; cam_c[2] = cx; cam_c[3] = cy;
            for (int i = 4; i < CALIB_NI; ++i) cam_c[i] = 0.0;
        }
        s_nact = na; s_fail = fail;
    }
    __syncthreads();
    const int nact = s_nact;
    int fail = s_fail;
    // thread a of wave 0 owns the view at position a of the active list: its accepted pose and squared error stay in registers
    double Rc[9], tc[3], vc = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rc[i] = 0.0;
    tc[0] = tc[1] = tc[2] = 0.0;
    if (!fail) {
        bool bad = false;
        if (tid < nact) {
            double Hv[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Hv[i] = H[(int64_t)act[tid] * 9 + i];
            bad = !calib_init_pose(Hv, cam_c[0], cam_c[1], cam_c[2], cam_c[3], Rc, tc);
#pragma unroll
            for (int i = 0; i < 9; ++i) pose[tid * 12 + i] = Rc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) pose[tid * 12 + 9 + i] = tc[i];
        }
        if (__syncthreads_or(bad)) fail = VBS_CALIB_DEGENERATE;
    }
    double cost_c = INFINITY, lambda = CALIB_LAMBDA0;
    int iters = 0;
    if (!fail) {
        bool fresh = true;                                                       // the blocks are to be taken at the accepted parameters
#pragma unroll 1
        for (int it = 0; it <= max_iter; ++it) {
            if (fresh) {
                calib_pass<true>(n, nact, act, img, cam_c, pose, X, Y, blk, vcost, part, A);
                cost_c = 0.0;
                for (int a = 0; a < nact; ++a) cost_c = cost_c + vcost[a];     // every thread, the same order
                if (tid < nact) vc = vcost[tid];
                fresh = false;
                if (!isfinite(cost_c)) { fail = VBS_CALIB_DEGENERATE; break; }  // (only at the start: a point behind its camera)
            }
            if (it == max_iter) break;
            if (!calib_factor(nact, lambda, A, blk, ci, S, dA, nullptr, work, &s_flag)) {
                ++iters;                                                         // counts as a rejected step
                lambda = lambda * 10.0;
                if (lambda > CALIB_LAMBDA_FAIL) { fail = VBS_CALIB_DEGENERATE; break; }
                continue;
            }
            // the trial: intrinsics on thread 0, each pose on its thread
            if (tid == 0)
                for (int i = 0; i < CALIB_NI; ++i) cam_t[i] = cam_c[i] + dA[i];
            if (tid < nact) {
                double d[6], R[9], t[3], dm = 0.0;
                calib_back_substitute(blk + tid * CALIB_NV, blk + tid * CALIB_NV + CALIB_NB + 21, ci + tid * 21, dA, d);
#pragma unroll
                for (int i = 0; i < 6; ++i) dm = fmax(dm, isfinite(d[i]) ? fabs(d[i]) : INFINITY);
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = tc[i];
                calib_apply_step(d, R, t);
#pragma unroll
                for (int i = 0; i < 9; ++i) pose[tid * 12 + i] = R[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) pose[tid * 12 + 9 + i] = t[i];
                vstep[tid] = dm;
            }
            __syncthreads();
            double dm = 0.0;
            for (int i = 0; i < CALIB_NI; ++i) dm = fmax(dm, fabs(dA[i]));
            for (int a = 0; a < nact; ++a) dm = fmax(dm, vstep[a]);
            if (!(dm >= PNP_LM_EPS)) break;                                      // converged: the step is not taken
            ++iters;
            calib_pass<false>(n, nact, act, img, cam_t, pose, X, Y, blk, vcost, part, A);
            double cost_t = 0.0;
            for (int a = 0; a < nact; ++a) cost_t = cost_t + vcost[a];
            if (cost_t <= cost_c) {
                lambda = fmax(lambda * 0.1, 1e-15);
                if (tid < nact) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rc[i] = pose[tid * 12 + i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) tc[i] = pose[tid * 12 + 9 + i];
                }
                if (tid == 0)
                    for (int i = 0; i < CALIB_NI; ++i) cam_c[i] = cam_t[i];
                fresh = true;
            } else {
                lambda = fmin(lambda * 10.0, 1e15);
            }
            __syncthreads();                                                     // (cam_c is read, vcost and pose are rewritten next)
        }
    }
    // the accepted poses and errors back into LDS, and the covariance of the intrinsics at lambda = 0
    bool have_std = false;
    if (!fail) {
        __syncthreads();
        if (tid < nact) {
#pragma unroll
            for (int i = 0; i < 9; ++i) pose[tid * 12 + i] = Rc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) pose[tid * 12 + 9 + i] = tc[i];
            vcost[tid] = vc;
        }
        have_std = calib_factor(nact, 0.0, A, blk, ci, S, dA, inv_diag, work, &s_flag);
    }
    __syncthreads();
    const int64_t ob = (int64_t)b;
    for (int v = tid; v < nv; v += CALIB_THREADS) {
        const int a = fail ? -1 : slot[v];
        for (int i = 0; i < 9; ++i) out.R[(ob * nv + v) * 9 + i] = a >= 0 ? pose[a * 12 + i] : NAN;
        for (int i = 0; i < 3; ++i) out.T[(ob * nv + v) * 3 + i] = a >= 0 ? pose[a * 12 + 9 + i] : NAN;
        out.view_rms[ob * nv + v] = a >= 0 ? sqrt(vcost[a] / (double)n) : NAN;
    }
    if (tid == 0) {
        const double points = (double)nact * (double)n;
        const double dof = 2.0 * points - (double)(CALIB_NI + 6 * nact);
        out.status[b] = fail;
        out.iterations[b] = iters;
        for (int i = 0; i < 4; ++i) out.K4[ob * 4 + i] = fail ? NAN : cam_c[i];
        for (int i = 0; i < 5; ++i) out.dist[ob * 5 + i] = fail ? NAN : cam_c[4 + i];
        out.rms[b] = fail ? NAN : sqrt(cost_c / points);
        for (int i = 0; i < CALIB_NI; ++i)
            out.std_intrinsics[ob * CALIB_NI + i] = (!fail && have_std && dof > 0.0) ? sqrt((cost_c / dof) * inv_diag[i]) : NAN;
    }
}

void launch_calib(const double* obj, int n, const double* img, int nv, const u8* view_mask, int nb, int w, int h, int max_iter,
                  double* H, int32_t* view_void, int32_t* status, double* K4, double* dist, double* R, double* T, double* rms,
                  double* view_rms, double* std_intrinsics, int32_t* iterations, hipStream_t s) {
    hipLaunchKernelGGL(k_calib_homography, dim3(nv), dim3(64), 0, s, obj, n, img, H, view_void);
    const CalibOut out{status, K4, dist, R, T, rms, view_rms, std_intrinsics, iterations};
    hipLaunchKernelGGL(k_calib_refine, dim3(nb), dim3(CALIB_THREADS), 0, s, obj, n, img, nv, view_mask, w, h, max_iter,
                       (const double*)H, (const int32_t*)view_void, out);
}
