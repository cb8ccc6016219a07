// f7: extrinsic calibration - calibrate_camera_extrinsics (extrinsic_calibration.py:81-123): cv2.solvePnPRansac(ITERATIVE,
// reprojectionError 8, iterationsCount 1000) + projectPoints + the mean error, for a batch of problems (one per frame of a
// recording) that share their world points and their sample table.
//   k_pnp_hypotheses   one thread per (problem, hypothesis): planar homography of 4 sample points -> nearest rotation -> 10
//                      Gauss-Newton steps on 6 -> inlier count of every valid point through the forward distortion model
//   k_pnp_refine       one workgroup per problem: the winner (highest count, lowest index), then Levenberg-Marquardt on the
//                      pixel error of its inliers, at most 20 steps
// Float64 without contraction, no atomics, every sum in a fixed order: two runs give the same bits, and a problem's result does
// not depend on the batch around it.  Nothing waits on another workgroup; every loop has a fixed bound.  gfx950, wave64.
#include "track_common.h"
#include "pnp_math.h"

#pragma clang fp contract(off)

#define PNP_MAX_POINTS VBS_PNP_MAX_POINTS

#define PNP_THREADS 256
#define PNP_SUMS 28                // 21 + 6 + 1

static PnpCam pnp_cam(const CamD& c) {
    return PnpCam{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, c.k[0], c.k[1], c.k[2], c.k[3], c.k[4]};
}

// observation i of problem b: the [B,N,2] float64 form, or columns 1, 2 of a tracker table row (valid where VBS_FLAG_TRACKED)
__device__ __forceinline__ bool pnp_observation(const double* __restrict__ image, const float* __restrict__ table,
                                                const u8* __restrict__ valid, int b, int n, int i, double* u, double* v) {
    const int64_t at = (int64_t)b * n + i;
    bool ok = valid ? valid[at] != 0 : true;
    if (image) {
        *u = image[2 * at]; *v = image[2 * at + 1];
    } else {
        const float* row = table + at * VBS_TABLE_COLS;
        ok = ok && (((int)row[0]) & VBS_FLAG_TRACKED);
        *u = (double)row[1]; *v = (double)row[2];
    }
    return ok && isfinite(*u) && isfinite(*v);
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_hypotheses(const double* __restrict__ world, int n, const double* __restrict__ image,
                                                                const float* __restrict__ table, const u8* __restrict__ valid,
                                                                CamD cam, PnpCam pc, const int32_t* __restrict__ samples, int nh,
                                                                double reproj2, int32_t* __restrict__ hyp_count,
                                                                double* __restrict__ hyp_pose) {
    __shared__ double W[3 * PNP_MAX_POINTS], xn[PNP_MAX_POINTS], yn[PNP_MAX_POINTS], uo[PNP_MAX_POINTS], vo[PNP_MAX_POINTS];
    __shared__ u8 ok[PNP_MAX_POINTS];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < n; i += PNP_THREADS) {
        double u = 0.0, v = 0.0, uu = 0.0, vu = 0.0;
        const bool good = pnp_observation(image, table, valid, b, n, i, &u, &v);
        if (good) undistort_point(cam, u, v, &uu, &vu);
        W[3 * i] = world[3 * i]; W[3 * i + 1] = world[3 * i + 1]; W[3 * i + 2] = world[3 * i + 2];
        uo[i] = u; vo[i] = v;
        xn[i] = (uu - pc.cx) / pc.fx; yn[i] = (vu - pc.cy) / pc.fy;
        ok[i] = good ? 1 : 0;
    }
    __syncthreads();
    const int h = blockIdx.x * PNP_THREADS + tid;
    if (h >= nh) return;
    int s[PNP_SAMPLE];
    bool live = true;
#pragma unroll
    for (int k = 0; k < PNP_SAMPLE; ++k) {
        s[k] = samples[h * PNP_SAMPLE + k];
        live = live && s[k] >= 0 && s[k] < n;
    }
#pragma unroll
    for (int k = 0; k < PNP_SAMPLE; ++k) {
        if (!live) s[k] = 0;                              // (never index past the staged points)
        live = live && ok[s[k]];
#pragma unroll
        for (int j = 0; j < k; ++j) live = live && s[j] != s[k];
    }
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (live) live = pnp_minimal(W, xn, yn, s, R, t, nullptr);
    int count = -1;
    if (live) {
        count = 0;
        for (int i = 0; i < n; ++i)
            if (ok[i] && pnp_err2(pc, R, t, W[3 * i], W[3 * i + 1], W[3 * i + 2], uo[i], vo[i]) <= reproj2) ++count;
    }
    const int64_t at = (int64_t)b * nh + h;
    hyp_count[at] = count;
#pragma unroll
    for (int i = 0; i < 9; ++i) hyp_pose[at * 12 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) hyp_pose[at * 12 + 9 + i] = t[i];
}

// sums[PNP_SUMS] over the workgroup -> every thread, in a fixed order: shuffles inside a wave, then the waves in wave order
template <int nv>
__device__ __forceinline__ void pnp_reduce(double* v, double (*part)[PNP_SUMS], double* total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < nv; ++q) {
        double x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);
        if (lane == 0) part[wave][q] = x;
    }
    __syncthreads();
    if (tid < nv) {
        double x = part[0][tid];
        for (int w = 1; w < PNP_THREADS / 64; ++w) x = x + part[w][tid];
        total[tid] = x;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_refine(const double* __restrict__ world, int n, const double* __restrict__ image,
                                                            const float* __restrict__ table, const u8* __restrict__ valid, PnpCam pc,
                                                            int nh, double reproj2, const int32_t* __restrict__ hyp_count,
                                                            const double* __restrict__ hyp_pose, int32_t* __restrict__ status,
                                                            double* __restrict__ pose, int32_t* __restrict__ inlier_count,
                                                            u8* __restrict__ inlier_mask, double* __restrict__ errors,
                                                            int32_t* __restrict__ winner) {
    __shared__ double part[PNP_THREADS / 64][PNP_SUMS], total[PNP_SUMS];
    __shared__ double trial[12];
    __shared__ int best_c[PNP_THREADS], best_h[PNP_THREADS];
    __shared__ int done;
    const int b = blockIdx.x, tid = threadIdx.x;
    constexpr int PER = PNP_MAX_POINTS / PNP_THREADS;
    // this thread's points: i = tid + k * PNP_THREADS
    double X[PER], Y[PER], Z[PER], uo[PER], vo[PER];
    bool good[PER], inl[PER];
    double cnt[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * PNP_THREADS;
        good[k] = false; inl[k] = false;
        X[k] = Y[k] = Z[k] = uo[k] = vo[k] = 0.0;
        if (i < n) {
            good[k] = pnp_observation(image, table, valid, b, n, i, &uo[k], &vo[k]);
            X[k] = world[3 * i]; Y[k] = world[3 * i + 1]; Z[k] = world[3 * i + 2];
        }
        if (good[k]) cnt[0] = cnt[0] + 1.0;
    }
    // the winner: highest count, ties to the lowest index - what a sequential "strictly better" scan keeps
    int bc = -1, bh = 0x7fffffff;
    for (int h = tid; h < nh; h += PNP_THREADS) {
        const int c = hyp_count[(int64_t)b * nh + h];
        if (c > bc) { bc = c; bh = h; }
    }
    best_c[tid] = bc; best_h[tid] = bh;
    pnp_reduce<1>(cnt, part, total);                      // (its barriers also publish best_c / best_h)
    const int n_valid = (int)total[0];
    for (int q = 0; q < PNP_THREADS; ++q) {               // every thread scans the same 256 entries: no further barrier
        const int c = best_c[q], h = best_h[q];
        if (c > bc || (c == bc && h < bh)) { bc = c; bh = h; }
    }
    const int fail = n_valid < 4 ? VBS_PNP_FEW_POINTS : (bc < 0 ? VBS_PNP_NO_HYPOTHESIS : 0);
    if (fail) {                                           // uniform over the workgroup
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (tid + k * PNP_THREADS < n) inlier_mask[(int64_t)b * n + tid + k * PNP_THREADS] = 0;
        if (tid < 12) pose[(int64_t)b * 12 + tid] = NAN;
        if (tid < 2) errors[(int64_t)b * 2 + tid] = NAN;
        if (tid == 0) { status[b] = fail; inlier_count[b] = 0; winner[b] = -1; }
        return;
    }
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = hyp_pose[((int64_t)b * nh + bh) * 12 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = hyp_pose[((int64_t)b * nh + bh) * 12 + 9 + i];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        inl[k] = good[k] && pnp_err2(pc, R, t, X[k], Y[k], Z[k], uo[k], vo[k]) <= reproj2;
        if (tid + k * PNP_THREADS < n) inlier_mask[(int64_t)b * n + tid + k * PNP_THREADS] = inl[k] ? 1 : 0;
    }
    // Levenberg-Marquardt on the pixel error of the inliers.  (R, t) is the trial pose of every thread; thread 0 keeps the
    // accepted pose, its normal equations and the damping, and broadcasts the next trial through LDS.
    double Rc[9], tc[3], Ac[21], gc[6], cost_c = INFINITY, lambda = 1e-3;
    bool have = false;
#pragma unroll 1
    for (int it = 0; it <= PNP_LM_STEPS; ++it) {
        double v[PNP_SUMS];
#pragma unroll
        for (int q = 0; q < PNP_SUMS; ++q) v[q] = 0.0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (inl[k]) {
                double Ju[6], Jv[6], ru, rv;
                if (pnp_pixel_jacobian(pc, R, t, X[k], Y[k], Z[k], uo[k], vo[k], Ju, Jv, &ru, &rv)) {
                    pnp_accumulate(Ju, Jv, ru, rv, v, v + 21);
                    v[27] = v[27] + (ru * ru + rv * rv);
                } else {
                    v[27] = INFINITY;                     // a trial that puts an inlier behind the camera is rejected
                }
            }
        }
        pnp_reduce<PNP_SUMS>(v, part, total);
        if (tid == 0) {
            const double cost = total[27];
            if (!have || cost <= cost_c) {
                if (have) lambda = fmax(lambda * 0.1, 1e-15);
#pragma unroll
                for (int i = 0; i < 9; ++i) Rc[i] = R[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) tc[i] = t[i];
#pragma unroll
                for (int i = 0; i < 21; ++i) Ac[i] = total[i];
#pragma unroll
                for (int i = 0; i < 6; ++i) gc[i] = total[21 + i];
                cost_c = cost; have = true;
            } else {
                lambda = fmin(lambda * 10.0, 1e15);
            }
            int stop = it == PNP_LM_STEPS;
            double d[6];
            if (!stop && !(isfinite(cost_c) && pnp_solve6(Ac, gc, lambda, d))) stop = 1;
            if (!stop) {
                double dm = 0.0;
#pragma unroll
                for (int i = 0; i < 6; ++i) dm = fmax(dm, fabs(d[i]));
                if (!(dm >= PNP_LM_EPS)) stop = 1;        // (also a NaN step)
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = tc[i];
            if (!stop) pnp_apply_step(d, R, t);
#pragma unroll
            for (int i = 0; i < 9; ++i) trial[i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) trial[9 + i] = t[i];
            done = stop;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = trial[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = trial[9 + i];
        const int stop = done;
        __syncthreads();                                  // (trial / done are rewritten in the next round)
        if (stop) break;                                  // uniform: (R, t) is the accepted pose
    }
    // what calibrate_camera_extrinsics prints and saves (:117-118): the mean pixel error over ALL valid points; and the inlier RMS
    double e[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (good[k]) {
            const double e2 = pnp_err2(pc, R, t, X[k], Y[k], Z[k], uo[k], vo[k]);
            e[0] = e[0] + sqrt(e2);
            if (inl[k]) { e[1] = e[1] + e2; e[2] = e[2] + 1.0; }
        }
    }
    pnp_reduce<3>(e, part, total);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) pose[(int64_t)b * 12 + i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pose[(int64_t)b * 12 + 9 + i] = t[i];
        status[b] = 0;
        inlier_count[b] = (int)total[2];
        winner[b] = bh;
        errors[(int64_t)b * 2] = total[0] / (double)n_valid;
        errors[(int64_t)b * 2 + 1] = sqrt(total[1] / total[2]);
    }
}

void launch_pnp(const double* world, int n, const double* image, const float* table, const u8* valid, int nb, const vbs_camera& cam,
                const int32_t* samples, int nh, double reproj_px, int32_t* hyp_count, double* hyp_pose, int32_t* status, double* pose,
                int32_t* inlier_count, u8* inlier_mask, double* errors, int32_t* winner, hipStream_t s) {
    const CamD cd = make_cam(cam);
    const PnpCam pc = pnp_cam(cd);
    const double reproj2 = reproj_px * reproj_px;
    // grid.y holds at most 65535 problems: a longer batch goes in slices (a problem's result does not depend on its batch)
    for (int b0 = 0; b0 < nb; b0 += 65535) {
        const int nbs = nb - b0 < 65535 ? nb - b0 : 65535;
        const int64_t o = (int64_t)b0;
        const double* img = image ? image + o * n * 2 : nullptr;
        const float* tab = table ? table + o * n * VBS_TABLE_COLS : nullptr;
        const u8* val = valid ? valid + o * n : nullptr;
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3((nh + PNP_THREADS - 1) / PNP_THREADS, nbs), dim3(PNP_THREADS), 0, s, world, n, img,
                           tab, val, cd, pc, samples, nh, reproj2, hyp_count + o * nh, hyp_pose + o * nh * 12);
        hipLaunchKernelGGL(k_pnp_refine, dim3(nbs), dim3(PNP_THREADS), 0, s, world, n, img, tab, val, pc, nh, reproj2,
                           (const int32_t*)(hyp_count + o * nh), (const double*)(hyp_pose + o * nh * 12), status + o, pose + o * 12,
                           inlier_count + o, inlier_mask + o * n, errors + o * 2, winner + o);
    }
}
