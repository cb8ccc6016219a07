// Shear, torsion and strain along a recording: how a marker's displacement depends on where the marker sits.
// Float64 without contraction, no atomics, the order of every sum stated in include/vbs.h: a result depends on its inputs only,
// never on the launch shape.
//   k_motion        the affine fit d_k ~ t_k + g_kx x + g_ky y of every frame over its used slots, with one round of outlier
//                   rejection (the rule of k_pose).  One wave per frame, VBS_MOTION_GROUP frames (waves) a workgroup.  What the
//                   frames of a workgroup share - pos and the slot mask - is staged ONCE into LDS (17 KB at 1024 slots: one
//                   chunk, so the only barrier is the one after staging and a wave past the end leaves there).  A frame's rows
//                   are read as they lie (32 bytes a slot at cols = 4: two 16-byte loads a lane, every byte of every line used).
//                   The sums are recomputed from `rec` in every sweep: means, centred sums, residuals with the argmax, and the
//                   same three over the kept set when reject_k > 0.  A wave without a fit skips the loads of the later sweeps.
//   k_local_strain  the same fit over the neighbourhood of every marker.  A workgroup takes VBS_LSTRAIN_GROUP frames one after
//                   another, thread i keeps slot i and its K neighbour indices in registers; a frame's flag, dX, dY, dZ are staged
//                   in LDS next to pos (41 KB), so the gather reads LDS.  The next frame's row is in flight while this one's
//                   neighbourhoods are added up.  One thread adds its members in list order: no fold.
#include "common.h"
#include "strain_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define MOTION_WAVES VBS_MOTION_GROUP
static_assert(MOTION_WAVES >= 1 && MOTION_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_FIELD_MAX_SLOTS <= 1024, "k_local_strain keeps one slot a thread");

struct MotionStage {                             // 17 KB
    double px[VBS_FIELD_MAX_SLOTS], py[VBS_FIELD_MAX_SLOTS];
    u8 sel[VBS_FIELD_MAX_SLOTS];
};
struct MotionPoint { double px, py, d[3]; };
struct MotionFit { double mx, my, md[3], gx[3], gy[3]; };

// r_k = e_k - (g_kx x + g_ky y) on the fit's own centred coordinates; -> q = r_X r_X + r_Y r_Y + r_Z r_Z, left to right
__device__ __forceinline__ double motion_resid(const MotionFit& F, const MotionPoint& p, double (&r)[3]) {
    const double x = p.px - F.mx, y = p.py - F.my;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = (p.d[k] - F.md[k]) - (F.gx[k] * x + F.gy[k] * y);
    return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}

__global__ __launch_bounds__(MOTION_WAVES * 64) void k_motion(const double* __restrict__ rec, int s, int cols,
                                                              const double* __restrict__ pos, const u8* __restrict__ slot_mask,
                                                              double reject_k, int frame_begin, int n_frames, int vec,
                                                              double* __restrict__ grad, double* __restrict__ strain,
                                                              double* __restrict__ residual) {
    __shared__ MotionStage S;
    for (int slot = threadIdx.x; slot < s; slot += MOTION_WAVES * 64) {
        const bool sel = !slot_mask || slot_mask[slot];          // what is not selected is never read into a value
        S.sel[slot] = sel ? 1 : 0;
        S.px[slot] = sel ? pos[2 * slot] : 0.0;
        S.py[slot] = sel ? pos[2 * slot + 1] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * MOTION_WAVES + (threadIdx.x >> 6);   // this wave's frame among those emitted
    if (fi >= n_frames) return;                                  // (a whole wave, after the only barrier)
    const double* frow = rec + ((int64_t)frame_begin + fi) * s * cols;

    // the point of a slot < s, or false: selected && this frame's flag is nonzero
    auto point = [&](int slot, MotionPoint& p) -> bool {
        if (!S.sel[slot]) return false;
        const double* r = frow + (int64_t)slot * cols;
        if (vec) {                                               // cols == 4 and 16-byte rows
            const double2 a = reinterpret_cast<const double2*>(r)[0], b = reinterpret_cast<const double2*>(r)[1];
            if (a.x == 0.0) return false;
            p.d[0] = a.y; p.d[1] = b.x; p.d[2] = b.y;
        } else {
            if (r[0] == 0.0) return false;
            p.d[0] = r[1]; p.d[1] = r[2]; p.d[2] = r[3];
        }
        p.px = S.px[slot]; p.py = S.py[slot];
        return true;
    };
    // means, centred sums and gradient over the used slots that `keep` passes; the centred sweep runs only for 3 <= count < below
    auto fit = [&](bool active, auto&& keep, int below, MotionFit& F, int& count) -> bool {
        double sm[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int c = 0;
        if (active)
            for (int slot = lane; slot < s; slot += 64) {
                MotionPoint p;
                if (!point(slot, p) || !keep(p)) continue;
                ++c;
                sm[0] = sm[0] + p.px; sm[1] = sm[1] + p.py;
                sm[2] = sm[2] + p.d[0]; sm[3] = sm[3] + p.d[1]; sm[4] = sm[4] + p.d[2];
            }
        c = wave_sum(c);
#pragma unroll
        for (int q = 0; q < 5; ++q) sm[q] = wave_sum(sm[q]);
        count = c;
        const double n = (double)c;
        F.mx = c > 0 ? sm[0] / n : 0.0; F.my = c > 0 ? sm[1] / n : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { F.md[k] = c > 0 ? sm[2 + k] / n : 0.0; F.gx[k] = 0.0; F.gy[k] = 0.0; }
        const bool enough = active && c >= 3 && c < below;
        double cs[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // xx, xy, yy, then xe_k, ye_k for k = X, Y, Z
        if (enough)
            for (int slot = lane; slot < s; slot += 64) {
                MotionPoint p;
                if (!point(slot, p) || !keep(p)) continue;
                const double x = p.px - F.mx, y = p.py - F.my;
                cs[0] = cs[0] + x * x; cs[1] = cs[1] + x * y; cs[2] = cs[2] + y * y;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double e = p.d[k] - F.md[k];
                    cs[3 + 2 * k] = cs[3 + 2 * k] + x * e; cs[4 + 2 * k] = cs[4 + 2 * k] + y * e;
                }
            }
#pragma unroll
        for (int q = 0; q < 9; ++q) cs[q] = wave_sum(cs[q]);
        const double det = cs[0] * cs[2] - cs[1] * cs[1];
        const bool exists = enough && fabs(det) > 1e-300;
        if (exists) {
#pragma unroll
            for (int k = 0; k < 3; ++k) strain_solve(cs[0], cs[1], cs[2], cs[3 + 2 * k], cs[4 + 2 * k], det, F.gx[k], F.gy[k]);
        }
        return exists;
    };
    // the largest q with the smallest slot among equals, over the wave; every lane gets the slot
    auto worst_fold = [&](double& wq, int& wi) {
        wave_argmax_down(wq, wi);
        wi = __shfl(wi, 0);
    };

    // ---- sweeps 0 - 2: means, centred sums -> gradient, residuals -> SSR and the worst slot ------------------------------------------
    MotionFit F;
    int cnt = 0;
    const bool fit1 = fit(true, [](const MotionPoint&) { return true; }, 0x7fffffff, F, cnt);
    double ss[3] = {0.0, 0.0, 0.0}, wq = 0.0;
    int wi = -1;
    if (fit1 || residual)
        for (int slot = lane; slot < s; slot += 64) {
            MotionPoint p;
            double r[3] = {0.0, 0.0, 0.0};
            const bool used = fit1 && point(slot, p);
            if (used) {
                const double q = motion_resid(F, p, r);
#pragma unroll
                for (int k = 0; k < 3; ++k) ss[k] = ss[k] + r[k] * r[k];
                if (q == q && (wi < 0 || q > wq)) { wq = q; wi = slot; }   // ascending slots: the earliest of equal maxima stays
            }
            if (residual) {
                double* o = residual + (fi * s + slot) * 4;
                o[0] = used ? 1.0 : 0.0; o[1] = r[0]; o[2] = r[1]; o[3] = r[2];
            }
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) ss[k] = wave_sum(ss[k]);
    worst_fold(wq, wi);
    const double n0 = (double)cnt;
    double n_used = n0, flag = fit1 ? 1.0 : 0.0;

    // ---- sweeps 3 - 5: one round of rejection; the kept set is decided by the FIRST fit in every one of them ------------------------
    if (reject_k > 0.0) {                                        // (a kernel argument: the same for every thread)
        const double ssr = (ss[0] + ss[1]) + ss[2];
        const bool rej = fit1 && ssr > 0.0;
        const double thr = (reject_k * reject_k) * (ssr / n0);
        const MotionFit F1 = F;
        auto keep = [&](const MotionPoint& p) -> bool {
            double r[3];
            return motion_resid(F1, p, r) <= thr;
        };
        MotionFit F2;
        int kc = 0;
        if (fit(rej, keep, cnt, F2, kc)) {                       // fewer kept than used, and a fit of their own
            double s2[3] = {0.0, 0.0, 0.0}, wq2 = 0.0;
            int wi2 = -1;
            for (int slot = lane; slot < s; slot += 64) {        // every USED slot gets its residual against the final fit
                MotionPoint p;
                if (!point(slot, p)) continue;
                const bool kept = keep(p);
                double r[3];
                const double q = motion_resid(F2, p, r);
                if (kept) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) s2[k] = s2[k] + r[k] * r[k];
                    if (q == q && (wi2 < 0 || q > wq2)) { wq2 = q; wi2 = slot; }
                }
                if (residual) {
                    double* o = residual + (fi * s + slot) * 4;
                    o[0] = kept ? 1.0 : 2.0; o[1] = r[0]; o[2] = r[1]; o[3] = r[2];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) ss[k] = wave_sum(s2[k]);
            worst_fold(wq2, wi2);
            wi = wi2;
            F = F2; n_used = (double)kc; flag = 2.0;
        }
    }

    if (lane != 0) return;
    const bool any = flag != 0.0;
    if (grad) {
        double* o = grad + fi * 12;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[4 * k] = flag;
            o[4 * k + 1] = any ? F.md[k] - F.gx[k] * F.mx - F.gy[k] * F.my : 0.0;
            o[4 * k + 2] = F.gx[k]; o[4 * k + 3] = F.gy[k];
        }
    }
    if (strain) {
        double* o = strain + fi * VBS_STRAIN_COLS;
        o[0] = flag; o[1] = n0; o[2] = n_used;
        if (any) {
            StrainInv v;
            strain_small(F.gx[0], F.gy[0], F.gx[1], F.gy[1], v);
            strain_finite(F.gx[0], F.gy[0], F.gx[1], F.gy[1], F.gx[2], F.gy[2], v);
            o[3] = v.dilation; o[4] = v.omega; o[5] = v.e1; o[6] = v.e2; o[7] = v.max_shear; o[8] = v.shear_deg;
            o[9] = v.rot_deg; o[10] = v.lambda1; o[11] = v.lambda2; o[12] = v.tilt_deg;
            o[13] = sqrt((ss[0] + ss[1]) / n_used); o[14] = sqrt(ss[2] / n_used);
            o[15] = (double)wi;
        } else {
#pragma unroll
            for (int c = 3; c < 15; ++c) o[c] = 0.0;
            o[15] = -1.0;
        }
    }
}

void launch_motion_series(const double* rec, int s, int cols, const double* pos, const u8* slot_mask, double reject_k,
                          int frame_begin, int frame_end, double* grad, double* strain, double* residual, hipStream_t st) {
    const int nf = frame_end - frame_begin;
    const int vec = cols == 4 && ((uintptr_t)rec & 15) == 0 ? 1 : 0;     // every row then starts on 16 bytes
    hipLaunchKernelGGL(k_motion, dim3((unsigned)(((int64_t)nf + MOTION_WAVES - 1) / MOTION_WAVES)), dim3(MOTION_WAVES * 64), 0, st, rec,
                       s, cols, pos, slot_mask, reject_k, frame_begin, nf, vec, grad, strain, residual);
}

struct LStrainStage {                            // 41 KB
    double px[VBS_FIELD_MAX_SLOTS], py[VBS_FIELD_MAX_SLOTS];
    double d[3][VBS_FIELD_MAX_SLOTS];            // dX, dY, dZ of the frame, 0.0 where the flag is 0
    u8 used[VBS_FIELD_MAX_SLOTS];
};

__global__ __launch_bounds__(1024) void k_local_strain(const double* __restrict__ rec, int s, int cols, const double* __restrict__ pos,
                                                       const int32_t* __restrict__ nbr, int K, int min_count, double det_rel,
                                                       int frame_begin, int n_frames, int vec, double* __restrict__ out) {
    __shared__ LStrainStage S;
    const int i = threadIdx.x;                                   // this thread's slot (the launch gives blockDim.x >= s)
    const bool mine = i < s;
    int nb[VBS_STRAIN_MAX_NBR];                                  // -1: no neighbour; an entry outside [0, s) is never an address
#pragma unroll
    for (int j = 0; j < VBS_STRAIN_MAX_NBR; ++j) {
        nb[j] = -1;
        if (mine && j < K) {
            const int v = nbr[(int64_t)i * K + j];
            nb[j] = v >= 0 && v < s ? v : -1;
        }
    }
    if (mine) { S.px[i] = pos[2 * i]; S.py[i] = pos[2 * i + 1]; }
    const int64_t f0 = (int64_t)blockIdx.x * VBS_LSTRAIN_GROUP;
    const int64_t f1 = f0 + VBS_LSTRAIN_GROUP < n_frames ? f0 + VBS_LSTRAIN_GROUP : n_frames;

    double fl = 0.0, v[3] = {0.0, 0.0, 0.0};
    auto fetch = [&](int64_t f) {                                // this slot's row of emitted frame f
        const double* r = rec + (((int64_t)frame_begin + f) * s + i) * cols;
        if (vec) {
            const double2 a = reinterpret_cast<const double2*>(r)[0], b = reinterpret_cast<const double2*>(r)[1];
            fl = a.x; v[0] = a.y; v[1] = b.x; v[2] = b.y;
        } else {
            fl = r[0]; v[0] = r[1]; v[1] = r[2]; v[2] = r[3];
        }
    };
    if (mine) fetch(f0);
    for (int64_t f = f0; f < f1; ++f) {                          // (f0, f1 are the workgroup's: every barrier is uniform)
        __syncthreads();                                         // every thread is done with the frame before
        if (mine) {
            const bool u = fl != 0.0;                            // an invalid entry is selected out here, never multiplied by zero
            S.used[i] = u ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) S.d[k][i] = u ? v[k] : 0.0;
        }
        __syncthreads();
        if (!mine) continue;
        const bool self = S.used[i] != 0;
        if (f + 1 < f1) fetch(f + 1);                            // in flight under the sums below

        int cnt = 0;
        double sm[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (self) {
#pragma unroll
            for (int j = -1; j < VBS_STRAIN_MAX_NBR; ++j) {      // the member list: i, nbr[i][0], ..
                const int m = j < 0 ? i : nb[j];
                if (m < 0 || !S.used[m]) continue;
                ++cnt;
                sm[0] = sm[0] + S.px[m]; sm[1] = sm[1] + S.py[m];
                sm[2] = sm[2] + S.d[0][m]; sm[3] = sm[3] + S.d[1][m]; sm[4] = sm[4] + S.d[2][m];
            }
        }
        double o[VBS_LSTRAIN_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (self && cnt >= min_count) {
            const double n = (double)cnt;
            const double mx = sm[0] / n, my = sm[1] / n, md[3] = {sm[2] / n, sm[3] / n, sm[4] / n};
            double cs[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = -1; j < VBS_STRAIN_MAX_NBR; ++j) {
                const int m = j < 0 ? i : nb[j];
                if (m < 0 || !S.used[m]) continue;
                const double x = S.px[m] - mx, y = S.py[m] - my;
                cs[0] = cs[0] + x * x; cs[1] = cs[1] + x * y; cs[2] = cs[2] + y * y;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double e = S.d[k][m] - md[k];
                    cs[3 + 2 * k] = cs[3 + 2 * k] + x * e; cs[4 + 2 * k] = cs[4 + 2 * k] + y * e;
                }
            }
            const double det = cs[0] * cs[2] - cs[1] * cs[1];
            if (det > det_rel * (cs[0] * cs[2])) {               // 1 - rho^2 > det_rel; a NaN refuses
                double gx[3], gy[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) strain_solve(cs[0], cs[1], cs[2], cs[3 + 2 * k], cs[4 + 2 * k], det, gx[k], gy[k]);
                StrainInv w;
                strain_small(gx[0], gy[0], gx[1], gy[1], w);
                o[0] = n; o[1] = w.dilation; o[2] = w.omega; o[3] = w.max_shear; o[4] = w.e1; o[5] = w.e2; o[6] = gx[2]; o[7] = gy[2];
            }
        }
        double* dst = out + (f * s + i) * VBS_LSTRAIN_COLS;
#pragma unroll
        for (int c = 0; c < VBS_LSTRAIN_COLS; ++c) dst[c] = o[c];
    }
}

void launch_local_strain(const double* rec, int s, int cols, const double* pos, const int32_t* nbr, int K, int min_count,
                         double det_rel, int frame_begin, int frame_end, double* out, hipStream_t st) {
    const int nf = frame_end - frame_begin;
    const int vec = cols == 4 && ((uintptr_t)rec & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_local_strain, dim3((unsigned)(((int64_t)nf + VBS_LSTRAIN_GROUP - 1) / VBS_LSTRAIN_GROUP)),
                       dim3((unsigned)((s + 63) / 64 * 64)), 0, st, rec, s, cols, pos, nbr, K, min_count, det_rel, frame_begin, nf, vec,
                       out);
}
