// Rigid motion along a recording: for every frame the rotation R, the translation t and optionally the scale s
// that carry a given point set Q (`source`, one row a slot) onto the frame's 3-D points P in the least-squares sense,
//     P ~ s R Q + t,
// by Horn's quaternion form of the absolute-orientation problem, and what that motion leaves per marker.  Float64 without
// contraction, + - * / and sqrt only (but the columns rms, rms0 and the four angles), no atomics, no LDS, no barrier; the operand
// order of every expression is stated in include/vbs.h and restated in tests/helpers/rigid_oracle.py.
//   k_rigid   one wave per frame, VBS_RIGID_GROUP frames a workgroup.  A wave reads the table directly and meets no barrier, so a
//             frame's result cannot depend on the frames next to it.  A fit is three sweeps - count and means, the nine products
//             and the two spreads, the residuals - and the kept set of the one round of rejection takes the same three through the
//             same code (the round loop stays rolled); a last sweep writes the residual record.  The 4 x 4 eigenproblem is
//             the cyclic Jacobi of fit_math.h, every lane alike: the six pairs are unrolled over constant indices and the sweep
//             loop stays rolled, so T and V live in registers (profiles/rigid_resource_usage.txt).
#include "common.h"
#include "fit_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define RGD_WAVES VBS_RIGID_GROUP
static_assert(RGD_WAVES >= 1 && RGD_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_RIGID_COLS == 33, "flag, count, n_used, qm [3], pm [3], w x y z, R [9], t [3], s, rms, rms0, four angles, gap");
static_assert(VBS_RIGID_SWEEPS >= 1, "at least one sweep");

// Horn's N from the nine products H [i * 3 + j] = sum q_i p_j, its leading eigenvector as a unit quaternion with w >= 0, and the
// distance lam - d2 of the two largest eigenvalues.
static __device__ __forceinline__ double rgd_quaternion(const double* H, double* quat) {
    const double Hxx = H[0], Hxy = H[1], Hxz = H[2], Hyx = H[3], Hyy = H[4], Hyz = H[5], Hzx = H[6], Hzy = H[7], Hzz = H[8];
    double T[4][4], V[4][4];
    T[0][0] = (Hxx + Hyy) + Hzz; T[1][1] = (Hxx - Hyy) - Hzz; T[2][2] = (Hyy - Hxx) - Hzz; T[3][3] = (Hzz - Hxx) - Hyy;
    T[0][1] = T[1][0] = Hyz - Hzy; T[0][2] = T[2][0] = Hzx - Hxz; T[0][3] = T[3][0] = Hxy - Hyx;
    T[1][2] = T[2][1] = Hxy + Hyx; T[1][3] = T[3][1] = Hzx + Hxz; T[2][3] = T[3][2] = Hyz + Hzy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < VBS_RIGID_SWEEPS; ++sweep) {
        jacobi_pair<4, 0, 1>(T, V); jacobi_pair<4, 0, 2>(T, V); jacobi_pair<4, 0, 3>(T, V);
        jacobi_pair<4, 1, 2>(T, V); jacobi_pair<4, 1, 3>(T, V); jacobi_pair<4, 2, 3>(T, V);
    }
    // the largest diagonal entry, the smaller index among equals; then the largest of the other three, likewise
    int k = 0;
    double lam = T[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (T[i][i] > lam) { k = i; lam = T[i][i]; v0 = V[0][i]; v1 = V[1][i]; v2 = V[2][i]; v3 = V[3][i]; }
    bool have = false;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i != k && (!have || T[i][i] > d2)) { have = true; d2 = T[i][i]; }
    const double nn = ((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3;
    const double nr = sqrt(nn);
    double w = v0 / nr, x = v1 / nr, y = v2 / nr, z = v3 / nr;
    const double first = x != 0.0 ? x : (y != 0.0 ? y : z);    // the first nonzero of x, y, z (0 where there is none)
    if (w < 0.0 || (w == 0.0 && first < 0.0)) { w = -w; x = -x; y = -y; z = -z; }
    quat[0] = w; quat[1] = x; quat[2] = y; quat[3] = z;
    return lam - d2;
}

// R row-major from the unit quaternion, the stated order
static __device__ __forceinline__ void rgd_rotation(const double* qt, double* R) {
    const double w = qt[0], x = qt[1], y = qt[2], z = qt[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__global__ __launch_bounds__(RGD_WAVES * 64) void k_rigid(const float* __restrict__ table, int m, const double* __restrict__ source,
                                                          const u8* __restrict__ slot_mask, int with_scale, double reject_k,
                                                          double gap_rel, int frame_begin, int n_frames, double* __restrict__ rigid,
                                                          double* __restrict__ coef, double* __restrict__ residual) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * RGD_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                  // (a whole wave: no barrier follows)
    const float* frow = table + ((int64_t)frame_begin + fi) * ((int64_t)m * VBS_TABLE_COLS);

    // the pair (Q, P) of a slot, or false: the common rule
    auto point = [&](int slot, double* q, double* p) -> bool {
        const double* sr = source + (int64_t)slot * 4;
        if (!((!slot_mask || slot_mask[slot]) && sr[0] != 0.0 && row_point(frow + (int64_t)slot * VBS_TABLE_COLS, p))) return false;
        q[0] = sr[1]; q[1] = sr[2]; q[2] = sr[3];
        return true;
    };
    // e = P - (s R Q + t) and e . e
    auto resid = [&](const double* q, const double* p, const double* R, const double* t, double s, double* e) -> double {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double rq = (R[i * 3 + 0] * q[0] + R[i * 3 + 1] * q[1]) + R[i * 3 + 2] * q[2];
            e[i] = p[i] - (s * rq + t[i]);
        }
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    };

    // the fit that stands and the first fit (f_*), which decides the kept set in every later sweep
    double qm[3] = {0.0, 0.0, 0.0}, pm[3] = {0.0, 0.0, 0.0}, quat[4] = {0.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    double f_R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double f_t[3] = {0.0, 0.0, 0.0}, f_s = 0.0, thr = 0.0, s = 0.0, gap = 0.0, ssr = 0.0, ss0 = 0.0;
    int flag = 0, cnt = 0, n_used = 0;
    auto kept = [&](const double* q, const double* p) -> bool {
        double e[3];
        return resid(q, p, f_R, f_t, f_s, e) <= thr;
    };

#pragma unroll 1
    for (int round = 0; round < 2; ++round) {                    // 0: the common set, 1: its kept slots (every test below is wave-uniform)
        const bool second = round == 1;
        double sq[3] = {0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0};
        int c = 0;
        for (int slot = lane; slot < m; slot += 64) {
            double q[3], p[3];
            if (!point(slot, q, p) || (second && !kept(q, p))) continue;
            ++c;
            sq[0] = sq[0] + q[0]; sq[1] = sq[1] + q[1]; sq[2] = sq[2] + q[2];
            sp[0] = sp[0] + p[0]; sp[1] = sp[1] + p[1]; sp[2] = sp[2] + p[2];
        }
        c = wave_sum(c);
#pragma unroll
        for (int k = 0; k < 3; ++k) { sq[k] = wave_sum(sq[k]); sp[k] = wave_sum(sp[k]); }
        const double n = (double)c;
        if (!second) {
            cnt = n_used = c;
#pragma unroll
            for (int k = 0; k < 3; ++k) { qm[k] = c > 0 ? sq[k] / n : 0.0; pm[k] = c > 0 ? sp[k] / n : 0.0; }
        } else if (c >= cnt) {
            break;                                               // nothing was rejected
        }
        if (c < 3) break;
        const double mq[3] = {sq[0] / n, sq[1] / n, sq[2] / n}, mp[3] = {sp[0] / n, sp[1] / n, sp[2] / n};

        double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sqq = 0.0, spp = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double q[3], p[3];
            if (!point(slot, q, p) || (second && !kept(q, p))) continue;
            const double qx = q[0] - mq[0], qy = q[1] - mq[1], qz = q[2] - mq[2];
            const double px = p[0] - mp[0], py = p[1] - mp[1], pz = p[2] - mp[2];
            H[0] = H[0] + qx * px; H[1] = H[1] + qx * py; H[2] = H[2] + qx * pz;
            H[3] = H[3] + qy * px; H[4] = H[4] + qy * py; H[5] = H[5] + qy * pz;
            H[6] = H[6] + qz * px; H[7] = H[7] + qz * py; H[8] = H[8] + qz * pz;
            sqq = sqq + ((qx * qx + qy * qy) + qz * qz);
            spp = spp + ((px * px + py * py) + pz * pz);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = wave_sum(H[k]);
        sqq = wave_sum(sqq); spp = wave_sum(spp);
        double qt[4];
        const double lead = rgd_quaternion(H, qt);
        const double den = sqq + spp;
        const bool formed = den > 0.0;
        const double g = formed ? lead / den : 0.0;
        if (!second) gap = g;
        if (!(formed && g > gap_rel)) break;                     // the two sets do not fix a rotation

        double Rn[9];
        rgd_rotation(qt, Rn);
        double sn = 1.0;
        if (with_scale && sqq > 0.0) {
            double D = Rn[0] * H[0];                             // D = sum_j sum_i R[j][i] H[i][j], j outer, i inner, from the left
            D = D + Rn[1] * H[3]; D = D + Rn[2] * H[6];
            D = D + Rn[3] * H[1]; D = D + Rn[4] * H[4]; D = D + Rn[5] * H[7];
            D = D + Rn[6] * H[2]; D = D + Rn[7] * H[5]; D = D + Rn[8] * H[8];
            sn = D / sqq;
        }
        double tn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double rq = (Rn[i * 3 + 0] * mq[0] + Rn[i * 3 + 1] * mq[1]) + Rn[i * 3 + 2] * mq[2];
            tn[i] = mp[i] - sn * rq;
        }

        double s1 = 0.0, s0 = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double q[3], p[3], e[3];
            if (!point(slot, q, p) || (second && !kept(q, p))) continue;
            s1 = s1 + resid(q, p, Rn, tn, sn, e);
            const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            s0 = s0 + ((dx * dx + dy * dy) + dz * dz);
        }
        s1 = wave_sum(s1); s0 = wave_sum(s0);
        const bool again = !second && reject_k > 0.0 && s1 > 0.0;
        if (again) {                                             // before the fit that stands is replaced: kept() reads f_*
            thr = (reject_k * reject_k) * (s1 / n);
#pragma unroll
            for (int k = 0; k < 9; ++k) f_R[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) f_t[k] = tn[k];
            f_s = sn;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { qm[k] = mq[k]; pm[k] = mp[k]; t[k] = tn[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) quat[k] = qt[k];
        s = sn; gap = g; ssr = s1; ss0 = s0;
        n_used = c; flag = second ? 2 : 1;
        if (!again) break;
    }

    double R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (flag) rgd_rotation(quat, R);                             // (the standing fit keeps its quaternion; the same expressions, the same bits)
    // ---- the residual record: (1, e) of the fit that stands for every used slot ----------------------------------------------------
    if (residual) {
        for (int slot = lane; slot < m; slot += 64) {
            double q[3], p[3], e[3] = {0.0, 0.0, 0.0};
            const bool in = flag >= 1 && point(slot, q, p) && (flag != 2 || kept(q, p));
            if (in) resid(q, p, R, t, s, e);
            double* o = residual + (fi * m + slot) * 4;
            o[0] = in ? 1.0 : 0.0; o[1] = in ? e[0] : 0.0; o[2] = in ? e[1] : 0.0; o[3] = in ? e[2] : 0.0;
        }
    }
    if (lane != 0) return;

    // ---- the columns (every lane holds the same values; lane 0 writes) ---------------------------------------------------------------
    const double fl = (double)flag;
    if (rigid) {
        double* o = rigid + fi * VBS_RIGID_COLS;
        const double nu = (double)n_used;
        const double w = quat[0], x = quat[1], y = quat[2], z = quat[3];
        o[0] = fl; o[1] = (double)cnt; o[2] = nu;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[3 + k] = qm[k]; o[6 + k] = pm[k]; o[22 + k] = t[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[9 + k] = quat[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) o[13 + k] = R[k];
        o[25] = s;
        o[26] = flag ? sqrt(ssr / nu) : 0.0;
        o[27] = flag ? sqrt(ss0 / nu) : 0.0;
        o[28] = flag ? (2.0 * atan2(sqrt((x * x + y * y) + z * z), w)) * VBS_DEG : 0.0;
        o[29] = flag ? atan2(sqrt(R[2] * R[2] + R[5] * R[5]), R[8]) * VBS_DEG : 0.0;
        o[30] = flag ? atan2(R[5], R[2]) * VBS_DEG : 0.0;
        o[31] = flag ? (2.0 * atan2(z, w)) * VBS_DEG : 0.0;
        o[32] = gap;
    }
    if (coef) {
        double* o = coef + fi * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[i * 4] = fl; o[i * 4 + 1] = R[i * 3]; o[i * 4 + 2] = R[i * 3 + 1]; o[i * 4 + 3] = R[i * 3 + 2]; }
        o[12] = fl; o[13] = t[0]; o[14] = t[1]; o[15] = t[2];
    }
}

void launch_rigid_series(const float* table, int m, const double* source, const u8* slot_mask, int with_scale, double reject_k,
                         double gap_rel, int frame_begin, int frame_end, double* rigid, double* coef, double* residual, hipStream_t s) {
    const int nf = frame_end - frame_begin;
    hipLaunchKernelGGL(k_rigid, dim3((unsigned)(((int64_t)nf + RGD_WAVES - 1) / RGD_WAVES)), dim3(RGD_WAVES * 64), 0, s, table, m,
                       source, slot_mask, with_scale, reject_k, gap_rel, frame_begin, nf, rigid, coef, residual);
}
