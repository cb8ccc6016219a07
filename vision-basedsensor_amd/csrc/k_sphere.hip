// Bonnet contact geometry along a recording: the sphere the unloaded markers lie on - fitted per frame or given
// and held -, the markers that lie inside it by more than contact_depth (the contact), the plane through those alone, and from the
// two the contact normal, the tool offset, the spot radius and the spot centre; per marker the radial deviation and, against a given
// point set, the displacement resolved in the shell's own frame.  Float64 without contraction, + - * / and sqrt only (but the two
// angles), no atomics, no LDS, no barrier; the operand order of every expression is stated in include/vbs.h and restated in
// tests/helpers/sphere_oracle.py.
//   k_sphere  one wave per frame, VBS_SPHERE_GROUP frames a workgroup.  A wave reads the table directly and meets no barrier, so a
//             frame's result cannot depend on the frames next to it.  A fit is three sweeps - count and mean, the 13 sums, the radial
//             residuals - and the kept set of the one round of rejection takes the same three through the same code (the round loop
//             stays rolled); two sweeps form the contact set and its scatter, a last one writes the two records.  The 4 x 4 LDL' and
//             the 3 x 3 Jacobi (fit_math.h) run in every lane alike over constant indices, so they live in registers
//             (profiles/sphere_resource_usage.txt).
#include "common.h"
#include "fit_math.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define SPH_WAVES VBS_SPHERE_GROUP
static_assert(SPH_WAVES >= 1 && SPH_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_SPHERE_COLS == 31, "flag, n_fit, n_fit_used, rejected, C [3], R, rms_fit, n_used, n_contact, centroid [3], three "
                                     "depths, deepest, n [3], dist, offset, spot radius, two angles, spot centre [3], plane_rms, gap");
static_assert(VBS_SPHERE_SWEEPS >= 1, "at least one sweep");

// The 4 x 4 normal equations in basis order (ux, uy, uz, 1), all pivots or nothing: false at the first pivot that does not pass.
// beta = (2 cx, 2 cy, 2 cz, kappa).
static __device__ __forceinline__ bool sph_solve(const double (&N)[4][4], const double (&g)[4], double piv_rel, double (&beta)[4]) {
    double Lm[4][4], d[4], y[4];
    if (ldl_factor(N, piv_rel, Lm, d) < 4) return false;
    ldl_forward(Lm, d, g, 4, y);
    ldl_back<4>(Lm, y, beta);
    return true;
}

__global__ __launch_bounds__(SPH_WAVES * 64) void k_sphere(const float* __restrict__ table, int m, int given, double gx, double gy,
                                                           double gz, double gr, const u8* __restrict__ fit_mask,
                                                           const u8* __restrict__ slot_mask, const double* __restrict__ source,
                                                           double contact_depth, double piv_rel, double gap_rel, double reject_k,
                                                           int frame_begin, int n_frames, double* __restrict__ sphere,
                                                           double* __restrict__ radial, double* __restrict__ decomp) {
    const int lane = threadIdx.x & 63;
    const int64_t fi = (int64_t)blockIdx.x * SPH_WAVES + (threadIdx.x >> 6);
    if (fi >= n_frames) return;                                  // (a whole wave: no barrier follows)
    const float* frow = table + ((int64_t)frame_begin + fi) * ((int64_t)m * VBS_TABLE_COLS);

    // the point of a slot selected by `mask`, or false: the used rule
    auto point = [&](const u8* mask, int slot, double* p) -> bool {
        return (!mask || mask[slot]) && row_point(frow + (int64_t)slot * VBS_TABLE_COLS, p);
    };
    // |P - C|^2
    auto dist2 = [](const double* p, const double* c) -> double {
        const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
        return (dx * dx + dy * dy) + dz * dz;
    };

    // the sphere that stands and the first fit (f_*), which decides the kept set in every later sweep
    double C[3] = {0.0, 0.0, 0.0}, R = 0.0, ssr = 0.0, f_C[3] = {0.0, 0.0, 0.0}, f_R = 0.0, thr = 0.0;
    int have = 0, n_fit = 0, n_fit_used = 0, rejected = 0;
    auto kept = [&](const double* p) -> bool {
        const double rho = sqrt(dist2(p, f_C)) - f_R;
        return rho * rho <= thr;
    };

    if (given) {
        C[0] = gx; C[1] = gy; C[2] = gz; R = gr; have = 1;
        int c = 0;
        double s1 = 0.0;
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(fit_mask, slot, p)) continue;
            ++c;
            const double rho = sqrt(dist2(p, C)) - R;
            s1 = s1 + rho * rho;
        }
        n_fit = n_fit_used = wave_sum(c);
        ssr = wave_sum(s1);
    } else {
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {                // 0: the fit set, 1: its kept slots (every test below is wave-uniform)
            const bool second = round == 1;
            double sp[3] = {0.0, 0.0, 0.0};
            int c = 0;
            for (int slot = lane; slot < m; slot += 64) {
                double p[3];
                if (!point(fit_mask, slot, p) || (second && !kept(p))) continue;
                ++c;
                sp[0] = sp[0] + p[0]; sp[1] = sp[1] + p[1]; sp[2] = sp[2] + p[2];
            }
            c = wave_sum(c);
#pragma unroll
            for (int k = 0; k < 3; ++k) sp[k] = wave_sum(sp[k]);
            if (!second) n_fit = n_fit_used = c;
            else if (c >= n_fit) break;                          // nothing was rejected
            if (c < 4) break;
            const double n = (double)c;
            const double pm[3] = {sp[0] / n, sp[1] / n, sp[2] / n};

            // Sx Sy Sz, Sxx Sxy Sxz Syy Syz Szz, Ss, Sxs Sys Szs
            double S[13] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int slot = lane; slot < m; slot += 64) {
                double p[3];
                if (!point(fit_mask, slot, p) || (second && !kept(p))) continue;
                const double ux = p[0] - pm[0], uy = p[1] - pm[1], uz = p[2] - pm[2];
                const double s = (ux * ux + uy * uy) + uz * uz;
                S[0] = S[0] + ux; S[1] = S[1] + uy; S[2] = S[2] + uz;
                S[3] = S[3] + ux * ux; S[4] = S[4] + ux * uy; S[5] = S[5] + ux * uz;
                S[6] = S[6] + uy * uy; S[7] = S[7] + uy * uz; S[8] = S[8] + uz * uz;
                S[9] = S[9] + s;
                S[10] = S[10] + ux * s; S[11] = S[11] + uy * s; S[12] = S[12] + uz * s;
            }
#pragma unroll
            for (int k = 0; k < 13; ++k) S[k] = wave_sum(S[k]);
            double N[4][4];
            N[0][0] = S[3]; N[1][1] = S[6]; N[2][2] = S[8]; N[3][3] = n;
            N[1][0] = N[0][1] = S[4]; N[2][0] = N[0][2] = S[5]; N[2][1] = N[1][2] = S[7];
            N[3][0] = N[0][3] = S[0]; N[3][1] = N[1][3] = S[1]; N[3][2] = N[2][3] = S[2];
            const double g[4] = {S[10], S[11], S[12], S[9]};
            double beta[4] = {0.0, 0.0, 0.0, 0.0};
            if (!sph_solve(N, g, piv_rel, beta)) break;
            const double cx = beta[0] / 2.0, cy = beta[1] / 2.0, cz = beta[2] / 2.0;
            const double R2 = beta[3] + ((cx * cx + cy * cy) + cz * cz);
            if (!(R2 > 0.0)) break;                              // no real sphere
            const double Cn[3] = {pm[0] + cx, pm[1] + cy, pm[2] + cz}, Rn = sqrt(R2);

            double s1 = 0.0;
            for (int slot = lane; slot < m; slot += 64) {
                double p[3];
                if (!point(fit_mask, slot, p) || (second && !kept(p))) continue;
                const double rho = sqrt(dist2(p, Cn)) - Rn;
                s1 = s1 + rho * rho;
            }
            s1 = wave_sum(s1);
            const bool again = !second && reject_k > 0.0 && s1 > 0.0;
            if (again) {                                         // kept() reads f_*
                thr = (reject_k * reject_k) * (s1 / n);
                f_C[0] = Cn[0]; f_C[1] = Cn[1]; f_C[2] = Cn[2]; f_R = Rn;
            }
            C[0] = Cn[0]; C[1] = Cn[1]; C[2] = Cn[2]; R = Rn; ssr = s1;
            n_fit_used = c; have = 1; rejected = second ? 1 : 0;
            if (!again) break;
        }
    }

    // ---- the contact set: the used slots deeper inside the sphere than contact_depth -------------------------------------------------
    const double Rc = R - contact_depth, thr2 = Rc * Rc;
    const bool can = have && Rc > 0.0;
    int nu = 0, nc = 0, bi = -1;
    double sc[3] = {0.0, 0.0, 0.0}, dsum = 0.0, bv = 0.0;
    for (int slot = lane; slot < m; slot += 64) {
        double p[3];
        if (!point(slot_mask, slot, p)) continue;
        ++nu;
        if (!can) continue;
        const double r2 = dist2(p, C);
        if (!(r2 < thr2)) continue;
        ++nc;
        sc[0] = sc[0] + p[0]; sc[1] = sc[1] + p[1]; sc[2] = sc[2] + p[2];
        dsum = dsum + (R - sqrt(r2));
        if (bi < 0 || -r2 > bv) { bv = -r2; bi = slot; }         // (ascending slots: the smaller one among equals stays)
    }
    nu = wave_sum(nu); nc = wave_sum(nc);
#pragma unroll
    for (int k = 0; k < 3; ++k) sc[k] = wave_sum(sc[k]);
    dsum = wave_sum(dsum);
    wave_argmax_down(bv, bi);
    bv = __shfl(bv, 0); bi = __shfl(bi, 0);
    const double ncd = (double)nc;
    double cm[3] = {0.0, 0.0, 0.0};
    if (nc > 0) { cm[0] = sc[0] / ncd; cm[1] = sc[1] / ncd; cm[2] = sc[2] / ncd; }

    // ---- the plane through the contact slots alone ---------------------------------------------------------------------------------------
    double nrm[3] = {0.0, 0.0, 0.0}, dist = 0.0, lmin = 0.0, gap = 0.0;
    bool plane = false;
    if (nc >= 3) {
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};            // xx xy xz yy yz zz
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            if (!point(slot_mask, slot, p) || !(dist2(p, C) < thr2)) continue;
            const double qx = p[0] - cm[0], qy = p[1] - cm[1], qz = p[2] - cm[2];
            A[0] = A[0] + qx * qx; A[1] = A[1] + qx * qy; A[2] = A[2] + qx * qz;
            A[3] = A[3] + qy * qy; A[4] = A[4] + qy * qz; A[5] = A[5] + qz * qz;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = wave_sum(A[k]);
        const double tr = (A[0] + A[3]) + A[5];
        if (tr > 0.0) {
            double T[3][3], V[3][3];
            T[0][0] = A[0]; T[1][1] = A[3]; T[2][2] = A[5];
            T[0][1] = T[1][0] = A[1]; T[0][2] = T[2][0] = A[2]; T[1][2] = T[2][1] = A[4];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
            for (int sweep = 0; sweep < VBS_SPHERE_SWEEPS; ++sweep) {
                jacobi_pair<3, 0, 1>(T, V); jacobi_pair<3, 0, 2>(T, V); jacobi_pair<3, 1, 2>(T, V);
            }
            // the smallest diagonal entry, the smaller index among equals; then the smaller of the other two
            int k = 0;
            double l0 = T[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];
#pragma unroll
            for (int i = 1; i < 3; ++i)
                if (T[i][i] < l0) { k = i; l0 = T[i][i]; v0 = V[0][i]; v1 = V[1][i]; v2 = V[2][i]; }
            bool seen = false;
            double l1 = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (i != k && (!seen || T[i][i] < l1)) { seen = true; l1 = T[i][i]; }
            gap = (l1 - l0) / tr;
            const double nr = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
            double nx = v0 / nr, ny = v1 / nr, nz = v2 / nr;
            double dd = (nx * (C[0] - cm[0]) + ny * (C[1] - cm[1])) + nz * (C[2] - cm[2]);
            if (dd < 0.0) { nx = -nx; ny = -ny; nz = -nz; dd = -dd; }
            if (gap > gap_rel && dd > 0.0) {
                plane = true;
                nrm[0] = nx; nrm[1] = ny; nrm[2] = nz; dist = dd; lmin = l0;
            }
        }
    }

    // ---- the records -----------------------------------------------------------------------------------------------------------------
    if (radial) {
        for (int slot = lane; slot < m; slot += 64) {
            double p[3];
            const bool in = have && point(slot_mask, slot, p);
            double* o = radial + (fi * m + slot) * 2;
            o[0] = in ? 1.0 : 0.0;
            o[1] = in ? sqrt(dist2(p, C)) - R : 0.0;
        }
    }
    if (decomp) {
        for (int slot = lane; slot < m; slot += 64) {
            double p[3], dn = 0.0, dm = 0.0, da = 0.0;
            const double* sr = source + (int64_t)slot * 4;
            bool in = have && point(slot_mask, slot, p) && sr[0] != 0.0;
            if (in) {
                const double qx = sr[1], qy = sr[2], qz = sr[3];
                const double wx = qx - C[0], wy = qy - C[1], wz = qz - C[2];
                const double wn = sqrt((wx * wx + wy * wy) + wz * wz);
                in = wn > 0.0;
                if (in) {
                    const double hx = wx / wn, hy = wy / wn, hz = wz / wn;
                    const double h2 = hx * hx + hy * hy;
                    double ax = 0.0, ay = 1.0, ex = 1.0, ey = 0.0, ez = 0.0;
                    if (h2 != 0.0) {
                        const double h = sqrt(h2);
                        ax = -hy / h; ay = hx / h;
                        ex = ay * hz; ey = -(ax * hz); ez = ax * hy - ay * hx;
                    }
                    const double Dx = p[0] - qx, Dy = p[1] - qy, Dz = p[2] - qz;
                    dn = (Dx * hx + Dy * hy) + Dz * hz;
                    dm = (Dx * ex + Dy * ey) + Dz * ez;
                    da = Dx * ax + Dy * ay;
                }
            }
            double* o = decomp + (fi * m + slot) * 4;
            o[0] = in ? 1.0 : 0.0; o[1] = in ? dn : 0.0; o[2] = in ? dm : 0.0; o[3] = in ? da : 0.0;
        }
    }
    if (lane != 0 || !sphere) return;

    // ---- the columns (every lane holds the same values; lane 0 writes) ---------------------------------------------------------------
    double* o = sphere + fi * VBS_SPHERE_COLS;
#pragma unroll
    for (int k = 0; k < VBS_SPHERE_COLS; ++k) o[k] = 0.0;
    o[0] = !have ? 0.0 : (nc == 0 ? 1.0 : (plane ? 3.0 : 2.0));
    o[1] = (double)n_fit; o[2] = (double)n_fit_used; o[3] = (double)rejected; o[9] = (double)nu;
    o[17] = -1.0;
    if (!have) return;
    o[4] = C[0]; o[5] = C[1]; o[6] = C[2]; o[7] = R;
    o[8] = n_fit_used > 0 ? sqrt(ssr / (double)n_fit_used) : 0.0;
    o[10] = ncd;
    o[30] = gap;
    if (nc == 0) return;
    o[11] = cm[0]; o[12] = cm[1]; o[13] = cm[2];
    o[14] = dsum; o[15] = dsum / ncd; o[16] = R - sqrt(-bv); o[17] = (double)bi;
    if (!plane) return;
    o[18] = nrm[0]; o[19] = nrm[1]; o[20] = nrm[2];
    o[21] = dist; o[22] = R - dist;
    const double h2 = R * R - dist * dist;
    o[23] = sqrt(h2 > 0.0 ? h2 : 0.0);
    o[24] = atan2(sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1]), nrm[2]) * VBS_DEG;
    o[25] = atan2(nrm[1], nrm[0]) * VBS_DEG;
    o[26] = C[0] - dist * nrm[0]; o[27] = C[1] - dist * nrm[1]; o[28] = C[2] - dist * nrm[2];
    o[29] = sqrt((lmin > 0.0 ? lmin : 0.0) / ncd);
}

void launch_sphere_series(const float* table, int m, const double* given, const u8* fit_mask, const u8* slot_mask, const double* source,
                          double contact_depth, double piv_rel, double gap_rel, double reject_k, int frame_begin, int frame_end,
                          double* sphere, double* radial, double* decomp, hipStream_t s) {
    const int nf = frame_end - frame_begin;
    const double gx = given ? given[0] : 0.0, gy = given ? given[1] : 0.0, gz = given ? given[2] : 0.0, gr = given ? given[3] : 0.0;
    hipLaunchKernelGGL(k_sphere, dim3((unsigned)(((int64_t)nf + SPH_WAVES - 1) / SPH_WAVES)), dim3(SPH_WAVES * 64), 0, s, table, m,
                       given ? 1 : 0, gx, gy, gz, gr, fit_mask, slot_mask, source, contact_depth, piv_rel, gap_rel, reject_k,
                       frame_begin, nf, sphere, radial, decomp);
}
