// a13: _marker_center's last step (marker_detection.py:196-249) from the tables the labelling kernels leave.
//   k_finalize  : per frame: centroids, fitEllipse (:208) from the vertex moments via two normal-
//                 equation solves in float64, then the sequential contour <-> centre matching (:203-243).
//   k_finalize_track : the same, followed by the frame's tracking rows (track_common.h) in the same launch.
#include "ccl_common.h"
#include "track_common.h"

// fitEllipse from vertex moments (see oracle/stages.py:fit_ellipse for the algorithm being followed)
// Gaussian elimination with partial pivoting, fully unrolled: the row swap is a chain of predicated exchanges instead of
// a run-time row index, so the system stays in registers (indexed by a run-time pivot row it lived in scratch memory:
// 288 bytes per lane).  Same operations in the same order as the rolled form.
template <int N>
__device__ __forceinline__ bool solve_sym(double (&A)[N * N], double (&b)[N]) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        int p = c;
        double best = fabs(A[c * N + c]);
#pragma unroll
        for (int r = c + 1; r < N; ++r)
            if (fabs(A[r * N + c]) > best) { best = fabs(A[r * N + c]); p = r; }
        if (!(best > 1e-300)) return false;
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            if (p == r) {
#pragma unroll
                for (int k = 0; k < N; ++k) { const double t = A[c * N + k]; A[c * N + k] = A[r * N + k]; A[r * N + k] = t; }
                const double t = b[c]; b[c] = b[r]; b[r] = t;
            }
        }
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            const double f = A[r * N + c] / A[c * N + c];
#pragma unroll
            for (int k = c; k < N; ++k) A[r * N + k] -= f * A[c * N + k];
            b[r] -= f * b[c];
        }
    }
#pragma unroll
    for (int c = N - 1; c >= 0; --c) {
        double v = b[c];
#pragma unroll
        for (int k = c + 1; k < N; ++k) v -= A[c * N + k] * b[k];
        b[c] = v / A[c * N + c];
    }
    return true;
}

// m[a][b] (a+b<=4) about a point shifted by (sx, sy): sum (x-sx)^a (y-sy)^b
__device__ __forceinline__ void shift_moments(const double (&in)[5][5], double sx, double sy, double (&out)[5][5]) {
    const double C[5][5] = {{1, 0, 0, 0, 0}, {1, 1, 0, 0, 0}, {1, 2, 1, 0, 0}, {1, 3, 3, 1, 0}, {1, 4, 6, 4, 1}};
    const double px[5] = {1, -sx, sx * sx, -sx * sx * sx, sx * sx * sx * sx};
    const double py[5] = {1, -sy, sy * sy, -sy * sy * sy, sy * sy * sy * sy};
    // (every loop has constant bounds and is unrolled: the tables stay in registers)
#pragma unroll
    for (int a = 0; a <= 4; ++a)
#pragma unroll
        for (int b = 0; b <= 4; ++b) {
            if (a + b > 4) continue;
            double v = 0;
#pragma unroll
            for (int i = 0; i <= 4; ++i)
#pragma unroll
                for (int j = 0; j <= 4; ++j)
                    if (i <= a && j <= b) v += C[a][i] * C[b][j] * px[a - i] * py[b - j] * in[i][j];
            out[a][b] = v;
        }
}

// Did the int64 vertex moments S of a contour stay inside 64 bits?  With x, y the integer offsets from the first pixel
// (|x| <= W - 1, 0 <= y <= H - 1) every |x^a y^b|, a + b <= 4, is at most 1 + x^4 + y^4, so every |S[k]| is at most
// n + sum x^4 + sum y^4 <= n + S[3] (W - 1)^2 + S[5] (H - 1)^2.  n, S[3] = sum x^2 and S[5] = sum y^2 themselves cannot
// overflow inside the run capacity ("Range of the vertex moments": below 2^20, 2^44 and 2^50), so the test is sound; it refuses
// from about 5/3 of the true fourth moment, i.e. a contour 10 % shorter than the first that overflows.  (The sums are
// accumulated modulo 2^64, so only the final value has to fit.)
__device__ __forceinline__ bool moments_in_range(const i64* S, int H, int W) {
    const double wx = (double)(W - 1) * (double)(W - 1), wy = (double)(H - 1) * (double)(H - 1);
    return (double)S[0] + (double)S[3] * wx + (double)S[5] * wy < 9.0e18;           // 2^63 = 9.22e18
}

// out: cx, cy, w, h, angle (float32-rounded, w <= h), nvert, ok
__device__ void fit_ellipse_moments(const i64* S, int ax, int ay, double* out) {
    const double PI = 3.14159265358979323846;
    double n = (double)S[0];
    out[5] = n;
    out[6] = 0.0;
    if (S[0] < 5) return;
    // float32 mean of the absolute coordinates, like Point2f accumulation in cv2
    float cx32 = (float)((double)S[0] * ax + (double)S[1]) / (float)n;
    float cy32 = (float)((double)S[0] * ay + (double)S[2]) / (float)n;
    double M0[5][5] = {{0}}, M[5][5];
    M0[0][0] = (double)S[0];
    M0[1][0] = (double)S[1];  M0[0][1] = (double)S[2];
    M0[2][0] = (double)S[3];  M0[1][1] = (double)S[4];  M0[0][2] = (double)S[5];
    M0[3][0] = (double)S[6];  M0[2][1] = (double)S[7];  M0[1][2] = (double)S[8];  M0[0][3] = (double)S[9];
    M0[4][0] = (double)S[10]; M0[3][1] = (double)S[11]; M0[2][2] = (double)S[12]; M0[1][3] = (double)S[13];
    M0[0][4] = (double)S[14];
    shift_moments(M0, (double)cx32 - ax, (double)cy32 - ay, M);
    double r2 = (M[2][0] + M[0][2]) / n;
    if (!(r2 > 0.0)) return;
    double scale = 100.0 / (n * sqrt(r2) * 1.2732395447351628);
    double sp[5] = {1, scale, scale * scale, scale * scale * scale, scale * scale * scale * scale};
    double m[5][5];
#pragma unroll
    for (int a = 0; a <= 4; ++a)
#pragma unroll
        for (int b = 0; b <= 4; ++b)
            if (a + b <= 4) m[a][b] = M[a][b] * sp[a + b];
    double A[25] = {
        m[4][0],  m[2][2],  m[3][1],  -m[3][0], -m[2][1],
        m[2][2],  m[0][4],  m[1][3],  -m[1][2], -m[0][3],
        m[3][1],  m[1][3],  m[2][2],  -m[2][1], -m[1][2],
        -m[3][0], -m[1][2], -m[2][1], m[2][0],  m[1][1],
        -m[2][1], -m[0][3], -m[1][2], m[1][1],  m[0][2]};
    double g[5] = {-1e4 * m[2][0], -1e4 * m[0][2], -1e4 * m[1][1], 1e4 * m[1][0], 1e4 * m[0][1]};
    // conditioning guard, in the spirit of cv2's singular-value test (w[0]*FLT_EPSILON > w[4])
    double tr = A[0] + A[6] + A[12] + A[18] + A[24];
    if (!solve_sym<5>(A, g)) return;
#pragma unroll
    for (int i = 0; i < 5; ++i) if (!isfinite(g[i])) return;
    (void)tr;
    double det = 4.0 * g[0] * g[1] - g[2] * g[2];
    if (!(fabs(det) > 1e-300)) return;
    double rp0 = (2.0 * g[1] * g[3] - g[2] * g[4]) / det;
    double rp1 = (2.0 * g[0] * g[4] - g[2] * g[3]) / det;
    double mu[5][5];
    shift_moments(m, rp0, rp1, mu);
    double A3[9] = {mu[4][0], mu[2][2], mu[3][1], mu[2][2], mu[0][4], mu[1][3], mu[3][1], mu[1][3], mu[2][2]};
    double g3[3] = {mu[2][0], mu[0][2], mu[1][1]};
    if (!solve_sym<3>(A3, g3)) return;
    const double min_eps = 1e-8;
    double ang = -0.5 * atan2(g3[2], g3[1] - g3[0]);
    double t;
    if (fabs(g3[2]) > min_eps) t = g3[2] / sin(-2.0 * ang);
    else t = g3[1] - g3[0];
    double r_2 = fabs(g3[0] + g3[1] - t);
    if (r_2 > min_eps) r_2 = sqrt(2.0 / r_2);
    double r_3 = fabs(g3[0] + g3[1] + t);
    if (r_3 > min_eps) r_3 = sqrt(2.0 / r_3);
    float ecx = (float)(rp0 / scale) + cx32;
    float ecy = (float)(rp1 / scale) + cy32;
    float wd = (float)(r_2 * 2.0 / scale);
    float ht = (float)(r_3 * 2.0 / scale);
    float fang = (float)(ang * 180.0 / PI);
    if (wd > ht) {
        float tt = wd; wd = ht; ht = tt;
        fang = (float)(90.0 + ang * 180.0 / PI);
    }
    if (fang < -180.f) fang += 360.f;
    if (fang > 360.f) fang -= 360.f;
    if (!(isfinite(wd) && isfinite(ht) && isfinite(ecx) && isfinite(ecy))) return;
    out[0] = ecx; out[1] = ecy; out[2] = wd; out[3] = ht; out[4] = fang;
    out[6] = 1.0;
}

// cv2.pointPolygonTest(contour, pt, False) >= 0 for the outer border polygon of component cid, decided from the 2x2
// pixel cell around the (float32-rounded) point; pr = component ids of the cell's pixels (x, y), (x+1, y), (x, y+1),
// (x+1, y+1) as left by k_ccl / k_probe_slow (0xFFFF = background or outside the image).
__device__ bool inside_polygon(const unsigned short* __restrict__ pr, double px, double py, u32 cid) {
    const float xf = (float)px, yf = (float)py;
    const float fx = xf - floorf(xf), fy = yf - floorf(yf);
    const bool c00 = pr[0] == cid;
    if (fx == 0.f && fy == 0.f) return c00;
    if (fy == 0.f) return c00 && pr[1] == cid;
    if (fx == 0.f) return c00 && pr[2] == cid;
    const bool c10 = pr[1] == cid, c01 = pr[2] == cid, c11 = pr[3] == cid;
    const int cnt = (int)c00 + c10 + c01 + c11;
    if (cnt == 4) return true;
    if (cnt == 3) {
        if (!c11) return fx + fy <= 1.f;
        if (!c00) return fx + fy >= 1.f;
        if (!c10) return fy >= fx;
        return fx >= fy;
    }
    if (cnt == 2) {
        if (c00 && c11) return fx == fy;
        if (c10 && c01) return fx + fy == 1.f;
    }
    return false;
}

// frame n, by one workgroup of 256 threads
__device__ __forceinline__ void finalize_frame(int n, const u32* __restrict__ ncomp_all,
                                               const u64* __restrict__ band_sums,
                                               const u32* __restrict__ area_first,
                                               const i64* __restrict__ area_sums,
                                               const unsigned short* __restrict__ probe_all,
                                               u32* __restrict__ fstat, double* __restrict__ ell_all,
                                               double* __restrict__ det64, int32_t* __restrict__ cnt64,
                                               double* __restrict__ det32, int32_t* __restrict__ cnt32,
                                               int H, int W, int WW, int maxm, int stop, int force_seq) {
    __shared__ double bx[1024], by[1024];
    __shared__ u8 unmatched[1024];
    __shared__ int claim[1024], wsum[4];
    // per opened component (at most CCL_OPEN_COMPS = 512 of them: k_stage, k_stage_lat and k_label all stop there)
    __shared__ int best_of[CCL_OPEN_COMPS];
    __shared__ double thr_s[CCL_OPEN_COMPS], ecx_s[CCL_OPEN_COMPS], ecy_s[CCL_OPEN_COMPS];   // (:219) threshold, ellipse centre
    __shared__ u64 best_d[CCL_OPEN_COMPS];
    __shared__ int dup_s;
    const int tid = threadIdx.x;
    int status = (int)fstat[n * 8 + 2];
    if (status != 0) {
        if (tid == 0) { cnt64[n] = status; if (cnt32) cnt32[n] = status; }
        return;
    }
    const int nb_ = min((int)ncomp_all[n * 2 + 0], 1024), na = min((int)ncomp_all[n * 2 + 1], CCL_OPEN_COMPS);   // (never past the tables)
    const u64* bs = band_sums + (int64_t)n * maxm * 4;
    for (int i = tid; i < nb_; i += blockDim.x) {
        double c = (double)bs[i * 4 + 0];
        bx[i] = (double)bs[i * 4 + 1] / c;             // center_of_mass: integer sums, one division
        by[i] = (double)bs[i * 4 + 2] / c;
        unmatched[i] = 1;
    }
    double* ell = ell_all + (int64_t)n * maxm * 8;
    const u32* af = area_first + (int64_t)n * maxm;
    int wide = 0;
    for (int i = tid; i < na; i += blockDim.x) {
        u32 fp = af[i];
        const i64* S = area_sums + ((int64_t)n * maxm + i) * VBS_AREA_SUMS;
        wide |= !moments_in_range(S, H, W);
        fit_ellipse_moments(S, fp % W, fp / W, ell + i * 8);
    }
    if (__syncthreads_or(wide)) {                       // a contour too long for 64-bit moments: the frame is over capacity
        if (tid == 0) {
            cnt64[n] = VBS_ECAPACITY;
            if (cnt32) cnt32[n] = VBS_ECAPACITY;
            atomicMin((int*)&fstat[n * 8 + 2], VBS_ECAPACITY);
        }
        return;
    }
    if (stop == 1) return;
    const unsigned short* probe = probe_all + (int64_t)n * maxm * 4;
    double* d64 = det64 + (int64_t)n * maxm * 6;
    double* d32 = det32 ? det32 + (int64_t)n * maxm * 6 : nullptr;

    // ---- matching (:203-243).  The reference walks the contours in order and gives each the nearest
    // still-unmatched centre inside it.  Every contour first gets its nearest admissible centre among
    // ALL centres, in parallel; if no centre is claimed twice, the sequential walk would have made exactly
    // these choices (a contour loses its first choice only to an earlier contour with the same choice).
    // Otherwise (never seen on marker frames) one wave replays the reference's sequential loop.
    // A centre can only lie inside the polygon of a component that owns a pixel of the 2x2 cell around it (every
    // accepting branch of inside_polygon needs one), so the search runs from the centres: a thread per centre tries the
    // at most four components of its probe cell, and a contour keeps the smallest (distance, index) offered to it - the
    // order the reference's strict "<" over ascending indices produces - through two LDS atomic minima: the distance's
    // bit pattern (monotone for non-negative doubles), then the index among the centres at that distance.
    for (int i = tid; i < nb_; i += blockDim.x) claim[i] = 0;
    for (int c = tid; c < na; c += blockDim.x) {
        const double* e = ell + c * 8;
        double thr = -1.0;
        if (e[6] != 0.0 && e[5] >= 5.0) {               // len(contour) >= 5 (:204) and a valid fit
            const double w = e[2], hh = e[3], minor = (w > hh) ? hh : w;
            if (!(minor < 5.0)) thr = (minor / 10.0) * (minor / 10.0);     // (:219)
        }
        thr_s[c] = thr;
        ecx_s[c] = e[0]; ecy_s[c] = e[1];               // (the matching below reads the centres a few times: not from memory)
        best_d[c] = ~0ull;
        best_of[c] = 0x7FFFFFFF;
    }
    if (tid == 0) dup_s = force_seq;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = tid; i < nb_; i += blockDim.x) {
            const unsigned short* pr = probe + i * 4;
            const double cx = bx[i], cy = by[i];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const u32 cid = pr[q4];
                if (cid >= (u32)na) continue;
                bool seen = false;
#pragma unroll
                for (int q5 = 0; q5 < 4; ++q5) seen |= (q5 < q4) && (pr[q5] == cid);
                if (seen) continue;
                const double thr = thr_s[cid];
                if (!(thr >= 0.0)) continue;
                const double dx = cx - ecx_s[cid], dy = cy - ecy_s[cid], d = dx * dx + dy * dy;
                if (!(d < thr) || !inside_polygon(pr, cx, cy, cid)) continue;
                const u64 key = (u64)__double_as_longlong(d);
                if (pass == 0) atomicMin(&best_d[cid], key);
                else if (key == best_d[cid]) atomicMin(&best_of[cid], i);
            }
        }
        __syncthreads();
    }
    for (int c = tid; c < na; c += blockDim.x) {
        const int bi = best_of[c] == 0x7FFFFFFF ? -1 : best_of[c];
        best_of[c] = bi;
        if (bi >= 0 && atomicAdd(&claim[bi], 1) > 0) dup_s = 1;
    }
    __syncthreads();
    if (!dup_s) {
        // output order = contour order = descending component id; rank by a block scan over reversed ids
        const int per = (na + blockDim.x - 1) / blockDim.x;
        const int r0 = tid * per, r1 = min(r0 + per, na);
        int mine = 0;
        for (int r = r0; r < r1; ++r) mine += (best_of[na - 1 - r] >= 0);
        int inc = mine;
        const int lane = tid & 63, wave = tid >> 6;
        for (int d = 1; d < 64; d <<= 1) { int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int base = inc - mine;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        for (int r = r0; r < r1; ++r) {
            int ci = na - 1 - r, bi = best_of[ci];
            if (bi < 0) continue;
            const double* e = ell + ci * 8;
            double w = e[2], hh = e[3], ang = e[4], major, minor, eang;
            if (w > hh) { major = w; minor = hh; eang = ang; }
            else { major = hh; minor = w; eang = ang + 90.0; }
            double* o = d64 + base * 6;
            o[0] = bx[bi]; o[1] = by[bi]; o[2] = major; o[3] = minor; o[4] = eang; o[5] = bi + 1;
            if (d32) {
                double* f = d32 + base * 6;
                f[0] = bx[bi]; f[1] = by[bi]; f[2] = major; f[3] = minor; f[4] = eang; f[5] = bi + 1;
            }
            ++base;
        }
        if (tid == (int)blockDim.x - 1) { cnt64[n] = base; if (cnt32) cnt32[n] = base; }
        return;
    }
    if (tid >= 64) return;
    // ---- sequential replay in cv2 contour order (last component found first), one wave -------------
    int count = 0;
    for (int ci = na - 1; ci >= 0; --ci) {
        const double* e = ell + ci * 8;
        if (e[6] == 0.0 || e[5] < 5.0) continue;       // len(contour) < 5 (:204) or no fit
        double ecx = e[0], ecy = e[1], w = e[2], hh = e[3], ang = e[4];
        double major, minor, eang;
        if (w > hh) { major = w; minor = hh; eang = ang; }
        else { major = hh; minor = w; eang = ang + 90.0; }
        if (minor < 5.0) continue;                      // (:219)
        double thr = (minor / 10.0) * (minor / 10.0);
        double best = 1e300;
        int bi = -1;
        for (int i = tid; i < nb_; i += 64) {
            if (!unmatched[i]) continue;
            double dx = bx[i] - ecx, dy = by[i] - ecy;
            double d = dx * dx + dy * dy;
            if (d < thr && d < best &&
                inside_polygon(probe + i * 4, bx[i], by[i], (u32)ci)) {
                best = d; bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            double ob = __shfl_xor(best, off);
            int oi = __shfl_xor(bi, off);
            if (oi >= 0 && (bi < 0 || ob < best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        }
        if (bi >= 0) {
            if (tid == 0) {
                unmatched[bi] = 0;
                double* o = d64 + count * 6;
                o[0] = bx[bi]; o[1] = by[bi]; o[2] = major; o[3] = minor; o[4] = eang; o[5] = bi + 1;
                if (d32) {
                    double* f = d32 + count * 6;
                    f[0] = bx[bi]; f[1] = by[bi]; f[2] = major; f[3] = minor; f[4] = eang; f[5] = bi + 1;
                }
            }
            ++count;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (tid == 0) { cnt64[n] = count; if (cnt32) cnt32[n] = count; }
}

__global__ __launch_bounds__(256) void k_finalize(const u32* __restrict__ ncomp_all, const u64* __restrict__ band_sums,
                                                  const u32* __restrict__ area_first, const i64* __restrict__ area_sums,
                                                  const unsigned short* __restrict__ probe_all,
                                                  u32* __restrict__ fstat, double* __restrict__ ell_all,
                                                  double* __restrict__ det64, int32_t* __restrict__ cnt64,
                                                  double* __restrict__ det32, int32_t* __restrict__ cnt32,
                                                  int H, int W, int WW, int maxm, int stop, int force_seq) {
    finalize_frame(blockIdx.x, ncomp_all, band_sums, area_first, area_sums, probe_all, fstat, ell_all, det64, cnt64, det32, cnt32,
                   H, W, WW, maxm, stop, force_seq);
}

void launch_finalize(vbs_handle* h, Workspace& w, int nb, double* det, int32_t* counts, hipStream_t s) {
    VBS_LAUNCH(h, s, "k_finalize", k_finalize, dim3(nb), dim3(256), 0, s, w.ncomp, w.band_sums, w.area_first,
                       w.area_sums, w.probe, w.fstat, w.ell, w.det64,
                       w.cnt, det, counts, h->H, h->W, h->WW, h->maxm, VBS_KNOB("VBS_FINAL_STOP"),
                       h->force_seq_match ? 1 : 0);                 // (vbs_set_option: exercises the sequential replay)
}

// The few-frames path: a13 and a15 (+ a19 / a20) of a frame in ONE launch - the same workgroup fits and matches the
// frame's detections, then tracks them against the reference IDs (a launch on a dependent stream costs ~ 5 us, as much as
// either kernel works on one frame).  Same code, same results as k_finalize followed by k_track.
__global__ __launch_bounds__(256) void k_finalize_track(const u32* __restrict__ ncomp_all, const u64* __restrict__ band_sums,
                                                        const u32* __restrict__ area_first, const i64* __restrict__ area_sums,
                                                        const unsigned short* __restrict__ probe_all,
                                                        u32* __restrict__ fstat, double* __restrict__ ell_all,
                                                        double* __restrict__ det64, int32_t* __restrict__ cnt64,
                                                        double* __restrict__ det32, int32_t* __restrict__ cnt32,
                                                        int H, int W, int WW, int maxm, int force_seq,
                                                        const double* __restrict__ ref_xy, int m_ref, double min_dist,
                                                        float* __restrict__ table, int do3d, CamD cam, double min_size) {
    finalize_frame(blockIdx.x, ncomp_all, band_sums, area_first, area_sums, probe_all, fstat, ell_all, det64, cnt64, det32, cnt32,
                   H, W, WW, maxm, 0, force_seq);
    // (the frame's detections and count were written by THIS workgroup: the barrier's workgroup-scope release / acquire is
    //  all their readers need - an agent-scope fence here writes back and invalidates the XCD's L2 for nothing)
    __syncthreads();
    track_frame(blockIdx.x, det64, cnt64, maxm, ref_xy, m_ref, min_dist, table, do3d, cam, min_size);
}

void launch_finalize_track(vbs_handle* h, Workspace& w, int nb, double* det, int32_t* counts, const double* ref_xy, int m_ref,
                           double min_dist, float* table, const vbs_camera* cam, double min_size, hipStream_t s) {
    CamD c{};
    if (cam) c = make_cam(*cam);
    VBS_LAUNCH(h, s, "k_finalize_track", k_finalize_track, dim3(nb), dim3(256), 0, s, w.ncomp, w.band_sums, w.area_first,
               w.area_sums, w.probe, w.fstat, w.ell, w.det64, w.cnt, det, counts, h->H, h->W, h->WW, h->maxm,
               h->force_seq_match ? 1 : 0, ref_xy, m_ref, min_dist, table, cam ? 1 : 0, c, min_size);
}
