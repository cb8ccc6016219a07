// Chessboard corners (row f8): cv2.findChessboardCorners + cv2.cornerSubPix of intrinsic_calibration.py:76-81 and
// DiameterValidation.py:50, restated.  tests/helpers/chess_oracle.py states the same three steps in NumPy.
//   k_chess_response  gray tile + 9-pixel halo in LDS once -> integer ChESS response of the tile + 4 -> 9x9 non-maximum
//                     suppression -> one 64-bit key per candidate in the slot of its 5x5 cell (two candidates never share a
//                     cell, so a tile has CH_SLOTS slots and nothing depends on scheduling).  The response map itself leaves
//                     the CU only through the nullable `response` output.
//   k_chess_order     one workgroup per frame: the VBS_CHESS_MAX_CANDIDATES largest keys (bitwise search for the cut, rank sort),
//                     then one thread per seed walks its lattice; the first seed whose maximal lattice is pw x ph wins.  Integer
//                     arithmetic only.
//   k_corner_subpix   one wave per corner: cv2.cornerSubPix; float32 patch and window, float64 sums reduced in a fixed tree.
// No float atomics anywhere; the integer LDS atomics of k_chess_order only count, and what they count does not depend on order.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)           // the sub-pixel arithmetic is compared with NumPy, which fuses nothing

#define CH_TW 32
#define CH_TH 16
#define CH_HALO 9                        // 5 (ring radius) + 4 (suppression radius)
#define CH_CELL 5
#define CH_SX ((CH_TW + CH_CELL - 1) / CH_CELL)
#define CH_SY ((CH_TH + CH_CELL - 1) / CH_CELL)
#define CH_SLOTS (CH_SX * CH_SY)
#define CH_GW (CH_TW + 2 * CH_HALO)
#define CH_GH (CH_TH + 2 * CH_HALO)
#define CH_RW (CH_TW + 8)
#define CH_RH (CH_TH + 8)
#define CH_KEY_BITS 46                   // R <= 5 * 4 * 510 < 2^14 above the 32 position bits
#define CH_NEG INT32_MIN
#define CH_STRENGTH_RATIO 8              // weak maxima of texture between the corners of a real shot take no part in a walk

static __device__ __forceinline__ int ch_abs(int v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(256) void k_chess_response(const u8* __restrict__ gray, int h, int w, int64_t stride_n,
                                                        int64_t stride_row, u64* __restrict__ slots,
                                                        int32_t* __restrict__ response) {
    __shared__ u8 g[CH_GH][CH_GW + 2];
    __shared__ int r[CH_RH][CH_RW];
    __shared__ u64 sl[CH_SLOTS];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * CH_TW, y0 = blockIdx.y * CH_TH;
    const u8* src = gray + (int64_t)n * stride_n;
    for (int i = tid; i < CH_GH * CH_GW; i += 256) {
        const int ly = i / CH_GW, lx = i % CH_GW, py = y0 - CH_HALO + ly, px = x0 - CH_HALO + lx;
        g[ly][lx] = (px >= 0 && px < w && py >= 0 && py < h) ? src[(int64_t)py * stride_row + px] : (u8)0;
    }
    if (tid < CH_SLOTS) sl[tid] = 0;
    __syncthreads();
    for (int i = tid; i < CH_RH * CH_RW; i += 256) {
        const int ry = i / CH_RW, rx = i % CH_RW, py = y0 - 4 + ry, px = x0 - 4 + rx;
        int v = CH_NEG;
        if (px >= 5 && px < w - 5 && py >= 5 && py < h - 5) {
            const int cy = ry + 5, cx = rx + 5;      // the same pixel in g
            const int dx[16] = {0, 2, 3, 5, 5, 5, 3, 2, 0, -2, -3, -5, -5, -5, -3, -2};
            const int dy[16] = {5, 5, 3, 2, 0, -2, -3, -5, -5, -5, -3, -2, 0, 2, 3, 5};
            int s[16], tot = 0, sr = 0, dr = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) { s[k] = g[cy + dy[k]][cx + dx[k]]; tot += s[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) sr += ch_abs((s[k] + s[k + 8]) - (s[k + 4] + s[k + 12]));
#pragma unroll
            for (int k = 0; k < 8; ++k) dr += ch_abs(s[k] - s[k + 8]);
            const int loc = g[cy][cx] + g[cy - 1][cx] + g[cy + 1][cx] + g[cy][cx - 1] + g[cy][cx + 1];
            v = 5 * (sr - dr) - ch_abs(5 * tot - 16 * loc);
        }
        r[ry][rx] = v;
    }
    __syncthreads();
    for (int i = tid; i < CH_TH * CH_TW; i += 256) {
        const int ly = i / CH_TW, lx = i % CH_TW, py = y0 + ly, px = x0 + lx;
        if (px >= w || py >= h) continue;
        const int v = r[ly + 4][lx + 4];
        if (response) response[((int64_t)n * h + py) * w + px] = v;
        if (v <= 0) continue;
        bool keep = true;
        for (int dy = -4; dy <= 4 && keep; ++dy)
            for (int dx = -4; dx <= 4; ++dx) {
                const int o = r[ly + 4 + dy][lx + 4 + dx];
                const bool before = dy < 0 || (dy == 0 && dx < 0);
                if ((dx | dy) != 0 && (before ? o >= v : o > v)) { keep = false; break; }
            }
        if (keep) sl[(ly / CH_CELL) * CH_SX + lx / CH_CELL] = ((u64)(u32)v << 32) | (u64)(0xFFFFFFFFu - (u32)(py * w + px));
    }
    __syncthreads();
    if (tid < CH_SLOTS)
        slots[(((int64_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * CH_SLOTS + tid] = sl[tid];
}

// ---- ordering: the per-seed lattice walk (chess_oracle._Walk, statement for statement) ----------------------------------------
struct ChPts { const int* x; const int* y; int m; };

static __device__ int ch_find(const ChPts& p, int qx, int qy, i64 lim2) {     // nearest (lowest index on ties), 16 d^2 <= lim2
    int best = -1;
    i64 bd = INT64_MAX;
    for (int k = 0; k < p.m; ++k) {
        const i64 dx = p.x[k] - qx, dy = p.y[k] - qy, d = dx * dx + dy * dy;
        if (d < bd) { bd = d; best = k; }
    }
    return (best >= 0 && 16 * bd <= lim2) ? best : -1;
}

// walk from `start` by (sx, sy), the step re-estimated at every corner; the indices go to out[]; -1 = more than `limit`
static __device__ int ch_chain(const ChPts& p, int start, int sx, int sy, int limit, unsigned char* out) {
    int n = 0, cur = start;
    for (;;) {
        const int c = ch_find(p, p.x[cur] + sx, p.y[cur] + sy, (i64)sx * sx + (i64)sy * sy);
        if (c < 0) return n;
        if (n == limit) return -1;
        out[n++] = (unsigned char)c;
        sx = p.x[c] - p.x[cur];
        sy = p.y[c] - p.y[cur];
        cur = c;
    }
}

// the rest of a row whose element c0 is already in nw[]: 1 complete, -1 incomplete
static __device__ int ch_fill_row(const ChPts& p, const unsigned char* row, unsigned char* nw, int n, int c0) {
    for (int c = c0 + 1; c < n; ++c) {
        const int sx = p.x[nw[c - 1]] - p.x[row[c - 1]], sy = p.y[nw[c - 1]] - p.y[row[c - 1]];
        const int f = ch_find(p, p.x[row[c]] + sx, p.y[row[c]] + sy, (i64)sx * sx + (i64)sy * sy);
        if (f < 0) return -1;
        nw[c] = (unsigned char)f;
    }
    for (int c = c0 - 1; c >= 0; --c) {
        const int sx = p.x[nw[c + 1]] - p.x[row[c + 1]], sy = p.y[nw[c + 1]] - p.y[row[c + 1]];
        const int f = ch_find(p, p.x[row[c]] + sx, p.y[row[c]] + sy, (i64)sx * sx + (i64)sy * sy);
        if (f < 0) return -1;
        nw[c] = (unsigned char)f;
    }
    return 1;
}

// g: seed row, then the rows on the +v side in order, then the rows on the -v side going away from the seed.
// Returns nu (corners per row) and sets npos / nneg, or 0 when the maximal lattice through s is not pw x ph / ph x pw.
static __device__ int ch_seed(const ChPts& p, int s, int pw, int ph, unsigned char* g, int* npos_out, int* nneg_out) {
    if (p.m < pw * ph) return 0;
    int a = -1, b = -1;
    i64 ad = INT64_MAX, bd = 0;
    for (int k = 0; k < p.m; ++k) {
        if (k == s) continue;
        const i64 dx = p.x[k] - p.x[s], dy = p.y[k] - p.y[s], d = dx * dx + dy * dy;
        if (d < ad) { ad = d; a = k; }
    }
    if (a < 0) return 0;
    int ux = p.x[a] - p.x[s], uy = p.y[a] - p.y[s];
    const i64 uu = (i64)ux * ux + (i64)uy * uy;
    for (int k = 0; k < p.m; ++k) {          // nearest neighbour between 60 and 120 degrees of u, at most twice as long
        if (k == s) continue;
        const i64 wx = p.x[k] - p.x[s], wy = p.y[k] - p.y[s], ww = wx * wx + wy * wy, dot = ux * wx + uy * wy;
        if (4 * dot * dot <= uu * ww && ww <= 4 * uu && (b < 0 || ww < bd)) { b = k; bd = ww; }
    }
    if (b < 0) return 0;
    int vx = p.x[b] - p.x[s], vy = p.y[b] - p.y[s];
    if ((i64)ux * vy - (i64)uy * vx < 0) {
        int t = ux; ux = vx; vx = t;
        t = uy; uy = vy; vy = t;
    }
    const int big = pw > ph ? pw : ph;
    const int nn = ch_chain(p, s, -ux, -uy, big, g);
    if (nn < 0) return 0;
    for (int i = 0; i < nn / 2; ++i) { const unsigned char t = g[i]; g[i] = g[nn - 1 - i]; g[nn - 1 - i] = t; }
    g[nn] = (unsigned char)s;
    const int np = ch_chain(p, s, ux, uy, big, g + nn + 1);
    if (np < 0) return 0;
    const int nu = nn + 1 + np, c0 = nn;
    if (nu != pw && nu != ph) return 0;
    const int max_rows = pw * ph / nu;
    int rows = 1, cnt[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const unsigned char* cur = g;
        int sx = side ? -vx : vx, sy = side ? -vy : vy;
        for (;;) {
            const int f = ch_find(p, p.x[cur[c0]] + sx, p.y[cur[c0]] + sy, (i64)sx * sx + (i64)sy * sy);
            if (f < 0) break;
            if (rows == max_rows) return 0;                  // larger than the pattern, or incomplete: no lattice either way
            unsigned char* nw = g + rows * nu;
            nw[c0] = (unsigned char)f;
            if (ch_fill_row(p, cur, nw, nu, c0) < 0) return 0;
            sx = p.x[nw[c0]] - p.x[cur[c0]];
            sy = p.y[nw[c0]] - p.y[cur[c0]];
            cur = nw;
            ++rows;
            ++cnt[side];
        }
    }
    if (!((nu == pw && rows == ph) || (nu == ph && rows == pw))) return 0;
    *npos_out = cnt[0];
    *nneg_out = cnt[1];
    return nu;
}

__global__ __launch_bounds__(256) void k_chess_order(const u64* __restrict__ slots, int nslots, int w, int pw, int ph,
                                                     int32_t* __restrict__ peaks, int32_t* __restrict__ found,
                                                     int32_t* __restrict__ n_candidates, double* __restrict__ corners) {
    __shared__ int cnt, winner;
    __shared__ u64 sel[VBS_CHESS_MAX_CANDIDATES];
    __shared__ int cx[VBS_CHESS_MAX_CANDIDATES], cy[VBS_CHESS_MAX_CANDIDATES], cr[VBS_CHESS_MAX_CANDIDATES];
    const int tid = threadIdx.x, n = blockIdx.x, K = VBS_CHESS_MAX_CANDIDATES, npts = pw * ph;
    const u64* S = slots + (int64_t)n * nslots;
    if (tid == 0) { cnt = 0; winner = K; }
    __syncthreads();
    int c = 0;
    for (int i = tid; i < nslots; i += 256) c += S[i] != 0;
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    const int total = cnt;
    __syncthreads();
    u64 thr = 1;                             // keys are > 0 (R > 0)
    if (total > K) {                         // the K-th largest key, bit by bit
        thr = 0;
        for (int b = CH_KEY_BITS - 1; b >= 0; --b) {
            const u64 trial = thr | (1ull << b);
            if (tid == 0) cnt = 0;
            __syncthreads();
            c = 0;
            for (int i = tid; i < nslots; i += 256) c += S[i] >= trial;
            if (c) atomicAdd(&cnt, c);
            __syncthreads();
            if (cnt >= K) thr = trial;
            __syncthreads();
        }
    }
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int i = tid; i < nslots; i += 256) {
        const u64 k = S[i];
        if (k >= thr) {                      // keys are distinct: exactly min(total, K) of them
            const int at = atomicAdd(&cnt, 1);
            if (at < K) sel[at] = k;
        }
    }
    __syncthreads();
    const int m = cnt < K ? cnt : K;
    if (tid < m) {                           // rank sort: the order of the compaction above does not matter
        const u64 k = sel[tid];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += sel[j] > k;
        const u32 pos = 0xFFFFFFFFu - (u32)k;
        cx[rank] = (int)(pos % (u32)w);
        cy[rank] = (int)(pos / (u32)w);
        cr[rank] = (int)(k >> 32);
    }
    __syncthreads();
    unsigned char g[VBS_CHESS_MAX_PATTERN + 8];              // a seed row of up to 2 * 128 + 1 before its length is checked
    int npos = 0, nneg = 0, nu = 0;
    if (tid < m) {
        // a seed walks only over candidates at least 1 / CH_STRENGTH_RATIO as strong as itself: a prefix of the sorted list
        int ms = tid + 1;
        while (ms < m && CH_STRENGTH_RATIO * cr[ms] >= cr[tid]) ++ms;
        const ChPts p{cx, cy, ms};
        nu = ch_seed(p, tid, pw, ph, g, &npos, &nneg);
        if (nu) atomicMin(&winner, tid);
    }
    __syncthreads();
    const int win = winner;
    if (tid == 0) {
        n_candidates[n] = total;
        found[n] = win < K;
    }
    if (win == K) {
        for (int i = tid; i < npts * 2; i += 256) {
            peaks[(int64_t)n * npts * 2 + i] = -1;
            corners[(int64_t)n * npts * 2 + i] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }
    if (tid != win) return;
    const int nv = 1 + npos + nneg;
    auto G = [&](int j, int i) -> int {      // row j along the row step, column i along the column step
        return j < nneg ? g[(1 + npos + (nneg - 1 - j)) * nu + i] : g[(j - nneg) * nu + i];
    };
    int best = -1, by = 0, bx = 0;
    for (int k = 0; k < 4; ++k) {            // the four rotations (np.rot90(grid, -k)); those whose rows have pw corners
        const bool same = (k & 1) == 0;
        if (same ? !(nu == pw && nv == ph) : !(nv == pw && nu == ph)) continue;
        const int q = k == 0 ? G(0, 0) : k == 1 ? G(nv - 1, 0) : k == 2 ? G(nv - 1, nu - 1) : G(0, nu - 1);
        if (best < 0 || cy[q] < by || (cy[q] == by && cx[q] < bx)) { best = k; by = cy[q]; bx = cx[q]; }
    }
    for (int r = 0; r < ph; ++r)
        for (int cc = 0; cc < pw; ++cc) {
            const int q = best == 0 ? G(r, cc) : best == 1 ? G(nv - 1 - cc, r) : best == 2 ? G(nv - 1 - r, nu - 1 - cc)
                                                                                          : G(cc, nu - 1 - r);
            const int64_t o = ((int64_t)n * npts + r * pw + cc) * 2;
            peaks[o] = cx[q];
            peaks[o + 1] = cy[q];
            corners[o] = (double)cx[q];
            corners[o + 1] = (double)cy[q];
        }
}

// ---- cv2.cornerSubPix, one wave (= one workgroup) per corner ---------------------------------------------------------------------
#define CH_MAXW VBS_CHESS_MAX_WIN
#define CH_PMAX (2 * CH_MAXW + 3)
#define CH_WMAX (2 * CH_MAXW + 1)

static __device__ __forceinline__ double ch_wave_sum(double v) {     // fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_corner_subpix(const u8* __restrict__ gray, int h, int w, int64_t stride_n,
                                                      int64_t stride_row, double* __restrict__ corners, int k, int wx, int wy,
                                                      int zx, int zy, int max_iter, double eps, int32_t* __restrict__ iters) {
    __shared__ float patch[CH_PMAX * CH_PMAX];
    __shared__ float mask[CH_WMAX * CH_WMAX];
    __shared__ float ex[CH_WMAX], ey[CH_WMAX];
    const int lane = threadIdx.x;
    const int64_t id = blockIdx.x;
    const u8* src = gray + (id / k) * stride_n;
    const int ww = 2 * wx + 1, wh = 2 * wy + 1, pw = ww + 2, ph = wh + 2;
    const double sx = corners[id * 2], sy = corners[id * 2 + 1];
    if (!(fabs(sx) < 1e9) || !(fabs(sy) < 1e9)) {            // NaN (a frame without a board) or absurd: left as it is
        if (iters && lane == 0) iters[id] = 0;
        return;
    }
    for (int i = lane; i < ww; i += 64) { const double t = (double)(i - wx) / wx; ex[i] = (float)exp(-t * t); }
    for (int i = lane; i < wh; i += 64) { const double t = (double)(i - wy) / wy; ey[i] = (float)exp(-t * t); }
    __syncthreads();
    const bool zone = zx >= 0 && zy >= 0 && 2 * zx + 1 < ww && 2 * zy + 1 < wh;
    for (int e = lane; e < ww * wh; e += 64) {
        const int i = e / ww, j = e % ww;
        const bool zero = zone && i >= wy - zy && i <= wy + zy && j >= wx - zx && j <= wx + zx;
        mask[e] = zero ? 0.0f : ey[i] * ex[j];
    }
    double cx = sx, cy = sy;
    int it = 0;
    for (;;) {
        __syncthreads();                                     // the mask (first round), the previous round's reads of patch
        for (int e = lane; e < pw * ph; e += 64) {           // cv2.getRectSubPix: bilinear, replicated border
            const int i = e / pw, j = e % pw;
            const double xs = cx - (pw - 1) * 0.5 + j, ys = cy - (ph - 1) * 0.5 + i;
            const double xf = floor(xs), yf = floor(ys), fx = xs - xf, fy = ys - yf;
            const int x0 = (int)fmin(fmax(xf, -1.0), (double)w), y0 = (int)fmin(fmax(yf, -1.0), (double)h);
            const int xa = min(max(x0, 0), w - 1), xb = min(max(x0 + 1, 0), w - 1);
            const int ya = min(max(y0, 0), h - 1), yb = min(max(y0 + 1, 0), h - 1);
            const u8* ra = src + (int64_t)ya * stride_row;
            const u8* rb = src + (int64_t)yb * stride_row;
            const double top = (double)ra[xa] * (1.0 - fx) + (double)ra[xb] * fx;
            const double bot = (double)rb[xa] * (1.0 - fx) + (double)rb[xb] * fx;
            patch[e] = (float)(top * (1.0 - fy) + bot * fy);
        }
        __syncthreads();
        double a = 0, b = 0, c = 0, bb1 = 0, bb2 = 0;
        for (int e = lane; e < ww * wh; e += 64) {
            const int i = e / ww, j = e % ww;
            const double m = mask[e];
            const double gx = (double)patch[(i + 1) * pw + j + 2] - (double)patch[(i + 1) * pw + j];
            const double gy = (double)patch[(i + 2) * pw + j + 1] - (double)patch[i * pw + j + 1];
            const double gxx = gx * gx * m, gxy = gx * gy * m, gyy = gy * gy * m;
            const double px = j - wx, py = i - wy;
            a += gxx;
            b += gxy;
            c += gyy;
            bb1 += gxx * px + gxy * py;
            bb2 += gxy * px + gyy * py;
        }
        a = ch_wave_sum(a);
        b = ch_wave_sum(b);
        c = ch_wave_sum(c);
        bb1 = ch_wave_sum(bb1);
        bb2 = ch_wave_sum(bb2);
        ++it;
        const double det = a * c - b * b;
        if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) break;
        const double scale = 1.0 / det;
        const double nx = cx + c * scale * bb1 - b * scale * bb2;
        const double ny = cy - b * scale * bb1 + a * scale * bb2;
        const double err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
        cx = nx;
        cy = ny;
        if (cx < 0 || cx >= w || cy < 0 || cy >= h) break;
        if (it >= max_iter || err <= eps * eps) break;
    }
    if (fabs(cx - sx) > wx || fabs(cy - sy) > wy) { cx = sx; cy = sy; }
    if (lane == 0) {
        corners[id * 2] = cx;
        corners[id * 2 + 1] = cy;
        if (iters) iters[id] = it;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
size_t chess_workspace_bytes(int n, int h, int w) {
    const size_t tiles = (size_t)((w + CH_TW - 1) / CH_TW) * ((h + CH_TH - 1) / CH_TH);
    return (size_t)n * tiles * CH_SLOTS * sizeof(u64);
}

void launch_corner_subpix(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, double* corners, int k,
                          int wx, int wy, int zx, int zy, int max_iter, double eps, int32_t* iters, hipStream_t s) {
    // one workgroup per corner; vbs_corner_subpix bounds n * k below 2^30, a grid's x extent
    hipLaunchKernelGGL(k_corner_subpix, dim3((unsigned)(n * k)), dim3(64), 0, s, gray, h, w, stride_n, stride_row, corners, k, wx, wy,
                       zx, zy, max_iter, eps, iters);
}

void launch_chess(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, int pw, int ph, double* corners,
                  int32_t* found, int32_t* peaks, int32_t* n_candidates, int32_t* response, u64* slots, hipStream_t s) {
    const int tx = (w + CH_TW - 1) / CH_TW, ty = (h + CH_TH - 1) / CH_TH;
    for (int off = 0; off < n; off += 65535) {               // gridDim.z
        const int nb = std::min(65535, n - off);
        hipLaunchKernelGGL(k_chess_response, dim3(tx, ty, nb), dim3(256), 0, s, gray + (int64_t)off * stride_n, h, w, stride_n,
                           stride_row, slots + (size_t)off * tx * ty * CH_SLOTS,
                           response ? response + (int64_t)off * h * w : nullptr);
    }
    hipLaunchKernelGGL(k_chess_order, dim3(n), dim3(256), 0, s, slots, tx * ty * CH_SLOTS, w, pw, ph, peaks, found, n_candidates,
                       corners);
    // findChessboardCorners' own refinement: window (2,2), 15 iterations, eps 0.1 (recalled from the 4.x source: DESIGN.md 7)
    launch_corner_subpix(gray, n, h, w, stride_n, stride_row, corners, pw * ph, 2, 2, -1, -1, 15, 0.1, nullptr, s);
}
