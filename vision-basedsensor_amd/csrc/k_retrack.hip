// f20: re-tracking a recording from its detections - prediction, gate, one-to-one match (the rule: include/vbs.h, vbs_retrack).
//   k_retrack_bin   parallel over frames: the finite detections of a frame hung into a 32 x 32 grid of cells (cell coordinates
//                   modulo the grid, pitch a power of two >= gate + 1) by a counting sort in LDS, the lists in ascending
//                   detection index; the grid goes to the workspace.
//   k_retrack_walk  ONE workgroup walks the frames in order (the chain along time is the only sequential part): the state of a
//                   slot lives in its thread's registers for the whole recording, the detections and the grid of frame f + 1
//                   are loaded into registers while frame f is matched and go to the other half of a double buffer in LDS.
//   k_retrack_rows  parallel over (frame, slot): the table rows from `assign` and `det`.
// The match is the sort over (d2, j, i) of the header in its parallel form: rounds in which every free slot names its best free
// candidate, every free detection its best free slot among ALL free slots that hold it as a candidate (LDS minima over d2,
// then over j), and the mutual pairs are fixed.  The smallest remaining pair is always mutual, so a round with a free slot that
// still has a candidate fixes at least one pair; the loop is bounded by min(m, cnt) + 1 all the same.  A slot keeps its first
// RT_LIST candidates in registers; one with more walks its 3 x 3 cells again in every round, so nothing is ever cut short: a
// gate several pitches wide is slower, never wrong.  No wait between workgroups or launches anywhere.
// Float64 without contraction, as the restatement in the tests computes.
#include <cmath>
#include "common.h"

#pragma clang fp contract(off)

typedef unsigned short u16;

#define RT_MAX VBS_RETRACK_MAX
#define RT_G 32                                 // cells per side
#define RT_CELLS (RT_G * RT_G)
#define RT_HDR (RT_CELLS + 4)                   // u16 per frame ahead of the order list: start[RT_CELLS + 1], the flag, 2 spare
#define RT_FLAG (RT_CELLS + 1)                  // 1 = the lists of this frame are usable, 0 = the plain scan
#define RT_BIN_THREADS 256
#define RT_DET_REGS 4                           // detections a thread of the walk holds in flight: 4 x 256 threads = RT_MAX
#define RT_LIST 4                               // candidates of a slot the walk keeps in registers
#define RT_NOBODY 0xFFFFFFFFFFFFFFFFull

static inline int rt_stride(int max_det) { return RT_HDR + ((max_det + 3) & ~3); }     // u16 per frame, 8-byte multiples
static inline size_t rt_assign_bytes(int n, int m) { return (((size_t)n * (size_t)m * sizeof(int32_t)) + 15) & ~(size_t)15; }

size_t retrack_workspace_bytes(int n, int m, int max_det) {
    return rt_assign_bytes(n, m) + (size_t)n * (size_t)rt_stride(max_det) * sizeof(u16) + 16;
}

__global__ __launch_bounds__(RT_BIN_THREADS) void k_retrack_bin(const double* __restrict__ det, const int32_t* __restrict__ counts,
                                                                int max_det, double inv_pitch, u16* __restrict__ grid, int stride) {
    __shared__ u16 cell[RT_MAX];
    __shared__ u32 start[RT_CELLS];
    __shared__ u32 part[RT_BIN_THREADS];
    __shared__ int beyond;
    const int f = blockIdx.x, tid = threadIdx.x;
    u16* g = grid + (int64_t)f * stride;
    const int cnt = min(counts[f], max_det);             // (a status < 0: an unusable frame, nothing of it is read)
    if (cnt <= 0) {
        if (tid == 0) g[RT_FLAG] = 0;
        return;
    }
    for (int i = tid; i < RT_CELLS; i += RT_BIN_THREADS) start[i] = 0;
    if (tid == 0) beyond = 0;
    __syncthreads();
    const double* d = det + (int64_t)f * max_det * VBS_DET_COLS;
    for (int i = tid; i < cnt; i += RT_BIN_THREADS) {
        const double x = d[(int64_t)i * VBS_DET_COLS], y = d[(int64_t)i * VBS_DET_COLS + 1];
        u16 c = 0xFFFF;                                  // not finite: in no list, never a candidate
        if (isfinite(x) && isfinite(y)) {
            const double fx = floor(x * inv_pitch), fy = floor(y * inv_pitch);
            if (fabs(fx) < 0x1p30 && fabs(fy) < 0x1p30) {
                c = (u16)((((int)fy & (RT_G - 1)) * RT_G) + ((int)fx & (RT_G - 1)));
                atomicAdd(&start[c], 1u);
            } else {
                beyond = 1;                              // the whole frame takes the plain scan
            }
        }
        cell[i] = c;
    }
    __syncthreads();
    if (beyond) {
        if (tid == 0) g[RT_FLAG] = 0;
        return;
    }
    // exclusive sums over the cells: a thread owns four consecutive cells
    const u32 a0 = start[4 * tid], a1 = start[4 * tid + 1], a2 = start[4 * tid + 2], a3 = start[4 * tid + 3];
    const u32 own = a0 + a1 + a2 + a3;
    part[tid] = own;
    __syncthreads();
    for (int off = 1; off < RT_BIN_THREADS; off <<= 1) {
        const u32 v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const u32 base = part[tid] - own;
    start[4 * tid] = base;
    start[4 * tid + 1] = base + a0;
    start[4 * tid + 2] = base + a0 + a1;
    start[4 * tid + 3] = base + a0 + a1 + a2;
    __syncthreads();
    for (int i = tid; i < RT_CELLS; i += RT_BIN_THREADS) g[i] = (u16)start[i];
    if (tid == 0) {
        g[RT_CELLS] = (u16)part[RT_BIN_THREADS - 1];
        g[RT_FLAG] = 1;
    }
    // the place of a detection inside its list = the detections of the same cell before it: ascending index without a sort
    for (int i = tid; i < cnt; i += RT_BIN_THREADS) {
        const u16 c = cell[i];
        if (c == 0xFFFF) continue;
        u32 r = 0;
        for (int k = 0; k < i; ++k) r += cell[k] == c ? 1u : 0u;
        g[RT_HDR + start[c] + r] = (u16)i;
    }
}

// fn(i) for every detection a slot has to look at: the lists of its 3 x 3 cells, or all of them.  The three cells of a grid row lie
// side by side in the order list unless the row wraps round the grid, so a row is one range
template <class F>
__device__ __forceinline__ void rt_for_each(bool lists, int cx0, int cy0, const u16* __restrict__ cs, const u16* __restrict__ ord,
                                            int cnt, F&& fn) {
    if (lists) {
        const int xa = (cx0 - 1) & (RT_G - 1);
#pragma unroll 1
        for (int dy = -1; dy <= 1; ++dy) {
            const int row = ((cy0 + dy) & (RT_G - 1)) * RT_G;
            if (xa <= RT_G - 3) {
                const int e = cs[row + xa + 3];
                for (int p = cs[row + xa]; p < e; ++p) fn((int)ord[p]);
            } else {
#pragma unroll 1
                for (int k = 0; k < 3; ++k) {
                    const int b = row + ((xa + k) & (RT_G - 1));
                    const int e = cs[b + 1];
                    for (int p = cs[b]; p < e; ++p) fn((int)ord[p]);
                }
            }
        }
    } else {
        for (int i = 0; i < cnt; ++i) fn(i);
    }
}

__global__ __launch_bounds__(RT_MAX) void k_retrack_walk(const double* __restrict__ det, const int32_t* __restrict__ counts, int n,
                                                         int max_det, const double* __restrict__ ref_xy, int m,
                                                         const double* __restrict__ state_in, double gate, double max_travel,
                                                         double vel_gain, int max_coast, double inv_pitch,
                                                         const u16* __restrict__ grid, int use_grid, int stride,
                                                         int32_t* __restrict__ assign,
                                                         double* __restrict__ dist2, int32_t* __restrict__ info,
                                                         double* __restrict__ state_out, int B) {
    __shared__ double sx[2][RT_MAX], sy[2][RT_MAX];
    __shared__ u32 sg[2][RT_HDR / 2];                    // start[RT_CELLS + 1] and the flag, as the workspace holds them
    __shared__ u32 so[2][RT_MAX / 2];                    // the order list
    __shared__ u64 dmin[RT_MAX];                         // per detection: the smallest d2 of a free slot that holds it (as bits)
    __shared__ int djm[RT_MAX];                          //                and the smallest such slot
    __shared__ u8 taken[RT_MAX];
    __shared__ int tally[3];                             // matched, with_candidate, contested of the frame
    const int tid = threadIdx.x, j = tid;                // (B = the workgroup's size: as an argument it is a scalar for good)
    const bool slot = j < m;
    const double g2 = gate * gate, t2 = max_travel * max_travel;
    const bool travel = isfinite(max_travel);
    double px = 0.0, py = 0.0, vx = 0.0, vy = 0.0, age = 0.0, seen = 0.0, ox = 0.0, oy = 0.0;
    if (slot) {
        ox = ref_xy[2 * j]; oy = ref_xy[2 * j + 1];
        px = ox; py = oy;
        if (state_in) {
            const double* s = state_in + (int64_t)j * VBS_RETRACK_STATE_COLS;
            px = s[0]; py = s[1]; vx = s[2]; vy = s[3]; age = s[4]; seen = s[5];
        }
    }

    // frame 0 goes straight into the first half of the buffer
    int c_cur = n > 0 ? counts[0] : 0, c_next = n > 1 ? counts[1] : 0;
    {
        const int cnt0 = min(c_cur, max_det);
        for (int i = tid; i < cnt0; i += B) {
            sx[0][i] = det[(int64_t)i * VBS_DET_COLS];
            sy[0][i] = det[(int64_t)i * VBS_DET_COLS + 1];
            dmin[i] = RT_NOBODY; djm[i] = 0x7FFFFFFF; taken[i] = 0;
        }
        if (use_grid && cnt0 > 0) {
            const u32* g32 = (const u32*)grid;
            for (int i = tid; i < RT_HDR / 2; i += B) sg[0][i] = g32[i];
            for (int i = tid; i < (cnt0 + 1) / 2; i += B) so[0][i] = g32[RT_HDR / 2 + i];
        }
        if (tid < 3) tally[tid] = 0;
    }
    __syncthreads();

    for (int f = 0; f < n; ++f) {
        const int cur = f & 1;
        const int used = c_cur >= 0 ? 1 : 0;
        const int cnt = max(min(c_cur, max_det), 0);
        const double* x_ = sx[cur];
        const double* y_ = sy[cur];
        const u16* cs = (const u16*)sg[cur];
        const u16* ord = (const u16*)so[cur];

        // frame f + 1 on its way to registers while this frame is matched.  Every load is unconditional, at an index clamped into
        // what the frame holds (into the frame itself past the last one): behind a branch the compiler waits for a load where it
        // is issued, and the latency of global memory would be paid several times per frame.  What a clamped load brings is
        // never stored
        const int cnt_n = max(min(c_next, max_det), 0);
        const int c_after = f + 2 < n ? counts[f + 2] : 0;
        double nx[RT_DET_REGS], ny[RT_DET_REGS];
        u32 ng[3], no[2];
        {
            const int fn = min(f + 1, n - 1);
            const double* dn = det + (int64_t)fn * max_det * VBS_DET_COLS;
            const int last = max(cnt_n, 1) - 1;
#pragma unroll
            for (int k = 0; k < RT_DET_REGS; ++k) {
                const int i = min(tid + k * B, last);
                nx[k] = dn[(int64_t)i * VBS_DET_COLS];
                ny[k] = dn[(int64_t)i * VBS_DET_COLS + 1];
            }
            const u32* g32 = (const u32*)(grid + (int64_t)fn * stride);
#pragma unroll
            for (int k = 0; k < 3; ++k) ng[k] = g32[min(tid + k * B, RT_HDR / 2 - 1)];
#pragma unroll
            for (int k = 0; k < 2; ++k) no[k] = g32[RT_HDR / 2 + min(tid + k * B, last / 2)];
        }

        // 1. the prediction, and the cells it reaches
        const double k_age = age + 1.0;
        const double qx = px + vx * k_age, qy = py + vy * k_age;
        const double cfx = floor(qx * inv_pitch), cfy = floor(qy * inv_pitch);
        const bool frame_lists = use_grid && cnt > 0 && cs[RT_FLAG] != 0;
        const bool lists = frame_lists && fabs(cfx) < 0x1p30 && fabs(cfy) < 0x1p30;      // (false for NaN)
        const int cx0 = lists ? (int)cfx : 0, cy0 = lists ? (int)cfy : 0;
        // 3. d2 of the pair (this slot, detection i) where it is a candidate, else -1
        auto pair_d2 = [&](int i) -> double {
            const double x = x_[i], y = y_[i];
            if (!(isfinite(x) && isfinite(y))) return -1.0;
            const double dx = qx - x, dy = qy - y;
            const double d2 = dx * dx + dy * dy;
            bool ok = d2 <= g2;
            if (travel) {
                const double tx = x - ox, ty = y - oy;
                ok = ok && tx * tx + ty * ty <= t2;
            }
            return ok ? d2 : -1.0;
        };

        // 4. one-to-one.  dmin, djm and taken were set for this frame before the barrier that ended the last one
        bool open = slot && cnt > 0;                     // unmatched, and may still have a free candidate
        int mine = -1;
        double mine_d2 = -1.0;
        // the first RT_LIST candidates stay in registers; a slot with more walks its cells again in every round
        int li[RT_LIST], n_cand = 0;
        double ld[RT_LIST];
#pragma unroll
        for (int k = 0; k < RT_LIST; ++k) { li[k] = 0; ld[k] = 0.0; }
        double bd = 0.0;
        int bi = -1;
        // what a free slot does with a free candidate in the first half of a round: its own best by (d2, i), and its bid
        auto bid = [&](int i, double d2) {
            if (bi < 0 || d2 < bd || (d2 == bd && i < bi)) { bd = d2; bi = i; }
            atomicMin(&dmin[i], (u64)__double_as_longlong(d2));                  // (d2 >= +0: its bits order as it does)
        };
        // fn(i, d2) for every FREE candidate of this slot
        auto for_free = [&](auto&& fn) {
            if (n_cand <= RT_LIST) {
#pragma unroll
                for (int k = 0; k < RT_LIST; ++k)
                    if (k < n_cand && !taken[li[k]]) fn(li[k], ld[k]);
            } else {
                rt_for_each(lists, cx0, cy0, cs, ord, cnt, [&](int i) {
                    if (taken[i]) return;
                    const double d2 = pair_d2(i);
                    if (d2 >= 0.0) fn(i, d2);
                });
            }
        };
        if (open) {                                      // round 0, first half: nothing is taken yet
            rt_for_each(lists, cx0, cy0, cs, ord, cnt, [&](int i) {
                const double d2 = pair_d2(i);
                if (d2 < 0.0) return;
#pragma unroll
                for (int k = 0; k < RT_LIST; ++k)
                    if (k == n_cand) { li[k] = i; ld[k] = d2; }
                ++n_cand;
                bid(i, d2);
            });
        }
        const bool has_candidate = n_cand > 0;
        const int first_best = bi;
        open = has_candidate;
        const int max_rounds = cnt > 0 ? min(m, cnt) + 1 : 0;            // (no detection: no round, no barrier)
        for (int round = 0; round < max_rounds; ++round) {
            if (round > 0) {
                for (int i = tid; i < cnt; i += B) { dmin[i] = RT_NOBODY; djm[i] = 0x7FFFFFFF; }
                __syncthreads();
                bd = 0.0; bi = -1;
                if (open) {
                    for_free(bid);
                    if (bi < 0) open = false;
                }
            }
            __syncthreads();
            if (open)
                for_free([&](int i, double d2) {
                    if ((u64)__double_as_longlong(d2) == dmin[i]) atomicMin(&djm[i], j);
                });
            __syncthreads();
            if (open && dmin[bi] == (u64)__double_as_longlong(bd) && djm[bi] == j) {
                mine = bi; mine_d2 = bd; taken[bi] = 1; open = false;
            }
            if (!__syncthreads_count(open ? 1 : 0)) break;       // (every slot has read the minima: the next round resets them)
        }

        // 5. the update
        if (slot) {
            if (mine >= 0) {
                const double x = x_[mine], y = y_[mine];
                if (seen == 1.0) {
                    const double ux = (x - px) / k_age, uy = (y - py) / k_age;
                    vx = vx + vel_gain * (ux - vx);
                    vy = vy + vel_gain * (uy - vy);
                }
                px = x; py = y; age = 0.0; seen = 1.0;
            } else {
                age = age + 1.0;
                if (age > (double)max_coast) { vx = 0.0; vy = 0.0; }
            }
            assign[(int64_t)f * m + j] = mine;
            if (dist2) dist2[(int64_t)f * m + j] = mine_d2;
        }
        if (info) {
            const int a = __popcll(__ballot(mine >= 0)), b = __popcll(__ballot(has_candidate));
            const int c = __popcll(__ballot(has_candidate && mine != first_best));
            if ((tid & 63) == 0) {
                if (a) atomicAdd(&tally[0], a);
                if (b) atomicAdd(&tally[1], b);
                if (c) atomicAdd(&tally[2], c);
            }
        }

        // frame f + 1 into the other half, its last reader was frame f - 1; and the minima and marks of its detections
#pragma unroll
        for (int k = 0; k < RT_DET_REGS; ++k) {
            const int i = tid + k * B;
            if (i < cnt_n) { sx[cur ^ 1][i] = nx[k]; sy[cur ^ 1][i] = ny[k]; }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = tid + k * B;
            if (i < RT_HDR / 2) sg[cur ^ 1][i] = ng[k];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * B;
            if (i < (cnt_n + 1) / 2) so[cur ^ 1][i] = no[k];
        }
        for (int i = tid; i < cnt_n; i += B) { dmin[i] = RT_NOBODY; djm[i] = 0x7FFFFFFF; taken[i] = 0; }
        c_cur = c_next;
        c_next = c_after;
        __syncthreads();
        if (info && tid == 0) {                          // (the next frame's sums come after its barriers)
            int32_t* o = info + (int64_t)f * VBS_RETRACK_INFO_COLS;
            o[0] = used; o[1] = tally[0]; o[2] = tally[1]; o[3] = tally[2];
            tally[0] = 0; tally[1] = 0; tally[2] = 0;
        }
    }

    if (slot && state_out) {
        double* s = state_out + (int64_t)j * VBS_RETRACK_STATE_COLS;
        s[0] = px; s[1] = py; s[2] = vx; s[3] = vy; s[4] = age; s[5] = seen;
    }
}

// the rows of vbs_track's table from the assignment: the detection cast once to float32, X Y Z zero
__global__ __launch_bounds__(256) void k_retrack_rows(const double* __restrict__ det, int max_det, const int32_t* __restrict__ assign,
                                                      int64_t rows, int m, float* __restrict__ table) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int a = assign[r];
    float o[VBS_TABLE_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if ((unsigned)a < (unsigned)max_det) {               // (-1, or anything that is no index: an empty row, never a read outside det)
        const double* d = det + ((r / m) * max_det + a) * VBS_DET_COLS;
        o[0] = (float)VBS_FLAG_TRACKED;
#pragma unroll
        for (int c = 0; c < 5; ++c) o[1 + c] = (float)d[c];
        o[9] = (float)a;
    }
    float* row = table + r * VBS_TABLE_COLS;
#pragma unroll
    for (int c = 0; c < VBS_TABLE_COLS; ++c) row[c] = o[c];
}

void launch_retrack(const double* det, const int32_t* counts, int n, int max_det, const double* ref_xy, int m, const double* state_in,
                    double gate, double max_travel, double vel_gain, int max_coast, int32_t* assign, float* table, double* dist2,
                    int32_t* info, double* state_out, void* workspace, hipStream_t st) {
    if (!assign) assign = (int32_t*)workspace;
    u16* grid = (u16*)((char*)workspace + rt_assign_bytes(n, m));
    double inv_pitch = 1.0;
    const int stride = rt_stride(max_det);
    const int use_grid = gate <= 4095.0 && n > 0;        // a wider gate: the plain scan in every frame, the grids stay unwritten
    if (use_grid) {
        int sh = 3;
        while ((double)(1 << sh) < gate + 1.0) ++sh;
        inv_pitch = 1.0 / (double)(1 << sh);
        hipLaunchKernelGGL(k_retrack_bin, dim3((unsigned)n), dim3(RT_BIN_THREADS), 0, st, det, counts, max_det, inv_pitch, grid, stride);
    }
    if (VBS_KNOB("VBS_RETRACK_STOP") == 1) return;       // (the debug library: the grid alone, for tools/gpu_retrack_rate.py)
    const int threads = m <= 256 ? 256 : (m <= 512 ? 512 : RT_MAX);      // a slot per thread, RT_DET_REGS detections per thread
    if (VBS_KNOB("VBS_RETRACK_STOP") != 2)               // (2: the grid and the rows without the walk, on whatever `assign` holds)
        hipLaunchKernelGGL(k_retrack_walk, dim3(1), dim3(threads), 0, st, det, counts, n, max_det, ref_xy, m, state_in, gate, max_travel,
                           vel_gain, max_coast, inv_pitch, (const u16*)grid, use_grid, stride, assign, dist2, info, state_out, threads);
    const int64_t rows = (int64_t)n * m;
    if (table && rows > 0)
        hipLaunchKernelGGL(k_retrack_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, det, max_det, (const int32_t*)assign,
                           rows, m, table);
}
