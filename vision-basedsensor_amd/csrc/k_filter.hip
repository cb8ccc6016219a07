// The dynamic-polishing analysis: the signed displacement of every slot from a reference frame with its sum over
// the slots, and a gap-aware zero-phase FIR along time for many series at once.  Float64 without contraction, no atomics, a
// stated order of every sum: a result depends on its inputs only, never on the launch shape (the rule of k_series.hip).
//   k_axis_displacement   one wave per frame; lane l adds slots l, l + 64, ... in ascending order, the 64 lane sums are folded
//                         a[i] + a[i + 32], then + 16, 8, 4, 2, 1
//   k_fir<NV>             tile = 64 series (the lanes) x FIR_TILE frames (FIR_WAVES waves x FIR_P outputs a lane, accumulators
//                         in registers); the input rows [first - h, last + h] of the tile stream ONCE, in ascending order,
//                         through a stage of FIR_ROWS rows in LDS, every wave adding a row to those of its outputs it reaches.
//                         One output therefore adds its 2h + 1 rows in ascending k whatever the tile, the range or s.
// The data is time-major, series on the fast axis: a wave's accesses to one frame row are contiguous.
#include "common.h"
#pragma clang fp contract(off)

#define FIR_P     8                      // outputs (consecutive frames) a lane keeps in registers
#define FIR_WAVES (VBS_FIR_TILE / FIR_P)
#define FIR_ROWS  16                     // input rows staged in LDS at a time: 16 x 64 x (NV + 1) doubles, 32 KB at NV = 3
static_assert(VBS_FIR_TILE % FIR_P == 0 && FIR_WAVES >= 1 && FIR_WAVES <= 16, "a tile is a whole number of waves");

template <int NV>
__global__ __launch_bounds__(FIR_WAVES * 64) void k_fir(const double* __restrict__ rec, int n, int s, int cols, HalfTaps taps,
                                                        int h, double need, int frame_begin, int frame_end,
                                                        double* __restrict__ out) {
    __shared__ double stage[FIR_ROWS][NV + 1][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t series = (int64_t)blockIdx.y * 64 + lane;
    const int64_t tile0 = (int64_t)frame_begin + (int64_t)blockIdx.x * VBS_FIR_TILE;           // first output frame of the tile
    const int64_t tile1 = tile0 + VBS_FIR_TILE < frame_end ? tile0 + VBS_FIR_TILE : frame_end;   // one past its last
    const int64_t f0 = tile0 + wave * FIR_P;                                                     // first output of this wave
    // rows outside [0, n) are invalid and add nothing: they are not visited at all
    const int64_t row_lo = tile0 - h > 0 ? tile0 - h : 0;
    const int64_t row_hi = tile1 - 1 + h < n - 1 ? tile1 - 1 + h : n - 1;
    const int64_t row_step = (int64_t)s * cols;

    double num[FIR_P][NV], den[FIR_P];
#pragma unroll
    for (int p = 0; p < FIR_P; ++p) {
        den[p] = 0.0;
#pragma unroll
        for (int v = 0; v < NV; ++v) num[p][v] = 0.0;
    }

    for (int64_t c0 = row_lo; c0 <= row_hi; c0 += FIR_ROWS) {
        const int rows = (int)(row_hi - c0 + 1 < FIR_ROWS ? row_hi - c0 + 1 : FIR_ROWS);
        __syncthreads();                                         // the stage's previous rows have been used by every wave
        for (int e = threadIdx.x; e < rows * 64 * (NV + 1); e += FIR_WAVES * 64) {
            const int r = e / (64 * (NV + 1)), q = e % (64 * (NV + 1)), sl = q / (NV + 1), c = q % (NV + 1);
            const int64_t sg = (int64_t)blockIdx.y * 64 + sl;
            stage[r][c][sl] = sg < s ? rec[(c0 + r) * row_step + sg * cols + c] : 0.0;       // (a series past s: flag 0)
        }
        __syncthreads();
        // this wave's outputs f0 .. f0 + FIR_P - 1 reach rows [f0 - h, f0 + FIR_P - 1 + h]
        int r_a = (int)(f0 - h - c0 > 0 ? f0 - h - c0 : 0);
        int r_b = (int)(f0 + FIR_P - 1 + h - c0 < rows - 1 ? f0 + FIR_P - 1 + h - c0 : rows - 1);
        for (int r = r_a; r <= r_b; ++r) {
            const bool valid = stage[r][0][lane] != 0.0;
            double x[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = stage[r][1 + v][lane];
#pragma unroll
            for (int p = 0; p < FIR_P; ++p) {
                const int k = (int)(c0 + r - f0) - p;            // wave-uniform
                if (k < -h || k > h) continue;
                const double w = taps.half[k < 0 ? -k : k];
                if (valid) {                                     // selected out, never multiplied by zero
                    den[p] = den[p] + w;
#pragma unroll
                    for (int v = 0; v < NV; ++v) num[p][v] = num[p][v] + w * x[v];
                }
            }
        }
    }

    if (series >= s) return;
#pragma unroll
    for (int p = 0; p < FIR_P; ++p) {
        const int64_t f = f0 + p;
        if (f >= tile1) break;
        const double* in = rec + f * row_step + series * cols;
        double* o = out + ((f - frame_begin) * s + series) * (1 + 2 * NV);
        const bool valid = in[0] != 0.0;
        const bool ok = valid && den[p] >= need;
        o[0] = valid ? (ok ? 3.0 : 1.0) : 0.0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double y = 0.0, res = 0.0;
            if (ok) {
                y = num[p][v] / den[p];
                res = in[1 + v] - y;
            }
            o[1 + v] = y;
            o[1 + NV + v] = res;
        }
    }
}

// half [n_half] HOST.  need = min_coverage * sw, sw = the ascending sum of all 2 n_half - 1 taps (one IEEE product of the two).
void launch_fir_series(const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half, double need,
                       int frame_begin, int frame_end, double* out, hipStream_t st) {
    const HalfTaps t = half_taps_arg(half, n_half);
    const dim3 grid((unsigned)(((int64_t)frame_end - frame_begin + VBS_FIR_TILE - 1) / VBS_FIR_TILE), (unsigned)((s + 63) / 64));
    const dim3 block(FIR_WAVES * 64);
#define FIR_CASE(NV)                                                                                                          \
    case NV: hipLaunchKernelGGL(k_fir<NV>, grid, block, 0, st, rec, n, s, cols, t, n_half - 1, need, frame_begin, frame_end, out); break
    switch (n_values) {
        FIR_CASE(1); FIR_CASE(2); FIR_CASE(3); FIR_CASE(4); FIR_CASE(5); FIR_CASE(6); FIR_CASE(7);
    }
#undef FIR_CASE
}

// One wave per emitted frame.  axis [fe - fb][m_ref][4] = flag, dX, dY, dZ (may be null); total [fe - fb][5] = complete,
// sum dX, sum dY, sum dZ, count (may be null).  A slot the mask leaves out is a slot whose flags are clear.
__global__ __launch_bounds__(64) void k_axis_displacement(const float* __restrict__ table, int m_ref, int ref_frame,
                                                          const u8* __restrict__ slot_mask, int frame_begin,
                                                          double* __restrict__ axis, double* __restrict__ total) {
    const int lane = threadIdx.x;
    const int64_t f = (int64_t)frame_begin + blockIdx.x;
    const float* row = table + f * m_ref * VBS_TABLE_COLS;
    const float* ref = table + (int64_t)ref_frame * m_ref * VBS_TABLE_COLS;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0, want = 0;
    for (int slot = lane; slot < m_ref; slot += 64) {
        const float* p = row + (int64_t)slot * VBS_TABLE_COLS;
        const float* r = ref + (int64_t)slot * VBS_TABLE_COLS;
        const bool in_ref = (!slot_mask || slot_mask[slot]) && ((int)r[0] & VBS_FLAG_XYZ);
        const bool ok = in_ref && ((int)p[0] & VBS_FLAG_XYZ);
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if (ok) {
            dx = (double)p[6] - (double)r[6]; dy = (double)p[7] - (double)r[7]; dz = (double)p[8] - (double)r[8];
            sx = sx + dx; sy = sy + dy; sz = sz + dz;
            ++cnt;
        }
        want += in_ref ? 1 : 0;
        if (axis) {
            double* a = axis + ((int64_t)blockIdx.x * m_ref + slot) * VBS_AXIS_COLS;
            a[0] = ok ? 1.0 : 0.0; a[1] = dx; a[2] = dy; a[3] = dz;
        }
    }
    if (!total) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {                    // lane i: a[i] + a[i + off]; lanes >= off are not read again
        sx = sx + __shfl_down(sx, off); sy = sy + __shfl_down(sy, off); sz = sz + __shfl_down(sz, off);
        cnt += __shfl_down(cnt, off); want += __shfl_down(want, off);
    }
    if (lane == 0) {
        double* t = total + (int64_t)blockIdx.x * VBS_TOTAL_COLS;
        t[0] = (want >= 1 && cnt == want) ? 1.0 : 0.0; t[1] = sx; t[2] = sy; t[3] = sz; t[4] = (double)cnt;
    }
}

void launch_axis_displacement(vbs_handle* h, const float* table, int m_ref, int ref_frame, const u8* slot_mask, int frame_begin,
                              int frame_end, double* axis, double* total, hipStream_t s) {
    VBS_LAUNCH(h, s, "k_axis_displacement", k_axis_displacement, dim3((unsigned)(frame_end - frame_begin)), dim3(64), 0, s, table,
               m_ref, ref_frame, slot_mask, frame_begin, axis, total);
}
