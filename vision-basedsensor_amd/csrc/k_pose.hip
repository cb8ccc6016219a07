// Pose misalignment along a recording: for every frame the deviation of the displacement field from a reference
// state, the plane through its end points, tilt, steep direction, residual and one round of outlier rejection.  Float64 without
// contraction, no atomics, the order of every sum stated in include/vbs.h (the rule of k_axis_displacement): a result depends on
// its inputs only, never on the launch shape.
//   k_pose   one wave per frame, VBS_POSE_GROUP frames (waves) a workgroup.  What every frame of a workgroup shares - the rows of
//            start_frame, ref_disp, ref_xyz and the slot mask - is staged ONCE into LDS, POSE_CHUNK slots at a time (one chunk
//            for up to 512 markers; a longer table restages per sweep).  A wave reads its frame's 40-byte rows 64 slots at a time
//            as ONE contiguous 2560-byte run (8-byte loads, every fetched byte of every line used once) into its own LDS tile and
//            picks flag and X, Y, Z from there, instead of three strided loads a lane that touch every line three times.
//            The sums are recomputed from the table in every sweep: means / field, centred sums, SSR, and the same three over
//            the kept set when reject_k > 0.
#include "common.h"
#include "wave_fold.h"
#pragma clang fp contract(off)

#define POSE_WAVES VBS_POSE_GROUP
#define POSE_CHUNK (POSE_WAVES * 64)             // slots staged at a time: thread t of the workgroup stages slot c0 + t
#define POSE_ROW   (64 * VBS_TABLE_COLS)         // dwords of 64 table rows
static_assert(POSE_WAVES >= 1 && POSE_WAVES <= 16, "a workgroup is at most 1024 threads");
static_assert(VBS_TABLE_COLS % 2 == 0, "a frame's rows are a whole number of 8-byte pairs");

struct PoseStage {                               // 50.5 KB with the tiles at POSE_WAVES = 8
    double rd[3][POSE_CHUNK];                    // ref_disp dX, dY, dZ
    double rp[3][POSE_CHUNK];                    // ref_x, ref_y, shell ? ref_z : 0.0
    float x0[3][POSE_CHUNK];                     // X, Y, Z of start_frame's row
    u8 sel[POSE_CHUNK];                          // selected && ref_disp flag != 0 && start_frame's row has VBS_FLAG_XYZ
};

struct PosePoint { double dx, dy, dz, sx, sy, sz, px, py, pz; };

// One sweep over the slots in the stated order: lane l meets slots l, l + 64, ... ascending.  body(slot, cs, row): cs = the
// slot's place in the staged chunk, row = its 10 floats of this wave's frame (not valid for slot >= m_ref).  EVERY thread of
// the workgroup calls this the same number of times (the barriers); a wave with nothing to do passes active = false.
template <class Body>
__device__ __forceinline__ void pose_sweep(PoseStage& S, float* tile, const float* __restrict__ table, int m_ref,
                                           const float* __restrict__ start_row, const double* __restrict__ ref_disp,
                                           const double* __restrict__ ref_xyz, const u8* __restrict__ slot_mask, int shell,
                                           bool restage, bool al8, const float* __restrict__ frow, bool active, Body&& body) {
    const int lane = threadIdx.x & 63;
    const int row_dw = m_ref * VBS_TABLE_COLS;                   // (m_ref <= 65535 * 64: fits)
    for (int c0 = 0; c0 < m_ref; c0 += POSE_CHUNK) {
        if (restage) {
            __syncthreads();                                     // every wave is done with the chunk before
            const int t = threadIdx.x, slot = c0 + t;
            bool sel = false;
            double rd[3] = {0.0, 0.0, 0.0}, rp[3] = {0.0, 0.0, 0.0};
            float x0[3] = {0.f, 0.f, 0.f};
            if (slot < m_ref) {
                const float* r = start_row + (int64_t)slot * VBS_TABLE_COLS;
                const double* d = ref_disp + (int64_t)slot * 4;
                sel = (!slot_mask || slot_mask[slot]) && d[0] != 0.0 && ((int)r[0] & VBS_FLAG_XYZ);
                if (sel) {                                       // what is not selected is never read into a value
                    const double* p = ref_xyz + (int64_t)slot * 3;
                    rd[0] = d[1]; rd[1] = d[2]; rd[2] = d[3];
                    rp[0] = p[0]; rp[1] = p[1]; rp[2] = shell ? p[2] : 0.0;
                    x0[0] = r[6]; x0[1] = r[7]; x0[2] = r[8];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { S.rd[k][t] = rd[k]; S.rp[k][t] = rp[k]; S.x0[k][t] = x0[k]; }
            S.sel[t] = sel ? 1 : 0;
            __syncthreads();
        }
        if (!active) continue;
        const int lim = m_ref - c0 < POSE_CHUNK ? m_ref - c0 : POSE_CHUNK;
        for (int g = 0; g < lim; g += 64) {
            const int d0 = (c0 + g) * VBS_TABLE_COLS;            // first dword of the 64 rows, even
            const int nd = row_dw - d0 < POSE_ROW ? row_dw - d0 : POSE_ROW;
            __builtin_amdgcn_wave_barrier();                     // (the tile's previous rows have been used by every lane)
            if (al8) {
                const float2* src = reinterpret_cast<const float2*>(frow + d0);
                for (int i = lane; i < nd / 2; i += 64) reinterpret_cast<float2*>(tile)[i] = src[i];
            } else {
                for (int i = lane; i < nd; i += 64) tile[i] = frow[d0 + i];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            body(c0 + g + lane, g + lane, tile + lane * VBS_TABLE_COLS);
        }
    }
}

__global__ __launch_bounds__(POSE_WAVES * 64) void k_pose(const float* __restrict__ table, int m_ref, int start_frame,
                                                          const double* __restrict__ ref_disp, const double* __restrict__ ref_xyz,
                                                          const u8* __restrict__ slot_mask, int shell, double scale, double reject_k,
                                                          int frame_begin, int n_frames, int al8, double* __restrict__ deviation,
                                                          double* __restrict__ field, double* __restrict__ pose) {
    __shared__ PoseStage S;
    __shared__ __attribute__((aligned(16))) float tiles[POSE_WAVES][POSE_ROW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t fi = (int64_t)blockIdx.x * POSE_WAVES + wave;  // this wave's frame among those emitted
    const bool live = fi < n_frames;                             // a wave past the end still stages and meets the barriers
    const int64_t row_step = (int64_t)m_ref * VBS_TABLE_COLS;
    const float* frow = table + ((int64_t)frame_begin + (live ? fi : 0)) * row_step;
    const float* start_row = table + (int64_t)start_frame * row_step;
    float* tile = tiles[wave];
    const bool many = m_ref > POSE_CHUNK;                        // more than one chunk: every sweep stages again

    // the point of a slot, or false: common = staged selection && this frame's row has a 3-D point.  The expressions are those of
    // fit_math.h's end_point (which k_posecov and k_shape call), here on the staged operands
    auto point = [&](int slot, int cs, const float* row, PosePoint& p) -> bool {
        if (slot >= m_ref || !S.sel[cs] || !((int)row[0] & VBS_FLAG_XYZ)) return false;
        p.dx = ((double)row[6] - (double)S.x0[0][cs]) - S.rd[0][cs];
        p.dy = ((double)row[7] - (double)S.x0[1][cs]) - S.rd[1][cs];
        p.dz = ((double)row[8] - (double)S.x0[2][cs]) - S.rd[2][cs];
        p.sx = scale * p.dx; p.sy = scale * p.dy; p.sz = scale * p.dz;
        p.px = S.rp[0][cs] + p.sx; p.py = S.rp[1][cs] + p.sy; p.pz = S.rp[2][cs] + p.sz;
        return true;
    };
#define POSE_SWEEP(restage, active, ...) \
    pose_sweep(S, tile, table, m_ref, start_row, ref_disp, ref_xyz, slot_mask, shell, restage, al8 != 0, frow, active, __VA_ARGS__)

    // ---- sweep 0: the deviation field, its means, the means of the end points --------------------------------------------------
    double sp[3] = {0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0}, smag = 0.0;
    int cnt = 0, want = 0;
    POSE_SWEEP(true, live, [&](int slot, int cs, const float* row) {
        PosePoint p = {};
        const bool ok = point(slot, cs, row, p);
        if (slot < m_ref && S.sel[cs]) ++want;
        if (ok) {
            ++cnt;
            sp[0] = sp[0] + p.px; sp[1] = sp[1] + p.py; sp[2] = sp[2] + p.pz;
            sd[0] = sd[0] + p.sx; sd[1] = sd[1] + p.sy; sd[2] = sd[2] + p.sz;
            smag = smag + sqrt(p.dx * p.dx + p.dy * p.dy + p.dz * p.dz);
        }
        if (deviation && slot < m_ref) {
            double* o = deviation + (fi * m_ref + slot) * 4;
            o[0] = ok ? 1.0 : 0.0; o[1] = ok ? p.dx : 0.0; o[2] = ok ? p.dy : 0.0; o[3] = ok ? p.dz : 0.0;
        }
    });
    cnt = wave_sum(cnt); want = wave_sum(want);
#pragma unroll
    for (int k = 0; k < 3; ++k) { sp[k] = wave_sum(sp[k]); sd[k] = wave_sum(sd[k]); }
    smag = wave_sum(smag);
    const double n0 = (double)cnt;
    if (field && live && lane == 0) {
        double* o = field + fi * VBS_POSEFIELD_COLS;
        o[0] = (want >= 1 && cnt == want) ? 1.0 : 0.0; o[1] = n0;
        o[2] = cnt > 0 ? sd[0] / n0 : 0.0; o[3] = cnt > 0 ? sd[1] / n0 : 0.0; o[4] = cnt > 0 ? sd[2] / n0 : 0.0;
        o[5] = cnt > 0 ? smag / n0 : 0.0;
    }
    if (!pose) return;                                           // (the same for every thread of the grid)

    // ---- sweeps 1, 2: centred sums -> plane, residuals -> SSR -------------------------------------------------------------------
    double m1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m1[k] = cnt > 0 ? sp[k] / n0 : 0.0;
    double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                     // xx, xy, yy, xz, yz
    POSE_SWEEP(many, live && cnt >= 3, [&](int slot, int cs, const float* row) {
        PosePoint p = {};
        if (!point(slot, cs, row, p)) return;
        const double x = p.px - m1[0], y = p.py - m1[1], z = p.pz - m1[2];
        c[0] = c[0] + x * x; c[1] = c[1] + x * y; c[2] = c[2] + y * y; c[3] = c[3] + x * z; c[4] = c[4] + y * z;
    });
#pragma unroll
    for (int q = 0; q < 5; ++q) c[q] = wave_sum(c[q]);
    const double det1 = c[0] * c[2] - c[1] * c[1];
    const bool plane1 = live && cnt >= 3 && fabs(det1) > 1e-300;
    double a = 0.0, b = 0.0, cc = 0.0, ssr = 0.0;
    if (plane1) {
        a = (c[3] * c[2] - c[4] * c[1]) / det1; b = (c[4] * c[0] - c[3] * c[1]) / det1;
        cc = m1[2] - a * m1[0] - b * m1[1];
    }
    POSE_SWEEP(many, plane1, [&](int slot, int cs, const float* row) {
        PosePoint p = {};
        if (!point(slot, cs, row, p)) return;
        const double x = p.px - m1[0], y = p.py - m1[1], z = p.pz - m1[2];
        const double r = z - (a * x + b * y);
        ssr = ssr + r * r;
    });
    ssr = wave_sum(ssr);
    double n_used = n0, flag = plane1 ? 1.0 : 0.0;

    // ---- sweeps 3 - 5: one round of rejection; the kept set is decided by the FIRST plane in every one of them -------------------
    if (reject_k > 0.0) {                                        // (a kernel argument: the same for every thread)
        const bool rej = plane1 && ssr > 0.0;
        const double thr = (reject_k * reject_k) * (ssr / n0);
        const double a1 = a, b1 = b;
        auto kept = [&](const PosePoint& p) -> bool {
            const double x = p.px - m1[0], y = p.py - m1[1], z = p.pz - m1[2];
            const double r = z - (a1 * x + b1 * y);
            return r * r <= thr;
        };
        double kp[3] = {0.0, 0.0, 0.0};
        int kc = 0;
        POSE_SWEEP(many, rej, [&](int slot, int cs, const float* row) {
            PosePoint p = {};
            if (!point(slot, cs, row, p) || !kept(p)) return;
            ++kc;
            kp[0] = kp[0] + p.px; kp[1] = kp[1] + p.py; kp[2] = kp[2] + p.pz;
        });
        kc = wave_sum(kc);
#pragma unroll
        for (int k = 0; k < 3; ++k) kp[k] = wave_sum(kp[k]);
        const bool redo = rej && kc < cnt && kc >= 3;
        const double n2 = (double)kc;
        double m2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) m2[k] = kc > 0 ? kp[k] / n2 : 0.0;
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        POSE_SWEEP(many, redo, [&](int slot, int cs, const float* row) {
            PosePoint p = {};
            if (!point(slot, cs, row, p) || !kept(p)) return;
            const double x = p.px - m2[0], y = p.py - m2[1], z = p.pz - m2[2];
            e[0] = e[0] + x * x; e[1] = e[1] + x * y; e[2] = e[2] + y * y; e[3] = e[3] + x * z; e[4] = e[4] + y * z;
        });
#pragma unroll
        for (int q = 0; q < 5; ++q) e[q] = wave_sum(e[q]);
        const double det2 = e[0] * e[2] - e[1] * e[1];
        const bool plane2 = redo && fabs(det2) > 1e-300;
        double a2 = 0.0, b2 = 0.0, ssr2 = 0.0;
        if (plane2) { a2 = (e[3] * e[2] - e[4] * e[1]) / det2; b2 = (e[4] * e[0] - e[3] * e[1]) / det2; }
        POSE_SWEEP(many, plane2, [&](int slot, int cs, const float* row) {
            PosePoint p = {};
            if (!point(slot, cs, row, p) || !kept(p)) return;
            const double x = p.px - m2[0], y = p.py - m2[1], z = p.pz - m2[2];
            const double r = z - (a2 * x + b2 * y);
            ssr2 = ssr2 + r * r;
        });
        ssr2 = wave_sum(ssr2);
        if (plane2) {
            a = a2; b = b2; cc = m2[2] - a2 * m2[0] - b2 * m2[1];
            ssr = ssr2; n_used = n2; flag = 2.0;
        }
    }
#undef POSE_SWEEP

    if (live && lane == 0) {
        double* o = pose + fi * VBS_POSE_COLS;
        const bool any = flag != 0.0;
        o[0] = flag; o[1] = a; o[2] = b; o[3] = cc;
        o[4] = any ? atan(sqrt(a * a + b * b)) * VBS_DEG : 0.0;
        o[5] = any ? atan2(b, a) * VBS_DEG : 0.0;
        o[6] = any ? sqrt(ssr / n_used) : 0.0;
        o[7] = n_used;
    }
}

void launch_pose_series(vbs_handle* h, const float* table, int m_ref, int start_frame, const double* ref_disp, const double* ref_xyz,
                        const u8* slot_mask, int shell, double scale, double reject_k, int frame_begin, int frame_end,
                        double* deviation, double* field, double* pose, hipStream_t s) {
    const int nf = frame_end - frame_begin;
    const int al8 = ((uintptr_t)table & 7) == 0 ? 1 : 0;         // every frame's rows then start on 8 bytes (40 m_ref bytes a frame)
    VBS_LAUNCH(h, s, "k_pose", k_pose, dim3((unsigned)(((int64_t)nf + POSE_WAVES - 1) / POSE_WAVES)), dim3(POSE_WAVES * 64), 0, s, table,
               m_ref, start_frame, ref_disp, ref_xyz, slot_mask, shell, scale, reject_k, frame_begin, nf, al8, deviation, field,
               pose);
}
