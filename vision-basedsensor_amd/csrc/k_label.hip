// a11 / a12: the general labelling kernel (marker_detection.py:176-196 on bit-packed planes), behind every faster route.
//   k_label     : one workgroup per (frame, mask): runs of 1-bits are the union-find nodes, parents
//                 live in LDS, unions between adjacent rows with LDS atomicMin; the root of a
//                 component is its first run in raster order, so component ids come out in
//                 ndimage.label order (:176) and reversed they are cv2.findContours' order (:196).
//                 band mask (4-connectivity): count / sum x / sum y per component (center_of_mass :181)
//                 open mask (8-connectivity): integer moments up to order 4 of the CHAIN_APPROX_SIMPLE
//                 contour vertices, classified per border pixel from its 8-neighbourhood by a LUT (make_contour_lut).
#include <algorithm>
#include <cstdlib>

#include "morph_wave.h"

// find with path halving.  Parents only ever move to a smaller-indexed member of the same set (hooking is an
// atomicMin on a root, halving stores an ancestor), so the racy 32-bit stores are benign: a lost hook is
// re-established by uf_union's retry with the value atomicMin returned.
__device__ __forceinline__ u32 uf_find(volatile u32* parent, u32 x) {
    for (;;) {
        u32 p = parent[x];
        if (p == x) return x;
        u32 gp = parent[p];
        if (gp == p) return p;
        parent[x] = gp;
        x = gp;
    }
}

// read-only walk to the root (flatten phase: there, every store must be a final root)
__device__ __forceinline__ u32 uf_root(volatile u32* parent, u32 x) {
    u32 p;
    while ((p = parent[x]) != x) x = p;
    return x;
}

__device__ __forceinline__ void uf_union(u32* parent, u32 a, u32 b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { u32 t = a; a = b; b = t; }
        u32 old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// node (run) index of the run that contains bit k of word j in `row`
__device__ __forceinline__ u32 node_of(const u64* __restrict__ row, const u32* __restrict__ wb, int j,
                                       int k) {
    int jj = j, kk = k, start;
    for (;;) {
        u64 w = row[jj];
        u64 below = (kk == 63) ? ~0ull : ((1ull << (kk + 1)) - 1ull);
        u64 z = ~w & below;
        if (z) { start = 64 - __clzll(z); break; }
        if (jj == 0 || !(row[jj - 1] >> 63)) { start = 0; break; }
        --jj;
        kk = 63;
    }
    u64 w = row[jj];
    u64 prev = (jj > 0) ? (row[jj - 1] >> 63) : 0ull;
    u64 starts = w & ~((w << 1) | prev);
    u64 lowmask = start ? ((1ull << start) - 1ull) : 0ull;
    return wb[jj] + (u32)__popcll(starts & lowmask);
}

__device__ __forceinline__ u32 block_exclusive_scan(u32 v, u32* tmp, u32* total) {
    // 1024 threads = 16 waves; tmp has >= 17 entries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        u32 t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) tmp[wave] = inc;
    __syncthreads();
    if (wave == 0) {                                   // scan of the (<= 16) wave totals by one wave
        const int nw = blockDim.x >> 6;
        u32 t = lane < nw ? tmp[lane] : 0u, ti = t;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            u32 o = __shfl_up(ti, d);
            if (lane >= d) ti += o;
        }
        if (lane < nw) tmp[lane] = ti - t;
        if (lane == nw - 1) tmp[16] = ti;
    }
    __syncthreads();
    u32 ex = inc - v + tmp[wave];
    *total = tmp[16];
    __syncthreads();
    return ex;
}

// moment index of x^a y^b, a+b <= 4:  (0,0) (1,0) (0,1) (2,0) (1,1) (0,2) (3,0) (2,1) (1,2) (0,3) (4,0) (3,1) (2,2) (1,3) (0,4)
#define NONE32 0xFFFFFFFFu

__device__ __forceinline__ u32 wave_scan_incl(u32 x) {   // inclusive prefix sum over the 64 lanes
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ u32 wave_last(u32 x) { return (u32)__builtin_amdgcn_readlane((int)x, 63); }


// Per-lane view of G = 64 / WW consecutive image rows ("a step"): lane = g * WW + j holds word j (64 px) of row
// y0 + g, the run-start bits in it, the node index of the first run that starts in it, and the node of the run that
// enters it from the left (NONE32 if none).  Lanes are in raster order, so one wave-wide prefix sum numbers the runs.
struct RowState {
    u64 w, st;
    u32 base, cin;
};

// Build the state of a step from its words (lanes outside the step hold 0).  `j` = word column of the lane,
// `rowbase` = node index of the step's first run (wave-uniform), advanced past the step.
__device__ __forceinline__ RowState make_row_state(u64 w, int j, u32& rowbase) {
    RowState s;
    s.w = w;
    // (cross-lane moves run with all lanes enabled and are selected afterwards: a DPP read from an exec-masked
    //  lane returns 0, so they must never sit inside a conditional)
    const u64 msb_all = (u64)(dpp_shr1((u32)(w >> 32)) >> 31);
    const u64 msb = j ? msb_all : 0ull;                   // bit 63 of the word to the left in the row
    s.st = w & ~((w << 1) | msb);
    const u32 c = __popcll(s.st);
    const u32 inc = wave_scan_incl(c);
    s.base = rowbase + inc - c;
    rowbase += wave_last(inc);
    // node entering from the left = last run of word j-1, which is that word's last start, or - when word j-1 is
    // all ones inside one long run - the run entering IT (resolved by iterating; one pass unless runs span > 64 px)
    const bool cont = (w & 1ull) && msb;
    const bool full = cont && (w == ~0ull);
    const u32 last_here = c ? s.base + c - 1 : NONE32;
    u32 lastnode = last_here;
    s.cin = NONE32;
    for (int it = 0; it < 64; ++it) {
        u32 upn = dpp_shr1(lastnode);
        u32 ncin = cont ? upn : NONE32;                  // cont implies j > 0
        u32 nlast = c ? last_here : (full ? ncin : NONE32);
        bool changed = (ncin != s.cin) || (nlast != lastnode);
        s.cin = ncin;
        lastnode = nlast;
        if (!__any(changed)) break;
    }
    return s;
}

__device__ __forceinline__ RowState zero_state() { RowState z = {0ull, 0ull, 0u, NONE32}; return z; }

// state of the word to the left / right in the same row (zeros at the row ends)
__device__ __forceinline__ RowState state_left(const RowState& s, int j) {
    RowState r;
    r.w = dpp_shr1(s.w); r.st = dpp_shr1(s.st); r.base = dpp_shr1(s.base); r.cin = dpp_shr1(s.cin);
    return j ? r : zero_state();
}
__device__ __forceinline__ RowState state_right(const RowState& s, int j, int WW) {
    RowState r;
    r.w = dpp_shl1(s.w); r.st = dpp_shl1(s.st); r.base = dpp_shl1(s.base); r.cin = dpp_shl1(s.cin);
    return (j + 1 < WW) ? r : zero_state();
}

// state held by another lane (ds_bpermute; executed by every lane)
__device__ __forceinline__ RowState state_from(const RowState& s, int src) {
    RowState r;
    r.w = __shfl(s.w, src); r.st = __shfl(s.st, src); r.base = __shfl(s.base, src); r.cin = __shfl(s.cin, src);
    return r;
}

// node (run) index of the run containing bit k of this lane's word
__device__ __forceinline__ u32 node_in_row(const RowState& s, int k) {
    const u64 below = k ? ((1ull << k) - 1ull) : 0ull;
    const u64 z = ~s.w & below;
    if (z) {
        const int stpos = 64 - __clzll(z);
        return s.base + (u32)__popcll(s.st & ((1ull << stpos) - 1ull));
    }
    if ((s.w & 1ull) && s.cin != NONE32) return s.cin;
    return s.base;
}

// unions of the runs of this lane's word (`cur`) with the runs of the row above (`prev` = same column, one row up):
// 4-connectivity (m = 0) or 8 (m = 1).  Cross-lane moves first, by every lane; the loops after them may diverge.
__device__ __forceinline__ void link_rows(u32* parent, const RowState& cur, const RowState& prev, int j, int WW, int m) {
    const RowState pl = state_left(prev, j), pr = state_right(prev, j, WW);
    const u64 B = cur.w, A = prev.w;
    u64 adj = A;
    if (m == 1) adj |= (A << 1) | (A >> 1) | (pl.w >> 63) | (pr.w << 63);
    u64 mB = (B & adj) ? B : 0ull;
    while (mB) {                                       // groups of consecutive 1s of B inside this word
        u64 lowbit = mB & (~mB + 1ull);
        u64 t = mB + lowbit;
        u64 g = mB & ~t;
        mB &= t;
        if (!(g & adj)) continue;
        const u32 nb_ = node_in_row(cur, __ffsll((long long)g) - 1);
        u64 rm = g;
        if (m == 1) rm |= (g << 1) | (g >> 1);
        u64 mA = A & rm;
        while (mA) {
            u64 lb = mA & (~mA + 1ull);
            u64 t2 = mA + lb;
            u64 ga = mA & ~t2;
            mA &= t2;
            uf_union(parent, node_in_row(prev, __ffsll((long long)ga) - 1), nb_);
        }
        if (m == 1) {
            if ((g & 1ull) && (pl.w >> 63)) uf_union(parent, node_in_row(pl, 63), nb_);
            if ((g >> 63) && (pr.w & 1ull)) uf_union(parent, node_in_row(pr, 0), nb_);
        }
    }
}

// component id of pixel (x, y) of the opened mask from the general path's tables, 0xFFFF when it is not foreground
__device__ __forceinline__ u32 comp_at(const u64* __restrict__ bits, const u32* __restrict__ wbase,
                                       const u32* __restrict__ node_comp, int H, int W, int WW, int x, int y) {
    if (x < 0 || y < 0 || x >= W || y >= H) return 0xFFFFu;
    const u64* row = bits + (int64_t)y * WW;
    if (!((row[x >> 6] >> (x & 63)) & 1ull)) return 0xFFFFu;
    return node_comp[node_of(row, wbase + (int64_t)y * WW, x >> 6, x & 63)];
}

// 4-deep register ring of step words: PF_INIT issues the loads of steps y0, y0+G, .., PF_NEXT hands out the step at
// y and issues the one at y + 4 G, so a step never waits for a load it has just issued.  Lane (g, j) holds word j of
// row y + g; rows >= ylim read as 0.
#define PF_LOAD(ptr, yy, ylim) ((act && (yy) < (ylim)) ? (inv ? (~(ptr)[(int64_t)(yy) * WW + j] & vmask) : (ptr)[(int64_t)(yy) * WW + j]) : 0ull)
#define PF_INIT(ptr, y0, ylim)                               \
    u64 pf0 = PF_LOAD(ptr, (y0) + g, ylim);                  \
    u64 pf1 = PF_LOAD(ptr, (y0) + G + g, ylim);              \
    u64 pf2 = PF_LOAD(ptr, (y0) + 2 * G + g, ylim);          \
    u64 pf3 = PF_LOAD(ptr, (y0) + 3 * G + g, ylim);
#define PF_NEXT(ptr, y, ylim, out)                           \
    out = pf0; pf0 = pf1; pf1 = pf2; pf2 = pf3;              \
    pf3 = PF_LOAD(ptr, (y) + 4 * G + g, ylim);

// One workgroup (16 waves) per (frame, mask).  Wave w owns the strip of rows [w R, (w+1) R), R = ceil(H / 16), and
// walks it top-down G = 64 / WW rows at a time (3 at W = 1280), lane = g * WW + j holding word j of row y0 + g:
// run starts, node indices (one wave prefix sum, raster order), the run entering from the left and the links to the
// row above come from registers, DPP moves and a few ds_bpermute; the union-find table lives in LDS (path halving,
// atomicMin hooking).  The 15 strip boundaries are linked at the end.  Node indices follow raster order, so the
// root (minimum) of a component is its first run and component ids come out in ndimage.label order.
// mode 0: label the band mask (blockIdx.y = 0, 4-conn) and the opened mask (1, 8-conn).
// mode 1: only for frames whose opened mask has holes (Euler check of mode 0): label its COMPLEMENT (4-conn), find the
//         background components that do not touch the image border (= holes) and fill them in open_bits: outer
//         contours, "inside the contour" and RETR_EXTERNAL's nesting rule are invariant under hole filling, and after
//         it every border is an outer border, which is what the per-pixel vertex table assumes.
// mode 2: relabel the (now hole-free) opened mask of those frames.
// MORPH = 14 | 8 (the few-frames path): the workgroup first makes the frame's band / opened planes itself (k_morph's waves,
// its sixteen in turn) - one launch less on a path where a launch costs as much as a kernel; 0: the planes are there
template <int MORPH>
// (band_bits / open_bits: plain pointers - the MORPH instances WRITE the planes (morph_wave) and read them back later in the
//  kernel; a write through a restrict-qualified pointer-to-const was undefined behaviour)
__global__ __launch_bounds__(1024) void k_label(u64* band_bits,
                                                u64* open_bits,
                                                u32* __restrict__ wbase_all, u32* __restrict__ node_pos_all,
                                                u32* __restrict__ node_comp_all, u32* __restrict__ ncomp_all,
                                                u32* __restrict__ band_first, u64* __restrict__ band_sums,
                                                u32* __restrict__ area_first, i64* __restrict__ area_sums,
                                                u32* __restrict__ fstat, const u8* __restrict__ lut_g,
                                                const u32* __restrict__ slow_flag, const u32* __restrict__ nslow,
                                                unsigned short* __restrict__ probe_all, int nb, int all, int H, int W, int WW,
                                                int maxm, int stop, const u64* __restrict__ mbits, const u64* __restrict__ abits,
                                                int mG, int mstrips, int mrps, int mwpf) {
    __shared__ u32 parent[VBS_RUN_CAP];                // union-find parents; later [m=1] the moment accumulators
    __shared__ u64 bnd_w[16][64];                      // last row of every strip: words,
    __shared__ u32 bnd_base[16][64], bnd_cin[16][64];  //   first-node indices, entering nodes
    __shared__ u32 wtot[16], wfirst[16];               // runs per strip, node index of the strip's first run
    __shared__ u32 acc_cnt[1024];                      // band: pixel counts;  open: first pixel (anchor) per component
    __shared__ u64 acc_sx[1024], acc_sy[1024];
    __shared__ u32 tmp[32];
    __shared__ u8 lut[256];
    __shared__ int euler4;                             // 4 x Euler number of the opened mask (bit quads)
    // Only the frames the fast path (k_ccl.hip) handed on (slow_flag; all of them when `all`): a workgroup takes such a
    // frame through the four stages in turn - label the band mask, label the opened mask, fill its holes (if any),
    // relabel it (if any was filled) - and then writes the probes k_finalize's polygon test reads.  Every exit of a
    // stage's body is workgroup-uniform, so it is a `continue` of the stage loop.
    if (nslow && *nslow == 0) return;                    // the fused kernel handed no frame on
    for (int n = blockIdx.x; n < nb; n += gridDim.x) {
    if (!all && !slow_flag[n]) continue;
    if (MORPH) {                                        // (the stage loop's first fence + barrier publish the planes)
        for (int wv = (int)(threadIdx.x >> 6); wv < mwpf; wv += 16)
            morph_wave<(MORPH ? MORPH : 14)>(mbits, abits, band_bits, open_bits, H, W, WW, mG, mstrips, mrps, n, wv);
    }
    for (int stage = 0; stage < 4; ++stage) {
    __threadfence();                                    // the previous stage's global writes (holes, filled bits, tables)
    __syncthreads();                                    // are visible; its readers of the LDS tables are done
    const int mode = stage < 2 ? 0 : stage - 1;
    const int m = stage == 0 ? 0 : (stage == 2 ? 2 : 1);    // 0 band (4-conn), 1 open (8-conn), 2 background of open
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int NW = H * WW;
    if (mode == 1 && fstat[n * 8 + 4] == 0) continue;    // no holes in this frame
    if (mode == 2 && fstat[n * 8 + 7] == 0) continue;    // nothing was filled
    const bool inv = (m == 2);                          // walk the complement of the opened mask
    const int mslot = (m == 2) ? 0 : m;                 // the background pass borrows the band pass's scratch tables
    const u64* bits = (m == 0 ? band_bits : open_bits) + (int64_t)n * NW;
    u32* wbase = wbase_all + ((int64_t)n * 2 + mslot) * NW;
    u32* node_pos = node_pos_all + ((int64_t)n * 2 + mslot) * VBS_RUN_CAP;
    u32* node_comp = node_comp_all + ((int64_t)n * 2 + mslot) * VBS_RUN_CAP;
    if (stop == 9) continue;
    if (tid < 256) lut[tid] = lut_g[tid];
    if (tid == 0) euler4 = 0;
    for (int i = tid; i < 1024; i += nthr) { acc_cnt[i] = 0; acc_sx[i] = 0; acc_sy[i] = 0; }
    const int R = (H + 15) / 16;
    const int ya = min(H, wave * R), yb = min(H, ya + R);                  // this wave's rows
    const int G = 64 / WW;                                                 // rows per step (WW <= 64)
    const int g = lane / WW, j = lane - g * WW;
    const bool act = g < G;
    const u64 vmask = valid_mask(j, W);
    const int up_src = g ? lane - WW : lane + (G - 1) * WW;                // lane holding the word one row up
    bnd_w[wave][lane] = 0; bnd_base[wave][lane] = 0; bnd_cin[wave][lane] = NONE32;

    // ---- 1: runs per strip -> first node index of every strip ---------------------------------------
    {
        u32 c = 0;
        PF_INIT(bits, ya, yb)
        for (int y = ya; y < yb; y += G) {
            u64 w; PF_NEXT(bits, y, yb, w)
            const u64 msb_all = (u64)(dpp_shr1((u32)(w >> 32)) >> 31);
            const u64 msb = j ? msb_all : 0ull;
            c += __popcll(w & ~((w << 1) | msb));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
        if (lane == 0) wtot[wave] = c;
    }
    __syncthreads();
    u32 nruns = 0, mybase = 0;
    for (int w = 0; w < 16; ++w) { if (w == wave) mybase = nruns; nruns += wtot[w]; }
    if (lane == 0) wfirst[wave] = mybase;
    if (nruns > VBS_RUN_CAP) {                          // block-uniform
        if (tid == 0) { if (m != 2) ncomp_all[n * 2 + m] = 0; atomicMin((int*)&fstat[n * 8 + 2], VBS_ECAPACITY); }
        continue;
    }

    // ---- 2: label the strip, G rows per step ------------------------------------------------------------
    RowState first_row = zero_state();
    {
        u32 rowbase = mybase;
        RowState last = zero_state();                   // previous step
        PF_INIT(bits, ya, yb)
        for (int y = ya; y < yb; y += G) {
            u64 w; PF_NEXT(bits, y, yb, w)
            const int yr = y + g;                       // this lane's row
            if (!__any(w != 0ull)) {                    // empty step (a third of a marker frame's rows): no run starts,
                if (act && yr < yb) wbase[(int64_t)yr * WW + j] = rowbase;     // nothing to link below either
                last = zero_state();
                continue;
            }
            RowState cur = make_row_state(w, j, rowbase);
            if (act && yr < yb) wbase[(int64_t)yr * WW + j] = cur.base;
            u64 st = cur.st;
            u32 nd = cur.base;
            while (st) {
                int k = __ffsll((long long)st) - 1;
                st &= st - 1;
                parent[nd] = nd;
                node_pos[nd] = (u32)(yr * W + 64 * j + k);
                ++nd;
            }
            // the row above: same step (g > 0) or the last row of the previous step (g == 0)
            const RowState a = state_from(cur, up_src), b = state_from(last, up_src);
            RowState prev = g ? a : b;
            if (!act) prev = zero_state();
            if (y == ya && g == 0) { first_row = cur; prev = zero_state(); }    // strip boundary: linked in pass 3
            __builtin_amdgcn_wave_barrier();            // the new nodes' parents are initialised before any union
            if (!(stop & 32)) link_rows(parent, cur, prev, j, WW, m == 1 ? 1 : 0);
            last = cur;
            if (y + G >= yb) {                          // last step: keep the strip's last row for the wave below
                const int gl = (yb - 1 - y);
                if (act && g == gl) { bnd_w[wave][j] = cur.w; bnd_base[wave][j] = cur.base; bnd_cin[wave][j] = cur.cin; }
            }
        }
    }
    __syncthreads();
    // ---- 3: link every strip's first row with the last row of the strip above --------------------------
    if (wave > 0 && ya < yb && !(stop & 32)) {
        RowState cur = (act && g == 0) ? first_row : zero_state();
        RowState prev = zero_state();
        if (act && g == 0) { prev.w = bnd_w[wave - 1][j]; prev.base = bnd_base[wave - 1][j]; prev.cin = bnd_cin[wave - 1][j]; }
        const u64 msb_all = (u64)(dpp_shr1((u32)(prev.w >> 32)) >> 31);
        const u64 msb = j ? msb_all : 0ull;
        prev.st = prev.w & ~((prev.w << 1) | msb);
        link_rows(parent, cur, prev, j, WW, m == 1 ? 1 : 0);
    }
    __syncthreads();
    if ((stop & 15) == 2) continue;

    // ---- D: flatten -------------------------------------------------------------------------------
    for (u32 i = tid; i < nruns; i += nthr) {
        u32 r = uf_root(parent, i);                    // no halving here: a late halving store could
        if (r != i) parent[i] = r;                     // overwrite another thread's final root
    }
    __syncthreads();

    // ---- E: component ids = rank of the root in raster order ---------------------------------------
    const int chunk2 = (nruns + nthr - 1) / nthr;
    const u32 r0 = tid * chunk2, r1 = min(r0 + (u32)chunk2, nruns);
    u32 nroot = 0;
    for (u32 i = r0; i < r1; ++i) nroot += (parent[i] == i);
    u32 ncomp;
    u32 cbase = block_exclusive_scan(nroot, tmp, &ncomp);
    if ((m != 2 && ncomp > (u32)maxm) || ncomp > 1024u || (m == 1 && ncomp * NMOM * 8u > sizeof(parent) / 2)) {
        if (tid == 0) { if (m != 2) ncomp_all[n * 2 + m] = 0; atomicMin((int*)&fstat[n * 8 + 2], VBS_ECAPACITY); }
        continue;
    }
    u32* first = (m == 0 ? band_first : area_first) + (int64_t)n * maxm;
    for (u32 i = r0; i < r1; ++i) {
        if (parent[i] == i) {
            const u32 pos = node_pos[i];                // first pixel of the component = start of its root run
            if (m != 2) first[cbase] = pos;
            if (m == 1) acc_cnt[cbase] = pos;          // LDS copy of the anchor for phase F
            parent[i] = i | ((cbase + 1) << 16);       // root: id in the high half
            ++cbase;
        }
    }
    __syncthreads();
    // component id of every node: to global (k_finalize's polygon test) and, as uint16, into the lower half of
    // the parent table (read the ids into registers first: the uint16 table overwrites the parents in place)
    constexpr int PER = (VBS_RUN_CAP + 1023) / 1024;
    unsigned short cids[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        u32 i = tid + k * 1024;
        u32 cid = 0;
        if (i < nruns) {
            u32 root = parent[i] & 0xFFFFu;
            cid = (parent[root] >> 16) - 1;
            node_comp[i] = cid;
        }
        cids[k] = (unsigned short)cid;
    }
    if (tid == 0 && m != 2) { ncomp_all[n * 2 + m] = ncomp; fstat[n * 8 + 5 + m] = ncomp; }
    __syncthreads();
    unsigned short* cid16 = reinterpret_cast<unsigned short*>(parent);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        u32 i = tid + k * 1024;
        if (i < nruns) cid16[i] = cids[k];
    }
    u64* acc = reinterpret_cast<u64*>(parent) + VBS_RUN_CAP / 4;           // upper half: [ncomp][15] moments (m = 1)
    if (m == 1) for (u32 c = tid; c < ncomp * NMOM; c += nthr) acc[c] = 0;
    __syncthreads();
    if ((stop & 15) == 4) continue;

    // ---- F: per-component sums, same walk; sums stay in registers and are flushed with LDS atomics when the
    //         component under the lane changes (a lane sees rows y0 + g, y0 + g + G, ... of one word column) --------
    if (m == 2) {
        // background components that touch the image border are the outside; the others are holes: fill them
        for (int pass = 0; pass < 2; ++pass) {
            u32 rowbase = wfirst[wave];
            PF_INIT(bits, ya, yb)
            for (int y = ya; y < yb; y += G) {
                u64 wv; PF_NEXT(bits, y, yb, wv)
                const int yr = y + g;
                RowState cur = make_row_state(wv, j, rowbase);
                u64 w = wv, fill = 0;
                while (w) {
                    u64 lowbit = w & (~w + 1ull);
                    u64 t = w + lowbit;
                    u64 gg = w & ~t;
                    w &= t;
                    const u32 cid = cid16[node_in_row(cur, __ffsll((long long)gg) - 1)];
                    if (pass == 0) {
                        const int xl = W - 1 - 64 * j;                   // bit of the last image column, if in this word
                        const bool edge = (yr == 0) || (yr == H - 1) || (j == 0 && (gg & 1ull)) ||
                                          (xl >= 0 && xl < 64 && ((gg >> xl) & 1ull));
                        if (edge && acc_cnt[cid] == 0) acc_cnt[cid] = 1;
                    } else if (acc_cnt[cid] == 0) {
                        fill |= gg;
                    }
                }
                if (pass == 1 && fill)
                    open_bits[(int64_t)n * NW + (int64_t)yr * WW + j] = (~wv & vmask) | fill;
            }
            __syncthreads();
        }
        u32 nholes = 0;
        for (u32 c = tid; c < ncomp; c += nthr) nholes += (acc_cnt[c] == 0);
        if (nholes) atomicAdd(&fstat[n * 8 + 7], nholes);
        continue;
    }
    // One work item per RUN (node): its position comes back from node_pos, its extent from the bits; every lane has
    // work (a word walk leaves most lanes idle on a marker frame) and the sums go to the component's LDS accumulators.
    if (m == 0) {
        for (u32 i = tid; i < nruns; i += nthr) {
            const u32 cid = cid16[i], pos = node_pos[i];
            const u32 y = pos / (u32)W, x0 = pos - y * (u32)W;
            const u64* row = bits + (int64_t)y * WW;
            int jw = (int)(x0 >> 6);
            const int b0 = (int)(x0 & 63);
            const u64 t = ~(row[jw] >> b0);
            u32 len = t ? (u32)(__ffsll((long long)t) - 1) : 64u;
            if (b0 + (int)len == 64)                     // reaches the word's last bit: continues while the next words start with 1s
                for (++jw; jw < WW; ++jw) {
                    const u64 nw = ~row[jw];
                    const u32 tz = nw ? (u32)(__ffsll((long long)nw) - 1) : 64u;
                    len += tz;
                    if (tz < 64) break;
                }
            atomicAdd(&acc_cnt[cid], len);
            atomicAdd(&acc_sx[cid], (u64)len * x0 + (u64)len * (len - 1) / 2);
            atomicAdd(&acc_sy[cid], (u64)len * (u64)y);
        }
        __syncthreads();
        u64* bs = band_sums + (int64_t)n * maxm * 4;
        for (u32 c = tid; c < ncomp; c += nthr) {
            bs[c * 4 + 0] = acc_cnt[c];
            bs[c * 4 + 1] = acc_sx[c];
            bs[c * 4 + 2] = acc_sy[c];
        }
    } else {
        // Euler number by bit quads (8-connected foreground): E = (Q1 - Q3 - 2 QD) / 4 over all 2x2 windows of the
        // zero-padded image; window (x, y) = pixels (x..x+1, y..y+1).  A work item counts the windows whose top row is
        // its word's row (and, for row 0, the padding row above it).  holes = components - E.
        int e4 = 0;
        for (int idx = tid; idx < NW; idx += nthr) {
            const int yr = idx / WW, jc = idx - yr * WW;
            const u64 wv = bits[idx];
            const u64 dn = yr + 1 < H ? bits[idx + WW] : 0ull;
            if (!(wv | dn) && !(yr == 0)) {
                if (jc + 1 >= WW) continue;
                if (!((bits[idx + 1] | (yr + 1 < H ? bits[idx + 1 + WW] : 0ull)) & 1ull)) continue;
            }
            const u64 wn_ = jc + 1 < WW ? bits[idx + 1] : 0ull;
            const u64 dn_ = (jc + 1 < WW && yr + 1 < H) ? bits[idx + 1 + WW] : 0ull;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 1 && yr != 0) continue;
                const u64 a = q ? 0ull : wv, an = q ? 0ull : wn_, bq = q ? wv : dn, bn = q ? wn_ : dn_;
                if (a | bq | (an & 1ull) | (bn & 1ull)) {
                    u64 a1 = (a >> 1) | (an << 63), b1 = (bq >> 1) | (bn << 63);
                    u64 x2 = (a ^ a1) ^ (bq ^ b1);
                    u64 pairs = (a & a1) | (a & bq) | (a & b1) | (a1 & bq) | (a1 & b1) | (bq & b1);
                    u64 qd = (a & b1 & ~a1 & ~bq) | (a1 & bq & ~a & ~b1);
                    e4 += __popcll(x2 & ~pairs) - __popcll(x2 & pairs) - 2 * __popcll(qd);
                    if (jc == 0) e4 += (int)((a ^ bq) & 1ull);               // window x = -1: only (0,y), (0,y+1)
                }
            }
        }
        for (u32 i = tid; i < nruns; i += nthr) {
            const u32 cid = cid16[i], pos = node_pos[i];
            const int y = (int)(pos / (u32)W), x0 = (int)(pos - (u32)y * (u32)W);
            const u32 fp = acc_cnt[cid];
            const int ay = (int)(fp / (u32)W), ax = (int)(fp - (u32)ay * (u32)W);
            const u64* rowm = bits + (int64_t)y * WW;
            const bool hasu = y > 0, hasd = y + 1 < H;
            i64 s[NMOM];
#pragma unroll
            for (int q = 0; q < NMOM; ++q) s[q] = 0;
            bool more = true;
            for (int jw = x0 >> 6; more && jw < WW; ++jw) {      // word segments of the run
                const u64 w = rowm[jw];
                const int lo = jw == (x0 >> 6) ? (x0 & 63) : 0;
                const u64 t = ~(w >> lo);
                const int len = t ? __ffsll((long long)t) - 1 : 64;
                if (len == 0) break;                             // (the run ended exactly at the previous word's last bit)
                const int hi = lo + len - 1;
                more = hi == 63;
                const u64 gg = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull)) & ~((1ull << lo) - 1ull);
                const bool contR = more && jw + 1 < WW && (rowm[jw + 1] & 1ull);     // the run goes on in the next word
                const u64 up = hasu ? rowm[jw - WW] : 0ull, dn = hasd ? rowm[jw + WW] : 0ull;
                u64 upL = 0, upR = 0, dnL = 0, dnR = 0;  // edge bits of the neighbouring words, only where a pixel needs them
                if (lo == 0 && jw > 0) { upL = hasu ? rowm[jw - 1 - WW] >> 63 : 0ull; dnL = hasd ? rowm[jw - 1 + WW] >> 63 : 0ull; }
                if (hi == 63 && jw + 1 < WW) { upR = hasu ? rowm[jw + 1 - WW] & 1ull : 0ull; dnR = hasd ? rowm[jw + 1 + WW] & 1ull : 0ull; }
                const u64 E = (gg >> 1) | (contR ? 1ull << 63 : 0ull);
                const u64 Wd = (gg << 1) | (jw > (x0 >> 6) ? 1ull : 0ull);
                const u64 NE = (up >> 1) | (upR << 63), NWd = (up << 1) | upL;
                const u64 SE = (dn >> 1) | (dnR << 63), SW = (dn << 1) | dnL;
                u64 bg = gg & ~(up & dn & E & Wd);
                // pixels inside a straight horizontal edge (patterns 241 / 31: no vertex, lut = 0) are dropped by bit
                // operations, so the long top / bottom rows of a blob do not cost one loop turn per pixel
                bg &= ~(E & Wd & ((~up & ~NE & ~NWd & dn & SE & SW) | (up & NE & NWd & ~dn & ~SE & ~SW)));
                while (bg) {
                    const int k = __ffsll((long long)bg) - 1;
                    bg &= bg - 1;
                    const u32 pat = (u32)((E >> k) & 1ull) | ((u32)((NE >> k) & 1ull) << 1) |
                                    ((u32)((up >> k) & 1ull) << 2) | ((u32)((NWd >> k) & 1ull) << 3) |
                                    ((u32)((Wd >> k) & 1ull) << 4) | ((u32)((SW >> k) & 1ull) << 5) |
                                    ((u32)((dn >> k) & 1ull) << 6) | ((u32)((SE >> k) & 1ull) << 7);
                    const int mult = lut[pat];
                    if (!mult) continue;
                    const int dx = 64 * jw + k - ax, dy = y - ay;
                    if (max(abs(dx), abs(dy)) <= 150) {          // 4 * 150^4 < 2^31: products in 32 bits, sums in 64
                        const int x2 = dx * dx, y2 = dy * dy, mx = mult * dx, my = mult * dy;
                        s[0] += mult;
                        s[1] += mx;                 s[2] += my;
                        s[3] += mx * dx;            s[4] += mx * dy;            s[5] += my * dy;
                        s[6] += mx * x2;            s[7] += my * x2;            s[8] += mx * y2;
                        s[9] += my * y2;
                        s[10] += mult * x2 * x2;    s[11] += mx * x2 * dy;      s[12] += mult * x2 * y2;
                        s[13] += mx * dy * y2;      s[14] += mult * y2 * y2;
                    } else {
                        const i64 ml = mult, dl = dx, el = dy, x2 = dl * dl, y2 = el * el;
                        s[0] += ml;
                        s[1] += ml * dl;            s[2] += ml * el;
                        s[3] += ml * x2;            s[4] += ml * dl * el;       s[5] += ml * y2;
                        s[6] += ml * x2 * dl;       s[7] += ml * x2 * el;       s[8] += ml * dl * y2;
                        s[9] += ml * y2 * el;
                        s[10] += ml * x2 * x2;      s[11] += ml * x2 * dl * el; s[12] += ml * x2 * y2;
                        s[13] += ml * dl * el * y2; s[14] += ml * y2 * y2;
                    }
                }
                if (!contR) break;
            }
#pragma unroll
            for (int q = 0; q < NMOM; ++q)
                if (s[q]) atomicAdd(&acc[cid * NMOM + q], (u64)s[q]);
        }
        if (e4) atomicAdd(&euler4, e4);
        __syncthreads();
        i64* as = area_sums + (int64_t)n * maxm * VBS_AREA_SUMS;
        for (u32 c = tid; c < ncomp * NMOM; c += nthr) as[(c / NMOM) * VBS_AREA_SUMS + (c % NMOM)] = (i64)acc[c];
        if (tid == 0) fstat[n * 8 + 4] = (u32)((int)ncomp - euler4 / 4);       // holes in the opened mask
    }
    }                                                   // stages
    // probes: component ids of the 2x2 pixel cell around every band centroid (the fast path writes them itself)
    __threadfence();
    __syncthreads();
    if ((int)fstat[n * 8 + 2] == 0) {
        const int NW = H * WW;
        const u64* obits = open_bits + (int64_t)n * NW;
        const u32* wb1 = wbase_all + ((int64_t)n * 2 + 1) * NW;
        const u32* nc1 = node_comp_all + ((int64_t)n * 2 + 1) * VBS_RUN_CAP;
        const u64* bs = band_sums + (int64_t)n * maxm * 4;
        unsigned short* pr = probe_all + (int64_t)n * maxm * 4;
        const u32 nband = ncomp_all[n * 2 + 0];
        for (u32 i = threadIdx.x; i < nband; i += blockDim.x) {
            const double cn = (double)bs[i * 4 + 0];
            const float xf = (float)((double)bs[i * 4 + 1] / cn), yf = (float)((double)bs[i * 4 + 2] / cn);
            const int ix = (int)floorf(xf), iy = (int)floorf(yf);
            pr[i * 4 + 0] = (unsigned short)comp_at(obits, wb1, nc1, H, W, WW, ix, iy);
            pr[i * 4 + 1] = (unsigned short)comp_at(obits, wb1, nc1, H, W, WW, ix + 1, iy);
            pr[i * 4 + 2] = (unsigned short)comp_at(obits, wb1, nc1, H, W, WW, ix, iy + 1);
            pr[i * 4 + 3] = (unsigned short)comp_at(obits, wb1, nc1, H, W, WW, ix + 1, iy + 1);
        }
    }
    }                                                   // frames
}

// ms == null: k_label<0> over the frames flagged in w.slow_flag (`all`: every frame), planes as they lie in the workspace; with
// `nslow` it leaves at once when that counts no frame.  ms (behind k_stage_lat): k_label<ns>, which makes the planes itself.
void launch_label(vbs_handle* h, Workspace& w, int nb, int all, const u32* nslow, const MorphStrips* ms, hipStream_t s) {
    const auto kernel = !ms ? k_label<0> : h->bp.ns == 14 ? k_label<14> : k_label<8>;      // (one signature)
    const MorphStrips m = ms ? *ms : MorphStrips{0, 0, 0, 0};
    VBS_LAUNCH(h, s, "k_label", kernel, dim3(ms ? nb : std::min(nb, 64)), dim3(1024), 0, s, w.band_bits, w.open_bits, w.wbase,
               w.node_pos, w.node_comp, w.ncomp, w.band_first, w.band_sums, w.area_first, w.area_sums, w.fstat, h->lut, w.slow_flag,
               nslow, w.probe, nb, all, h->H, h->W, h->WW, h->maxm, ms ? 0 : VBS_KNOB("VBS_LABEL_STOP"),
               (const u64*)(ms ? w.mask_bits : nullptr), (const u64*)(ms ? w.area_bits : nullptr), m.G, m.strips, m.rps, m.wpf);
}
