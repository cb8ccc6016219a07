// a4-a5: two uint8 GaussianBlurs (OpenCV fixed-point model), DoG + 15 (mod 256), inRange - the model is in blur_common.h.
// k_blur_mfma evaluates both passes of both blurs as banded-Toeplitz products on the int8 matrix cores, for every geometry;
// k_blur16.hip has the faster kernel for frames it takes, and launch_blur, which chooses.
#include <algorithm>

#include "blur_common.h"

// ---- MFMA path -------------------------------------------------------------------------------------
// A 101-tap separable blur is 140 MACs per pixel per pass: compute-bound on the vector ALU (v_dot4 at half
// rate), but a banded-Toeplitz matrix product for the matrix cores, and exact there: taps < 128 and
// p - 128 are int8, v_mfma_i32_32x32x32_i8 accumulates in int32.
//
//   horizontal  Hs[y][x]  = sum_k (p[y][xw+k] - 128) * tap[k - x - (LEFT - R)]        (A = image rows from LDS,
//                                                                                       B = Toeplitz, constant)
//               H = Hs + 128 * 256                                                      (taps sum to 256)
//   vertical    V[x][y]   = sum_k Hs_hi[k][x] * tap[..] * 256 + sum_k (Hs_lo[k][x] - 128) * tap[..] + const
//
// One wave owns a 32-column strip and slides down it 32 rows per step.  The horizontal result tile (column
// on the lane, 16 rows in the accumulator registers) is split into its signed high byte and its low byte
// (offset by 128), packed four rows to a dword and used directly as the A operand of the vertical product
// (X^T * T^T sums over the accumulator's row index, so no lane movement and no LDS).  The last NK tiles are
// kept in a register ring, so every horizontal tile is computed once.  The vertical result has the output
// row on the lane and 16 columns in registers: each lane assembles its row's 16 mask bits from sign bits
// and the two lane halves are OR-ed into the 32-bit half word of the bit image.

// reflect-101 bytes of one 16-byte chunk that touches the image border or is not dword aligned
__device__ __forceinline__ uint4 fetch_chunk_slow(const u8* src, int px, int W) {
    u32 w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        u32 v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (u32)src[reflect101(px + 4 * d + b, W)] << (8 * b);
        w[d] = v;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int NK, int SA0, int NKA, bool U8OUT>
__global__ __launch_bounds__(256, 2) void k_blur_mfma(const u8* __restrict__ gray, int64_t gstride_n,
                                                      int64_t gstride_row, const uint4* __restrict__ frags,
                                                      u64* __restrict__ bits, u8* __restrict__ area_u8,
                                                      u32* __restrict__ fstat, int H, int W, int WW,
                                                      int tiles_per_seg, int k3, int k8, int span_i, int dbg_arg) {
#ifdef VBS_DEBUG_KNOBS
    const int dbg = dbg_arg;                            // tools/gpu_ncc_phase.py: phase timing by early exit
#else
    constexpr int dbg = 0;
#endif
    constexpr int LEFT = 32 * ((NK - 1) / 2);
    constexpr int ROWB = 128 + 32 * (NK - 1);          // bytes staged per image row
    constexpr int CH = ROWB / 16;
    constexpr int STRIDE = ROWB + 16;                  // 68 (52) dwords: 16 consecutive rows hit all banks
    constexpr int NIT = (32 * CH + 255) / 256;
    __shared__ __align__(16) u8 tile[2][32 * STRIDE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform, and known to the compiler to be
    const int hh = lane >> 5, m = lane & 31;
    const int X0 = blockIdx.x * 128, n = blockIdx.z;
    const int tilesY = (H + 31) / 32;
    const int tile0 = blockIdx.y * tiles_per_seg;
    const int ntiles = min(tiles_per_seg, tilesY - tile0);
    if (ntiles <= 0) return;
    const int Y0 = tile0 * 32, nsteps = ntiles + NK - 1;
    const u8* g = gray + (int64_t)n * gstride_n;
    const bool aligned = ((gstride_row & 3) == 0) && ((gstride_n & 3) == 0) && ((reinterpret_cast<uintptr_t>(gray) & 3) == 0);
    const bool rows24 = gstride_row > 0 && gstride_row < (1 << 24) && (int64_t)H * gstride_row < (1ll << 31);   // (uniform)

    v4i bh[NK], bha[NKA], tv[NK], tva[NKA];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        uint4 a = frags[(0 * NK + s) * 64 + lane], b = frags[(1 * NK + s) * 64 + lane];
        bh[s] = v4i{(int)a.x, (int)a.y, (int)a.z, (int)a.w};
        tv[s] = v4i{(int)b.x, (int)b.y, (int)b.z, (int)b.w};
    }
#pragma unroll
    for (int s = 0; s < NKA; ++s) {
        uint4 a = frags[(2 * NK + s) * 64 + lane], b = frags[(2 * NK + NKA + s) * 64 + lane];
        bha[s] = v4i{(int)a.x, (int)a.y, (int)a.z, (int)a.w};
        tva[s] = v4i{(int)b.x, (int)b.y, (int)b.z, (int)b.w};
    }

    // this thread's chunks of the staged tile: row, pixel offset, LDS offset; fast = plain 16-byte load
    int c_row[NIT], c_px[NIT], c_lds[NIT];
    bool c_on[NIT], c_fast[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        int c = tid + 256 * it;
        c_on[it] = c < 32 * CH;
        c_row[it] = c / CH;
        int ch = c - c_row[it] * CH;
        c_px[it] = X0 - LEFT + 16 * ch;
        c_lds[it] = c_row[it] * STRIDE + 16 * ch;
        c_fast[it] = aligned && c_px[it] >= 0 && c_px[it] + 16 <= W;
    }
    // plain chunks are loaded a step ahead into registers and written to LDS at the end of the step; border chunks
    // (few, only in the first / last workgroup of a row) are gathered byte by byte at commit time.  (Two steps ahead,
    // paid for by reading the small kernel's vertical fragments from LDS: measured slower, 1.65 against 1.44 us.)
    uint4 stage[NIT];
    auto row_of = [&](int t, int it) { return g + (int64_t)reflect101(Y0 - LEFT + 32 * t + c_row[it], H) * gstride_row; };
    auto fetch = [&](int t) {
#pragma unroll
        for (int it = 0; it < NIT; ++it)
            if (c_on[it] && c_fast[it]) {
                // (rows24: the row pitch and a frame's size fit 24 / 31 bits - one full-rate multiply and a 32-bit
                //  offset from the scalar frame pointer instead of a 64-bit multiply per chunk and step)
                const u32* s32 = rows24 ? reinterpret_cast<const u32*>(g + (u32)(__mul24(reflect101(Y0 - LEFT + 32 * t + c_row[it], H), (int)gstride_row) + c_px[it]))
                                        : reinterpret_cast<const u32*>(row_of(t, it) + c_px[it]);
                stage[it] = make_uint4(s32[0], s32[1], s32[2], s32[3]);
            }
    };
    auto commit = [&](int t, int buf) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (!c_on[it]) continue;
            if (c_fast[it]) {
                uint4 v = stage[it];
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                *reinterpret_cast<uint4*>(&tile[buf][c_lds[it]]) = v;
            } else {
                uint4 v = fetch_chunk_slow(row_of(t, it), c_px[it], W);
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                *reinterpret_cast<uint4*>(&tile[buf][c_lds[it]]) = v;
            }
        }
    };

    v4i rLh[NK], rLl[NK], rSh[NK], rSl[NK];            // ring of horizontal tiles: large / small kernel, hi / lo bytes
#pragma unroll
    for (int s = 0; s < NK; ++s) rLh[s] = rLl[s] = rSh[s] = rSl[s] = v4i{0, 0, 0, 0};
    const int xw = X0 + 32 * wave;                     // first column of this wave's strip
    u32* const bits32 = reinterpret_cast<u32*>(bits) + ((int64_t)n * H * WW + (xw >> 6)) * 2 + ((xw >> 5) & 1);   // (uniform)
    const u32 colmask = xw + 32 <= W ? 0xFFFFFFFFu : (xw >= W ? 0u : ((1u << (W - xw)) - 1u));
    // sum tap*H = 256*Dhi + Dlo + 256*(128 + 32768); + 2^15 to round; the large kernel also carries
    // (15 - thresh) << 16 so that its high word is im_blur_8 + 15 - thresh (mod 2^16)
    // (host computes k3 = 256*(128+32768) + 2^15, k8 = k3 + (15 - thresh) << 16, span = hi - thresh)
    const u32 span = (u32)span_i;
    u32 total = 0, pend_off = 0xFFFFFFFFu, pend_full = 0;

    fetch(0);
    commit(0, 0);
    // every load issued so far (the operand fragments above all) has landed: without this the loop's first uses
    // keep a vmcnt wait that, in steady state, stalls on the prefetch of the next tile instead
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
    __syncthreads();
    for (int t0 = 0; t0 < nsteps; t0 += NK) {
#pragma unroll
        for (int u = 0; u < NK; ++u) {
            const int t = t0 + u;
            if (t >= nsteps) break;                    // uniform
            const bool more = t + 1 < nsteps;
            if (more) fetch(t + 1);
            const u8* tb = &tile[t & 1][m * STRIDE + 32 * wave + 16 * hh];
            v4i a[NK];
#pragma unroll
            for (int s = 0; s < NK; ++s) a[s] = *reinterpret_cast<const v4i*>(tb + 32 * s);
            {
                v16i acc = {};
#pragma unroll
                for (int s = 0; s < NK; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bh[s], acc, 0, 0, 0);
                pack_tile(acc, rLh[u], rLl[u]);
            }
            {
                v16i acc = {};
#pragma unroll
                for (int s = 0; s < NKA; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[SA0 + s], bha[s], acc, 0, 0, 0);
                pack_tile(acc, rSh[u], rSl[u]);
            }
            if (t >= NK - 1 && dbg != 2) {
                v16i d8 = {}, d3 = {};
#pragma unroll
                for (int o = 0; o < NK; ++o) d8 = __builtin_amdgcn_mfma_i32_32x32x32_i8(rLh[(u + 1 + o) % NK], tv[o], d8, 0, 0, 0);
#pragma unroll
                for (int o = 0; o < NKA; ++o) d3 = __builtin_amdgcn_mfma_i32_32x32x32_i8(rSh[(u + 1 + SA0 + o) % NK], tva[o], d3, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) d8[i] = (d8[i] << 8) + k8;
#pragma unroll
                for (int o = 0; o < NK; ++o) d8 = __builtin_amdgcn_mfma_i32_32x32x32_i8(rLl[(u + 1 + o) % NK], tv[o], d8, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) d3[i] = (d3[i] << 8) + k3;
#pragma unroll
                for (int o = 0; o < NKA; ++o) d3 = __builtin_amdgcn_mfma_i32_32x32x32_i8(rSl[(u + 1 + SA0 + o) % NK], tva[o], d3, 0, 0, 0);
                if (dbg == 1) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) asm volatile("" :: "v"(d8[i]), "v"(d3[i]));
                } else {
                u32 sgn = 0;                           // bit i = 1 when register i is OUT of range
#pragma unroll
                for (int i = 15; i >= 0; --i) {
                    u32 dg = (((u32)d8[i] >> 16) - ((u32)d3[i] >> 16)) & 255u;   // (blur_8 - blur_3 + 15 - thresh) mod 256 (:128)
                    sgn = __builtin_amdgcn_alignbit(sgn, span - dg, 31);
                }
                u32 w16 = ~sgn & 0xFFFFu;              // register i = column (i&3) + 8(i>>2) + 4*half
                u32 w32 = ((w16 & 0xFu) | ((w16 & 0xF0u) << 4) | ((w16 & 0xF00u) << 8) | ((w16 & 0xF000u) << 12)) << (4 * hh);
                const int y = Y0 + 32 * (t - (NK - 1)) + m;
                w32 = (y < H) ? (w32 & colmask) : 0u;
                u32 full = w32 | (u32)__shfl_xor((int)w32, 32);
                if (hh == 0 && y < H && (xw >> 6) < WW) {    // stored behind this step's commit (below)
                    pend_off = (u32)__mul24(y, 2 * WW);
                    pend_full = full;
                    total += __popc(full);
                }
                if (U8OUT && y < H) {                    // uint8 image for the staged API: 4 pixels per store where possible
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int x = xw + 8 * q + 4 * hh;
                        const u32 nib = (w32 >> (8 * q + 4 * hh)) & 15u;
                        const u32 four = ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;      // bit r -> byte r = 0 / 255
                        u8* dst = area_u8 + ((int64_t)n * H + y) * W + x;
                        if (((W & 3) == 0) && x + 3 < W && ((reinterpret_cast<uintptr_t>(area_u8) & 3) == 0)) {
                            *reinterpret_cast<u32*>(dst) = four;
                        } else {
                            for (int r = 0; r < 4; ++r)
                                if (x + r < W) dst[r] = (u8)(four >> (8 * r));
                        }
                    }
                }
                }                                      // (dbg != 1)
            }
            if (more) commit(t + 1, (t + 1) & 1);
            // The mask word goes out only now: issued before the commit, its acknowledgement would be part of the commit's
            // wait for the prefetched rows, every step and for all four waves at the barrier.
            if (pend_off != 0xFFFFFFFFu) { bits32[pend_off] = pend_full; pend_off = 0xFFFFFFFFu; }
            __syncthreads();
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) total += __shfl_xor((int)total, off);
    if (lane == 0 && total) atomicAdd(&fstat[n * 8 + 0], total);
}

// Toeplitz operand fragments in the lane layout of v_mfma_i32_32x32x32_i8 (lane = 32*half + column; a
// lane's 16 bytes pair with the other operand's 16 bytes of the same half, so only the pairing matters):
//   horizontal (B operand, k = pixel of the staged window): byte e of half h is window pixel 32s + 16h + e
//   vertical   (B operand, k = row of ring tile o):         byte 4q + r of half h is tile row 8q + 4h + r
std::vector<u32> blur_mfma_fragments(const std::vector<int>& taps_a, const std::vector<int>& taps_b, int nk,
                                     int sa0, int nka) {
    const int left = 32 * ((nk - 1) / 2);
    std::vector<u32> out((size_t)(2 * nk + 2 * nka) * 64 * 4, 0);
    auto fill = [&](int frag, const std::vector<int>& taps, int kbase, bool vertical) {
        const int R = (int)taps.size() / 2;
        for (int lane = 0; lane < 64; ++lane) {
            const int h = lane >> 5, col = lane & 31;
            for (int e = 0; e < 16; ++e) {
                int k = kbase + (vertical ? 8 * (e >> 2) + 4 * h + (e & 3) : 16 * h + e);
                int idx = k - col - (left - R);
                u32 v = (idx >= 0 && idx <= 2 * R) ? (u32)taps[idx] : 0u;
                out[((size_t)frag * 64 + lane) * 4 + (e >> 2)] |= v << (8 * (e & 3));
            }
        }
    };
    for (int s = 0; s < nk; ++s) { fill(0 * nk + s, taps_b, 32 * s, false); fill(1 * nk + s, taps_b, 32 * s, true); }
    for (int s = 0; s < nka; ++s) {
        fill(2 * nk + s, taps_a, 32 * (sa0 + s), false);
        fill(2 * nk + nka + s, taps_a, 32 * (sa0 + s), true);
    }
    return out;
}

void launch_blur_mfma(vbs_handle* h, Workspace& w, const u8* gray, int64_t gstride_n, int64_t gstride_row, int nb,
                      u8* area_u8, hipStream_t s) {
    const int k3 = 256 * (128 + 32768) + 32768, k8 = k3 + (15 - h->bp.thresh) * 65536;
    const int gx = (h->P + 127) / 128, tilesY = (h->H + 31) / 32;
    int nseg = std::min(tilesY, std::max(1, (1024 + gx * nb - 1) / (gx * nb)));     // few frames: split columns
    const int tps = (tilesY + nseg - 1) / nseg;
    nseg = (tilesY + tps - 1) / tps;
    dim3 grid(gx, nseg, nb);
#define BLUR_GO(NK, SA0, NKA, U8)                                                                            \
    VBS_LAUNCH(h, s, "k_blur_mfma", (k_blur_mfma<NK, SA0, NKA, U8>), grid, dim3(256), 0, s, gray, gstride_n, \
               gstride_row, h->blur_frags, w.area_bits, area_u8, w.fstat, h->H, h->W, h->WW, tps, k3, k8,  \
               h->bp.hi - h->bp.thresh, VBS_KNOB("VBS_BLUR_DBG"))
    if (!h->bp.small) { if (area_u8) BLUR_GO(5, 1, 3, true); else BLUR_GO(5, 1, 3, false); }
    else { if (area_u8) BLUR_GO(3, 0, 3, true); else BLUR_GO(3, 0, 3, false); }
#undef BLUR_GO
}
