// a9 / a10: the bit planes the labelling kernels read (marker_detection.py:166-195).
//   k_threshold : uint8 mask / area_mask -> 1 bit per pixel (the HBM-streaming stage: 16 px per lane
//                 per load, SWAR non-zero test, v_dot4 bit gather, 4 lanes -> one 64-bit word)
//   k_morph     : band = mask & ~erode_ns(mask)   (maximum/minimum_filter :171-174, window -ns/2..ns/2-1,
//                 pixels outside the image ignored == scipy 'reflect' for a min/max filter)
//                 open = dilate5(erode5(area))    (cv2.morphologyEx MORPH_OPEN 5x5 :195)
//                 (one wave's share: morph_wave.h)
#include <algorithm>

#include "morph_wave.h"

__device__ __forceinline__ u32 nz4(u32 x) {       // 4 bytes -> 4 bits (byte != 0)
    u32 t = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) >> 7;
    return __builtin_amdgcn_udot4(t & 0x01010101u, 0x08040201u, 0u, false);
}

__device__ __forceinline__ u32 nz16(uint4 v) {
    return nz4(v.x) | (nz4(v.y) << 4) | (nz4(v.z) << 8) | (nz4(v.w) << 12);
}

__global__ __launch_bounds__(256) void k_threshold(const u8* __restrict__ mask,
                                                   const u8* __restrict__ area,
                                                   u64* __restrict__ mbits, u64* __restrict__ abits,
                                                   int nb, int H, int W, int P, int WW, int vec_ok) {
    // frames are folded into one index space so that every wave is full; no early return because
    // the 4-lane word assembly below shuffles across lanes.
    const int per_row = P / 16;
    int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < (int64_t)nb * H * per_row;
    int n = 0, y = 0, t = 0;
    if (live) {
        n = (int)(gid / ((int64_t)H * per_row));
        int64_t r = gid - (int64_t)n * H * per_row;
        y = (int)(r / per_row);
        t = (int)(r - (int64_t)y * per_row);
    }
    const int x0 = t * 16;
    u32 bm = 0, ba = 0;
    if (live && x0 < W) {
        int64_t off = ((int64_t)n * H + y) * W + x0;
        if (vec_ok && x0 + 16 <= W) {
            bm = nz16(*reinterpret_cast<const uint4*>(mask + off));
            ba = nz16(*reinterpret_cast<const uint4*>(area + off));
        } else {
            for (int k = 0; k < 16 && x0 + k < W; ++k) {
                bm |= (u32)(mask[off + k] != 0) << k;
                ba |= (u32)(area[off + k] != 0) << k;
            }
        }
    }
    u64 wm = (u64)bm | ((u64)__shfl_down(bm, 1) << 16) | ((u64)__shfl_down(bm, 2) << 32) |
             ((u64)__shfl_down(bm, 3) << 48);
    u64 wa = (u64)ba | ((u64)__shfl_down(ba, 1) << 16) | ((u64)__shfl_down(ba, 2) << 32) |
             ((u64)__shfl_down(ba, 3) << 48);
    if (live && (t & 3) == 0) {
        int64_t o = ((int64_t)n * H + y) * WW + (t >> 2);
        mbits[o] = wm;
        abits[o] = wa;
    }
}

void launch_threshold(vbs_handle* h, Workspace& w, const u8* mask, const u8* area, int nb, hipStream_t s) {
    int64_t total = (int64_t)nb * h->H * (h->P / 16);
    int vec_ok = (h->W % 16 == 0) && (((uintptr_t)mask | (uintptr_t)area) % 16 == 0);
    VBS_LAUNCH(h, s, "k_threshold", k_threshold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mask, area,
                       w.mask_bits, w.area_bits, nb, h->H, h->W, h->P, h->WW, vec_ok);
}

// ------------------------------------------------------------------------------------------------
template <int NS14>
__global__ __launch_bounds__(256) void k_morph(const u64* __restrict__ mbits, const u64* __restrict__ abits,
                                               u64* __restrict__ band, u64* __restrict__ opn, const u32* __restrict__ only,
                                               const u32* __restrict__ nslow,
                                               int nb, int H, int W, int WW, int G, int strips, int rows_per_strip,
                                               int waves_per_frame) {
    if (nslow && *nslow == 0) return;                    // the fused kernel handed no frame on
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = gw / waves_per_frame;
    if (n >= nb || (only && !only[n])) return;           // wave-uniform (`only`: just the frames the fused path handed on)
    morph_wave<NS14>(mbits, abits, band, opn, H, W, WW, G, strips, rows_per_strip, n, gw - n * waves_per_frame);
}

void launch_morph(vbs_handle* h, Workspace& w, int nb, const u32* only, hipStream_t s) {
    const int G = 64 / h->WW;                            // strips per wave (WW <= 64)
    // strips per frame: enough waves to fill the chip several times over, but strips much longer than the ns - 1 rows
    // each re-reads
    // one round of resident waves when the batch is large (94 / 78 VGPRs: 5 / 6 waves per SIMD on 1024 SIMDs; with 6144
    // waves the large branch ran a full round and then a 20 % one), else as many as the strip length allows
    const int resident = (h->bp.ns == 14 ? 5 : 6) * 1024;
    int wpf = resident / std::max(nb, 1);
    if (wpf < 4) wpf = (2 * resident + nb - 1) / nb;     // small strips would dominate: take two rounds instead
    if (VBS_KNOB("VBS_MORPH_WPF")) wpf = VBS_KNOB("VBS_MORPH_WPF");
    wpf = std::max(1, std::min(wpf, h->H / (2 * h->bp.ns) / G));      // strips of at least 2 ns rows
    const int strips = wpf * G, rps = (h->H + strips - 1) / strips;
    const int waves = nb * wpf;
    dim3 grid((waves + 3) / 4);
    if (h->bp.ns == 14)
        VBS_LAUNCH(h, s, "k_morph", k_morph<14>, grid, dim3(256), 0, s, w.mask_bits, w.area_bits, w.band_bits, w.open_bits,
                   only, only ? w.slow_total : nullptr, nb, h->H, h->W, h->WW, G, strips, rps, wpf);
    else
        VBS_LAUNCH(h, s, "k_morph", k_morph<8>, grid, dim3(256), 0, s, w.mask_bits, w.area_bits, w.band_bits, w.open_bits,
                   only, only ? w.slow_total : nullptr, nb, h->H, h->W, h->WW, G, strips, rps, wpf);
}

// ------------------------------------------------------------------------------------------------
// CHAIN_APPROX_SIMPLE vertex multiplicity of a border pixel from its 8-neighbourhood (bit d = neighbour
// in chain direction d is foreground).  The outer border visits the pixel once per maximal arc of
// background neighbours that contains a 4-neighbour (an arc made of one diagonal pixel is stepped
// over diagonally); arriving from the foreground neighbour that precedes the arc and leaving to the
// one that follows it, the point is kept iff the two step directions differ.
void make_contour_lut(u8 out[256]) {
    for (int p = 0; p < 256; ++p) {
        int cnt = 0;
        if (p == 0) {
            cnt = 1;                                     // isolated pixel: written once
        } else if (p != 255) {
            for (int a = 0; a < 8; ++a) {
                // arc starts at direction a: a is background, a-1 is foreground
                if (((p >> a) & 1) || !((p >> ((a + 7) & 7)) & 1)) continue;
                int b = a;
                bool has4 = false;
                while (!((p >> (b & 7)) & 1)) {
                    if (((b & 7) & 1) == 0) has4 = true;
                    ++b;
                }
                if (!has4) continue;
                int q = (a + 7) & 7;                      // neighbour before the arc
                int r = b & 7;                            // neighbour after the arc
                int dir_in = (q + 4) & 7;                 // step q -> p
                int dir_out = r;                          // step p -> r
                if (dir_in != dir_out) ++cnt;
            }
        }
        out[p] = (u8)cnt;
    }
}
