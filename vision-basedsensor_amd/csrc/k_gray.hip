// a3: BGR->gray (marker_detection.py:114), the fixed-point cvtColor of cv2 on uint8 - bit-exact, like the blurs behind it.
#include "common.h"

// gray pixels of 4 consecutive BGR pixels (12 bytes as 3 dwords): cv2's fixed-point weights (common.h gray_coef)
__device__ __forceinline__ u32 bgr4_to_gray(u32 a, u32 b, u32 c, const GrayCoef& gc) {
    const u32 g0 = (gc.cb * (a & 255u) + gc.cg * ((a >> 8) & 255u) + gc.cr * ((a >> 16) & 255u) + gc.half) >> gc.shift;
    const u32 g1 = (gc.cb * (a >> 24) + gc.cg * (b & 255u) + gc.cr * ((b >> 8) & 255u) + gc.half) >> gc.shift;
    const u32 g2 = (gc.cb * ((b >> 16) & 255u) + gc.cg * (b >> 24) + gc.cr * (c & 255u) + gc.half) >> gc.shift;
    const u32 g3 = (gc.cb * ((c >> 8) & 255u) + gc.cg * ((c >> 16) & 255u) + gc.cr * (c >> 24) + gc.half) >> gc.shift;
    return g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
}

// cvtColor(BGR2GRAY) (or a plain copy for 1 channel) into the pitched gray plane the blur reads: a streaming kernel,
// 16 pixels per thread (three 16-byte loads, one 16-byte store) when the rows are 16-byte aligned: 0.85-1.0 us per
// 1280x1024 frame (5.3-6.2 TB/s of its 5.2 MB).  It runs in line in front of the blur (converting a pass ahead on a side
// stream measured no faster: profiles/NOTES.md section 9).
// (Converting inside the blur's own loader was built and measured: LDS-DMA staging of the raw bytes kept the matrix
//  operands in registers only at the price of 50 spilled VGPRs - 5 us per frame against 1.45.)
__global__ __launch_bounds__(256) void k_gray(const u8* __restrict__ frames, int channels, int64_t stride_n,
                                              int64_t stride_row, u8* __restrict__ gray, int H, int W, int P, GrayCoef gc,
                                              int vec_ok, int flat) {
    __shared__ __align__(16) uint4 raw[2][3 * 256];     // 24 KB: the 48 bytes of each thread's 16 pixels, loaded coalesced
    const int n = blockIdx.z;
    if (flat) {
        // dense BGR frame (row stride 3 W, gray pitch W): one run of H W pixels, 2 x 4096 per block, loaded as consecutive
        // 16-byte pieces by consecutive lanes (both halves in flight together, streamed past the caches) and handed to
        // their owners through LDS
        const int64_t npx = (int64_t)H * W, pb = (int64_t)blockIdx.x * 8192;
        const u8* src = frames + (int64_t)n * stride_n;
        u8* dstf = gray + (int64_t)n * H * P;
        if (pb + 8192 <= npx) {                          // block-uniform
            const uint4* s4 = reinterpret_cast<const uint4*>(src + pb * 3);
            uint4 v[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                typedef u32 u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(s4 + q * 256 + threadIdx.x));
                v[q] = make_uint4(t.x, t.y, t.z, t.w);
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) raw[q / 3][(q % 3) * 256 + threadIdx.x] = v[q];
            __syncthreads();
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const uint4 r0 = raw[hf][3 * threadIdx.x], r1 = raw[hf][3 * threadIdx.x + 1], r2 = raw[hf][3 * threadIdx.x + 2];
                *reinterpret_cast<uint4*>(dstf + pb + 4096 * hf + threadIdx.x * 16) =
                    make_uint4(bgr4_to_gray(r0.x, r0.y, r0.z, gc), bgr4_to_gray(r0.w, r1.x, r1.y, gc),
                               bgr4_to_gray(r1.z, r1.w, r2.x, gc), bgr4_to_gray(r2.y, r2.z, r2.w, gc));
            }
        } else {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int64_t p0 = pb + 4096 * hf + threadIdx.x * 16;
                if (p0 >= npx) return;                   // (H W is a multiple of 16 in flat mode)
                const uint4* s4 = reinterpret_cast<const uint4*>(src + p0 * 3);
                const uint4 r0 = s4[0], r1 = s4[1], r2 = s4[2];
                *reinterpret_cast<uint4*>(dstf + p0) =
                    make_uint4(bgr4_to_gray(r0.x, r0.y, r0.z, gc), bgr4_to_gray(r0.w, r1.x, r1.y, gc),
                               bgr4_to_gray(r1.z, r1.w, r2.x, gc), bgr4_to_gray(r2.y, r2.z, r2.w, gc));
            }
        }
        return;
    }
    // rows with their own stride (a crop view, a pitched plane): thread = (row, 16-pixel piece), pieces of consecutive rows
    // side by side in a block - a 480-pixel row fills 30 of a block's 256 threads when every block takes one row
    // (0.73 us per 480x450 BGR frame of the reference's cropped configuration, the largest kernel of that workload)
    const int ppr = P >> 4, idx = blockIdx.x * 256 + threadIdx.x;
    const int y = idx / ppr, x0 = (idx - y * ppr) * 16;
    if (y >= H) return;
    const u8* src = frames + (int64_t)n * stride_n + (int64_t)y * stride_row;
    u8* dst = gray + ((int64_t)n * H + y) * P + x0;
    if (vec_ok && channels == 3 && x0 + 16 <= W) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src + (int64_t)x0 * 3);
        const uint4 r0 = s4[0], r1 = s4[1], r2 = s4[2];
        *reinterpret_cast<uint4*>(dst) = make_uint4(bgr4_to_gray(r0.x, r0.y, r0.z, gc), bgr4_to_gray(r0.w, r1.x, r1.y, gc),
                                                    bgr4_to_gray(r1.z, r1.w, r2.x, gc), bgr4_to_gray(r2.y, r2.z, r2.w, gc));
        return;
    }
    u32 out[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; ++k) {
        const int x = x0 + k;
        u32 v = 0;
        if (x < W) {
            if (channels == 1) {
                v = src[x];
            } else {   // cv2 8-bit BGR2GRAY, fixed point (coefficient set: common.h gray_coef)
                const u8* p = src + (int64_t)x * channels;
                v = (gc.cb * p[0] + gc.cg * p[1] + gc.cr * p[2] + gc.half) >> gc.shift;
            }
        }
        out[k >> 2] |= v << (8 * (k & 3));
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
}

// the cvtColor stage on its own (vbs_bgr2gray): dense [n,H,W] output, one pixel per thread
__global__ void k_gray_dense(const u8* __restrict__ frames, int64_t stride_n, int64_t stride_row,
                             u8* __restrict__ out, int H, int W, GrayCoef gc) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= W) return;
    const u8* p = frames + (int64_t)n * stride_n + (int64_t)y * stride_row + (int64_t)x * 3;
    out[((int64_t)n * H + y) * W + x] = (u8)((gc.cb * p[0] + gc.cg * p[1] + gc.cr * p[2] + gc.half) >> gc.shift);
}

void launch_gray_dense(vbs_handle* h, const u8* frames, int nb, int64_t stride_n, int64_t stride_row, u8* out,
                       hipStream_t s) {
    dim3 grid((h->W + 255) / 256, h->H, nb);
    VBS_LAUNCH(h, s, "k_gray_dense", k_gray_dense, grid, dim3(256), 0, s, frames, stride_n, stride_row, out, h->H, h->W,
               gray_coef(h->gray_bits));
}

void launch_gray(vbs_handle* h, const u8* frames, int nb, int channels, int64_t stride_n,
                 int64_t stride_row, u8* gray, hipStream_t s) {
    const int vec_ok = (reinterpret_cast<uintptr_t>(frames) % 16 == 0) && (stride_n % 16 == 0) && (stride_row % 16 == 0);
    const int flat = vec_ok && channels == 3 && stride_row == (int64_t)h->W * 3 && h->P == h->W && ((int64_t)h->H * h->W) % 16 == 0;
    dim3 grid = flat ? dim3((unsigned)(((int64_t)h->H * h->W + 8191) / 8192), 1, nb)
                     : dim3((unsigned)(((int64_t)h->H * (h->P / 16) + 255) / 256), 1, nb);
    VBS_LAUNCH(h, s, "k_gray", k_gray, grid, dim3(256), 0, s, frames, channels, stride_n, stride_row, gray,
                       h->H, h->W, h->P, gray_coef(h->gray_bits), vec_ok, flat);
}
