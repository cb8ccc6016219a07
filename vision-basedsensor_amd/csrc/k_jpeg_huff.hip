// Motion-JPEG entropy decode on the device: baseline Huffman scans WITHOUT restart intervals, decoded as
// self-synchronising subsequences - Klein & Wiseman's parallel Huffman decoding as Weissenberger & Schmidt apply it to JPEG
// ("Accelerating JPEG Decompression on GPUs", 2021).  A Huffman decoder started at a wrong bit position falls into step with
// the true code-word boundaries after a few symbols, so every thread starts at a multiple of S bits with a guessed state,
// and rounds of "decode the next subsequence, compare with what its owner found" establish the true state at every
// subsequence's start.
//   k_jpeg_huff  one workgroup per frame, 256 threads, the frame's decode tables in LDS, NO communication between
//                workgroups.  Phases per chunk of 256 subsequences, separated by __syncthreads(): speculate, synchronise,
//                count (exclusive scan of the blocks completed), write (dense int16 blocks, DC as differences).
//   k_jpeg_dc    per component an inclusive scan of the DC differences in that component's scan order, one wave each.
// Input: the de-stuffed scans vbs_mjpeg_scan_batch staged.  Output: ent / tab / frame_base as vbs_mjpeg_reconstruct reads them.
// The decode step is csrc/jpeg_huff_common.h, shared with the host emulation of the debug library.
// Bounds: every loop is bounded by a launch-time quantity (scan_bits, blocks per frame, threads per chunk); scan reads are
// clamped to the staged length + guard; every store index is checked against the frame's block count; speculative chains
// decode garbage by design and write nothing outside the workgroup's LDS arrays.
#include <hip/hip_runtime.h>

#include "../../include/vbs.h"
#include "jpeg_huff_common.h"

namespace {

constexpr int HT = 256;           // threads = subsequences per chunk

__constant__ uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Info { int32_t v[8]; };

__global__ __launch_bounds__(HT) void k_jpeg_huff(const uint8_t* __restrict__ stage, const int64_t* __restrict__ scan_off,
                                                  const int64_t* __restrict__ scan_bits_, const int32_t* __restrict__ table_set,
                                                  const vbs_huff_set* __restrict__ sets, int n_sets, Info info, uint32_t S,
                                                  uint32_t* __restrict__ ent, uint32_t* __restrict__ tab,
                                                  int64_t* __restrict__ frame_base, int32_t* __restrict__ status) {
    __shared__ vbs_huff_set T;
    __shared__ vbs_huff_state s[HT + 1];
    __shared__ uint32_t cnt[HT];
    __shared__ uint32_t wsum[HT / 64];
    __shared__ uint8_t zz[64];
    __shared__ unsigned long long fail;
    const int n = blockIdx.x, i = threadIdx.x;
    vbs_huff_geom g;
    vbs_huff_geom_init(g, info.v, zz);
    const int64_t cap = info.v[6] / 2;
    // the frame's constant table row and base: every block dense
    for (int b = i; b < g.nblk; b += HT) tab[(int64_t)n * g.nblk + b] = (uint32_t)(32 * b) << 7 | 127u;
    if (i == 0) { frame_base[n] = (int64_t)n * cap; fail = ~0ull; }
    if (i < 64) zz[i] = ZZ[i];
    const int64_t bits64 = scan_bits_[n];
    const int32_t ts = table_set[n];
    if (ts < 0 || ts >= n_sets || bits64 < 0 || bits64 > VBS_MJPEG_DEVICE_BITS_MAX) {           // (uniform over the workgroup)
        if (i == 0) status[n] = (ts < 0 || ts >= n_sets || bits64 < 0) ? VBS_EINVAL : VBS_MJPEG_SHORT;
        return;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(sets + ts);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
        for (int k = i; k < (int)(sizeof(vbs_huff_set) / 4); k += HT) dst[k] = src[k];
    }
    const uint32_t scan_bits = (uint32_t)bits64;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(stage + scan_off[n]);
    int16_t* coef = reinterpret_cast<int16_t*>(ent + (int64_t)n * cap);
    const uint32_t nsub = (uint32_t)(((uint64_t)scan_bits + S - 1) / S);
    vbs_huff_state carry{0u, 0u};
    uint32_t base_blocks = 0;
    __syncthreads();
    for (uint32_t sub0 = 0; sub0 < nsub && base_blocks < (uint32_t)g.nblk; sub0 += HT) {        // (uniform: both are shared values)
        const int nt = (int)min((uint32_t)HT, nsub - sub0);
        const uint64_t cbase = (uint64_t)sub0 * S;
        auto end_of = [&](int j) { return (uint32_t)min(cbase + (uint64_t)(j + 1) * S, (uint64_t)scan_bits); };
        // 1. speculate
        vbs_huff_state st{0u, VBS_HUFF_INVALID};
        bool active = false;
        if (i == 0) s[0] = carry;
        if (i < nt) {
            st = i ? vbs_huff_state{(uint32_t)cbase + (uint32_t)i * S, 0u} : carry;
            uint32_t blocks = 0;
            vbs_huff_run<false>(T, words, scan_bits, g, st, end_of(i), blocks, 0u, nullptr);
            s[i + 1] = st;
            cnt[i] = blocks;
            active = st.cz != VBS_HUFF_INVALID;
        }
        __syncthreads();
        // 2. synchronise: in round r thread i is at subsequence i + r, so no two threads touch the same entry in a round;
        // a position is visited in later rounds by lower threads, and thread 0's chain is the true one
        for (int r = 1; r < nt; ++r) {
            const int j = i + r;
            if (active && j < nt) {
                uint32_t blocks = 0;
                vbs_huff_run<false>(T, words, scan_bits, g, st, end_of(j), blocks, 0u, nullptr);
                const bool eq = vbs_huff_same(st, s[j + 1]);
                s[j + 1] = st;
                cnt[j] = blocks;
                if (eq || st.cz == VBS_HUFF_INVALID) active = false;
            } else active = false;
            if (!__syncthreads_or(active ? 1 : 0)) break;
        }
        // 3. count: exclusive scan of the blocks completed per subsequence
        const uint32_t mine = i < nt ? cnt[i] : 0u;
        uint32_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if ((i & 63) >= d) incl += up;
        }
        if ((i & 63) == 63) wsum[i >> 6] = incl;
        __syncthreads();
        uint32_t before = base_blocks, total = base_blocks;
        for (int w = 0; w < HT / 64; ++w) {
            if (w < (i >> 6)) before += wsum[w];
            total += wsum[w];
        }
        const uint32_t b0 = before + incl - mine;
        // 4. write
        if (i < nt && b0 < (uint32_t)g.nblk) {
            vbs_huff_state w = s[i];
            int rc = w.cz == VBS_HUFF_INVALID ? VBS_HUFF_STEP_INVALID : VBS_HUFF_STEP_OK;
            uint32_t blocks = 0;
            if (rc == VBS_HUFF_STEP_OK) rc = vbs_huff_run<true>(T, words, scan_bits, g, w, end_of(i), blocks, b0, coef);
            if (rc != VBS_HUFF_STEP_OK) atomicMin(&fail, (unsigned long long)(sub0 + i) << 2 | (unsigned long long)rc);   // (LDS)
        }
        carry = s[nt];
        base_blocks = total;
        __syncthreads();                                  // (s, cnt and wsum are rewritten by the next chunk)
    }
    if (i == 0) {
        int rc = VBS_OK;
        if (fail != ~0ull) rc = (fail & 3ull) == VBS_HUFF_STEP_SHORT ? VBS_MJPEG_SHORT : VBS_EINVAL;
        else if (base_blocks < (uint32_t)g.nblk) rc = VBS_MJPEG_SHORT;
        status[n] = rc;
    }
}

// DC differences -> DC values, in place: wave c of the frame's workgroup scans component c in its scan order
__global__ __launch_bounds__(256) void k_jpeg_dc(uint32_t* __restrict__ ent, const int32_t* __restrict__ status, Info info) {
    const int n = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (status[n] != VBS_OK) return;
    vbs_huff_geom g;
    vbs_huff_geom_init(g, info.v, nullptr);
    if (c >= g.ncomp) return;
    int16_t* coef = reinterpret_cast<int16_t*>(ent + (int64_t)n * (info.v[6] / 2));
    const int32_t count = c ? g.mcux * g.mcuy : g.base[1];
    int pred = 0;
    for (int32_t k0 = 0; k0 < count; k0 += 64) {
        const int32_t k = k0 + lane;
        int32_t sb = -1;
        int v = 0;
        if (k < count) {
            sb = vbs_huff_dc_block(g, c, k);
            if (sb < 0 || sb >= g.nblk) sb = -1;
            else v = coef[(int64_t)sb * 64];
        }
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(v, d, 64);
            if (lane >= d) v += up;
        }
        v += pred;
        if (sb >= 0) coef[(int64_t)sb * 64] = (int16_t)v;
        pred = __shfl(v, 63, 64);
    }
}

}  // namespace

extern "C" int vbs_mjpeg_huffman_device(const uint8_t* stage, const int64_t* scan_off, const int64_t* scan_bits, const int32_t* table_set,
                                        const void* sets, int n_sets, int n, const int32_t* info, int subseq_bits, uint32_t* ent,
                                        uint32_t* tab, int64_t* frame_base, int32_t* status, void* stream) {
    if (!stage || !scan_off || !scan_bits || !table_set || !sets || !info || !ent || !tab || !frame_base || !status || n < 0 ||
        n > 65535 || n_sets < 0 || ((uintptr_t)stage & (VBS_MJPEG_SCAN_ALIGN - 1)))
        return VBS_EINVAL;
    if (subseq_bits == 0) subseq_bits = VBS_MJPEG_SUBSEQ_BITS;
    if (subseq_bits < 128 || subseq_bits > 65536 || (subseq_bits & 31)) return VBS_EINVAL;
    if (info[5] != 0 || (info[2] != 1 && info[2] != 3) || info[3] < 1 || info[3] > 2 || info[4] < 1 || info[4] > 2 || info[0] < 1 ||
        info[1] < 1 || info[6] < 64)
        return VBS_EINVAL;
    {
        vbs_huff_geom g;                                  // info[6] must be the geometry's own block count: it sizes ent and tab
        vbs_huff_geom_init(g, info, nullptr);
        if ((int64_t)g.nblk * 64 != info[6]) return VBS_EINVAL;
    }
    if (n == 0) return VBS_OK;
    hipStream_t s = (hipStream_t)stream;
    Info in;
    for (int k = 0; k < 8; ++k) in.v[k] = info[k];
    if (hipMemsetAsync(ent, 0, (size_t)n * (size_t)(info[6] / 2) * 4, s) != hipSuccess) return VBS_EHIP;
    hipLaunchKernelGGL(k_jpeg_huff, dim3(n), dim3(HT), 0, s, stage, scan_off, scan_bits, table_set, (const vbs_huff_set*)sets, n_sets, in,
                       (uint32_t)subseq_bits, ent, tab, frame_base, status);
    hipLaunchKernelGGL(k_jpeg_dc, dim3(n), dim3(256), 0, s, ent, status, in);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}
