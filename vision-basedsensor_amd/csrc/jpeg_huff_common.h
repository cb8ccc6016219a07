// The decode step of the device-side Huffman decoder (k_jpeg_huff.hip) and of its host emulation (host_mjpeg.hip, debug library
// only): one function, compiled for both, so that what is fuzzed on a CPU is what runs on the GPU.
//
// The scan is the DE-STUFFED byte stream that vbs_mjpeg_scan_batch stages (no FF 00 pairs, cut at the first marker, zero guard
// bytes behind it), read as big-endian 32-bit words.  Decoder state at a bit position: (p, c, z) = bit address of the next code
// word, index of the current block within the MCU (it selects the component and with it the DC / AC tables), zig-zag index
// of the next coefficient (0: a DC code is expected).  A step reads at most 16 code bits + 15 value bits = 31 bits from p.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VBS_HD __host__ __device__ __forceinline__
#else
#define VBS_HD inline
#endif

// one Huffman table as Huff::build makes it: the 9-bit look-ahead ((length << 8) | symbol, 0 = longer than 9 bits) and the
// canonical rows for the longer codes
struct vbs_huff_table {
    int32_t maxcode[18];
    int32_t valptr[17];
    int32_t mincode[17];
    uint16_t look[512];
    uint8_t vals[256];
};
// the tables of one frame BY COMPONENT (a gray frame uses slot 0 only; the others are copies of it)
struct vbs_huff_set {
    vbs_huff_table dc[3], ac[3];
};

struct vbs_huff_geom {
    int32_t ncomp, hs, vs, mcux, mcuy;
    int32_t bpm;                  // blocks per MCU: hs * vs + 2, or 1 for gray
    int32_t nluma;                // hs * vs
    int32_t nblk;                 // blocks per frame
    int32_t base[3], bw[3];       // per component: first storage block, blocks per row of its padded grid
    const uint8_t* zigzag;        // 64 entries, in the memory of whoever runs the step
};

VBS_HD void vbs_huff_geom_init(vbs_huff_geom& g, const int32_t* info, const uint8_t* zigzag) {
    g.ncomp = info[2]; g.hs = info[3]; g.vs = info[4];
    g.mcux = (info[0] + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (info[1] + 8 * g.vs - 1) / (8 * g.vs);
    g.nluma = g.hs * g.vs;
    g.bpm = g.ncomp == 1 ? 1 : g.nluma + 2;
    g.bw[0] = g.mcux * g.hs; g.bw[1] = g.bw[2] = g.mcux;
    g.base[0] = 0;
    g.base[1] = g.mcux * g.hs * g.mcuy * g.vs;
    g.base[2] = g.base[1] + g.mcux * g.mcuy;
    g.nblk = g.ncomp == 1 ? g.base[1] : g.base[2] + g.mcux * g.mcuy;
    g.zigzag = zigzag;
}

#define VBS_HUFF_INVALID 0xFFFFFFFFu
struct vbs_huff_state {
    uint32_t p;                   // bit address in the frame's scan
    uint32_t cz;                  // c << 6 | z, or VBS_HUFF_INVALID
};
// INVALID compares unequal to everything, itself included
VBS_HD bool vbs_huff_same(const vbs_huff_state& a, const vbs_huff_state& b) {
    return a.cz != VBS_HUFF_INVALID && b.cz != VBS_HUFF_INVALID && a.p == b.p && a.cz == b.cz;
}

#define VBS_HUFF_STEP_OK      0
#define VBS_HUFF_STEP_INVALID 1   // no code of <= 16 bits, z beyond 63, DC category > 11
#define VBS_HUFF_STEP_SHORT   2   // the step needs bits beyond the scan's end

// 32 bits from bit address p (< scan_bits); the word index is clamped to the staged length + guard
VBS_HD uint32_t vbs_huff_peek(const uint32_t* words, uint32_t scan_bits, uint32_t p) {
    const uint32_t last = ((scan_bits + 31u) >> 5) + 1u;         // still inside the guard (VBS_MJPEG_SCAN_GUARD bytes)
    uint32_t w = p >> 5;
    w = w < last ? w : last - 1u;
    const uint64_t v = (uint64_t)__builtin_bswap32(words[w]) << 32 | __builtin_bswap32(words[w + 1u]);
    return (uint32_t)((v << (p & 31u)) >> 32);
}

// code word at the top of `bits` -> symbol (-1: none of <= 16 bits), its length in len
VBS_HD int vbs_huff_symbol(const vbs_huff_table& t, uint32_t bits, int& len) {
    const uint32_t e = t.look[bits >> 23];
    if (e) { len = (int)(e >> 8); return (int)(e & 255u); }
    int l = 10;
    int32_t code = (int32_t)(bits >> 22);
    while (l <= 16 && code > t.maxcode[l]) { ++l; code = (int32_t)(bits >> (32 - l)); }
    if (l > 16) return -1;
    len = l;
    return t.vals[(t.valptr[l] + code - t.mincode[l]) & 255];
}

VBS_HD int vbs_huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One symbol.  st -> the state behind it.  zz >= 0: a coefficient `val` at zig-zag index zz of the current block was decoded
// (val may be 0 for a DC difference of category 0; the DC value is the DIFFERENCE).  done: the block is complete.
// On a status other than OK the state is INVALID.
VBS_HD int vbs_huff_step(const vbs_huff_set& T, const uint32_t* words, uint32_t scan_bits, const vbs_huff_geom& g,
                         vbs_huff_state& st, int& zz, int& val, bool& done) {
    const uint32_t c = st.cz >> 6, z = st.cz & 63u;
    const uint32_t comp = c < (uint32_t)g.nluma ? 0u : c - (uint32_t)g.nluma + 1u;
    const uint32_t bits = vbs_huff_peek(words, scan_bits, st.p);
    zz = -1; val = 0; done = false;
    int len = 0, used, rc = VBS_HUFF_STEP_OK;
    uint32_t nz = z;
    const int sym = vbs_huff_symbol(z == 0 ? T.dc[comp] : T.ac[comp], bits, len);
    if (sym < 0) { rc = VBS_HUFF_STEP_INVALID; used = 16; }
    else if (z == 0) {
        if (sym > 11) { rc = VBS_HUFF_STEP_INVALID; used = len; }
        else {
            used = len + sym;
            zz = 0;
            val = sym ? vbs_huff_extend((int)((bits << len) >> (32 - sym)), sym) : 0;
            nz = 1;
        }
    } else {
        const int r = sym >> 4, sz = sym & 15;
        used = len + sz;
        if (!sz) {
            if (r == 15) { nz = z + 16; if (nz > 63u) rc = VBS_HUFF_STEP_INVALID; }
            else done = true;                                     // EOB
        } else {
            nz = z + (uint32_t)r;
            if (nz > 63u) rc = VBS_HUFF_STEP_INVALID;
            else {
                zz = (int)nz;
                val = vbs_huff_extend((int)((bits << len) >> (32 - sz)), sz);
                if (++nz == 64u) done = true;
            }
        }
    }
    if (st.p + (uint32_t)used > scan_bits) rc = VBS_HUFF_STEP_SHORT;   // (zero guard bits were read: whatever they gave is void)
    if (rc != VBS_HUFF_STEP_OK) { st.cz = VBS_HUFF_INVALID; zz = -1; done = false; return rc; }
    st.p += (uint32_t)used;
    if (done) { nz = 0; st.cz = (c + 1u == (uint32_t)g.bpm ? 0u : c + 1u) << 6; }
    else st.cz = c << 6 | nz;
    return VBS_HUFF_STEP_OK;
}

// scan-order block index b (MCU after MCU, within it component after component) with c = b % bpm -> the block's number in
// entropy()'s order: component after component, row-major over the component's padded block grid
VBS_HD int32_t vbs_huff_storage_block(const vbs_huff_geom& g, uint32_t b, uint32_t c) {
    const int32_t mcu = (int32_t)(b / (uint32_t)g.bpm);
    const int32_t my = mcu / g.mcux, mx = mcu - my * g.mcux;
    if (c < (uint32_t)g.nluma) {
        const int32_t v = (int32_t)c / g.hs, h = (int32_t)c - v * g.hs;
        return (my * g.vs + v) * g.bw[0] + mx * g.hs + h;
    }
    return (c == (uint32_t)g.nluma ? g.base[1] : g.base[2]) + my * g.mcux + mx;      // (no indexed access: g stays in registers)
}
// k-th block of component comp IN SCAN ORDER (the order of its DC predictions) -> storage block
VBS_HD int32_t vbs_huff_dc_block(const vbs_huff_geom& g, int comp, int32_t k) {
    const int32_t hv = comp ? 1 : g.nluma, hsc = comp ? 1 : g.hs, vsc = comp ? 1 : g.vs;
    const int32_t mcu = k / hv, r = k - mcu * hv, v = r / hsc, h = r - v * hsc;
    const int32_t my = mcu / g.mcux, mx = mcu - my * g.mcux;
    const int32_t base = comp == 0 ? 0 : (comp == 1 ? g.base[1] : g.base[2]), bw = comp ? g.mcux : g.bw[0];
    return base + (my * vsc + v) * bw + mx * hsc + h;
}

// Runs `st` until its p reaches `end` (<= scan_bits), counting the blocks it completes.  WRITE: `blk` is the scan-order index
// of the block in progress; every non-zero coefficient of a block below g.nblk is stored at coef[storage block][zigzag[zz]]
// and decoding stops for good at block g.nblk.  Every step consumes at least one bit: at most end - p steps.
template <bool WRITE>
VBS_HD int vbs_huff_run(const vbs_huff_set& T, const uint32_t* words, uint32_t scan_bits, const vbs_huff_geom& g,
                        vbs_huff_state& st, uint32_t end, uint32_t& blocks, uint32_t blk, int16_t* coef) {
    int32_t sb = 0;
    if (WRITE) {
        if (blk >= (uint32_t)g.nblk) return VBS_HUFF_STEP_OK;
        sb = vbs_huff_storage_block(g, blk, st.cz >> 6);
    }
    while (st.cz != VBS_HUFF_INVALID && st.p < end) {
        int zz, val;
        bool done;
        const int rc = vbs_huff_step(T, words, scan_bits, g, st, zz, val, done);
        if (rc != VBS_HUFF_STEP_OK) return rc;
        if (WRITE && zz >= 0 && val != 0 && sb >= 0 && sb < g.nblk) coef[(int64_t)sb * 64 + g.zigzag[zz & 63]] = (int16_t)val;
        if (done) {
            ++blocks;
            if (WRITE) {
                if (++blk >= (uint32_t)g.nblk) return VBS_HUFF_STEP_OK;
                sb = vbs_huff_storage_block(g, blk, st.cz >> 6);
            }
        }
    }
    return VBS_HUFF_STEP_OK;
}
