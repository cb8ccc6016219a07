// Baseline JPEG encoder on the device: the annotated tracking video (`_tracked.avi`, marker_detection.py:69-76,453) as
// Motion-JPEG.  The bytes equal Pillow's `Image.save(buf, "JPEG", quality=q)` (libjpeg-turbo defaults: 4:2:0, islow
// forward DCT, standard Annex K Huffman tables, no optimisation), restated from the published libjpeg algorithms:
//   jccolor.c   fixed-point RGB -> YCbCr (16 fraction bits)
//   jcprepct.c  bottom-edge replication (full-resolution rows of the last row group, then whole downsampled rows)
//   jcsample.c  right-edge replication and h2v2_downsample with its 1, 2, 1, 2 ... rounding bias
//   jfdctint.c  "islow" forward DCT (CONST_BITS 13, PASS1_BITS 2)
//   jcdctmgr.c  quantisation by reciprocal multiplication (compute_reciprocal, 16-bit DCTELEM)
//   jccoefct.c  dummy blocks at the right and bottom edges of the MCU grid (AC zero, DC copied)
//   jchuff.c    code emission, 0xFF00 stuffing, padding of the last byte with 1-bits
//   jcmarker.c  SOI, APP0 JFIF 1.01, DQT x2, SOF0, DHT x4 (Y DC, Y AC, C DC, C AC), SOS, EOI
// Pipeline (all on the device; only the finished files cross PCIe):
//   k_jenc_tables  (1 thread)             quality -> quantisation tables, reciprocals, Huffman codes, the header bytes
//   k_jenc_coef    (thread per block)     pixels -> quantised coefficients in zigzag order, int16 [n][blocks][64]
//   k_jenc_dummy   (thread per MCU)       DC of the dummy blocks of the last MCU row / column
//   k_jenc_bits    (thread per block)     code length of every block (its DC difference needs the previous block's DC)
//   k_jenc_scan    (workgroup per frame)  exclusive scan of the lengths -> bit offsets; zeroes the frame's word stream
//   k_jenc_pack    (thread per block)     the block's bits into the word stream (atomicOr on the words it shares)
//   k_jenc_count   (workgroup per frame)  file size = header + bytes + one stuffing byte per 0xFF + EOI
//   k_jenc_write   (workgroup per frame)  header, stuffed scan and EOI at the frame's offset in the packed payload
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vbs.h"

namespace {

constexpr int HDR = VBS_JPEG_HEADER_BYTES;
constexpr int BLOCK_BITS_MAX = VBS_JPEG_BLOCK_BITS_MAX;

__host__ __device__ constexpr int natural_order(int k) {
    constexpr int z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

// jcparam.c: the IJG example tables of ITU-T T.81 Annex K.1 (natural order)
constexpr uint8_t STD_QUANT[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99}};
// ITU-T T.81 Annex K.3: the "typical" Huffman tables libjpeg installs when it does not optimise (index 0 luma, 1 chroma)
constexpr uint8_t STD_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t STD_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t STD_AC_VALS[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// What k_jenc_tables derives from the quality, in the workspace (read by every other kernel)
struct Tables {
    uint32_t recip[2][64], corr[2][64], shift[2][64];   // jcdctmgr.c divisors of quantval << 3, natural order
    uint32_t dc[2][16];                                 // (size << 16) | code, by magnitude category
    uint32_t ac[2][256];                                // (size << 16) | code, by run << 4 | size symbol
    uint8_t header[HDR];
};

struct Geom {
    int W, H, mcux, mcuy, nblk, ybw, ybh, chh;         // chh = chroma rows that belong to the image, ceil(H / 2)
    int64_t sn, sr;                                     // input strides (bytes) of a frame and a row
    int64_t words;                                      // word-stream capacity of one frame
    int64_t frame_bound;                                // bytes of one file at most
};

// ---- tables (jcparam.c, jcdctmgr.c, jchuff.c, jcmarker.c) ----------------------------------------------------------
__host__ __device__ inline void put16(uint8_t* p, int v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }

__host__ __device__ inline int clz32(uint32_t x) { return x ? __builtin_clz(x) : 32; }

__host__ __device__ inline void make_huff(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {                     // canonical codes (jchuff.c jpeg_make_c_derived_tbl)
        for (int i = 0; i < bits[l - 1]; ++i, ++p) out[vals[p]] = ((uint32_t)l << 16) | (uint32_t)code++;
        code <<= 1;
    }
}

// quality (1..100) and frame size -> t (one thread: a few hundred table entries and the 623 header bytes)
__host__ __device__ inline void build_tables(Tables* t, int quality, int W, int H) {
    uint8_t qv[2][64];
    // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline = TRUE)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            int v = ((int)STD_QUANT[c][k] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            qv[c][k] = (uint8_t)v;
            // compute_reciprocal(quantval << 3) for a 16-bit DCTELEM; the divisor is >= 8, never the identity case
            const uint32_t d = (uint32_t)v << 3;
            int r = 16 + (31 - clz32(d));
            uint32_t fq = (1u << r) / d, cr = d / 2;
            const uint32_t fr = (1u << r) % d;
            if (fr == 0) { fq >>= 1; --r; }
            else if (fr <= d / 2) ++cr;
            else ++fq;
            t->recip[c][k] = fq;
            t->corr[c][k] = cr;
            t->shift[c][k] = (uint32_t)r;
        }
    uint8_t dcvals[12];
    for (int i = 0; i < 12; ++i) dcvals[i] = (uint8_t)i;
    for (int c = 0; c < 2; ++c) {
        for (int s = 0; s < 16; ++s) t->dc[c][s] = 0;
        for (int s = 0; s < 256; ++s) t->ac[c][s] = 0;
        make_huff(STD_DC_BITS[c], dcvals, t->dc[c]);
        make_huff(STD_AC_BITS[c], STD_AC_VALS[c], t->ac[c]);
    }
    uint8_t* h = t->header;
    int p = 0;
    h[p++] = 0xFF; h[p++] = 0xD8;                                              // SOI
    const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int k = 0; k < 18; ++k) h[p++] = app0[k];                             // JFIF 1.01, aspect 1:1, no thumbnail
    for (int c = 0; c < 2; ++c) {                                              // DQT, one segment per table, zigzag order
        h[p++] = 0xFF; h[p++] = 0xDB; put16(h + p, 67); p += 2;
        h[p++] = (uint8_t)c;
        for (int k = 0; k < 64; ++k) h[p++] = qv[c][natural_order(k)];
    }
    h[p++] = 0xFF; h[p++] = 0xC0; put16(h + p, 17); p += 2;                    // SOF0
    h[p++] = 8; put16(h + p, H); p += 2; put16(h + p, W); p += 2; h[p++] = 3;
    const uint8_t comps[9] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (int k = 0; k < 9; ++k) h[p++] = comps[k];
    for (int c = 0; c < 2; ++c) {                                              // DHT: DC then AC of luma, then of chroma
        int n = 0;
        for (int l = 0; l < 16; ++l) n += STD_DC_BITS[c][l];
        h[p++] = 0xFF; h[p++] = 0xC4; put16(h + p, 19 + n); p += 2; h[p++] = (uint8_t)c;
        for (int l = 0; l < 16; ++l) h[p++] = STD_DC_BITS[c][l];
        for (int k = 0; k < n; ++k) h[p++] = (uint8_t)k;
        n = 0;
        for (int l = 0; l < 16; ++l) n += STD_AC_BITS[c][l];
        h[p++] = 0xFF; h[p++] = 0xC4; put16(h + p, 19 + n); p += 2; h[p++] = (uint8_t)(0x10 | c);
        for (int l = 0; l < 16; ++l) h[p++] = STD_AC_BITS[c][l];
        for (int k = 0; k < n; ++k) h[p++] = STD_AC_VALS[c][k];
    }
    const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int k = 0; k < 14; ++k) h[p++] = sos[k];
}

__global__ void k_jenc_tables(Tables* t, int quality, int W, int H) { build_tables(t, quality, W, H); }

// ---- per block: pixels -> quantised coefficients --------------------------------------------------------------------
// jccolor.c rgb_ycc_convert: FIX(x) = round(x * 65536); the +ONE_HALF / +ONE_HALF-1 roundings live in its tables
__host__ __device__ inline int ycc(const uint8_t* px, int comp) {
    const int b = px[0], g = px[1], r = px[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

#define JDESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// jfdctint.c jpeg_fdct_islow on one row or column (stride s) of d, in place
template <int S, bool PASS2>
__host__ __device__ inline void fdct_1d(int* d) {
    constexpr int SH = PASS2 ? 15 : 11;                 // CONST_BITS +/- PASS1_BITS
    const int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S];
    const int tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
    const int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S];
    const int tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (PASS2) {
        d[0] = JDESCALE(tmp10 + tmp11, 2);
        d[4 * S] = JDESCALE(tmp10 - tmp11, 2);
    } else {
        d[0] = (tmp10 + tmp11) * 4;
        d[4 * S] = (tmp10 - tmp11) * 4;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2 * S] = JDESCALE(z1 + tmp13 * 6270, SH);
    d[6 * S] = JDESCALE(z1 - tmp12 * 15137, SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7 * S] = JDESCALE(t4 + z1 + z3, SH);
    d[5 * S] = JDESCALE(t5 + z2 + z4, SH);
    d[3 * S] = JDESCALE(t6 + z2 + z3, SH);
    d[S] = JDESCALE(t7 + z1 + z4, SH);
}

// block b (scan order: MCU-major, Y00 Y01 Y10 Y11 Cb Cr) of frame `f` -> zz[64]; dummy blocks get zeros here and their DC
// in k_jenc_dummy
__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }

__host__ __device__ inline void block_coefs(const uint8_t* __restrict__ fr, const Geom& g, const Tables* __restrict__ t, int b,
                                            int16_t* __restrict__ out) {
    const int mcu = b / 6, k = b % 6, mx = mcu % g.mcux, my = mcu / g.mcux;
    int d[64];
    int comp;
    if (k < 4) {
        const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
        if (by >= g.ybh || bx >= g.ybw) {                                      // jccoefct.c dummy block
#pragma unroll
            for (int i = 0; i < 64; i += 2) *(uint32_t*)(out + i) = 0;
            return;
        }
        comp = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int py = imin(8 * by + y, g.H - 1);                           // bottom / right edges replicated
#pragma unroll
            for (int x = 0; x < 8; ++x) d[8 * y + x] = ycc(fr + py * g.sr + 3 * imin(8 * bx + x, g.W - 1), 0) - 128;
        }
    } else {
        comp = k - 3;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            // rows past the image's chroma rows repeat its last one (jcprepct.c expand_bottom_edge on downsampled rows)
            const int cy = imin(8 * my + y, g.chh - 1);
            const uint8_t* r0 = fr + 2 * cy * g.sr;
            const uint8_t* r1 = fr + imin(2 * cy + 1, g.H - 1) * g.sr;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int cx = 8 * mx + x;
                const int c0 = 3 * imin(2 * cx, g.W - 1), c1 = 3 * imin(2 * cx + 1, g.W - 1);
                const int s = ycc(r0 + c0, comp) + ycc(r0 + c1, comp) + ycc(r1 + c0, comp) + ycc(r1 + c1, comp);
                d[8 * y + x] = ((s + 1 + (x & 1)) >> 2) - 128;                 // bias 1, 2, 1, 2 ... (8 mx is even)
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct_1d<1, false>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct_1d<8, true>(d + c);
    const int q = comp ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 64; i += 2) {
        int v[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nat = natural_order(i + j);
            const int x = d[nat];
            const uint32_t a = (uint32_t)(x < 0 ? -x : x);
            const int mag = (int)(((a + t->corr[q][nat]) * t->recip[q][nat]) >> t->shift[q][nat]);
            v[j] = x < 0 ? -mag : mag;
        }
        *(uint32_t*)(out + i) = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
    }
}

__global__ void __launch_bounds__(256) k_jenc_coef(const uint8_t* __restrict__ frames, Geom g, const Tables* __restrict__ t,
                                                   int16_t* __restrict__ coef) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= g.nblk) return;
    block_coefs(frames + (int64_t)blockIdx.y * g.sn, g, t, b, coef + ((int64_t)blockIdx.y * g.nblk + b) * 64);
}

// jccoefct.c: a dummy block copies the DC of the block before it in the MCU (right edge) or of the MCU's last block of the
// row above (bottom edge); the MCU's blocks are visited in order, so a chain resolves
__host__ __device__ inline void dummy_dc(const Geom& g, int16_t* __restrict__ coef_frame, int mcu) {
    const int mx = mcu % g.mcux, my = mcu / g.mcux;
    if (2 * mx + 2 <= g.ybw && 2 * my + 2 <= g.ybh) return;
    int16_t* base = coef_frame + (int64_t)6 * mcu * 64;
    for (int k = 0; k < 4; ++k) {
        const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
        if (by >= g.ybh) base[64 * k] = base[64 * 1];
        else if (bx >= g.ybw) base[64 * k] = base[64 * (k - 1)];
    }
}

__global__ void k_jenc_dummy(Geom g, int16_t* __restrict__ coef) {
    const int mcu = blockIdx.x * blockDim.x + threadIdx.x;
    if (mcu < g.mcux * g.mcuy) dummy_dc(g, coef + (int64_t)blockIdx.y * g.nblk * 64, mcu);
}

// ---- jchuff.c encode_one_block -----------------------------------------------------------------------------------------
__host__ __device__ inline int dc_pred_block(int b) {   // scan index of the same component's previous block, -1 = none
    const int mcu = b / 6, k = b % 6;
    if (k >= 1 && k <= 3) return b - 1;
    if (mcu == 0) return -1;
    return k == 0 ? b - 3 : b - 6;
}

template <class Sink>
__host__ __device__ inline void encode_block(const int16_t* __restrict__ zz, int pred, const uint32_t* __restrict__ dct,
                                             const uint32_t* __restrict__ act, Sink& s) {
    int temp = zz[0] - pred, temp2 = temp;
    if (temp < 0) { temp = -temp; --temp2; }
    int nbits = 32 - clz32((uint32_t)temp);
    s.put(dct[nbits] & 0xFFFF, dct[nbits] >> 16);
    if (nbits) s.put((uint32_t)temp2 & ((1u << nbits) - 1), nbits);
    int r = 0;
    for (int k = 1; k < 64; ++k) {
        temp = zz[k];
        if (temp == 0) { ++r; continue; }
        while (r > 15) { s.put(act[0xF0] & 0xFFFF, act[0xF0] >> 16); r -= 16; }
        temp2 = temp;
        if (temp < 0) { temp = -temp; --temp2; }
        nbits = 32 - clz32((uint32_t)temp);
        const uint32_t c = act[(r << 4) + nbits];
        s.put(c & 0xFFFF, c >> 16);
        s.put((uint32_t)temp2 & ((1u << nbits) - 1), nbits);
        r = 0;
    }
    if (r > 0) s.put(act[0] & 0xFFFF, act[0] >> 16);
}

struct CountSink {
    uint32_t n = 0;
    __host__ __device__ void put(uint32_t, uint32_t len) { n += len; }
};

// Bits of one block at bit offset `pos` of its frame's word stream (bit 0 = the most significant bit of word 0).  Words the
// block fills alone are stored; the first and the last, which it may share with its neighbours, are OR-ed.
struct PackSink {
    uint32_t* words;
    uint64_t acc;                                       // pending bits, left-aligned in the low `nacc` bits
    uint32_t nacc;
    int64_t w;                                          // word the pending bits start in
    bool first;
    __device__ PackSink(uint32_t* wd, uint32_t pos) : words(wd), acc(0), nacc(pos & 31), w(pos >> 5), first((pos & 31) != 0) {}
    __device__ void put(uint32_t code, uint32_t len) {
        acc = (acc << len) | code;
        nacc += len;
        if (nacc >= 32) {
            const uint32_t word = (uint32_t)(acc >> (nacc - 32));
            if (first) atomicOr(words + w, word);
            else words[w] = word;
            first = false;
            ++w;
            nacc -= 32;
            acc &= (nacc ? ((1ull << nacc) - 1) : 0ull);
        }
    }
    __device__ void flush() {
        if (nacc) atomicOr(words + w, (uint32_t)(acc << (32 - nacc)));
    }
};

__global__ void __launch_bounds__(256) k_jenc_bits(Geom g, const Tables* __restrict__ t, const int16_t* __restrict__ coef,
                                                   uint32_t* __restrict__ bits) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= g.nblk) return;
    const int64_t fb = (int64_t)blockIdx.y * g.nblk;
    const int p = dc_pred_block(b), c = b % 6 >= 4 ? 1 : 0;
    CountSink s;
    encode_block(coef + (fb + b) * 64, p < 0 ? 0 : coef[(fb + p) * 64], t->dc[c], t->ac[c], s);
    bits[fb + b] = s.n;
}

// one workgroup per frame: exclusive scan of the blocks' lengths; frame total in total[f]; zeroes the words the scan uses
__global__ void __launch_bounds__(1024) k_jenc_scan(Geom g, const uint32_t* __restrict__ bits, uint32_t* __restrict__ off,
                                                    uint32_t* __restrict__ total, uint32_t* __restrict__ words) {
    __shared__ uint32_t part[1024];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int per = (g.nblk + 1023) / 1024;
    const int a = min(tid * per, g.nblk), e = min(a + per, g.nblk);
    const uint32_t* bf = bits + (int64_t)f * g.nblk;
    uint32_t s = 0;
    for (int i = a; i < e; ++i) s += bf[i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                // Hillis-Steele inclusive scan
        const uint32_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - s;
    uint32_t* of = off + (int64_t)f * g.nblk;
    for (int i = a; i < e; ++i) { of[i] = run; run += bf[i]; }
    const uint32_t tot = part[1023];
    if (tid == 0) total[f] = tot;
    const int64_t nw = ((int64_t)tot + 31) / 32;
    uint32_t* wf = words + (int64_t)f * g.words;
    for (int64_t i = tid; i < nw; i += 1024) wf[i] = 0;
}

__global__ void __launch_bounds__(256) k_jenc_pack(Geom g, const Tables* __restrict__ t, const int16_t* __restrict__ coef,
                                                   const uint32_t* __restrict__ off, uint32_t* __restrict__ words) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= g.nblk) return;
    const int64_t fb = (int64_t)blockIdx.y * g.nblk;
    const int p = dc_pred_block(b), c = b % 6 >= 4 ? 1 : 0;
    PackSink s(words + (int64_t)blockIdx.y * g.words, off[fb + b]);
    encode_block(coef + (fb + b) * 64, p < 0 ? 0 : coef[(fb + p) * 64], t->dc[c], t->ac[c], s);
    s.flush();
}

// byte j of a frame's scan before stuffing; the last byte's unused low bits are 1 (jchuff.c flush_bits)
__host__ __device__ inline uint32_t scan_byte(const uint32_t* wf, int64_t j, uint32_t tot) {
    uint32_t v = (wf[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF;
    const uint32_t rem = tot & 7;
    if (rem && j == (int64_t)(tot >> 3)) v |= 0xFFu >> rem;
    return v;
}

// Per frame: bytes of the scan and how many of them are 0xFF, split over the workgroup's threads in equal runs
__device__ __forceinline__ uint32_t block_ff_scan(const uint32_t* wf, int64_t nbytes, uint32_t tot, int64_t* a, int64_t* e,
                                                  uint32_t* part, uint32_t* mine) {
    const int tid = threadIdx.x;
    const int64_t per = (nbytes + 1023) / 1024;
    *a = min((int64_t)tid * per, nbytes);
    *e = min(*a + per, nbytes);
    uint32_t s = 0;
    for (int64_t j = *a; j < *e; ++j) s += scan_byte(wf, j, tot) == 0xFF;
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    *mine = s;
    return part[1023];
}

__global__ void __launch_bounds__(1024) k_jenc_count(Geom g, const uint32_t* __restrict__ total, const uint32_t* __restrict__ words,
                                                     int32_t* __restrict__ sizes) {
    __shared__ uint32_t part[1024];
    const int f = blockIdx.x;
    const uint32_t tot = total[f];
    const int64_t nbytes = ((int64_t)tot + 7) / 8;
    int64_t a, e;
    uint32_t mine;
    const uint32_t ff = block_ff_scan(words + (int64_t)f * g.words, nbytes, tot, &a, &e, part, &mine);
    if (threadIdx.x == 0) sizes[f] = (int32_t)(HDR + nbytes + ff + 2);
}

__global__ void __launch_bounds__(1024) k_jenc_write(Geom g, const Tables* __restrict__ t, const uint32_t* __restrict__ total,
                                                     const uint32_t* __restrict__ words, const int32_t* __restrict__ sizes,
                                                     uint8_t* __restrict__ payload, int64_t payload_bytes,
                                                     int64_t* __restrict__ offsets) {
    __shared__ uint32_t part[1024];
    __shared__ int64_t base_s;
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int64_t o = 0;
        for (int i = 0; i < f; ++i) o += sizes[i];
        base_s = o;
        offsets[f] = o;
    }
    const uint32_t tot = total[f];
    const int64_t nbytes = ((int64_t)tot + 7) / 8;
    const uint32_t* wf = words + (int64_t)f * g.words;
    int64_t a, e;
    uint32_t mine;
    block_ff_scan(wf, nbytes, tot, &a, &e, part, &mine);           // (its barriers also publish base_s)
    const int64_t base = base_s;
    if (base + sizes[f] > payload_bytes) return;                   // (cannot happen with the documented bound)
    uint8_t* out = payload + base;
    for (int i = tid; i < HDR; i += 1024) out[i] = t->header[i];
    int64_t o = HDR + a + (part[tid] - mine);
    for (int64_t j = a; j < e; ++j) {
        const uint32_t v = scan_byte(wf, j, tot);
        out[o++] = (uint8_t)v;
        if (v == 0xFF) out[o++] = 0;
    }
    if (tid == 0) {
        const int64_t end = sizes[f];
        out[end - 2] = 0xFF;
        out[end - 1] = 0xD9;
    }
}

struct Layout {
    Geom g;
    int64_t tables, coef, bits, off, total, words, end;
};

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

int layout(int W, int H, int n, Layout* L) {
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || n < 0 || n > 65535) return VBS_EINVAL;
    Geom& g = L->g;
    g.W = W; g.H = H;
    g.mcux = (W + 15) / 16; g.mcuy = (H + 15) / 16;
    g.ybw = (W + 7) / 8; g.ybh = (H + 7) / 8; g.chh = (H + 1) / 2;
    const int64_t nblk = (int64_t)g.mcux * g.mcuy * 6;
    if (nblk * BLOCK_BITS_MAX >= ((int64_t)1 << 32)) return VBS_EINVAL;   // bit offsets are 32-bit
    g.nblk = (int)nblk;
    g.words = (nblk * BLOCK_BITS_MAX + 31) / 32 + 1;
    g.frame_bound = HDR + 2 * ((nblk * BLOCK_BITS_MAX + 7) / 8) + 2;
    const int64_t nn = n > 0 ? n : 1;
    int64_t p = 0;
    L->tables = p; p = align256(p + (int64_t)sizeof(Tables));
    L->coef = p;   p = align256(p + nn * nblk * 64 * 2);
    L->bits = p;   p = align256(p + nn * nblk * 4);
    L->off = p;    p = align256(p + nn * nblk * 4);
    L->total = p;  p = align256(p + nn * 4);
    L->words = p;  p = align256(p + nn * g.words * 4);
    L->end = p;
    return VBS_OK;
}

}  // namespace

extern "C" int vbs_jpeg_encode_workspace(int width, int height, int n, int64_t* workspace_bytes, int64_t* payload_bytes,
                                         int64_t* frame_bound) {
    Layout L;
    if (layout(width, height, n, &L) != VBS_OK) return VBS_EINVAL;
    if (workspace_bytes) *workspace_bytes = L.end;
    if (payload_bytes) *payload_bytes = (int64_t)n * L.g.frame_bound;
    if (frame_bound) *frame_bound = L.g.frame_bound;
    return VBS_OK;
}

extern "C" int vbs_jpeg_encode(const uint8_t* frames, int n, int width, int height, int64_t stride_n, int64_t stride_row,
                               int quality, void* workspace, int64_t workspace_bytes, uint8_t* payload, int64_t payload_bytes,
                               int64_t* offsets, int32_t* sizes, void* stream) {
    Layout L;
    if (layout(width, height, n, &L) != VBS_OK || quality < 1 || quality > 100) return VBS_EINVAL;
    if (n == 0) return VBS_OK;
    if (!frames || !workspace || !payload || !offsets || !sizes || workspace_bytes < L.end ||
        payload_bytes < (int64_t)n * L.g.frame_bound || stride_row < 3 * (int64_t)width ||
        (n > 1 && stride_n < stride_row * height))
        return VBS_EINVAL;
    Geom g = L.g;
    g.sn = stride_n; g.sr = stride_row;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    Tables* t = (Tables*)(ws + L.tables);
    int16_t* coef = (int16_t*)(ws + L.coef);
    uint32_t* bits = (uint32_t*)(ws + L.bits);
    uint32_t* off = (uint32_t*)(ws + L.off);
    uint32_t* total = (uint32_t*)(ws + L.total);
    uint32_t* words = (uint32_t*)(ws + L.words);
    const dim3 bgrid((unsigned)((g.nblk + 255) / 256), (unsigned)n);
    const int nmcu = g.mcux * g.mcuy;
    hipLaunchKernelGGL(k_jenc_tables, dim3(1), dim3(1), 0, s, t, quality, width, height);
    hipLaunchKernelGGL(k_jenc_coef, bgrid, dim3(256), 0, s, frames, g, t, coef);
    hipLaunchKernelGGL(k_jenc_dummy, dim3((unsigned)((nmcu + 255) / 256), (unsigned)n), dim3(256), 0, s, g, coef);
    hipLaunchKernelGGL(k_jenc_bits, bgrid, dim3(256), 0, s, g, t, coef, bits);
    hipLaunchKernelGGL(k_jenc_scan, dim3((unsigned)n), dim3(1024), 0, s, g, bits, off, total, words);
    hipLaunchKernelGGL(k_jenc_pack, bgrid, dim3(256), 0, s, g, t, coef, off, words);
    hipLaunchKernelGGL(k_jenc_count, dim3((unsigned)n), dim3(1024), 0, s, g, total, words, sizes);
    hipLaunchKernelGGL(k_jenc_write, dim3((unsigned)n), dim3(1024), 0, s, g, t, total, words, sizes, payload, payload_bytes,
                       offsets);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

#ifdef VBS_DEBUG_KNOBS
namespace {
// the word stream of k_jenc_pack (bit 0 = the most significant bit of word 0), one bit at a time into zeroed words
struct HostSink {
    uint32_t* words;
    uint64_t pos;
    void put(uint32_t code, uint32_t len) {
        for (uint32_t i = len; i-- > 0; ++pos)
            if ((code >> i) & 1) words[pos >> 5] |= 0x80000000u >> (pos & 31);
    }
};
}  // namespace

// ONE frame (HOST memory, BGR, rows stride_row bytes apart) through the __host__ __device__ functions the kernels above run -
// build_tables, block_coefs, dummy_dc, encode_block, scan_byte - with plain loops in place of threads: debug library only, not
// declared in vbs.h.  `file` has room for file_cap >= the frame bound of vbs_jpeg_encode_workspace; *file_bytes = its length.
// What this does NOT run, and what therefore rests on the GPU tests alone: PackSink (the words a block shares with its
// neighbours, atomicOr), the two workgroup scans (k_jenc_scan's bit offsets, block_ff_scan's stuffing offsets), the zeroing of
// the word stream, and k_jenc_count / k_jenc_write (sizes, offsets, the placement of the stuffed bytes in the payload).
extern "C" int vbs_dbg_jpeg_encode_emulate(const uint8_t* frame, int width, int height, int64_t stride_row, int quality,
                                           uint8_t* file, int64_t file_cap, int64_t* file_bytes) {
    Layout L;
    if (layout(width, height, 1, &L) != VBS_OK || quality < 1 || quality > 100) return VBS_EINVAL;
    if (!frame || !file || !file_bytes || stride_row < 3 * (int64_t)width || file_cap < L.g.frame_bound) return VBS_EINVAL;
    Geom g = L.g;
    g.sn = 0; g.sr = stride_row;
    Tables* t = new Tables;
    uint32_t* mem = new uint32_t[(size_t)g.nblk * 32 + (size_t)g.words]();   // coefficients (dword stores), then the words
    int16_t* coef = (int16_t*)mem;
    uint32_t* words = mem + (size_t)g.nblk * 32;
    build_tables(t, quality, width, height);
    for (int b = 0; b < g.nblk; ++b) block_coefs(frame, g, t, b, coef + (int64_t)b * 64);
    for (int mcu = 0; mcu < g.mcux * g.mcuy; ++mcu) dummy_dc(g, coef, mcu);
    HostSink s{words, 0};
    for (int b = 0; b < g.nblk; ++b) {
        const int p = dc_pred_block(b), c = b % 6 >= 4 ? 1 : 0;
        encode_block(coef + (int64_t)b * 64, p < 0 ? 0 : coef[(int64_t)p * 64], t->dc[c], t->ac[c], s);
    }
    const uint32_t tot = (uint32_t)s.pos;
    const int64_t nbytes = ((int64_t)tot + 7) / 8;
    int64_t o = 0;
    for (int i = 0; i < HDR; ++i) file[o++] = t->header[i];
    for (int64_t j = 0; j < nbytes; ++j) {
        const uint32_t v = scan_byte(words, j, tot);
        file[o++] = (uint8_t)v;
        if (v == 0xFF) file[o++] = 0;
    }
    file[o++] = 0xFF; file[o++] = 0xD9;
    *file_bytes = o;
    delete[] mem;
    delete t;
    return VBS_OK;
}
#endif
