// One wave's share of the band / opened planes of a frame: k_morph (k_morph.hip) runs it over a batch, the few-frames
// instances of the general labelling kernel (k_label.hip, MORPH != 0) over their own frame.
#pragma once
#include "ccl_common.h"

// horizontal window AND / OR of one row word over dx in [lo, hi] (lo <= 0 <= hi, hi - lo < 64) given its left / right
// neighbour words.  The 128 bits from position lo on are combined with themselves shifted by 1, 2, 4, ... (AND and OR
// are idempotent, so the last shift may overlap): log2(window) steps instead of one per offset.
template <bool ERODE>
__device__ __forceinline__ u64 hmorph(u64 wl, u64 wc, u64 wr, int lo, int hi) {
    const int pre = -lo, n = hi - lo + 1;               // bit p of (ulo, uhi) = pixel p - pre
    u64 ulo = pre ? ((wl >> (64 - pre)) | (wc << pre)) : wc;
    u64 uhi = pre ? ((wc >> (64 - pre)) | (wr << pre)) : wr;
    int have = 1;
    while (have < n) {
        const int s = min(have, n - have);
        const u64 slo = (ulo >> s) | (uhi << (64 - s)), shi = uhi >> s;      // (positions past the 128 bits are never used)
        ulo = ERODE ? (ulo & slo) : (ulo | slo);
        uhi = ERODE ? (uhi & shi) : (uhi | shi);
        have += s;
    }
    return ulo;                                          // bit i = AND / OR of pixels i + lo .. i + hi
}

// band = mask & ~erode_ns(mask) and open = dilate5(erode5(area)), separably, as a stream down the image:
// a wave holds G = 64 / WW strips of rows side by side (lane = strip * WW + word column) and takes one image row per
// step; the horizontal passes get their neighbour words by DPP lane shifts, the vertical passes are delay lines in
// registers (the ns-row AND by doubling: 2, 4, 8, ns rows).  No LDS, no barrier; a strip re-reads only the ns - 1 rows
// above / below it.  (The first version staged 32-row tiles in LDS behind four barriers: 0.31 us per 1280x1024 frame.)
// Outside the image erosion sees 1s (pixels ignored), dilation sees 0s - scipy 'reflect' / cv2's default border.
// one wave: the G strips `wv` G .. of frame n
template <int NS14>                                      // ns = 14 (large frames) or 8 (small)
__device__ __forceinline__ void morph_wave(const u64* __restrict__ mbits, const u64* __restrict__ abits,
                                           u64* __restrict__ band, u64* __restrict__ opn, int H, int W, int WW, int G, int strips,
                                           int rows_per_strip, int n, int wv) {
    const int lane = threadIdx.x & 63;
    const int sidx = wv * G + lane / WW, j = lane % WW;
    const bool act = lane < G * WW && sidx < strips;
    const int ra = min(sidx * rows_per_strip, H), rb = min(ra + rows_per_strip, H);
    const int64_t fo = (int64_t)n * H * WW;
    const u64* M = mbits + fo;
    const u64* A = abits + fo;
    const u64 vm = valid_mask(j, W);
    const bool hasl = j > 0, hasr = j + 1 < WW;
    constexpr int LO = -(NS14 / 2), HI = NS14 / 2 - 1;    // window rows / columns y + LO .. y + HI
    // every lane runs the same number of steps (DPP moves need all lanes): the longest strip of the wave
    // input rows ra + LO .. : the band row yb needs rows up to yb + HI, the opened row yo rows up to yo + 4
    const int nsteps = rows_per_strip + (NS14 - 1 > 4 - LO ? NS14 - 1 : 4 - LO);
    // delay lines (index 0 = newest)
    u64 h1 = ~0ull, a2[2] = {~0ull, ~0ull}, a4[4] = {~0ull, ~0ull, ~0ull, ~0ull}, a8[6] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    u64 e5[4] = {~0ull, ~0ull, ~0ull, ~0ull}, d5[4] = {0, 0, 0, 0};
    // rows are loaded three steps ahead of their use (nothing else hides the load latency: there is no other work between
    // two steps of a wave)
    auto ld = [&](const u64* src, int row, bool ok) { return (ok && row >= 0 && row < H) ? src[(int64_t)row * WW + j] : 0ull; };
    auto ldc = [&](int row) { return (act && row >= ra && row < rb) ? M[(int64_t)row * WW + j] : 0ull; };
    const int tb = ra + LO;
    u64 mq0 = ld(M, tb, act), mq1 = ld(M, tb + 1, act), mq2 = ld(M, tb + 2, act);
    u64 aq0 = ld(A, tb, act), aq1 = ld(A, tb + 1, act), aq2 = ld(A, tb + 2, act);
    u64 cq0 = ldc(tb - HI), cq1 = ldc(tb + 1 - HI), cq2 = ldc(tb + 2 - HI);
    for (int k = 0; k < nsteps; ++k) {
        const int t = tb + k;                            // input row of this step
        const bool tin = act && t >= 0 && t < H;
        const u64 mw = mq0, aw = aq0, mc = cq0;
        mq0 = mq1; mq1 = mq2; mq2 = ld(M, t + 3, act);
        aq0 = aq1; aq1 = aq2; aq2 = ld(A, t + 3, act);
        cq0 = cq1; cq1 = cq2; cq2 = ldc(t + 3 - HI);
        const int yb = t - HI;                           // band row completed by this step (window yb + LO .. yb + HI = t)
        const bool bout = act && yb >= ra && yb < rb;
        // ---- horizontal erosions (neighbour words by lane shift; rows outside the image are all ones) ----
        u64 hm, ha;
        {
            const u64 wc = tin ? (mw | ~vm) : ~0ull, wl_ = dpp_shr1(wc), wr_ = dpp_shl1(wc);
            hm = hmorph<true>(hasl ? wl_ : ~0ull, wc, hasr ? wr_ : ~0ull, LO, HI);
            const u64 ac = tin ? (aw | ~vm) : ~0ull, al_ = dpp_shr1(ac), ar_ = dpp_shl1(ac);
            ha = hmorph<true>(hasl ? al_ : ~0ull, ac, hasr ? ar_ : ~0ull, -2, 2);
        }
        // ---- vertical erosion over NS14 rows by doubling: a2[t-1], a4[t-3], a8[t-7], then rows t-NS14+1 .. t ----
        u64 e14;
        {
            const u64 n2 = h1 & hm;                      // rows t-1, t
            const u64 n4 = a2[1] & n2;                   // rows t-3 .. t      (a2[1] = rows t-3, t-2)
            if (NS14 == 14) {
                const u64 n8 = a4[3] & n4;               // rows t-7 .. t      (a4[3] = rows t-7 .. t-4)
                e14 = a8[5] & n8;                        // rows t-13 .. t     (a8[5] = rows t-13 .. t-6)
                a8[5] = a8[4]; a8[4] = a8[3]; a8[3] = a8[2]; a8[2] = a8[1]; a8[1] = a8[0]; a8[0] = n8;
            } else {
                e14 = a4[3] & n4;                        // ns = 8: rows t-7 .. t
            }
            a4[3] = a4[2]; a4[2] = a4[1]; a4[1] = a4[0]; a4[0] = n4;
            a2[1] = a2[0]; a2[0] = n2;
            h1 = hm;
        }
        if (bout) band[fo + (int64_t)yb * WW + j] = mc & ~e14 & vm;
        // ---- open: vertical erosion over 5 rows -> row t-2 (0 outside the image), horizontal dilation, vertical
        //      dilation over 5 rows -> row t-4 ----
        {
            const int ye = t - 2;
            u64 ve = ha & e5[0] & e5[1] & e5[2] & e5[3];
            e5[3] = e5[2]; e5[2] = e5[1]; e5[1] = e5[0]; e5[0] = ha;
            ve = (act && ye >= 0 && ye < H) ? (ve & vm) : 0ull;
            const u64 vl_ = dpp_shr1(ve), vr_ = dpp_shl1(ve);
            const u64 hd = hmorph<false>(hasl ? vl_ : 0ull, ve, hasr ? vr_ : 0ull, -2, 2);
            const u64 o = hd | d5[0] | d5[1] | d5[2] | d5[3];
            d5[3] = d5[2]; d5[2] = d5[1]; d5[1] = d5[0]; d5[0] = hd;
            const int yo = t - 4;
            if (act && yo >= ra && yo < rb) opn[fo + (int64_t)yo * WW + j] = o & vm;
        }
    }
}
