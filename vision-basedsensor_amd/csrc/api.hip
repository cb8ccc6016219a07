// C-ABI of include/vbs.h: workspace management, host-side constant tables, kernel sequencing.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "common.h"

// ---- host tables -----------------------------------------------------------------------------------
// OpenCV 4 bit-exact uint8 Gaussian kernel in 8 fractional bits (see oracle/stages.py:gaussian_kernel_q8)
static std::vector<int> gaussian_taps_q8(int ksize, double sigma) {
    std::vector<double> v(ksize);
    const double scale2x = -0.125 / (sigma * sigma);
    for (int i = 0; i < ksize; ++i) {
        double xi = (double)(1 - ksize + 2 * i);
        v[i] = std::exp(xi * xi * scale2x);
    }
    const int n2 = (ksize - 1) / 2;
    double s = 0;
    for (int i = 0; i < n2; ++i) s += v[i];
    s = 2.0 * s + 1.0;
    const double mul = 1.0 / s;
    std::vector<int> out(ksize, 0);
    double err = 0;
    int tot = 0;
    for (int i = 0; i < ksize / 2; ++i) {
        double adj = v[i] * mul * 256.0 + err;
        int v0 = (int)std::nearbyint(adj);             // round half to even (cvRound)
        err = adj - v0;
        out[i] = out[ksize - 1 - i] = v0;
        tot += v0;
    }
    out[ksize / 2] = 256 - 2 * tot;
    return out;
}

static void ncc_consts(int l, double sigma, NccConst* nc) {
    std::vector<double> ax(l), e(l);
    // np.linspace(-(l-1)/2, (l-1)/2, l): start + i*step, last point exact
    const double start = -(l - 1) / 2.0, stop = (l - 1) / 2.0, step = (stop - start) / (l - 1);
    for (int i = 0; i < l; ++i) ax[i] = (i == l - 1) ? stop : start + i * step;
    double se = 0;
    for (int i = 0; i < l; ++i) { e[i] = std::exp(-0.5 * ax[i] * ax[i] / (sigma * sigma)); se += e[i]; }
    for (int i = 0; i < VBS_NCC_MAXL; ++i) nc->g[i] = i < l ? e[i] / se : 0.0;
    nc->cg[0] = 0.0;
    for (int i = 0; i < VBS_NCC_MAXL; ++i) nc->cg[i + 1] = nc->cg[i] + nc->g[i];
    // template statistics as `_normxcorr2` forms them: t = K / sum(K), tbar = mean(t), T2 = sum((t - tbar)^2)
    std::vector<double> K((size_t)l * l);
    double sk = 0;
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
            K[(size_t)i * l + j] = std::exp(-0.5 * (ax[j] * ax[j] + ax[i] * ax[i]) / (sigma * sigma));
            sk += K[(size_t)i * l + j];
        }
    double st = 0;
    for (auto& x : K) { x /= sk; st += x; }
    nc->tbar = st / ((double)l * l);
    double t2 = 0;
    for (auto& x : K) t2 += (x - nc->tbar) * (x - nc->tbar);
    nc->T2 = t2;
    nc->l2 = (double)l * l;
    nc->inv_l2 = 1.0 / nc->l2;
    nc->thr2 = 0.1 * 0.1;
}

// ---- handle ------------------------------------------------------------------------------------------
template <typename T>
static int dev_alloc(vbs_handle* h, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T) + 256) != hipSuccess) {
        h->err = "hipMalloc failed (" + std::to_string(count * sizeof(T)) + " bytes)";
        return VBS_ENOMEM;
    }
    h->allocs.push_back(q);
    *p = (T*)q;
    return VBS_OK;
}

extern "C" int vbs_version(void) { return 100; }

extern "C" int vbs_contour_lut(uint8_t out[256]) {
    if (!out) return VBS_EINVAL;
    make_contour_lut(out);
    return VBS_OK;
}

extern "C" int vbs_step_lut(uint32_t out[256]) {
    if (!out) return VBS_EINVAL;
    make_step_lut(out);
    return VBS_OK;
}

extern "C" int vbs_gaussian_taps_q8(int ksize, double sigma, int32_t* out) {
    if (!out || ksize < 1 || !(ksize & 1) || !(sigma > 0)) return VBS_EINVAL;
    std::vector<int> k = gaussian_taps_q8(ksize, sigma);
    for (int i = 0; i < ksize; ++i) out[i] = k[i];
    return VBS_OK;
}

extern "C" int vbs_ncc_template(int l, double sigma, double* g, double* stats) {
    if (!g || !stats || l < 2 || l > VBS_NCC_MAXL || !(sigma > 0)) return VBS_EINVAL;
    NccConst nc;
    ncc_consts(l, sigma, &nc);
    for (int i = 0; i < l; ++i) g[i] = nc.g[i];
    stats[0] = nc.tbar; stats[1] = nc.T2; stats[2] = nc.l2; stats[3] = nc.thr2;
    return VBS_OK;
}

// The empty-window bound behind k_ncc_mfma's pre-scan.  A window without an area pixel has G = 0 and c = 0, so
// num = -mu (sum_t - n tbar) with sum_t the template mass and n the sample count of the window's in-image part: it is
// background whatever the frame's mean mu >= 0 as long as d0 = sum_t - n tbar >= 0, and the kernel's border tiles decide it
// so without the exact path for d0 > -1e-4.  -> the minimum of d0 over every cut a height x width frame can produce (row cuts
// x column cuts; rows / columns with the same cut share their sums, so the first and last l of each suffice), in float64
// with the sums formed as vbs_create forms ncc_ry / ncc_rx.  `tbar_shift` is added to the template mean (tests).
static double ncc_trim_guard(const NccConst& nc, int l, int height, int width, double tbar_shift) {
    const int lo = -((l - 1) - (l - 1) / 2);
    auto cuts = [&](int size) {
        std::vector<std::pair<int, double>> out;
        for (int p = 0; p < size; ++p) {
            if (p == l && size - l > l) p = size - l;   // (the positions between have the whole window, as position l - 1 has)
            double s = 0;
            int cnt = 0;
            for (int j = 0; j < l; ++j) { const int pp = p + lo + j; if (pp >= 0 && pp < size) { s += nc.g[j]; ++cnt; } }
            out.emplace_back(cnt, s);
        }
        return out;
    };
    const auto rows = cuts(height), cols = cuts(width);
    double mn = 1e300;
    for (const auto& r : rows)
        for (const auto& c : cols) mn = std::min(mn, r.second * c.second - (double)(r.first * c.first) * (nc.tbar + tbar_shift));
    return mn;
}
static constexpr double NCC_TRIM_SLACK = -5e-5;         // half of the -1e-4 the kernel's border decision allows

extern "C" int vbs_ncc_trim_guard(int l, double sigma, int height, int width, double tbar_shift, double* min_d0) {
    if (l < 2 || l > VBS_NCC_MAXL || !(sigma > 0) || height < 1 || width < 1) return VBS_EINVAL;
    NccConst nc;
    ncc_consts(l, sigma, &nc);
    const double mn = ncc_trim_guard(nc, l, height, width, tbar_shift);
    if (min_d0) *min_d0 = mn;
    return mn > NCC_TRIM_SLACK ? 1 : 0;
}

extern "C" int vbs_destroy(vbs_handle* h) {
    if (!h) return VBS_EINVAL;
    (void)hipSetDevice(h->device);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->series_ws) (void)hipFree(h->series_ws);
    delete h;
    return VBS_OK;
}

extern "C" const char* vbs_last_error(const vbs_handle* h) { return h ? h->err.c_str() : "null handle"; }

// The per-pass buffers of one workspace (its gray plane comes later: need_gray) and its NCC counters <- 0
static int alloc_workspace(vbs_handle* h, Workspace& w) {
    const size_t B = (size_t)h->maxb, M = (size_t)h->maxm, HW = (size_t)h->H * h->WW;
    int rc;
#define ALLOC(field, count) if ((rc = dev_alloc(h, &w.field, (count))) != VBS_OK) return rc
    ALLOC(area_bits, B * HW); ALLOC(mask_bits, B * HW); ALLOC(band_bits, B * HW);
    ALLOC(open_bits, B * HW);
    ALLOC(wbase, B * 2 * HW);
    if (2 * HW < (size_t)16 * SG_REC) ALLOC(stage_mrec, B * 16 * SG_REC);   // (k_stage.hip: stage_geom)
    ALLOC(node_pos, B * 2 * VBS_RUN_CAP); ALLOC(node_comp, B * 2 * VBS_RUN_CAP);
    ALLOC(ncomp, B * 2);
    ALLOC(band_first, B * M); ALLOC(band_sums, B * M * 4);
    ALLOC(area_first, B * M); ALLOC(area_sums, B * M * VBS_AREA_SUMS);
    ALLOC(ell, B * M * 8); ALLOC(det64, B * M * 6);
    ALLOC(cnt, B);
    ALLOC(probe, B * M * 4); ALLOC(ncc_tot, 4);
    // one allocation, one fill per pass: k_stage_lat's headers | slow counter | slow flags | frame statistics
    ALLOC(lat_hdr, (size_t)VBS_LAT_MAXN * VBS_LAT_HDR + 4 + B + B * 8 + 8);     // (+ one spare word: displacement's first-frame cell)
#undef ALLOC
    w.slow_total = w.lat_hdr + (size_t)VBS_LAT_MAXN * VBS_LAT_HDR;
    w.slow_flag = w.slow_total + 4;
    w.fstat = w.slow_flag + B;
    // the few-frames labelling kernel's scratch: optional (without it such passes take the batch kernel), at most 256 MB
    w.lat_slots = 0;
    if (const size_t per = stage_lat_scratch(h)) {
        const size_t slots = std::min<size_t>(std::min<size_t>(B, VBS_LAT_MAXN), ((size_t)256 << 20) / per);
        if (slots >= 1 && dev_alloc(h, &w.lat_scratch, per * slots) == VBS_OK) w.lat_slots = (int)slots;
        else { w.lat_scratch = nullptr; h->err.clear(); (void)hipGetLastError(); }
    }
    HIPCHK(h, hipMemset(w.ncc_tot, 0, 4 * sizeof(u64)));
    return VBS_OK;
}

extern "C" int vbs_create(int device, int height, int width, int max_markers, int max_batch,
                          vbs_handle** out) {
    if (!out) return VBS_EINVAL;
    *out = nullptr;
    if (height < 64 || width < 128 || width > 4096 || max_markers < 1 || max_markers > 1024 || max_batch < 1)
        return VBS_EINVAL;                                  // k_label keeps one row (<= 64 words) per wave
    vbs_handle* h = new (std::nothrow) vbs_handle();
    if (!h) return VBS_ENOMEM;
    *out = h;                                           // returned even on failure so the text can be read
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) { h->err = "hipSetDevice failed"; return VBS_EHIP; }
    h->H = height; h->W = width; h->maxm = max_markers; h->maxb = max_batch;
    h->P = (width + 63) / 64 * 64;
    h->WW = h->P / 64;
    BranchParams& bp = h->bp;
    bp.small = height <= 480;                           // marker_detection.py:117
    double sa, sb, ts;
    if (bp.small) { bp.taps_a = 21; sa = 4.56; bp.taps_b = 35; sb = 11.4; bp.ncc_l = 33; ts = 7.4; bp.thresh = 35; bp.hi = 180; bp.ns = 8; }
    else { bp.taps_a = 39; sa = 8.0; bp.taps_b = 101; sb = 20.0; bp.ncc_l = 80; ts = 13.0; bp.thresh = 20; bp.hi = 200; bp.ns = 14; }
    bp.ncc_lo = -((bp.ncc_l - 1) - (bp.ncc_l - 1) / 2);
    bp.ncc_hi = (bp.ncc_l - 1) / 2;
    if (height <= bp.taps_b / 2 + 4 || width <= bp.taps_b / 2 + 4) { h->err = "frame smaller than the blur radius"; return VBS_EINVAL; }
    ncc_consts(bp.ncc_l, ts, &h->ncc);
    std::vector<u32> frags, frags16h, frags16v;
    {   // the int8 matrix-core blur needs taps < 128 that sum to 256 (true for every sigma >= 1)
        std::vector<int> ka = gaussian_taps_q8(bp.taps_a, sa), kb = gaussian_taps_q8(bp.taps_b, sb);
        int suma = 0, sumb = 0, mx = 0;
        for (int v : ka) { suma += v; mx = std::max(mx, v); }
        for (int v : kb) { sumb += v; mx = std::max(mx, v); }
        if (suma != 256 || sumb != 256 || mx > 127) { h->err = "internal: blur taps do not fit int8"; return VBS_EINVAL; }
        frags = bp.small ? blur_mfma_fragments(ka, kb, 3, 0, 3) : blur_mfma_fragments(ka, kb, 5, 1, 3);
        if (width >= (bp.small ? 176 : 240) && (width & 3) == 0) blur16_fragments(ka, kb, width, bp.small != 0, &frags16h, &frags16v);
    }

    int rc;
#define ALLOC(field, count) if ((rc = dev_alloc(h, &h->field, (count))) != VBS_OK) return rc
    ALLOC(ncc_rx, (size_t)width); ALLOC(ncc_ry, (size_t)height);
    ALLOC(lut, 256);
    ALLOC(step_lut, 256);
    ALLOC(blur_frags, frags.size() / 4);
    if (!frags16h.empty()) { ALLOC(blur16_h, frags16h.size() / 4); ALLOC(blur16_v, frags16v.size() / 4); }
    std::vector<u32> nfrags = ncc_mfma_fragments(h->ncc, bp.ncc_l);
    ALLOC(ncc_frags, nfrags.size() / 4);
    ALLOC(ncc_tab, (size_t)2 * VBS_NCC_MAXL + 1);
    ALLOC(ncc_rowf, (size_t)height);
    ALLOC(umap1, (size_t)height * width * 2); ALLOC(umap2, (size_t)height * width); ALLOC(uwtab, 4096);
#undef ALLOC
    std::vector<double> rx(width), ry(height);
    for (int x = 0; x < width; ++x) {
        double s = 0;
        for (int j = 0; j < bp.ncc_l; ++j) { int xx = x + bp.ncc_lo + j; if (xx >= 0 && xx < width) s += h->ncc.g[j]; }
        rx[x] = s;
    }
    for (int y = 0; y < height; ++y) {
        double s = 0;
        for (int j = 0; j < bp.ncc_l; ++j) { int yy = y + bp.ncc_lo + j; if (yy >= 0 && yy < height) s += h->ncc.g[j]; }
        ry[y] = s;
    }
    u8 lut[256];
    make_contour_lut(lut);
    HIPCHK(h, hipMemcpy(h->ncc_rx, rx.data(), width * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->ncc_ry, ry.data(), height * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->lut, lut, 256, hipMemcpyHostToDevice));
    u32 steps[256];
    make_step_lut(steps);
    HIPCHK(h, hipMemcpy(h->step_lut, steps, sizeof(steps), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->blur_frags, frags.data(), frags.size() * sizeof(u32), hipMemcpyHostToDevice));
    if (h->blur16_h) {
        HIPCHK(h, hipMemcpy(h->blur16_h, frags16h.data(), frags16h.size() * sizeof(u32), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->blur16_v, frags16v.data(), frags16v.size() * sizeof(u32), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(h->ncc_frags, nfrags.data(), nfrags.size() * sizeof(u32), hipMemcpyHostToDevice));
    {
        std::vector<float2> rowf(height);
        for (int y = 0; y < height; ++y) {
            const int ny = std::min(y + bp.ncc_hi, height - 1) - std::max(y + bp.ncc_lo, 0) + 1;
            rowf[y] = make_float2((float)ny, (float)ry[y]);
        }
        HIPCHK(h, hipMemcpy(h->ncc_rowf, rowf.data(), height * sizeof(float2), hipMemcpyHostToDevice));
    }
    // k_ncc_mfma may skip the strips and rows whose windows are empty only where such a window is background for certain
    h->ncc_trim_ok = ncc_trim_guard(h->ncc, bp.ncc_l, height, width, 0.0) > NCC_TRIM_SLACK;
    HIPCHK(h, hipMemcpy(h->ncc_tab, h->ncc.g, VBS_NCC_MAXL * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->ncc_tab + VBS_NCC_MAXL, h->ncc.cg, (VBS_NCC_MAXL + 1) * sizeof(double), hipMemcpyHostToDevice));
    {
        std::vector<int32_t> wt(4096);
        bilinear_weights_i16(wt.data());
        HIPCHK(h, hipMemcpy(h->uwtab, wt.data(), 4096 * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if ((rc = alloc_workspace(h, h->ws[0])) != VBS_OK) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    return VBS_OK;
}

static int check_launch(vbs_handle* h) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("kernel launch: ") + hipGetErrorString(e); return VBS_EHIP; }
    return VBS_OK;
}

static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// The gray plane of 3-channel / undistorted input ([maxb][H][P]) of workspace w: gray frames never touch it, so it is
// allocated at the first call that needs it, or by vbs_set_undistort.  Never under stream capture: there the call fails
// and says why.
static int need_gray(vbs_handle* h, Workspace& w, hipStream_t s) {
    const size_t bytes = (size_t)h->maxb * h->H * h->P;
    if (!w.gray) {
        if (capturing(s)) {
            h->err = "the gray plane of 3-channel / undistorted input is allocated at first use: run one such call (or "
                     "vbs_set_undistort) outside stream capture first";
            return VBS_EINVAL;
        }
        int rc = dev_alloc(h, &w.gray, bytes);
        if (rc != VBS_OK) return rc;
    }
    // the second workspace converts its own passes: its plane exists whenever the first one's does, so that a multi-pass
    // call on 3-channel frames captured into a graph finds it in place after ANY uncaptured 3-channel call
    if (h->nws == 2 && !h->ws[1].gray && !capturing(s)) {
        int rc = dev_alloc(h, &h->ws[1].gray, bytes);
        if (rc != VBS_OK) { h->err = "second pass workspace: " + h->err; return rc; }
    }
    return VBS_OK;
}

// THE clear of a pass, one launch: the slow counter, the frames' flags and their statistics <- 0 (one behind the other in one
// allocation), for the few-frames route k_stage_lat's headers in front of them as well.  Passes that do not label clear alike.
static void clear_pass(vbs_handle* h, Workspace& w, int nb, const LabelPlan& plan, hipStream_t s) {
    h->last_ws = &w;                                     // every pass records its workspace: vbs_frame_stats / vbs_stage_tables
    const size_t n = (size_t)4 + (size_t)h->maxb + (size_t)nb * 8;
    if (plan.route == LABEL_LAT) launch_fill(w.lat_hdr, 0u, (size_t)VBS_LAT_MAXN * VBS_LAT_HDR + n, s);
    else launch_fill(w.slow_total, 0u, n, s);
}

// One internal pass of the detection stage: the blur reads gray frames directly, others are converted or remapped first.
// (`plan`: the pass's label_plan - its clear happens here, so a caller that labels hands the same plan to launch_labelling)
static int detect_pass(vbs_handle* h, Workspace& w, const u8* frames, int nb, const LabelPlan& plan, int channels, int64_t stride_n,
                       int64_t stride_row, u8* mask_u8, u8* area_u8, double* ncc_out, hipStream_t s) {
    if (h->undist || channels != 1) { int rc = need_gray(h, w, s); if (rc != VBS_OK) return rc; }
    clear_pass(h, w, nb, plan, s);
    if (h->undist) {                                    // marker_detection.py:88-89: undistort, then cvtColor
        launch_remap(h, frames, nb, channels, stride_n, stride_row, w.gray, 1, s);
        launch_blur(h, w, w.gray, (int64_t)h->H * h->P, h->P, nb, area_u8, s);
    } else if (channels == 1) {
        launch_blur(h, w, frames, stride_n, stride_row, nb, area_u8, s);
    } else {
        launch_gray(h, frames, nb, channels, stride_n, stride_row, w.gray, s);
        launch_blur(h, w, w.gray, (int64_t)h->H * h->P, h->P, nb, area_u8, s);
    }
    launch_ncc(h, w, nb, mask_u8, ncc_out, s);
    return check_launch(h);
}

// vbs_find_markers / vbs_ncc_map: detect_pass over passes of maxb frames, each writing its slice of the outputs given
static int detect_loop(vbs_handle* h, const u8* frames, int n, int channels, int64_t stride_n, int64_t stride_row,
                       u8* mask, u8* area_mask, double* ncc, hipStream_t s) {
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    for (int off = 0; off < n; off += h->maxb) {
        const int nb = std::min(h->maxb, n - off);
        int rc = detect_pass(h, h->ws[0], frames + (int64_t)off * stride_n, nb, label_plan(h, h->ws[0], nb), channels, stride_n,
                             stride_row, mask ? mask + off * hw : nullptr, area_mask ? area_mask + off * hw : nullptr,
                             ncc ? ncc + off * hw : nullptr, s);
        if (rc != VBS_OK) return rc;
    }
    return VBS_OK;
}

extern "C" int vbs_find_markers(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                                int64_t stride_row, uint8_t* mask, uint8_t* area_mask, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || n < 0 || (channels != 1 && channels != 3) || stride_row < (int64_t)h->W * channels) {
        h->err = "vbs_find_markers: bad argument";
        return VBS_EINVAL;
    }
    return detect_loop(h, frames, n, channels, stride_n, stride_row, mask, area_mask, nullptr, (hipStream_t)stream);
}

extern "C" int vbs_bgr2gray(vbs_handle* h, const uint8_t* frames, int n, int64_t stride_n, int64_t stride_row,
                            uint8_t* gray, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || !gray || n < 0 || stride_row < (int64_t)h->W * 3) { h->err = "vbs_bgr2gray: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    if (n) launch_gray_dense(h, frames, n, stride_n, stride_row, gray, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_ncc_map(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                           int64_t stride_row, double* ncc, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || !ncc || n < 0 || (channels != 1 && channels != 3) || stride_row < (int64_t)h->W * channels) {
        h->err = "vbs_ncc_map: bad argument";
        return VBS_EINVAL;
    }
    return detect_loop(h, frames, n, channels, stride_n, stride_row, nullptr, nullptr, ncc, (hipStream_t)stream);
}

extern "C" int vbs_normxcorr2(vbs_handle* h, const uint8_t* area_mask, int n, double* ncc, uint8_t* mask,
                              void* stream) {
    if (!h) return VBS_EINVAL;
    if (!area_mask || n < 0 || (!ncc && !mask)) { h->err = "vbs_normxcorr2: bad argument"; return VBS_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    Workspace& w = h->ws[0];
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    for (int off = 0; off < n; off += h->maxb) {
        int nb = std::min(h->maxb, n - off);
        clear_pass(h, w, nb, label_plan(h, w, nb), s);
        launch_threshold(h, w, area_mask + off * hw, area_mask + off * hw, nb, s);
        launch_popcount(h, w, nb, s);
        launch_ncc(h, w, nb, mask ? mask + off * hw : nullptr, ncc ? ncc + off * hw : nullptr, s);
        int rc = check_launch(h);
        if (rc != VBS_OK) return rc;
    }
    return VBS_OK;
}

static int add_second_workspace(vbs_handle* h);

extern "C" int vbs_set_option(vbs_handle* h, int option, int value) {
    if (!h) return VBS_EINVAL;
    switch (option) {
        case VBS_OPT_PASS_STREAMS:
            if (value != 1 && value != 2) break;
            h->pass_streams = value;
            // an explicit 2 builds the second workspace NOW (a set-up call: allocations, copies, a device synchronisation),
            // so that no later vbs_track_to_3d has to - and a call captured into a graph finds it in place
            if (value == 2) { int rc = add_second_workspace(h); if (rc != VBS_OK) return rc; }
            return VBS_OK;
        case VBS_OPT_FORCE_SEQ_MATCH: h->force_seq_match = value != 0; return VBS_OK;
        case VBS_OPT_NCC_MARGIN:
            if (value < 0 || value > 100000) break;
            h->ncc_margin_ppm = value;
            return VBS_OK;
        case VBS_OPT_STAGE_IMPL:
            if (value < 0 || value > 4) break;
            h->stage_impl = value;
            return VBS_OK;
        case VBS_OPT_LATENCY_FRAMES:
            if (value < 0 || value > VBS_LAT_MAXN) break;
            h->lat_frames = value;
            return VBS_OK;
        case VBS_OPT_BLUR_IMPL:
            if (value != 0 && value != 1) break;
            h->blur_impl = value;
            return VBS_OK;
        case VBS_OPT_GRAY_COEFFS:
            if (value != 14 && value != 15) break;
            h->gray_bits = value;
            return VBS_OK;
        default: break;
    }
    h->err = "vbs_set_option: unknown option or bad value";
    return VBS_EINVAL;
}

extern "C" int vbs_normxcorr2_general(int device, const double* tmpl, int th, int tw, const double* image, int h, int w,
                                      int mode, double* out, void* stream) {
    if (!tmpl || !image || !out || th < 1 || tw < 1 || h < 1 || w < 1 || mode < 0 || mode > 2) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    double* stats = nullptr;
    if (hipMallocAsync((void**)&stats, 4 * sizeof(double), (hipStream_t)stream) != hipSuccess) return VBS_ENOMEM;
    const int rc = launch_ncc_general(tmpl, th, tw, image, h, w, mode, out, stats, (hipStream_t)stream);
    (void)hipFreeAsync(stats, (hipStream_t)stream);
    if (rc != VBS_OK) return rc;
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_profile(vbs_handle* h, int enable) {
    if (!h) return VBS_EINVAL;
    for (auto& r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    h->recs.clear();
    h->prof = enable != 0;
    return VBS_OK;
}

extern "C" int vbs_profile_read(vbs_handle* h, char* buf, int cap) {
    if (!h || !buf || cap < 2) return VBS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    std::vector<std::string> names;
    std::vector<double> tot;
    std::vector<long> cnt;
    for (auto& r : h->recs) {
        float ms = 0;
        HIPCHK(h, hipEventElapsedTime(&ms, r.a, r.b));
        size_t i = 0;
        for (; i < names.size(); ++i) if (names[i] == r.name) break;
        if (i == names.size()) { names.push_back(r.name); tot.push_back(0); cnt.push_back(0); }
        tot[i] += ms; cnt[i] += 1;
    }
    std::string out;
    for (size_t i = 0; i < names.size(); ++i)
        out += names[i] + " " + std::to_string(cnt[i]) + " " + std::to_string(tot[i]) + "\n";
    if ((int)out.size() + 1 > cap) { h->err = "vbs_profile_read: buffer too small"; return VBS_EINVAL; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return VBS_OK;
}

extern "C" int vbs_set_undistort(vbs_handle* h, const double* K9, const double* dist, int ndist, double* newK9,
                                 void* stream) {
    if (!h) return VBS_EINVAL;
    if (!K9) { h->undist = false; return VBS_OK; }      // NULL camera matrix switches undistortion off
    if (ndist < 0 || ndist > 5 || (ndist && !dist) || !(K9[0] > 0) || !(K9[4] > 0)) {
        h->err = "vbs_set_undistort: bad argument";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = need_gray(h, h->ws[0], (hipStream_t)stream);     // (a set-up call: the plane the undistorted frames go to)
    if (rc != VBS_OK) return rc;
    rc = setup_undistort(h, K9, dist, ndist, (hipStream_t)stream);
    if (rc != VBS_OK) return rc;
    h->undist = true;
    if (newK9) for (int i = 0; i < 9; ++i) newK9[i] = h->newK[i];
    return check_launch(h);
}

extern "C" int vbs_undistort_frames(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                                    int64_t stride_row, uint8_t* out, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || !out || n < 0 || (channels != 1 && channels != 3) || stride_row < (int64_t)h->W * channels) {
        h->err = "vbs_undistort_frames: bad argument";
        return VBS_EINVAL;
    }
    if (!h->undist) { h->err = "vbs_undistort_frames: call vbs_set_undistort first"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    if (n) launch_remap(h, frames, n, channels, stride_n, stride_row, out, 0, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_frame_stats(vbs_handle* h, uint32_t* out, int n) {
    if (!h || !out || n < 0 || n > h->maxb) return VBS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());                   // (the last pass may have run on the handle's own stream)
    HIPCHK(h, hipMemcpy(out, h->last_ws->fstat, (size_t)n * 8 * sizeof(u32), hipMemcpyDeviceToHost));
    return VBS_OK;
}

extern "C" int vbs_stage_tables(vbs_handle* h, int n, uint32_t* ncomp, uint64_t* band_sums, uint32_t* area_first,
                                int64_t* area_sums, uint16_t* probe, uint32_t* slow) {
    if (!h || n < 0 || n > h->maxb) return VBS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const size_t N = (size_t)n, M = (size_t)h->maxm;
    const Workspace& w = *h->last_ws;
    if (ncomp) HIPCHK(h, hipMemcpy(ncomp, w.ncomp, N * 2 * sizeof(u32), hipMemcpyDeviceToHost));
    if (band_sums) HIPCHK(h, hipMemcpy(band_sums, w.band_sums, N * M * 4 * sizeof(u64), hipMemcpyDeviceToHost));
    if (area_first) HIPCHK(h, hipMemcpy(area_first, w.area_first, N * M * sizeof(u32), hipMemcpyDeviceToHost));
    if (area_sums) HIPCHK(h, hipMemcpy(area_sums, w.area_sums, N * M * VBS_AREA_SUMS * sizeof(i64), hipMemcpyDeviceToHost));
    if (probe) HIPCHK(h, hipMemcpy(probe, w.probe, N * M * 4 * sizeof(unsigned short), hipMemcpyDeviceToHost));
    if (slow) HIPCHK(h, hipMemcpy(slow, w.slow_flag, N * sizeof(u32), hipMemcpyDeviceToHost));
    return VBS_OK;
}

extern "C" int vbs_ellipse_table(vbs_handle* h, int n, double* out) {
    if (!h || !out || n < 0 || n > h->maxb) return VBS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->last_ws->ell, (size_t)n * h->maxm * 8 * sizeof(double), hipMemcpyDeviceToHost));
    return VBS_OK;
}

extern "C" int vbs_ncc_counters(vbs_handle* h, uint64_t out[3], int reset) {
    if (!h || !out) return VBS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i) out[i] = 0;
    for (int k = 0; k < h->nws; ++k) {                  // each workspace counts the passes it ran
        uint64_t t[3] = {0, 0, 0};
        HIPCHK(h, hipMemcpy(t, h->ws[k].ncc_tot, 3 * sizeof(u64), hipMemcpyDeviceToHost));
        if (reset) HIPCHK(h, hipMemset(h->ws[k].ncc_tot, 0, 4 * sizeof(u64)));
        for (int i = 0; i < 3; ++i) out[i] += t[i];
    }
    return VBS_OK;
}

extern "C" int vbs_undistort_points(int device, const double* pts, int n, const vbs_camera* cam, double* out,
                                    void* stream) {
    if (!pts || !out || !cam || n < 0) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n) launch_points(0, pts, n, *cam, out, nullptr, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_calculate_3d(int device, const double* uvd, int n, const vbs_camera* cam, double* xyz,
                                int32_t* ok, void* stream) {
    if (!uvd || !xyz || !ok || !cam || n < 0) return VBS_EINVAL;
    if (!(cam->K[0] > 0) || !(cam->K[4] > 0)) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n) launch_points(1, uvd, n, *cam, xyz, ok, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_pnp_ransac(int device, const double* world, int n_points, const double* image, const float* table,
                              const uint8_t* valid, int n_problems, const vbs_camera* cam, const int32_t* samples, int n_hyp,
                              double reproj_px, int32_t* hyp_count, double* hyp_pose, int32_t* status, double* pose,
                              int32_t* inlier_count, uint8_t* inlier_mask, double* errors, int32_t* winner, void* stream) {
    if (!world || (!image) == (!table) || !cam || !samples || !hyp_count || !hyp_pose || !status || !pose || !inlier_count ||
        !inlier_mask || !errors || !winner)
        return VBS_EINVAL;
    if (n_points < 1 || n_points > VBS_PNP_MAX_POINTS || n_hyp < 1 || n_hyp > VBS_PNP_MAX_HYPOTHESES || n_problems < 0 || !(reproj_px >= 0.0) || !std::isfinite(reproj_px) || !(cam->K[0] > 0) || !(cam->K[4] > 0))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n_problems)
        launch_pnp(world, n_points, image, table, valid, n_problems, *cam, samples, n_hyp, reproj_px, hyp_count, hyp_pose, status,
                   pose, inlier_count, inlier_mask, errors, winner, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int64_t vbs_retrack_workspace(int n, int m_ref, int max_det) {
    if (n < 0 || m_ref < 1 || max_det < 1) return VBS_EINVAL;
    if (m_ref > VBS_RETRACK_MAX || max_det > VBS_RETRACK_MAX) return VBS_ECAPACITY;
    return (int64_t)retrack_workspace_bytes(n, m_ref, max_det);
}

extern "C" int vbs_retrack(int device, const double* det, const int32_t* counts, int n, int max_det, const double* ref_xy, int m_ref,
                           const double* state_in, double gate, double max_travel, double vel_gain, int max_coast, int32_t* assign,
                           float* table, double* dist2, int32_t* info, double* state_out, void* workspace, void* stream) {
    if (!det || !counts || !ref_xy || !workspace || ((uintptr_t)workspace & 7) || (!assign && !table && !state_out) || n < 0 ||
        m_ref < 1 || max_det < 1 || !(gate >= 0.0) || !(vel_gain >= 0.0 && vel_gain <= 1.0) || max_coast < 0)
        return VBS_EINVAL;
    if (m_ref > VBS_RETRACK_MAX || max_det > VBS_RETRACK_MAX) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_retrack(det, counts, n, max_det, ref_xy, m_ref, state_in, gate, max_travel, vel_gain, max_coast, assign, table, dist2, info,
                   state_out, workspace, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_calibrate_camera(int device, const double* obj, int n_points, const double* img, int n_views,
                                    const uint8_t* view_mask, int n_problems, int w, int h, int max_iter, double* homography,
                                    int32_t* view_void, int32_t* status, double* K4, double* dist, double* R, double* T, double* rms,
                                    double* view_rms, double* std_intrinsics, int32_t* iterations, void* stream) {
    if (!obj || !img || !homography || !view_void || !status || !K4 || !dist || !R || !T || !rms || !view_rms || !std_intrinsics ||
        !iterations || n_points < 4 || n_views < 1 || n_problems < 1 || w < 1 || h < 1 || max_iter < 1)
        return VBS_EINVAL;
    if (n_views > VBS_CALIB_MAX_VIEWS || n_points > VBS_CHESS_MAX_PATTERN) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_calib(obj, n_points, img, n_views, view_mask, n_problems, w, h, max_iter, homography, view_void, status, K4, dist, R, T,
                 rms, view_rms, std_intrinsics, iterations, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int64_t vbs_chess_workspace(int n, int h, int w) {
    if (n < 0 || h < 1 || w < 1 || h > 16384 || w > 16384) return VBS_EINVAL;
    return (int64_t)chess_workspace_bytes(n, h, w);
}

extern "C" int vbs_chess_corners(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row,
                                 int pw, int ph, double* corners, int32_t* found, int32_t* peaks, int32_t* n_candidates,
                                 int32_t* response, void* workspace, void* stream) {
    if (!gray || !corners || !found || !peaks || !n_candidates || !workspace || n < 0 || h < 1 || w < 1 || h > 16384 ||
        w > 16384 || stride_row < w || pw < 2 || ph < 2 || ((uintptr_t)workspace & 7))
        return VBS_EINVAL;
    if ((int64_t)pw * ph > VBS_CHESS_MAX_PATTERN) return VBS_ECAPACITY;      // never cut short
    if ((int64_t)n * pw * ph >= (1 << 30)) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n) launch_chess(gray, n, h, w, stride_n, stride_row, pw, ph, corners, found, peaks, n_candidates, response, (u64*)workspace,
                        (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_corner_subpix(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row,
                                 double* corners, int k, int wx, int wy, int zx, int zy, int max_iter, double eps, int32_t* iters,
                                 void* stream) {
    if (!gray || !corners || n < 0 || k < 0 || h < 1 || w < 1 || h > 16384 || w > 16384 || stride_row < w || wx < 1 || wy < 1 ||
        wx > VBS_CHESS_MAX_WIN || wy > VBS_CHESS_MAX_WIN || max_iter < 1 || !(eps >= 0.0) || !std::isfinite(eps) ||
        (int64_t)n * k >= (1 << 30))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n && k) launch_corner_subpix(gray, n, h, w, stride_n, stride_row, corners, k, wx, wy, zx, zy, max_iter, eps, iters,
                                     (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_marker_center(vbs_handle* h, const uint8_t* mask, const uint8_t* area_mask, int n,
                                 double* det, int32_t* counts, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!mask || !area_mask || !det || !counts || n < 0) { h->err = "vbs_marker_center: bad argument"; return VBS_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    Workspace& w = h->ws[0];
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    for (int off = 0; off < n; off += h->maxb) {
        int nb = std::min(h->maxb, n - off);
        const LabelPlan plan = label_plan(h, w, nb);
        clear_pass(h, w, nb, plan, s);
        launch_threshold(h, w, mask + off * hw, area_mask + off * hw, nb, s);
        launch_labelling(h, w, nb, plan, s);
        launch_finalize(h, w, nb, det + (size_t)off * h->maxm * VBS_DET_COLS, counts + off, s);
        int rc = check_launch(h);
        if (rc != VBS_OK) return rc;
    }
    return VBS_OK;
}

// One pass of the diameter front end: gray (converted first when the frames are BGR) -> blurred, thresholded bits
static int diam_bits_pass(vbs_handle* h, Workspace& w, const u8* frames, int nb, int channels, int64_t stride_n,
                          int64_t stride_row, int thr, u64* bits, u64* zero_plane, hipStream_t s) {
    if (channels == 1) {
        launch_diam_threshold(h, frames, stride_n, stride_row, nb, thr, bits, zero_plane, s);
    } else {
        int rc = need_gray(h, w, s);
        if (rc != VBS_OK) return rc;
        launch_gray(h, frames, nb, channels, stride_n, stride_row, w.gray, s);
        launch_diam_threshold(h, w.gray, (int64_t)h->H * h->P, h->P, nb, thr, bits, zero_plane, s);
    }
    return VBS_OK;
}

static int diam_threshold_level(double threshold) {     // cv2.threshold on uint8: the level is floor(threshold)
    const double f = std::floor(threshold);
    return f < -1.0 ? -1 : (f > 255.0 ? 255 : (int)f);
}

extern "C" int vbs_threshold_bits(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                                  int64_t stride_row, double threshold, uint64_t* bits, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || !bits || n < 0 || (channels != 1 && channels != 3) || stride_row < (int64_t)h->W * channels ||
        !std::isfinite(threshold)) {
        h->err = "vbs_threshold_bits: bad argument";
        return VBS_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nw = (size_t)h->H * h->WW;
    for (int off = 0; off < n; off += h->maxb) {
        const int nb = std::min(h->maxb, n - off);
        int rc = diam_bits_pass(h, h->ws[0], frames + (int64_t)off * stride_n, nb, channels, stride_n, stride_row,
                                diam_threshold_level(threshold), (u64*)bits + off * nw, nullptr, s);
        if (rc == VBS_OK) rc = check_launch(h);
        if (rc != VBS_OK) return rc;
    }
    return VBS_OK;
}

extern "C" int vbs_measure_markers(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                                   int64_t stride_row, double threshold, double min_area, double min_circularity,
                                   double scale_px_per_mm, double offset_mm, double* rec, int32_t* counts, double* stats,
                                   void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || !rec || !counts || !stats || n < 0 || (channels != 1 && channels != 3) ||
        stride_row < (int64_t)h->W * channels || !std::isfinite(threshold) || !std::isfinite(min_area) ||
        !std::isfinite(min_circularity) || !(scale_px_per_mm > 0.0) || !std::isfinite(scale_px_per_mm) ||
        !std::isfinite(offset_mm)) {
        h->err = "vbs_measure_markers: bad argument";
        return VBS_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    Workspace& w = h->ws[0];
    HIPCHK(h, hipSetDevice(h->device));
    for (int off = 0; off < n; off += h->maxb) {
        const int nb = std::min(h->maxb, n - off);
        clear_pass(h, w, nb, label_plan(h, w, nb), s);
        int rc = diam_bits_pass(h, w, frames + (int64_t)off * stride_n, nb, channels, stride_n, stride_row,
                                diam_threshold_level(threshold), w.open_bits, w.band_bits, s);
        if (rc != VBS_OK) return rc;
        launch_diam_measure(h, w, nb, min_area, min_circularity, scale_px_per_mm, offset_mm,
                            rec + (size_t)off * h->maxm * VBS_DIAM_COLS, counts + off, stats + (size_t)off * VBS_DIAM_STATS_COLS, s);
        rc = check_launch(h);
        if (rc != VBS_OK) return rc;
    }
    return VBS_OK;
}

extern "C" int vbs_track(vbs_handle* h, const double* det, const int32_t* counts, int n, const double* ref_xy,
                         int m_ref, double min_dist, float* table, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!det || !counts || !ref_xy || !table || n < 0 || m_ref < 1) { h->err = "vbs_track: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    if (n) launch_track(h, det, counts, n, ref_xy, m_ref, min_dist, table, (hipStream_t)stream);
    return check_launch(h);
}

static int check_cam(vbs_handle* h, const vbs_camera* cam) {
    if (!cam) { h->err = "camera is NULL"; return VBS_EINVAL; }
    if (!(cam->K[0] > 0) || !(cam->K[4] > 0)) { h->err = "Focal lengths must be positive"; return VBS_EINVAL; }
    return VBS_OK;
}

extern "C" int vbs_solve3d(vbs_handle* h, float* table, int n, int m_ref, const vbs_camera* cam,
                           double min_marker_size_px, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || n < 0 || m_ref < 1) { h->err = "vbs_solve3d: bad argument"; return VBS_EINVAL; }
    int rc = check_cam(h, cam);
    if (rc != VBS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (n) launch_solve3d(h, table, n, m_ref, *cam, min_marker_size_px, (hipStream_t)stream);
    return check_launch(h);
}

// The second workspace of VBS_OPT_PASS_STREAMS = 2 (the per-pass buffers once more; geometry, options and tables are the
// handle's) plus the stream its passes run on and the two events that fork it from / join it to the caller's stream.
static int add_second_workspace(vbs_handle* h) {
    if (h->nws == 2) return VBS_OK;
    const size_t mark = h->allocs.size();
    auto build = [&]() -> int {
        HIPCHK(h, hipSetDevice(h->device));
        int rc = alloc_workspace(h, h->ws[1]);
        if (rc != VBS_OK) return rc;
        if (hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
            h->err = "stream / event creation failed";
            return VBS_EHIP;
        }
        HIPCHK(h, hipDeviceSynchronize());
        return VBS_OK;
    };
    int rc = build();
    if (rc != VBS_OK) {                                 // (whatever of it exists goes: nothing half-made stays on h)
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
        if (h->ev_join) (void)hipEventDestroy(h->ev_join);
        h->stream2 = nullptr; h->ev_fork = h->ev_join = nullptr;
        for (size_t i = mark; i < h->allocs.size(); ++i) (void)hipFree(h->allocs[i]);
        h->allocs.resize(mark);
        h->ws[1] = Workspace();
        h->err = "second pass workspace: " + h->err;
        return rc;
    }
    h->nws = 2;
    if (h->ws[0].gray) {                                // (need_gray: its plane exists whenever the first one's does)
        rc = dev_alloc(h, &h->ws[1].gray, (size_t)h->maxb * h->H * h->P);
        if (rc != VBS_OK) { h->err = "second pass workspace: " + h->err; return rc; }
    }
    return VBS_OK;
}

extern "C" int vbs_track_to_3d(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                               int64_t stride_row, const double* ref_xy, int m_ref, double min_dist,
                               const vbs_camera* cam, double min_marker_size_px, float* table, double* det,
                               int32_t* counts, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!frames || n < 0 || (channels != 1 && channels != 3) || stride_row < (int64_t)h->W * channels ||
        (table && (!ref_xy || m_ref < 1))) {
        h->err = "vbs_track_to_3d: bad argument";
        return VBS_EINVAL;
    }
    if (cam) { int rc = check_cam(h, cam); if (rc != VBS_OK) return rc; }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipSetDevice(h->device));
    // Several passes: odd passes on the second workspace and stream (VBS_OPT_PASS_STREAMS), so that the partly filled last
    // round of one pass's kernels runs next to the other pass - and, for BGR frames, the bandwidth-bound conversion of one pass
    // next to the matrix-core kernels of the other (each workspace converts into its own gray plane).  Every pass writes its own slice of the
    // caller's tables; the second stream starts behind what the caller's stream holds and is joined before the return.
    bool two = h->pass_streams == 2 && !h->prof && !h->undist && n > h->maxb;
    if (two && h->nws == 1) {
        // The second workspace normally exists by now (vbs_set_option(VBS_OPT_PASS_STREAMS, 2) builds it).  A handle left at
        // the default builds it at its first call that spans several passes - unless the caller's stream is being captured
        // (allocations and the device synchronisation of a set-up would break the capture), and if it cannot be built
        // (memory) the call simply runs every pass on the caller's stream: results are identical either way.
        if (capturing(s) || add_second_workspace(h) != VBS_OK) { two = false; h->err.clear(); }
    }
    if (two) {
        HIPCHK(h, hipEventRecord(h->ev_fork, s));
        HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    }
    auto join = [&](int code) {                          // (also on the error returns: an un-joined fork breaks a capture)
        if (two) {
            (void)hipEventRecord(h->ev_join, h->stream2);
            (void)hipStreamWaitEvent(s, h->ev_join, 0);
        }
        return code;
    };
    const int lead = two ? std::max(1, h->maxb / 2) : h->maxb;     // two pass streams: a first pass of half a batch puts them out of phase
    for (int k = 0, off = 0, nb = 0; off < n; off += nb, ++k) {
        nb = std::min(k == 0 ? lead : h->maxb, n - off);
        Workspace& w = h->ws[(two && (k & 1)) ? 1 : 0];
        hipStream_t ss = (two && (k & 1)) ? h->stream2 : s;
        const LabelPlan plan = label_plan(h, w, nb);
        int rc = detect_pass(h, w, frames + (int64_t)off * stride_n, nb, plan, channels, stride_n, stride_row, nullptr, nullptr,
                             nullptr, ss);
        if (rc != VBS_OK) return join(rc);
        launch_labelling(h, w, nb, plan, ss);
        if (table && plan.few)                           // a few frames: detections and tracking rows in one launch
                                                         // (for a batch pass the one launch measured nothing: 282.1 k against 283.1 k frames/s)
            launch_finalize_track(h, w, nb, det ? det + (size_t)off * h->maxm * VBS_DET_COLS : nullptr, counts ? counts + off : nullptr,
                                  ref_xy, m_ref, min_dist, table + (size_t)off * m_ref * VBS_TABLE_COLS, cam, min_marker_size_px, ss);
        else {
            launch_finalize(h, w, nb, det ? det + (size_t)off * h->maxm * VBS_DET_COLS : nullptr,
                            counts ? counts + off : nullptr, ss);
            if (table)
                launch_track_fused(h, w, nb, ref_xy, m_ref, min_dist, table + (size_t)off * m_ref * VBS_TABLE_COLS, cam,
                                   min_marker_size_px, ss);
        }
        rc = check_launch(h);
        if (rc != VBS_OK) return join(rc);
    }
    return join(VBS_OK);
}

extern "C" int vbs_displacement_range(vbs_handle* h, const float* table, int n, int m_ref, int warmup_frames,
                                      double min_marker_size_px, double max_displacement, int frame_begin,
                                      int frame_end, float* disp, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || !disp || n < 0 || m_ref < 1 || frame_begin < 0 || frame_end > n || frame_begin > frame_end) {
        h->err = "vbs_displacement: bad argument";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (frame_end > frame_begin)
        launch_displacement(h, h->ws[0], table, n, m_ref, warmup_frames, min_marker_size_px, max_displacement, frame_begin,
                            frame_end, disp, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_displacement(vbs_handle* h, const float* table, int n, int m_ref, int warmup_frames,
                                double min_marker_size_px, double max_displacement, float* disp, void* stream) {
    return vbs_displacement_range(h, table, n, m_ref, warmup_frames, min_marker_size_px, max_displacement, 0, n, disp,
                                  stream);
}

extern "C" int vbs_displacement_f64(int device, const double* table, int n, int m_ref, int warmup_frames,
                                    double min_marker_size_px, double max_displacement, double* disp,
                                    void* stream) {
    if (!table || !disp || n < 0 || m_ref < 1) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n) {
        int* cell = nullptr;                            // first-frame cell: a small stream-ordered allocation
        if (hipMallocAsync((void**)&cell, sizeof(int), (hipStream_t)stream) != hipSuccess) return VBS_ENOMEM;
        launch_displacement64(table, n, m_ref, warmup_frames, min_marker_size_px, max_displacement, disp, cell,
                              (hipStream_t)stream);
        (void)hipFreeAsync(cell, (hipStream_t)stream);
    }
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_plane_fit(vbs_handle* h, const float* table, int n, int m_ref, float* plane, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || !plane || n < 0 || m_ref < 1) { h->err = "vbs_plane_fit: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    if (n) launch_plane_fit(h, table, n, m_ref, plane, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_deviation_plane(vbs_handle* h, const float* vert_start, const float* vert_end, const float* tilt_start,
                                   const float* tilt_end, const float* ref_xyz, int m_ref, int shell_mode, double scale,
                                   float* deviation, float* out, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!vert_start || !vert_end || !tilt_start || !tilt_end || !ref_xyz || !deviation || !out || m_ref < 1 ||
        (shell_mode != 0 && shell_mode != 1)) {
        h->err = "vbs_deviation_plane: bad argument";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    launch_deviation_plane(h, vert_start, vert_end, tilt_start, tilt_end, ref_xyz, m_ref, shell_mode, scale, deviation, out,
                           (hipStream_t)stream);
    return check_launch(h);
}

// ---- the time axis (k_series.hip) ---------------------------------------------------------------------------------------
// The handle's scratch for these calls, `need` doubles: built at the first call, kept, grown only by a larger call (never
// under stream capture: hipFree / hipMalloc synchronise).
static int series_scratch(vbs_handle* h, size_t need, hipStream_t s) {
    if (need <= h->series_cap) return VBS_OK;
    if (capturing(s)) {
        h->err = "the scratch of the time-axis reductions has to grow, which cannot happen under stream capture: call once "
                 "with this shape before capturing";
        return VBS_ENOMEM;
    }
    if (h->series_ws) { HIPCHK(h, hipFree(h->series_ws)); h->series_ws = nullptr; h->series_cap = 0; }
    void* q = nullptr;
    if (hipMalloc(&q, need * sizeof(double)) != hipSuccess) {
        h->err = "hipMalloc failed (" + std::to_string(need * sizeof(double)) + " bytes)";
        return VBS_ENOMEM;
    }
    h->series_ws = (double*)q;
    h->series_cap = need;
    return VBS_OK;
}

// n frames from frame_begin on, m_ref slots: within what the kernels index (int frame numbers, 16-bit grid y of 64-slot tiles)
static bool series_shape_ok(int n, int m_ref, int frame_begin) {
    return n >= 1 && m_ref >= 1 && m_ref <= 65535 * 64 && frame_begin >= 0 && (int64_t)frame_begin + n <= 0x7fffffff;
}

extern "C" int vbs_series_chunks(int n, int frame_begin) {
    if (n < 1 || frame_begin < 0 || (int64_t)frame_begin + n > 0x7fffffff) return VBS_EINVAL;
    return series_chunks(n, frame_begin);
}

extern "C" int vbs_series_partial(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* records,
                                  void* stream) {
    if (!h) return VBS_EINVAL;
    if (!disp || !records || !series_shape_ok(n, m_ref, frame_begin)) { h->err = "vbs_series_partial: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    launch_series_partial(h, disp, n, m_ref, frame_begin, records, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_series_merge(vbs_handle* h, const double* records, int n_records, int m_ref, double* stats, double* prefix,
                                void* stream) {
    if (!h) return VBS_EINVAL;
    if (!records || !stats || n_records < 1 || !series_shape_ok(1, m_ref, 0)) { h->err = "vbs_series_merge: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    launch_series_finalize(h, records, n_records, m_ref, stats, prefix, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_series_stats(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* stats,
                                double* cumulative, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!disp || !stats || !series_shape_ok(n, m_ref, frame_begin)) { h->err = "vbs_series_stats: bad argument"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)series_chunks(n, frame_begin) * m_ref;
    int rc = series_scratch(h, cells * (VBS_SERIES_REC_COLS + 1), s);
    if (rc != VBS_OK) return rc;
    double *rec = h->series_ws, *prefix = rec + cells * VBS_SERIES_REC_COLS;
    launch_series_partial(h, disp, n, m_ref, frame_begin, rec, s);
    launch_series_finalize(h, rec, series_chunks(n, frame_begin), m_ref, stats, prefix, s);
    if (cumulative) launch_series_cumsum(h, disp, n, m_ref, frame_begin, prefix, cumulative, s);
    return check_launch(h);
}

extern "C" int vbs_series_stats_f64(int device, const double* disp, int n, int m_ref, int frame_begin, double* stats,
                                    double* cumulative, double* scratch, void* stream) {
    if (!disp || !stats || !scratch || !series_shape_ok(n, m_ref, frame_begin)) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)series_chunks(n, frame_begin) * m_ref;
    double *rec = scratch, *prefix = rec + cells * VBS_SERIES_REC_COLS;
    launch_series_partial64(disp, n, m_ref, frame_begin, rec, s);
    launch_series_finalize(nullptr, rec, series_chunks(n, frame_begin), m_ref, stats, prefix, s);
    if (cumulative) launch_series_cumsum64(disp, n, m_ref, frame_begin, prefix, cumulative, s);
    return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP;
}

extern "C" int vbs_window_means(vbs_handle* h, const float* table, int n, int m_ref, const int32_t* windows, int n_windows,
                                double* means, void* stream) {
    if (!h) return VBS_EINVAL;
    bool ok = table && windows && means && n_windows >= 1 && series_shape_ok(n, m_ref, 0);
    int longest = 1;
    for (int i = 0; ok && i < n_windows; ++i) {
        const int a = windows[2 * i], b = windows[2 * i + 1];
        ok = a >= 0 && b < n && a <= b;
        if (ok) longest = std::max(longest, b - a + 1);
    }
    const int pieces = (longest + VBS_SERIES_CHUNK - 1) / VBS_SERIES_CHUNK;
    if (!ok || pieces > 65535) { h->err = "vbs_window_means: bad argument (windows are inclusive [a, b] inside [0, n), a <= b)"; return VBS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int group = std::min(n_windows, VBS_WINDOWS_PER_LAUNCH);
    int rc = series_scratch(h, (size_t)group * pieces * m_ref * 4, s);
    if (rc != VBS_OK) return rc;
    for (int w0 = 0; w0 < n_windows; w0 += VBS_WINDOWS_PER_LAUNCH)        // (stream order keeps one group's scratch from the next)
        launch_window_means(h, table, m_ref, windows + 2 * w0, std::min(VBS_WINDOWS_PER_LAUNCH, n_windows - w0), pieces,
                            h->series_ws, means + (size_t)w0 * m_ref * VBS_WINDOW_COLS, s);
    return check_launch(h);
}

extern "C" int vbs_displacement_from_frame(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, double* out,
                                           void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || !out || !series_shape_ok(n, m_ref, 0) || ref_frame < 0 || ref_frame >= n ||
        ((int64_t)n * m_ref + 255) / 256 > 0x7fffffff) {
        h->err = "vbs_displacement_from_frame: bad argument";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    launch_disp_from_frame(h, table, n, m_ref, ref_frame, out, (hipStream_t)stream);
    return check_launch(h);
}

// ---- the dynamic polishing process (k_filter.hip) --------------------------------------------------------------------------
extern "C" int vbs_axis_displacement(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, const uint8_t* slot_mask,
                                     int frame_begin, int frame_end, double* axis, double* total, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || (!axis && !total) || !series_shape_ok(n, m_ref, 0) || ref_frame < 0 || ref_frame >= n || frame_begin < 0 ||
        frame_end > n || frame_begin > frame_end) {
        h->err = "vbs_axis_displacement: bad argument (ref_frame inside [0, n), 0 <= frame_begin <= frame_end <= n)";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (frame_end > frame_begin)
        launch_axis_displacement(h, table, m_ref, ref_frame, slot_mask, frame_begin, frame_end, axis, total, (hipStream_t)stream);
    return check_launch(h);
}

// ---- pose misalignment along a recording (k_pose.hip) ---------------------------------------------------------------------------
extern "C" int vbs_pose_series(vbs_handle* h, const float* table, int n, int m_ref, int start_frame, const double* ref_disp,
                               const double* ref_xyz, const uint8_t* slot_mask, int shell_mode, double scale, double reject_k,
                               int frame_begin, int frame_end, double* deviation, double* field, double* pose, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!table || !ref_disp || !ref_xyz || (!deviation && !field && !pose) || !series_shape_ok(n, m_ref, 0) || start_frame < 0 ||
        start_frame >= n || frame_begin < 0 || frame_end > n || frame_begin > frame_end || (shell_mode != 0 && shell_mode != 1) ||
        !std::isfinite(scale) || !std::isfinite(reject_k) || reject_k < 0.0) {
        h->err = "vbs_pose_series: bad argument (start_frame inside [0, n), 0 <= frame_begin <= frame_end <= n, reject_k >= 0, "
                 "scale and reject_k finite, shell_mode 0 or 1, at least one output)";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (frame_end > frame_begin)
        launch_pose_series(h, table, m_ref, start_frame, ref_disp, ref_xyz, slot_mask, shell_mode, scale, reject_k, frame_begin,
                           frame_end, deviation, field, pose, (hipStream_t)stream);
    return check_launch(h);
}

extern "C" int vbs_assign_ids(vbs_handle* h, const double* det, const int32_t* count, int num_layers, int id_mode,
                              int32_t* ids, double* ref_xy, int cap, int32_t* m_out, void* stream) {
    if (!h) return VBS_EINVAL;
    if (!det || !count || !ids || !ref_xy || !m_out || num_layers < 1 || cap < 1 || (id_mode != 0 && id_mode != 1)) {
        h->err = "vbs_assign_ids: bad argument";
        return VBS_EINVAL;
    }
    if (num_layers > VBS_IDS_MAX_LAYERS) {
        h->err = "vbs_assign_ids: num_layers above VBS_IDS_MAX_LAYERS";
        return VBS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    launch_assign_ids(h, det, count, num_layers, id_mode, ids, ref_xy, cap, m_out, (hipStream_t)stream);
    return check_launch(h);
}

#ifdef VBS_DEBUG_KNOBS
// tools/ builds only: k_stage_lat's per-frame header words of the last pass (phase stamps in words 80..), synchronising
extern "C" int vbs_debug_lat_hdr(vbs_handle* h, uint32_t* out, int frames) {
    if (!h || !out || frames < 1 || frames > VBS_LAT_MAXN) return VBS_EINVAL;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->last_ws->lat_hdr, (size_t)frames * VBS_LAT_HDR * sizeof(u32), hipMemcpyDeviceToHost));
    return VBS_OK;
}
#endif
