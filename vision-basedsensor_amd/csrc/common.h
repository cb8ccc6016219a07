// Internal definitions shared by the gfx950 kernels and the C-ABI (include/vbs.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/vbs.h"

typedef unsigned long long u64;
typedef long long i64;
typedef uint32_t u32;
typedef uint8_t u8;

#define VBS_NCC_MAXL 80
#define VBS_RUN_CAP 30720          // union-find nodes (runs) per mask per frame kept in LDS
#define VBS_AREA_SUMS 16           // n, 14 moments up to order 4, spare
#define VBS_LAT_MAXN 32            // passes of at most this many frames may take the few-frames labelling kernel (k_stage_lat.hip)
#define VBS_LAT_HDR 128            // dwords of counters / flags per frame of that kernel
#define VBS_WINDOWS_PER_LAUNCH 16  // k_window_partial takes its windows as kernel arguments; longer lists are launched in groups
#define VBS_DEG 57.29577951308232  // degrees per radian as every entry multiplies by it: x * VBS_DEG

struct BranchParams {              // marker_detection.py:117-126,129,170
    int taps_a, taps_b;            // GaussianBlur sizes
    int thresh, hi;                // inRange bounds
    int ncc_l;                     // template size
    int ncc_lo, ncc_hi;            // window offsets of mode='same'
    int ns;                        // max/min filter size (14 | 8)
    int small;                     // 1 = small-image branch
};

struct NccConst {
    double g[VBS_NCC_MAXL];        // 1-D normalised Gaussian, template = g (x) g
    double cg[VBS_NCC_MAXL + 1];   // cg[k] = g[0] + ... + g[k-1]
    double tbar, T2, l2, thr2;     // mean(template), sum((t-tbar)^2), l*l, 0.1*0.1
    double inv_l2;
};

// cv2.cvtColor(BGR2GRAY) on uint8 (marker_detection.py:114): (cb B + cg G + cr R + 2^(shift-1)) >> shift
struct GrayCoef { u32 cb, cg, cr, half, shift; };
static inline GrayCoef gray_coef(int bits) {
    return bits == 14 ? GrayCoef{1868u, 9617u, 4899u, 1u << 13, 14u} : GrayCoef{3735u, 19235u, 9798u, 1u << 14, 15u};
}

// The symmetric taps of k_fir, k_window_moments and k_poly_moments as a kernel argument: the centre weight, then the weights at
// distance 1 .. n_half - 1; 0.0 beyond.  half [n_half] HOST, checked by the caller
#define VBS_HALF_TAPS ((VBS_FIR_MAX_TAPS + 1) / 2)
static_assert(VBS_HALF_TAPS == VBS_ENV_MAX_HALF + 1 && VBS_HALF_TAPS == VBS_KIN_MAX_HALF + 1, "one length serves the three entries");
struct HalfTaps { double half[VBS_HALF_TAPS]; };
static inline HalfTaps half_taps_arg(const double* half, int n_half) {
    HalfTaps t{};
    for (int i = 0; i < n_half; ++i) t.half[i] = half[i];
    return t;
}

#ifdef VBS_DEBUG_KNOBS                                  // tools/ builds only: phase timing by early exit
#include <cstdlib>
#define VBS_KNOB(name) (getenv(name) ? atoi(getenv(name)) : 0)
#else
#define VBS_KNOB(name) 0
#endif

struct ProfRec { const char* name; hipEvent_t a, b; };

#define SG_REC 2048                // k_stage / k_stage_lat: segment records per frame, at most (StageGeom::rec_cap)

// What the kernels of one internal pass (at most maxb frames) write.  A handle has one, or two with VBS_OPT_PASS_STREAMS = 2.
struct Workspace {
    u8* gray = nullptr;   // [maxb][H][P]   gray plane of 3-channel / undistorted input; null until first needed (need_gray)
    u64* area_bits;    // [maxb][H][WW]
    u64* mask_bits;    // [maxb][H][WW]
    u64* band_bits;    // [maxb][H][WW]
    u64* open_bits;    // [maxb][H][WW]
    u32* wbase;        // [maxb][2][H*WW]   first node index of each word
    u32* stage_mrec = nullptr;   // k_stage's moment records when a frame's slice of wbase would hold fewer than SG_REC of them
                                 // (small frames with many blobs: the reference's real 65-dot layout); null = they live in wbase
    u32* node_pos;     // [maxb][2][RUN_CAP]  y*W + x0 of each run
    u32* node_comp;    // [maxb][2][RUN_CAP]  component id (0-based, raster order) of each run
    u32* ncomp;        // [maxb][2]
    u32* band_first;   // [maxb][maxm]
    u64* band_sums;    // [maxb][maxm][4]   count, sum x, sum y, spare
    u32* area_first;   // [maxb][maxm]
    i64* area_sums;    // [maxb][maxm][VBS_AREA_SUMS]  vertex moments about the component's first pixel.  The capacity limits alone
                       // do not keep them below 2^63: k_finalize reports VBS_ECAPACITY where a sum could leave 64 bits
    double* ell;       // [maxb][maxm][8]   cx, cy, w, h, angle, nvert, ok, spare
    double* det64;     // [maxb][maxm][6]
    int32_t* cnt;      // [maxb]
    unsigned short* probe;   // [maxb][maxm][4]  component ids of the 2x2 cell around every band centroid
    u64* ncc_tot;      // [4]  running NCC decision counters of the passes run here (vbs_ncc_counters sums the workspaces')
    u32* lat_hdr;      // [VBS_LAT_MAXN][VBS_LAT_HDR] k_stage_lat's per-frame counters; slow_total / slow_flag follow (one fill clears all)
    u32* slow_total;   // [1]  frames of this pass the fused kernel handed on (lets the general kernels leave at once)
    u32* slow_flag;    // [maxb]  non-zero = the fast labelling path handed the frame on (the value says why)
    u32* fstat;        // [maxb][8]  0: area popcount, 1: ambiguous ncc pixels, 2: status
    unsigned char* lat_scratch = nullptr;   // [VBS_LAT_MAXN][stage_lat_scratch()] what the workgroups of a frame share; null = path not available
    int lat_slots = 0;              // frames lat_scratch holds (min(max_batch, VBS_LAT_MAXN), fewer for very large frames)
};

struct vbs_handle {
    bool prof = false;                     // record a HIP event pair around every kernel launch
    std::vector<ProfRec> recs;
    int device, H, W, P, WW, maxm, maxb;   // P = row pitch (mult. of 64), WW = P/64 words per row
    BranchParams bp;
    NccConst ncc;
    std::string err;
    // ---- constant tables (vbs_create, vbs_set_undistort) ----
    uint4* blur_frags; // Toeplitz operand fragments of k_blur_mfma (blur_mfma_fragments)
    uint4* blur16_h = nullptr;   // k_blur16: horizontal fragments per 16-column strip (blur16_fragments); null = not built
    uint4* blur16_v = nullptr;   // k_blur16: the 12 vertical fragment variants
    double* ncc_rx;    // [W]  sum of g over the in-image part of the window (columns)
    double* ncc_ry;    // [H]
    uint4* ncc_frags;  // Toeplitz operand fragments of k_ncc_mfma (ncc_mfma_fragments)
    float2* ncc_rowf;  // [H] {rows of the NCC window inside the image, (float) ncc_ry}: border tiles of k_ncc_mfma
    bool ncc_trim_ok = false;   // an empty NCC window is background for every window cut of this frame size (ncc_trim_guard): k_ncc_mfma may skip them
    double* ncc_tab;   // [VBS_NCC_MAXL] g, then [VBS_NCC_MAXL + 1] cg: the exact path of k_ncc_mfma reads them from memory
    u8* lut;           // [256] contour vertex table
    u32* step_lut = nullptr;   // [256] outgoing chain steps of a border pixel (make_step_lut, k_diameter.hip)
    short* umap1;      // [H][W][2] int16 undistortion source pixel (CV_16SC2)
    unsigned short* umap2;   // [H][W] fractional index into the bilinear weight table
    int* uwtab;        // [1024][4] bilinear weights in 1/32768
    bool undist = false;     // frame undistortion enabled (vbs_set_undistort)
    double newK[9];
    // ---- options (vbs_set_option) ----
    int blur_impl = 0;              // VBS_OPT_BLUR_IMPL: 0 k_blur16 where it applies, 1 always k_blur_mfma
    int pass_streams = 2;           // VBS_OPT_PASS_STREAMS
    int stage_impl = 0;             // VBS_OPT_STAGE_IMPL, 0..4: read and documented by label_plan (labelling.hip)
    int gray_bits = 15;             // VBS_OPT_GRAY_COEFFS, the BGR2GRAY fixed-point coefficient set: 15 (OpenCV 4) | 14 (OpenCV <= 3.4.1)
    bool force_seq_match = false;   // VBS_OPT_FORCE_SEQ_MATCH
    int ncc_margin_ppm = 0;         // VBS_OPT_NCC_MARGIN: test hook, widens the float32 filter's margin
    int lat_frames = 24;            // VBS_OPT_LATENCY_FRAMES: passes of <= this many frames take k_stage_lat (0: never); label_plan
    // dynamic LDS declared (hipFuncSetAttribute) for k_stage / k_ccl<0|1> / k_stage_lat through this handle
    size_t stage_lds_set[2] = {0, 0}, ccl_lds_set[2] = {0, 0}, lat_lds_set = 0;
    // ---- per-pass workspaces ----
    // VBS_OPT_PASS_STREAMS = 2: the internal passes of vbs_track_to_3d alternate between ws[0] on the caller's stream and
    // ws[1] on `stream2`; ws[1], the stream and its fork / join events are built at first use (nws = 2)
    Workspace ws[2];
    int nws = 1;
    Workspace* last_ws = ws;               // the workspace of the last internal pass (vbs_frame_stats, vbs_stage_tables)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<void*> allocs;
    // ---- scratch of the time-axis reductions (k_series.hip): sized by the call, built at first use, only ever grown ----
    double* series_ws = nullptr;
    size_t series_cap = 0;                 // doubles
};

// global chunks of VBS_SERIES_CHUNK frames that frames [frame_begin, frame_begin + n) touch (n >= 1, frame_begin >= 0)
static inline int series_chunks(int n, int frame_begin) {
    return (int)(((int64_t)frame_begin + n - 1) / VBS_SERIES_CHUNK - frame_begin / VBS_SERIES_CHUNK + 1);
}

#define HIPCHK(h, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return VBS_EHIP;                                                              \
        }                                                                                 \
    } while (0)

// kernel launch with optional event bracketing on the launch stream (vbs_profile / vbs_profile_read)
#define VBS_LAUNCH(h, s, name, ...)                                                       \
    do {                                                                                  \
        hipEvent_t a_ = nullptr, b_ = nullptr;                                            \
        if ((h)->prof) {                                                                  \
            (void)hipEventCreate(&a_); (void)hipEventCreate(&b_); (void)hipEventRecord(a_, s); \
        }                                                                                 \
        hipLaunchKernelGGL(__VA_ARGS__);                                                  \
        if ((h)->prof) { (void)hipEventRecord(b_, s); (h)->recs.push_back({name, a_, b_}); } \
    } while (0)

// ---- launchers (each enqueues on `s`; nb = frames in this pass, whose buffers are those of workspace `w`) ----------
void launch_gray(vbs_handle* h, const u8* frames, int nb, int channels, int64_t stride_n,
                 int64_t stride_row, u8* gray, hipStream_t s);
void launch_gray_dense(vbs_handle* h, const u8* frames, int nb, int64_t stride_n, int64_t stride_row, u8* out,
                       hipStream_t s);
void launch_blur(vbs_handle* h, Workspace& w, const u8* gray, int64_t gstride_n, int64_t gstride_row, int nb,
                 u8* area_u8, hipStream_t s);
void launch_blur_mfma(vbs_handle* h, Workspace& w, const u8* gray, int64_t gstride_n, int64_t gstride_row, int nb,
                      u8* area_u8, hipStream_t s);          // k_blur_mfma.hip: what launch_blur (k_blur16.hip) falls back on
void launch_ncc(vbs_handle* h, Workspace& w, int nb, u8* mask_u8, double* ncc_out, hipStream_t s);
void launch_ncc_mfma(vbs_handle* h, Workspace& w, int nb, u8* mask_u8, hipStream_t s);   // k_ncc_mfma.hip: launch_ncc (k_ncc_map.hip) without a map
void launch_points(int which, const double* in, int n, const vbs_camera& cam, double* out, int32_t* ok,
                   hipStream_t s);
void launch_threshold(vbs_handle* h, Workspace& w, const u8* mask, const u8* area, int nb, hipStream_t s);
// Labelling (a9 - a12: band / open planes, their components and sums).  How a pass does it is decided ONCE, by label_plan
// (labelling.hip); clear_pass (api.hip) and launch_labelling take that plan, so what is cleared and what runs cannot disagree.
enum LabelRoute { LABEL_LAT, LABEL_FUSED, LABEL_CCL, LABEL_GENERAL };     // k_stage_lat | k_stage | k_morph + k_ccl | k_label<0> for every frame
// stage_threads: k_stage's threads per frame (LABEL_LAT / LABEL_FUSED); few: at most VBS_OPT_LATENCY_FRAMES frames, whatever the route
struct LabelPlan { LabelRoute route; int stage_threads; bool few; };
LabelPlan label_plan(const vbs_handle* h, const Workspace& w, int nb);
// The caller has run clear_pass with THIS plan for this workspace on this stream: no launcher below clears anything.
void launch_labelling(vbs_handle* h, Workspace& w, int nb, const LabelPlan& plan, hipStream_t s);
int stage_threads(const vbs_handle* h, int nb);          // k_stage.hip: 768 or 256
bool launch_stage_lat(vbs_handle* h, Workspace& w, int nb, hipStream_t s);     // false: not for this pass (geometry, scratch, LDS refused)
bool launch_stage(vbs_handle* h, Workspace& w, int nb, int nt, hipStream_t s);   // false: geometry outside the fused path
bool launch_ccl(vbs_handle* h, Workspace& w, int nb, hipStream_t s);           // false: geometry outside the round-2 fast path
void launch_morph(vbs_handle* h, Workspace& w, int nb, const u32* only, hipStream_t s);    // `only`: just the frames flagged there
struct MorphStrips { int G, strips, rps, wpf; };         // morph_wave's split of a frame: strips per wave, strips, rows per strip, waves
void launch_label(vbs_handle* h, Workspace& w, int nb, int all, const u32* nslow, const MorphStrips* ms, hipStream_t s);
void launch_finalize(vbs_handle* h, Workspace& w, int nb, double* det, int32_t* counts, hipStream_t s);
void launch_track(vbs_handle* h, const double* det, const int32_t* counts32, int nb,
                  const double* ref_xy, int m_ref, double min_dist, float* table, hipStream_t s);
void launch_solve3d(vbs_handle* h, float* table, int n, int m_ref, const vbs_camera& cam,
                    double min_size, hipStream_t s);
void launch_displacement(vbs_handle* h, Workspace& w, const float* table, int n, int m_ref, int warmup,
                         double min_size, double max_disp, int f0, int f1, float* disp, hipStream_t s);
void launch_plane_fit(vbs_handle* h, const float* table, int n, int m_ref, float* plane,
                      hipStream_t s);
void launch_deviation_plane(vbs_handle* h, const float* vs, const float* ve, const float* ts, const float* te, const float* ref,
                            int m_ref, int shell, double scale, float* dev, float* out, hipStream_t s);
void launch_assign_ids(vbs_handle* h, const double* det, const int32_t* count, int num_layers, int full_mode,
                       int32_t* ids_out, double* xy_out, int cap, int32_t* m_out, hipStream_t s);
void make_contour_lut(u8 out[256]);
void make_step_lut(u32 out[256]);
// k_diameter.hip: blur + inverse threshold of gray frames -> bits [nb][H][WW] (zero_plane, if given, <- 0), and the chain from
// the bits in w.open_bits (w.band_bits empty) to records, counts and statistics
void launch_diam_threshold(vbs_handle* h, const u8* gray, int64_t stride_n, int64_t stride_row, int nb, int thr, u64* bits,
                           u64* zero_plane, hipStream_t s);
void launch_diam_measure(vbs_handle* h, Workspace& w, int nb, double min_area, double min_circ, double scale, double offset_mm,
                         double* rec, int32_t* counts, double* stats, hipStream_t s);
std::vector<u32> ncc_mfma_fragments(const NccConst& nc, int l);
std::vector<u32> blur_mfma_fragments(const std::vector<int>& taps_a, const std::vector<int>& taps_b, int nk,
                                     int sa0, int nka);
void blur16_fragments(const std::vector<int>& taps_s, const std::vector<int>& taps_l, int W, bool small, std::vector<u32>* hfrag,
                      std::vector<u32>* vfrag);
void launch_track_fused(vbs_handle* h, Workspace& w, int nb, const double* ref_xy, int m_ref, double min_dist,
                        float* table, const vbs_camera* cam, double min_size, hipStream_t s);
// launch_finalize + launch_track_fused as one launch (k_finalize_track: passes of a few frames)
void launch_finalize_track(vbs_handle* h, Workspace& w, int nb, double* det, int32_t* counts, const double* ref_xy, int m_ref,
                           double min_dist, float* table, const vbs_camera* cam, double min_size, hipStream_t s);
void launch_popcount(vbs_handle* h, Workspace& w, int nb, hipStream_t s);
size_t stage_lat_scratch(const vbs_handle* h);          // bytes of scratch per frame k_stage_lat needs for this geometry (0: not taken)
// n 32-bit words <- value, as a KERNEL on `s`: the per-pass clears of the hot path.  (Not hipMemsetAsync: captured into a HIP
// graph, the memset nodes of a one-stream multi-pass call left the first pass's status words holding address-like garbage
// from the second replay on - tools/gpu_graph_debug.py, ROCm 7.2 - while kernel nodes replay exactly.)
void launch_fill(u32* p, u32 value, size_t n, hipStream_t s);
int launch_ncc_general(const double* T, int th, int tw, const double* I, int h, int w, int mode, double* out,
                       double* stats, hipStream_t s);
void launch_displacement64(const double* table, int n, int m_ref, int warmup, double min_size, double max_disp,
                           double* disp, int* fmin_scratch, hipStream_t s);
void launch_series_partial(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* rec, hipStream_t s);
void launch_series_partial64(const double* disp, int n, int m_ref, int frame_begin, double* rec, hipStream_t s);
void launch_series_finalize(vbs_handle* h, const double* rec, int n_rec, int m_ref, double* stats, double* prefix, hipStream_t s);   // h may be null
void launch_series_cumsum(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, const double* prefix, double* cum,
                          hipStream_t s);
void launch_series_cumsum64(const double* disp, int n, int m_ref, int frame_begin, const double* prefix, double* cum, hipStream_t s);
void launch_window_means(vbs_handle* h, const float* table, int m_ref, const int32_t* windows, int nw, int pieces, double* part,
                         double* means, hipStream_t s);
void launch_disp_from_frame(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, double* out, hipStream_t s);
// k_filter.hip (f10): signed displacement from a reference frame with its sum over the slots; gap-aware zero-phase FIR along time
void launch_axis_displacement(vbs_handle* h, const float* table, int m_ref, int ref_frame, const u8* slot_mask, int frame_begin,
                              int frame_end, double* axis, double* total, hipStream_t s);
void launch_fir_series(const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half, double need,
                       int frame_begin, int frame_end, double* out, hipStream_t st);
// k_pose.hip (f12): deviation field, plane, tilt, steep direction and residual of every frame against a reference state
void launch_pose_series(vbs_handle* h, const float* table, int m_ref, int start_frame, const double* ref_disp, const double* ref_xyz,
                        const u8* slot_mask, int shell, double scale, double reject_k, int frame_begin, int frame_end,
                        double* deviation, double* field, double* pose, hipStream_t s);
// k_field.hip (f13): the kernel smoother in space on the float64 matrix instruction (VBS_OK, or VBS_EHIP when the LDS it asks
// for is refused), and the contact patch of every map
int launch_field_map(const double* rec, int s, int cols, int n_values, const double* W, const double* wsum, int P,
                     double min_coverage, int frame_begin, int frame_end, double* map, hipStream_t st);
void launch_patch_stats(const double* map, int F, int P, int n_values, const double* grid_xy, int component, double sign, double thr,
                        double* patch, hipStream_t st);
// k_spectrum.hip (f14): the projection of every series onto a caller's basis on the float64 matrix instruction, and the harmonic
// fit and peak of those projections
void launch_project_series(const double* rec, int n, int s, int cols, int n_values, const double* basis, int R, double* proj,
                           hipStream_t st);
void launch_harmonic_fit(const double* proj, int s, int R, int n_values, int Q, int min_count, double det_min, double* fit,
                         double* peak, hipStream_t st);
// k_motion.hip (f15): the affine fit of every frame's displacement field with its invariants and residual, and the same fit over
// the neighbourhood of every marker
void launch_motion_series(const double* rec, int s, int cols, const double* pos, const u8* slot_mask, double reject_k,
                          int frame_begin, int frame_end, double* grad, double* strain, double* residual, hipStream_t st);
void launch_local_strain(const double* rec, int s, int cols, const double* pos, const int32_t* nbr, int K, int min_count,
                         double det_rel, int frame_begin, int frame_end, double* out, hipStream_t st);
// k_robust.hip (f16): gap-aware rolling median and MAD along time, the Hampel rule, the record with its spikes turned into gaps
void launch_hampel_series(const double* rec, int n, int s, int cols, int n_values, int half_window, int min_count, double thr,
                          double min_scale, int frame_begin, int frame_end, double* out, double* clean, hipStream_t st);
// k_envelope.hip (f17): the weighted sums of a sliding window at one frequency as a banded product on the float64 matrix
// instruction, and the floating-mean fit of every window
void launch_window_moments(const double* rec, int n, int s, int cols, int n_values, const double* carrier, const double* half,
                           int n_half, int frame_begin, int frame_end, double* mom, hipStream_t st);
void launch_window_fit(const double* mom, int F, int s, int n_values, double need, double det_min, double* fit, hipStream_t st);
// k_kinematics.hip (f19): the moments of a gap-aware weighted local polynomial fit along time as several banded products over one
// staged operand on the float64 matrix instruction, and the fit of every window with its fallback in degree
void launch_poly_moments(const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half, int degree,
                         int frame_begin, int frame_end, double* mom, hipStream_t st);
void launch_poly_fit(const double* mom, const double* rec, int s, int cols, int n_values, int degree, int half_window,
                     const double* thr, int fill_degree, int frame_begin, int frame_end, double* fit, double* filled,
                     hipStream_t st);
// k_modes.hip (f18): the cross moments of all pairs of series on the float64 matrix instruction, the covariance they give, its
// leading eigenpairs by orthogonal iteration (apply, orthogonalise, Ritz step), and the score of every mode in every frame
void launch_cross_moments(const double* rec, int n, int s, int cols, int n_values, const double* shift, double* mom, hipStream_t st);
void launch_covariance(const double* mom, int s, int n_values, int mode, int min_count, double denom, const u8* slot_mask, double* cov,
                       u8* ok, hipStream_t st);
void launch_leading_modes(const double* A, int C, int r, int iters, double tiny, double* work, double* values, double* modes,
                          double* resid, int32_t* info, hipStream_t st);
void launch_mode_scores(const double* rec, int s, int cols, int n_values, const double* center, const double* modes, int r,
                        double min_coverage, int frame_begin, int frame_end, double* scores, double* energy, hipStream_t st);
// k_steps.hip (f11): step response, peak search, dwell statistics
void launch_step_response(const double* rec, int n, int s, int cols, int n_values, int w, int min_count, double* out,
                          hipStream_t st);
void launch_find_steps(const double* resp, int n, int s, int resp_cols, int w, double thr2, int max_steps, int32_t* steps,
                       hipStream_t st);
void launch_dwell_stats(const double* rec, int n, int s, int cols, int n_values, const int32_t* steps, int steps_rows,
                        int max_steps, int guard, double* out, hipStream_t st);
// k_uncert.hip (f21): Jacobians of the 3-D solve by forward mode, the covariances of positions, displacements and their total,
// the pixel noise of a still segment.  obs [dev] [obs_rows (1 or m), 6]; cam_factor [host] [16, q]; ref [dev] [m, VBS_UNCERT_REF_COLS]
void launch_uncert_points(const double* uvd, int n, const vbs_camera& cam, double* xyz, double* j_obs, double* j_cam, int32_t* ok,
                          hipStream_t s);
void launch_uncert_cov(const float* table, int m, const vbs_camera& cam, const double* obs, int obs_rows, const double* cam_factor,
                       int q, int ref_frame, double min_size, double piv_rel, int frame_begin, int frame_end, double* ref, double* cov,
                       double* dcov, hipStream_t s);
void launch_uncert_total(const float* table, int m, const vbs_camera& cam, const double* obs, int obs_rows, const double* cam_factor,
                         int q, int ref_frame, const u8* slot_mask, double min_size, int frame_begin, int frame_end, double* ref,
                         double* total, hipStream_t s);
void launch_pixel_noise(const float* table, int m, int frame_begin, int frame_end, double* out, hipStream_t s);
// k_posecov.hip (f22): the covariance of the pose plane, its angles and t2; fix [dev] [m, VBS_UNCERT_REF_COLS], obs as above
void launch_pose_cov(const float* table, int m, int start_frame, const double* ref_disp, const double* ref_xyz, const u8* slot_mask,
                     int shell, double scale, double reject_k, const vbs_camera& cam, const double* obs, int obs_rows,
                     const double* cam_factor, int q, double min_size, double piv_rel, const float* ref_rows, int frame_begin,
                     int frame_end, double* fix, double* pose, double* pcov, hipStream_t s);
// k_shape.hip (f24): the quadric through the end points of every frame, its apex and curvatures, the residual per marker
void launch_shape_series(const float* table, int m, int start_frame, const double* ref_disp, const double* ref_xyz, const u8* slot_mask,
                         int shell, double scale, double length, double reject_k, int min_count, double piv_rel, double apex_rel,
                         double max_apex, int frame_begin, int frame_end, double* shape, double* coef, double* residual, hipStream_t s);
// k_rigid.hip (f25): rotation, translation and scale of every frame against a given point set, the residual per marker
void launch_rigid_series(const float* table, int m, const double* source, const u8* slot_mask, int with_scale, double reject_k,
                         double gap_rel, int frame_begin, int frame_end, double* rigid, double* coef, double* residual, hipStream_t s);
// k_rigid_ml.hip (f27): the noise-weighted pose from the start vbs_rigid_series left, its covariance, chi^2, the distance per marker
void launch_rigid_ml_series(const float* table, int m, const double* source, const double* cov, const double* start,
                            const double* residual, const double* source_cov, int iters, double piv_rel, int frame_begin,
                            int frame_end, double* ml, double* pcov, double* coef, double* mahal, hipStream_t s);
// k_sphere.hip (f26): the sphere of the markers (fitted, or `given` [4] read on the host), the contact set, its plane, the records
void launch_sphere_series(const float* table, int m, const double* given, const u8* fit_mask, const u8* slot_mask, const double* source,
                          double contact_depth, double piv_rel, double gap_rel, double reject_k, int frame_begin, int frame_end,
                          double* sphere, double* radial, double* decomp, hipStream_t s);
// k_pnp.hip (f7): hypotheses + refit of nb PnP problems; one of image / table is null
void launch_pnp(const double* world, int n, const double* image, const float* table, const u8* valid, int nb, const vbs_camera& cam,
                const int32_t* samples, int nh, double reproj_px, int32_t* hyp_count, double* hyp_pose, int32_t* status, double* pose,
                int32_t* inlier_count, u8* inlier_mask, double* errors, int32_t* winner, hipStream_t s);
// k_retrack.hip (f20): the grid of every frame, the walk along time, the table rows; `assign` null: the workspace holds it
size_t retrack_workspace_bytes(int n, int m, int max_det);
void launch_retrack(const double* det, const int32_t* counts, int n, int max_det, const double* ref_xy, int m, const double* state_in,
                    double gate, double max_travel, double vel_gain, int max_coast, int32_t* assign, float* table, double* dist2,
                    int32_t* info, double* state_out, void* workspace, hipStream_t st);
// k_refine.hip (f23): grey-level refinement of the tracked rows of a table, one wave a row; every output may be null
void launch_refine(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, const float* table, int m_ref,
                   double core_f, double disc_f, double ring_f, double min_contrast, double max_shift_f, int polarity,
                   int keep_unrefined, double* rec, i64* sums, float* table_out, hipStream_t s);
// k_calib.hip (f9): homographies of nv views, then nb calibration problems over subsets of them
void launch_calib(const double* obj, int n, const double* img, int nv, const u8* view_mask, int nb, int w, int h, int max_iter,
                  double* H, int32_t* view_void, int32_t* status, double* K4, double* dist, double* R, double* T, double* rms,
                  double* view_rms, double* std_intrinsics, int32_t* iterations, hipStream_t s);
// k_chess.hip (f8): response + candidates + ordering + the finder's own refinement; the refinement alone
size_t chess_workspace_bytes(int n, int h, int w);
void launch_chess(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, int pw, int ph, double* corners,
                  int32_t* found, int32_t* peaks, int32_t* n_candidates, int32_t* response, u64* slots, hipStream_t s);
void launch_corner_subpix(const u8* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, double* corners, int k,
                          int wx, int wy, int zx, int zy, int max_iter, double eps, int32_t* iters, hipStream_t s);
int setup_undistort(vbs_handle* h, const double* K9, const double* dist, int ndist, hipStream_t s);
void launch_remap(vbs_handle* h, const u8* frames, int nb, int channels, int64_t stride_n, int64_t stride_row,
                  u8* out, int to_gray, hipStream_t s);
void bilinear_weights_i16(int32_t* out);
void optimal_new_camera_matrix_alpha0(const double* K, const double* k, int w, int h, double* newK);
