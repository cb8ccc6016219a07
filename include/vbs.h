/* vbs.h — C-ABI of libvbs.so: MI355X (gfx950) marker tracking -> 3-D displacement.
 *
 * Drop-in boundary for the hot path of UPM-ROB-Lab/Vision-basedSensor.  The reference has no
 * FFI layer; its boundary is the Python call signatures of
 *   code/Marker_Tracking/marker_detection.py   (class MarkerTracker)
 *   code/Marker_Calibration/3d_reconstruction.py (class MarkerAnalysis)
 * and each entry point below names the reference function it replaces (file:line).  The Python
 * shims in `vision-basedsensor_amd/` bind these with ctypes and pass torch device pointers
 * (`tensor.data_ptr()`); nothing here depends on torch.
 *
 * Conventions
 *  - every pointer marked [dev] is device memory of the handle's GPU, owned by the caller;
 *    the library owns only the workspace inside `vbs_handle`.  No allocation on a hot call, with two stated
 *    exceptions that happen ONCE per handle and never under stream capture: the gray plane of 3-channel / undistorted
 *    input (first such call, or vbs_set_undistort), and the second pass workspace of a handle left at the default
 *    VBS_OPT_PASS_STREAMS (first call spanning several internal passes; vbs_set_option(h, VBS_OPT_PASS_STREAMS, 2)
 *    builds it ahead of time - do that before capturing calls into a graph).  The time-axis reductions size their
 *    scratch by the call instead (vbs_series_stats, vbs_window_means: built at the first call, grown only by a larger one);
 *  - calls are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *    the caller synchronises before reading results;
 *  - return value: VBS_OK or a negative status; `vbs_last_error` gives the text.  Per-frame
 *    conditions found on the device (capacity overflow) are reported in `counts[i]` as a negative
 *    status, because the host cannot see them without a synchronisation;
 *  - one handle per (device, stream); a handle is not thread-safe; one process per GPU.
 *  - images: uint8, pixel (frame i, row y, col x, channel c) at
 *        base + i*stride_n + y*stride_row + x*channels + c        (bytes)
 *    so a crop (marker_detection.py:78-85) is a pointer offset plus the original strides.
 */
#ifndef VBS_H
#define VBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBS_OK          0
#define VBS_EINVAL     -1   /* bad argument (ValueError in the shim)                          */
#define VBS_ECAPACITY  -2   /* more runs / components in a frame than the handle was sized for */
#define VBS_EHIP       -3   /* a HIP runtime call failed                                      */
#define VBS_ENOMEM     -4   /* workspace allocation failed                                    */
#define VBS_EINTERNAL  -5   /* per-frame (in counts[i]): a kernel's internal hand-shake timed out - the frame's result is
                               not to be trusted (never seen in practice: the wait is bounded so that a logic error or a
                               lost workgroup cannot hang the GPU, and it reports here instead of continuing silently) */

#define VBS_DET_COLS    6   /* x, y, major_axis, minor_axis, angle, label(band component, 1-based) */
#define VBS_TABLE_COLS 10   /* flags, Cx, Cy, major, minor, angle, X, Y, Z, det_index            */
#define VBS_FLAG_TRACKED 1  /* table col 0 bit: the reference ID matched a detection (2-D row)    */
#define VBS_FLAG_XYZ     2  /* table col 0 bit: the 3-D solve succeeded                           */
#define VBS_DISP_COLS   5   /* flag, dX, dY, dZ, |d|                                              */
#define VBS_PLANE_COLS  5   /* n_used, a, b, c, tilt_deg                                          */
#define VBS_DEVPLANE_COLS 9 /* n_common, a, b, c, tilt_deg, mean k*dX, mean k*dY, mean k*dZ, mean |d| */

typedef struct vbs_handle vbs_handle;

/* Camera of MarkerAnalysis.load_parameters (3d_reconstruction.py:70-130): every field is the
 * float32 value the reference stores; arithmetic on them is float64 as in the reference. */
typedef struct vbs_camera {
    float K[9];      /* row-major camera matrix            (:87-91)   */
    float dist[5];   /* k1 k2 p1 p2 k3                     (:98-102)  */
    float R[9];      /* row-major R_world_to_cam           (:109-112) */
    float T[3];      /* T_world_to_cam                     (:120-124) */
    float marker_diameter_mm;   /* Config.marker_diameter_mm (:21)   */
} vbs_camera;

/* Workspace for frames of `height` x `width` (after cropping).  `max_markers` bounds the connected
 * components per mask per frame, `max_batch` the frames processed per internal pass (larger
 * batches are looped).  height <= 480 selects the reference's small-image parameter set
 * (marker_detection.py:117-126,170).  Throughput: the labelling kernel runs three frames per compute unit at a time, so
 * passes that are a multiple of 768 frames suit an MI355X best (bench.py: 1536; 290-295 k frames/s against 280 k at 512 and
 * 292 k at 1368 or 1640); results do not depend on the pass size.
 *
 * Frame-size envelope: height >= 64 (no upper bound), 128 <= width <= 4096, 1 <= max_markers <= 1024, max_batch >= 1; anything
 * else is VBS_EINVAL and no handle.  Inside it the frame size alone decides which kernels run; results are the same on every
 * route (tests/test_gpu_geometry_edges.py holds each limit to the oracle).  WW = ceil(width / 64) words per row, G = 64 / WW:
 *   branch      height <= 480: blur taps 21 / 35, NCC template 33; else 39 / 101 and 80 (api.hip).
 *   k_blur16    from 176 (small branch) / 240 columns, width a multiple of 4, frames, rows and the base pointer 4-byte
 *               aligned; else k_blur_mfma (k_blur16.hip: blur16_takes).  Below 128 rows its column grid has one segment.
 *   k_gray      one flat pass when the frame is dense, 16-byte aligned, width a multiple of 64 and height * width one of 16;
 *               else row by row with a scalar tail (k_gray.hip: launch_gray).
 *   k_stage     height <= 2048 and tiles of R = ceil(height / ((threads / 64) * G)) <= 128 rows, for its 256- and its
 *               768-thread instance separately; where 256 refuses, 768 is tried (k_stage.hip: stage_geom).  With
 *               2049 <= width <= 4096 (G = 1) that is height <= 512 / <= 1536.
 *   k_stage_lat height <= 2048 and R = ceil(height / (4 C G)) <= 128 with C = clamp(ceil(ceil(height / (6 G)) / 4), 1, 16)
 *               workgroups (k_stage_lat.hip: lat_geom).  R reaches at most 32 below 2049 rows: only the height rule binds.
 *   k_ccl       height <= 2048 and height * ceil(WW / min(WW, 5)) < 65535 (k_ccl.hip: ccl_layout).
 *   These are the geometry rules only.  k_stage, k_stage_lat and k_ccl also refuse when the LDS their tables need (sized by
 *   the frame and max_markers) exceeds what a workgroup may have: 160 KB, a third of it for k_stage's 256-thread instance;
 *   k_ccl needs room for at least 1024 nodes.
 *   A route whose launcher refuses falls through: few frames (k_stage_lat) -> fused (k_stage) -> round 2 (k_morph, k_ccl)
 *   -> k_morph and k_label over every frame (labelling.hip).  Beyond 2048 rows every frame takes k_label. */
int vbs_create(int device, int height, int width, int max_markers, int max_batch, vbs_handle** out);
int vbs_destroy(vbs_handle* h);
const char* vbs_last_error(const vbs_handle* h);
int vbs_version(void);
/* Handle options.  VBS_OPT_GRAY_COEFFS: fixed-point coefficient set of cv2.cvtColor(BGR2GRAY) (marker_detection.py:114)
 * - 15 (default): OpenCV 4.x, (3735 B + 19235 G + 9798 R + 2^14) >> 15;  14: OpenCV <= 3.4.1, (1868 B + 9617 G +
 * 4899 R + 2^13) >> 14.  The two agree wherever B = G = R.  VBS_OPT_FORCE_SEQ_MATCH (test hook): 1 makes
 * vbs_marker_center replay the reference's sequential contour <-> centre matching (:203-243) instead of the parallel
 * form that is proven equal to it.
 * VBS_OPT_NCC_MARGIN (test hook, results identical): relative margin of the NCC's float32 filter in units of 1e-6
 * (never below the 20 the error bound needs); a wide margin sends thousands of pixels per frame through the queued
 * float64 re-evaluation.  VBS_OPT_STAGE_IMPL (test hook / fallback, results identical): 0 (default) runs band / open /
 * labelling / sums of `_marker_center` (:170-196) in the fused kernel (k_stage.hip) where the frame geometry allows it,
 * 1 always runs the separate kernels (k_morph + k_ccl) that other geometries take, 2 labels EVERY frame with the general
 * kernel (k_morph + k_label: what a frame with holes / beyond the fast path's tables takes), 3 is 0 with the fused kernel
 * at 768 threads per frame always, 4 is 0 with its 256-thread instance wherever the geometry allows (by itself the kernel
 * takes 256 threads for small frames and for passes of >= 512 large ones, 768 otherwise).  VBS_OPT_BLUR_IMPL (test hook /
 * fallback, results identical): 0 (default) runs the two GaussianBlurs (:118-129) on 16-column strips (k_blur16) where the
 * frame allows it (large branch, width >= 240 and a multiple of 8, rows that load as aligned dwords), 1 always runs the 32-column
 * kernel (k_blur_mfma) that every other frame takes.  VBS_OPT_PASS_STREAMS (tuning, results identical): 2 (default) lets
 * vbs_track_to_3d run the odd internal passes of a call with a SECOND WORKSPACE on the handle's own stream (forked from
 * and joined to the caller's stream by events), so that the tail of one pass's kernels
 * overlaps the next pass; 1 runs every pass on the caller's stream.  The second workspace is a second copy of every
 * per-pass buffer, nearly doubling the handle's device memory (the constant tables exist once).  Setting the option to 2
 * EXPLICITLY builds it at once (a set-up call: allocations, one device synchronisation; VBS_ENOMEM / VBS_EHIP if it cannot
 * be built).  A handle left at the default builds it at its first call that spans several passes; if that call's stream
 * is being captured, or the workspace cannot be built, the call runs every pass on the caller's stream instead.  (With vbs_profile on, passes run on
 * one stream: the per-kernel event timings would otherwise overlap.)  VBS_OPT_LATENCY_FRAMES (tuning, results identical):
 * an internal pass of at most this many frames (default 24, at most 32: 1 frame 128 against 264 us, 8: 185 / 324, 16: 269 / 356, 24: 346 / 390, 32: 424 / 406; the reference calls process() with ONE,
 * marker_detection.py:434-453) labels every frame with several workgroups (k_stage_lat) instead of one (k_stage); 0 = never. */
#define VBS_OPT_GRAY_COEFFS      1
#define VBS_OPT_FORCE_SEQ_MATCH  2
/* option 3 is retired (VBS_OPT_GRAY_SIDE_STREAM: BGR conversion a pass ahead on a side stream, no faster) and not reused */
#define VBS_OPT_NCC_MARGIN       4
#define VBS_OPT_STAGE_IMPL       5
#define VBS_OPT_BLUR_IMPL        6
#define VBS_OPT_PASS_STREAMS     7
#define VBS_OPT_LATENCY_FRAMES   8
int vbs_set_option(vbs_handle* h, int option, int value);
/* Motion-JPEG front end (the reference reads its AVI through cv2.VideoCapture, marker_detection.py:50-76).
 * vbs_mjpeg_probe: headers of one JPEG frame -> info[8] = {width, height, components, luma h, luma v, restart interval,
 * int16 coefficients per frame, plane bytes per frame}; VBS_EINVAL for a stream this decoder does not take (progressive,
 * arithmetic, 12-bit, sampling other than 4:4:4 / 4:2:2 / 4:2:0 / gray): the caller then decodes with its own reader.  A frame
 * without DHT segments (camera MJPG) is decoded with the standard tables of ITU-T T.81 Annex K.3.
 * vbs_mjpeg_entropy_batch: Huffman-decodes n frames (buf + offs[i], sizes[i]; all of the probed geometry) on `threads` host
 * threads into the compact form the device half reads (HOST memory, e.g. page-locked): tab [n][info[6] / 64] one word per 8x8
 * block (component after component, row-major over the padded block grid) = (first word of the block in ent, relative to the
 * frame's) << 7 | count; count <= 32 entry words (natural-order position << 16 | quantised value as uint16), or 127 = a dense
 * block of 64 int16; ent holds n * info[6] / 2 words, thread t packs its frames from word (its first frame) * info[6] / 2 on
 * and reports (first word, words used) in regions[2 t], regions[2 t + 1] (2 * threads int64): only those spans, tab,
 * frame_base [n] (a frame's first word) and qt [n][3][64] need to reach the device - typically a tenth of the pixels' bytes.
 * status[i] per frame; returns the number of frames that failed.  vbs_mjpeg_reconstruct: DEVICE copies of those arrays ->
 * BGR frames `out` (byte strides out_frame / out_row), planes = device scratch of n * info[7] bytes; dequantisation, the
 * 8x8 "islow" inverse DCT, "fancy" chroma upsampling and the YCbCr -> RGB tables as published in libjpeg, so that the
 * frames equal a libjpeg(-turbo) decode bit for bit; asynchronous on `stream`. */
int vbs_mjpeg_probe(const uint8_t* jpeg, int64_t size, int32_t* info);
int vbs_mjpeg_entropy_batch(const uint8_t* buf, const int64_t* offs, const int32_t* sizes, int n, const int32_t* info,
                            uint32_t* ent, uint32_t* tab, int64_t* frame_base, int64_t* regions, uint16_t* qt, int32_t* status,
                            int threads);
int vbs_mjpeg_reconstruct(const uint32_t* ent, const uint32_t* tab, const int64_t* frame_base, const uint16_t* qt, int n,
                          const int32_t* info, uint8_t* planes, uint8_t* out, int64_t out_frame, int64_t out_row, void* stream);
/* The entropy decode ON THE DEVICE (opt-in: MjpegDeviceDecoder(entropy="device")): scans WITHOUT restart intervals, decoded
 * as self-synchronising subsequences (Klein & Wiseman; Weissenberger & Schmidt 2021), one workgroup per frame.
 * vbs_mjpeg_scan_batch (HOST, `threads` C++ threads, no Huffman decoding): frames buf + offs[i], sizes[i] of a mapping of
 * buf_size bytes.  A chunk with offs[i] < 0, sizes[i] < 4, sizes[i] > INT32_MAX or offs[i] + sizes[i] > buf_size gets
 * status[i] = VBS_EINVAL and not one byte of it is read; so does a frame whose header does not parse or whose geometry is not
 * info's.  Per good frame: qt [n][3][64] as above, and the scan's bytes copied into `stage` WITH THE FF 00 STUFFING REMOVED AND
 * THE COPY ENDING AT THE FIRST MARKER, starting at scan_off[i] (a multiple of VBS_MJPEG_SCAN_ALIGN; `stage` itself must be
 * so aligned) and followed by at least VBS_MJPEG_SCAN_GUARD zero bytes (the device reads big-endian 32-bit words, two per
 * symbol, at most 11 bytes beyond the last scan byte); scan_bits[i] = 8 * the de-stuffed length (0 for a frame that has a
 * restart interval: the device reports it short and the caller decodes it on the host).  stage_cap must hold the sum over
 * the good chunks of (sizes[i] + VBS_MJPEG_SCAN_GUARD rounded up to VBS_MJPEG_SCAN_ALIGN), else VBS_EINVAL is returned;
 * thread t packs its frames from the offset the frames before its first could need at most and reports (first byte, bytes
 * used) in regions[2 t], regions[2 t + 1] (2 * threads int64): only those spans need to reach the device.  The decode tables
 * (9-bit look-ahead + canonical maxcode / valptr / mincode rows, by component; csrc/jpeg_huff_common.h) are built once per
 * DISTINCT set of the batch: sets = room for n * VBS_MJPEG_HUFF_SET_BYTES, *n_sets of them are written, table_set[i] = the
 * frame's.  Returns the number of frames that failed, or VBS_EINVAL.
 * vbs_mjpeg_huffman_device: DEVICE copies of stage, scan_off, scan_bits, table_set, sets -> ent, tab, frame_base exactly as
 * vbs_mjpeg_reconstruct reads them, every block dense: ent (n * info[6] / 2 words) is zero-filled and gets the int16
 * coefficients in natural order, tab[i][b] = (32 b) << 7 | 127, frame_base[i] = i * info[6] / 2.  subseq_bits: 0 (default,
 * VBS_MJPEG_SUBSEQ_BITS) or a multiple of 32 in [128, 65536].  status[i] (device, written by the frame's workgroup): VBS_OK;
 * VBS_MJPEG_SHORT when the scan's bits end before the last block is complete (libjpeg and the host decoder pad such a scan
 * with zero bits; the device does NOT reproduce that tail) or the scan is longer than VBS_MJPEG_DEVICE_BITS_MAX; VBS_EINVAL
 * when the true decode chain meets an impossible step (no code of <= 16 bits, a run beyond coefficient 63, a DC category
 * above 11) or table_set[i] is outside [0, n_sets).  A frame whose status is not VBS_OK has undefined ent contents: the
 * caller decodes it with vbs_mjpeg_entropy_batch and uploads the result into the frame's span of ent and its row of tab.
 * info[5] (restart interval) must be 0.  Asynchronous on `stream`; three launches (zero-fill, k_jpeg_huff, k_jpeg_dc). */
#define VBS_MJPEG_SCAN_ALIGN      16
#define VBS_MJPEG_SCAN_GUARD      16
#define VBS_MJPEG_HUFF_SET_BYTES  8928
#define VBS_MJPEG_SUBSEQ_BITS     1024
#define VBS_MJPEG_DEVICE_BITS_MAX 2147418112
#define VBS_MJPEG_SHORT           1   /* per-frame status of vbs_mjpeg_huffman_device, not an error of the call */
int vbs_mjpeg_scan_batch(const uint8_t* buf, int64_t buf_size, const int64_t* offs, const int64_t* sizes, int n, const int32_t* info,
                         uint8_t* stage, int64_t stage_cap, int64_t* scan_off, int64_t* scan_bits, int32_t* table_set, void* sets,
                         int32_t* n_sets, int64_t* regions, uint16_t* qt, int32_t* status, int threads);
int vbs_mjpeg_huffman_device(const uint8_t* stage, const int64_t* scan_off, const int64_t* scan_bits, const int32_t* table_set,
                             const void* sets, int n_sets, int n, const int32_t* info, int subseq_bits, uint32_t* ent, uint32_t* tab,
                             int64_t* frame_base, int32_t* status, void* stream);
/* The annotated tracking video (`_tracked.avi`, marker_detection.py:69-76,453) as Motion-JPEG, encoded on the device.
 * vbs_jpeg_encode: n BGR frames [dev] uint8 (frame / row strides in bytes, 3 bytes per pixel; a crop view is fine) -> one
 * complete JFIF file per frame, equal byte for byte to Pillow's `Image.save(buf, "JPEG", quality=quality)` (libjpeg-turbo
 * defaults: 4:2:0, islow DCT, Annex K Huffman tables, no optimisation).  File i is written at payload + offsets[i], sizes[i]
 * bytes long, the files back to back (offsets[0] = 0); offsets / sizes are DEVICE arrays.  No handle: the caller owns the
 * workspace [dev] and the payload [dev], sized by vbs_jpeg_encode_workspace (host-only, no GPU needed), which also reports the
 * bound on one file.  Entropy coding runs on the device; asynchronous on `stream`.
 * Payload bound: a block (8x8 samples) codes to at most VBS_JPEG_BLOCK_BITS_MAX bits (DC: an 11-bit code + 11 magnitude bits;
 * each of 63 AC coefficients: a 16-bit code + 10 magnitude bits; a ZRL or EOB replaces coefficients that would cost more),
 * byte stuffing at most doubles the scan, so one frame of B = 6 ceil(W/16) ceil(H/16) blocks takes at most
 * VBS_JPEG_HEADER_BYTES + 2 ceil(B VBS_JPEG_BLOCK_BITS_MAX / 8) + 2 (EOI) bytes; payload_bytes = n times that.
 * quality 1..100; frames of up to 65535 x 65535 whose scan bound stays below 2^32 bits. */
#define VBS_JPEG_BLOCK_BITS_MAX 1660
#define VBS_JPEG_HEADER_BYTES   623
int vbs_jpeg_encode_workspace(int width, int height, int n, int64_t* workspace_bytes, int64_t* payload_bytes,
                              int64_t* frame_bound);
int vbs_jpeg_encode(const uint8_t* frames, int n, int width, int height, int64_t stride_n, int64_t stride_row, int quality,
                    void* workspace, int64_t workspace_bytes, uint8_t* payload, int64_t payload_bytes, int64_t* offsets,
                    int32_t* sizes, void* stream);
/* MarkerTracker._draw_tracking (marker_detection.py:398-427), painted on every frame of a batch for the video:
 * frames [dev] uint8 BGR [n,H,W,3] (frame / row strides in bytes; a crop view is fine; not modified), det [dev] float64
 * [n,max_markers,VBS_DET_COLS] and table [dev] float32 [n,m_ref,VBS_TABLE_COLS] as vbs_track_to_3d writes them, ref_xy [dev]
 * float64 [m_ref,2] -> out [dev] uint8 [n,H,W,3] dense.  For each slot with VBS_FLAG_TRACKED, in slot order: the filled red
 * disc of radius 4 at (int(Cx), int(Cy)), the red arrow of thickness 2 (tipLength 0.25) from (int(Ox), int(Oy)), the yellow
 * major and the blue minor axis of thickness 2; a later primitive covers an earlier one.  Coordinates come from the float64
 * det rows (the table's det index, col 9).  Rasterisation restated from OpenCV 4.x imgproc/src/drawing.cpp (circle FILLED,
 * line/ThickLine with XY_SHIFT 16 and round caps, arrowedLine).  lastw [dev] int32 scratch of n*H*W.  Asynchronous. */
int vbs_draw_tracking(const uint8_t* frames, int n, int height, int width, int64_t stride_n, int64_t stride_row,
                      const double* det, int max_markers, const float* table, const double* ref_xy, int m_ref,
                      int32_t* lastw, uint8_t* out, void* stream);
/* host-only helper: the 256-entry table that classifies a border pixel's 8-neighbourhood into the
 * number of CHAIN_APPROX_SIMPLE vertices it contributes (bit d of the index = neighbour in chain
 * direction d is foreground; 0=E,1=NE,2=N,...,7=SE). */
int vbs_contour_lut(uint8_t out[256]);
/* host-only helper, the counterpart of vbs_contour_lut for the diameter validation: the 256-entry table of a border pixel's
 * OUTGOING chain steps (same index).  Bits 4 d .. 4 d + 3 of an entry = how many times the outer border leaves the pixel in
 * chain direction d; summed over the border pixels of hole-free foreground this is the full (unapproximated) chain of every
 * outer border: its unit and diagonal step counts and, with sum x dy - y dx over the steps, twice its signed area. */
int vbs_step_lut(uint32_t out[256]);
/* host-only helper: the body (no header line) of the tracker's CSV - `pandas.DataFrame(rows).to_csv(index=False)`,
 * marker_detection.py:464-468 - for n rows of three int64 columns (frameno, row, col) and nf float64 columns (Ox, Oy, Cx,
 * Cy, major_axis, minor_axis, angle), byte for byte: floats as Python's repr writes them (shortest digits that round-trip,
 * exponent form below 1e-4 and from 1e16), NaN as an empty cell.  Formatted by `threads` host threads into buf.
 * Returns the bytes written; a negative value -c when cap < c = the capacity that is always enough (n * (65 + 26 nf)). */
int64_t vbs_format_csv(const int64_t* frameno, const int64_t* row, const int64_t* col, const double* const* fcols, int nf,
                       int64_t n, char* buf, int64_t cap, int threads);
/* host-only helpers exposing the constant tables the kernels use, so they can be checked without a
 * GPU: the fixed-point GaussianBlur taps (sum 256; marker_detection.py:118-124 via cv2) and the 1-D
 * factor g of the NCC template with stats = {mean(t), sum((t-mean)^2), l*l, 0.1^2}
 * (_gkern :138-143, _normxcorr2 :152,162). */
int vbs_gaussian_taps_q8(int ksize, double sigma, int32_t* out);
int vbs_ncc_template(int l, double sigma, double* g, double* stats);
/* host-only: may the NCC kernel skip windows that hold no area pixel?  Such a window is background as long as
 * d0 = (template mass) - (samples) * mean(t) of its in-image part is not negative; -> 1 if the minimum of d0 over every
 * window cut of a height x width frame lies above -5e-5 (half of what the kernel's own decision allows), else 0
 * (vbs_create then leaves the kernel as it was for that handle); the minimum goes to *min_d0 if given.  tbar_shift is
 * added to mean(t): 0 for the library's own use, anything else only shows the check failing. */
int vbs_ncc_trim_guard(int l, double sigma, int height, int width, double tbar_shift, double* min_d0);
/* host-only: the tiling the fused labelling kernel (k_stage) gives a height x width frame whose set bits (mask | area) have the
 * bounding box [xlo, xhi] x [ylo, yhi] (xlo > xhi: an empty frame), for ns = 14 / 8 and 768 / 256 threads.  out[12] = the
 * full-frame tiling {words per row, row blocks per wave, row blocks, rows per block}, the frame's own {first word column,
 * words, row blocks per wave, row blocks, rows per block, first row}, the horizontal guard in pixels, and whether the frame's
 * own tiling differs from the full-frame one.  VBS_EINVAL for a geometry the kernel does not take. */
int vbs_stage_box_geom(int height, int width, int ns, int threads, int xlo, int xhi, int ylo, int yhi, int* out);

/* MarkerTracker._undistort_frame (marker_detection.py:93-109), optional (`calibration_params` in the config):
 * getOptimalNewCameraMatrix(K, D, (w,h), 0) + initUndistortRectifyMap(CV_16SC2) are evaluated ONCE here (the
 * reference rebuilds them per frame); afterwards vbs_find_markers / vbs_track_to_3d / vbs_ncc_map first remap every
 * frame (INTER_LINEAR, fixed point, constant border 0) exactly as `_preprocess_frame` does (:88-89).
 * K9 row-major float64 camera matrix, dist = up to 5 coefficients k1 k2 p1 p2 k3; newK9 (may be NULL) receives the
 * new camera matrix.  K9 == NULL switches undistortion off again. */
int vbs_set_undistort(vbs_handle* h, const double* K9, const double* dist, int ndist, double* newK9, void* stream);
/* The remap alone: frames [dev] uint8 (same addressing as below) -> out [dev] uint8 [n,h,w,channels] dense. */
int vbs_undistort_frames(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                         int64_t stride_row, uint8_t* out, void* stream);

/* cv2.cvtColor(frame, COLOR_BGR2GRAY) (marker_detection.py:114) on its own: frames [dev] uint8 BGR (3 channels,
 * addressing as above) -> gray [dev] uint8 [n,h,w] dense, with the handle's coefficient set (VBS_OPT_GRAY_COEFFS).
 * (Stage entry for parity tests; on the hot path the same conversion kernel runs in front of the blur.) */
int vbs_bgr2gray(vbs_handle* h, const uint8_t* frames, int n, int64_t stride_n, int64_t stride_row, uint8_t* gray,
                 void* stream);

/* MarkerTracker._find_markers (marker_detection.py:112-135): BGR2GRAY -> 2x GaussianBlur -> uint8
 * difference +15 (mod 256) -> inRange -> area_mask {0,255}; NCC with the Gaussian template
 * (_gkern :138, _normxcorr2 :146) -> mask {0,1} = ncc > 0.1.
 * frames [dev] uint8, channels 1 (gray) or 3 (BGR); mask / area_mask [dev] uint8 [n,h,w] dense
 * (either may be NULL). */
int vbs_find_markers(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                     int64_t stride_row, uint8_t* mask, uint8_t* area_mask, void* stream);

/* MarkerTracker._normxcorr2 (marker_detection.py:146-164) for the pipeline's own operands: the
 * float64 correlation map of area_mask with the template, ncc [dev] float64 [n,h,w] dense.
 * (Diagnostic / parity entry: the hot path never materialises this map.) */
int vbs_ncc_map(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                int64_t stride_row, double* ncc, void* stream);
/* The same stage from a given two-valued area_mask [dev] uint8 [n,h,w] (the reference call
 * `_normxcorr2(template, area_mask)` :132 with the template of the handle's branch): ncc [dev]
 * float64 [n,h,w] and / or mask [dev] uint8 [n,h,w] = ncc > 0.1 (:133); either may be NULL. */
int vbs_normxcorr2(vbs_handle* h, const uint8_t* area_mask, int n, double* ncc, uint8_t* mask,
                   void* stream);
/* MarkerTracker._normxcorr2(template, image, mode) (marker_detection.py:146-164) for ARBITRARY operands, no handle needed:
 * tmpl [dev] float64 [th,tw] (tw <= 256), image [dev] float64 [h,w], mode 0 'full' | 1 'same' | 2 'valid' (the window
 * scipy.signal.fftconvolve returns), out [dev] float64 of that mode's size ([h+th-1,w+tw-1] | [h,w] | [h-th+1,w-tw+1]).
 * Direct float64 evaluation; agrees with the reference's FFT route to its rounding.  Not on the hot path. */
int vbs_normxcorr2_general(int device, const double* tmpl, int th, int tw, const double* image, int h, int w, int mode,
                           double* out, void* stream);
/* Live kernel timing: while enabled, every kernel launch of this handle is bracketed by a HIP event
 * pair on the launch stream.  vbs_profile(h, on) clears the records; vbs_profile_read synchronises
 * and writes one text line per kernel: "<name> <launches> <total_ms>". */
int vbs_profile(vbs_handle* h, int enable);
int vbs_profile_read(vbs_handle* h, char* buf, int cap);
/* host copy of the per-frame counters of the LAST internal pass (of whichever workspace ran it): out[i*8 + {0: area_mask popcount,
 * 1: NCC pixels within 1e-9 (relative) of the 0.1 threshold, 2: status, 3: NCC pixels re-evaluated in float64,
 * 4: holes LEFT in the opened area mask (components - Euler number; holes are filled before contouring, like
 * cv2.findContours(RETR_EXTERNAL) ignores them, so this is 0 unless the fill pass ran out of capacity), 5 / 6: connected
 * components of the band / opened mask (the opened mask once its holes are filled: its external contours), 7: holes that were
 * filled}] (synchronises). */
int vbs_frame_stats(vbs_handle* h, uint32_t* out, int n);
/* Diagnostic / parity entry: host copies of the per-component tables the labelling kernels left for the first n frames of
 * the LAST internal pass (synchronises; any pointer may be NULL): ncomp [n][2] components of the band / opened mask,
 * band_sums [n][max_markers][4] (count, sum x, sum y, spare), area_first [n][max_markers] first pixel (y * w + x) of every
 * opened component, area_sums [n][max_markers][16] contour-vertex moments about it, probe [n][max_markers][4] component ids
 * of the 2x2 pixel cell around every band centroid (0xFFFF = background), slow [n] non-zero = the general kernel redid the frame (the value says why: +16 = in the opened-mask half; 1 slots, 2 components, 3 mailbox, 4 holes, 5 vertex multiplicity, 6 segments per tile, 7 records, 8 queued unions).
 * Entries past a frame's component counts are unspecified. */
int vbs_stage_tables(vbs_handle* h, int n, uint32_t* ncomp, uint64_t* band_sums, uint32_t* area_first, int64_t* area_sums,
                     uint16_t* probe, uint32_t* slow);
/* Diagnostic / parity entry: host copy of the ellipse table that the last step of _marker_center (k_finalize, or
 * k_finalize_track) left for the first n frames of the LAST internal pass (synchronises): out [n][max_markers][8], one row per
 * opened component in vbs_stage_tables' order = {0, 1: ellipse centre x, y; 2, 3: axes w <= h; 4: angle in degrees (all five
 * float32 values, as cv2.fitEllipse returns them); 5: contour vertices; 6: 1 = fitted, 0 = fewer than 5 vertices or a singular
 * system (columns 0 - 4 are then unspecified); 7: spare}.  Rows past a frame's opened-component count, and the rows of a frame
 * whose status is not VBS_OK, are unspecified. */
int vbs_ellipse_table(vbs_handle* h, int n, double* out);
/* Running totals over EVERY internal pass of the detection stage since the last reset (vbs_frame_stats only sees the
 * last pass): out = {NCC pixels inside the ambiguity band of the 0.1 threshold (`:133`; 0 = every decision equals the
 * float64 one), NCC pixels re-evaluated in float64, frames}.  Synchronises. */
int vbs_ncc_counters(vbs_handle* h, uint64_t out[3], int reset);

/* MarkerAnalysis._undistort_points (3d_reconstruction.py:185-193) and _calculate_3d_position
 * (:195-238) on float64 points, no handle needed: pts/out [dev] float64 [n,2]; uvd [dev] float64
 * [n,3] = (u, v, diameter_px); xyz [dev] float64 [n,3]; ok [dev] int32 [n] (0 where the reference
 * raises ValueError). */
int vbs_undistort_points(int device, const double* pts, int n, const vbs_camera* cam, double* out,
                         void* stream);
int vbs_calculate_3d(int device, const double* uvd, int n, const vbs_camera* cam, double* xyz,
                     int32_t* ok, void* stream);

/* ---- Extrinsic calibration (code/Marker_Calibration/extrinsic_calibration.py) -------------------------------------------------
 * vbs_pnp_ransac - calibrate_camera_extrinsics (extrinsic_calibration.py:81-123): cv2.solvePnPRansac(SOLVEPNP_ITERATIVE,
 * reprojectionError, iterationsCount) (:97-106), projectPoints and the mean reprojection error (:117-118), for n_problems
 * problems at once - one per frame of a recording - that share their world points and their sample table.  No handle needed.
 *   world [dev] float64 [n_points,3], n_points <= VBS_PNP_MAX_POINTS; exactly one of
 *   image [dev] float64 [n_problems,n_points,2] pixel positions (a non-finite one is invalid), or
 *   table [dev] float32 [n_problems,n_points,VBS_TABLE_COLS] as vbs_track_to_3d writes it: Cx, Cy of the rows with VBS_FLAG_TRACKED;
 *   valid [dev] uint8 [n_problems,n_points] (may be NULL = all): 0 removes a correspondence;
 *   cam: K and dist only (k1 k2 p1 p2 k3); samples [dev] int32 [n_hyp,VBS_PNP_SAMPLE], n_hyp <= VBS_PNP_MAX_HYPOTHESES: the
 *   point indices of every hypothesis, drawn by the caller (the same draws serve every problem, so a run is deterministic).
 * Every hypothesis: normalised points (the inverse model of vbs_undistort_points) -> planar homography of its first 4 points
 * (Z ignored, 8 x 8 elimination with partial pivoting) -> nearest rotation -> 10 Gauss-Newton steps on all 6 with their Z ->
 * the number of valid points whose pixel error through the forward Brown-Conrady model is <= reproj_px.  A hypothesis is VOID
 * (count -1) when its sample repeats an index, touches an invalid point, is singular, or puts a sample point behind the camera.
 *   hyp_count [dev] int32 [n_problems,n_hyp], hyp_pose [dev] float64 [n_problems,n_hyp,12] = R row-major, then T (outputs).
 * Every problem: the winner = highest count, ties to the lowest index; Levenberg-Marquardt (at most 20 steps, analytic Jacobian)
 * on the pixel error of the winner's inliers.  cv2 shortens the iteration count by its confidence and draws EPnP hypotheses from
 * 5 points: poses agree up to the optimiser, not bit for bit.
 *   status [dev] int32 [n_problems]: VBS_OK, VBS_PNP_FEW_POINTS (fewer than 4 valid points, :89-91) or VBS_PNP_NO_HYPOTHESIS
 *     (every hypothesis void: also fewer than VBS_PNP_SAMPLE valid points); a failed problem has NaN pose and errors, count 0,
 *     winner -1, and does not touch its neighbours;
 *   pose [dev] float64 [n_problems,12] = R_world_to_cam row-major, T_world_to_cam; inlier_count [dev] int32 [n_problems];
 *   inlier_mask [dev] uint8 [n_problems,n_points]: the WINNING HYPOTHESIS's inliers (not recomputed after the refit, as cv2);
 *   errors [dev] float64 [n_problems,2] = mean pixel error over ALL valid points (what :118 computes), RMS over the inliers;
 *   winner [dev] int32 [n_problems]: index of the winning hypothesis.
 * Float64, no atomics, fixed summation order: two runs give the same bits and a problem does not depend on its batch.
 * n_problems is not limited (more than 65535 run as several launch pairs); the hypothesis buffers are what grows with it. */
#define VBS_PNP_SAMPLE            6
#define VBS_PNP_MAX_POINTS     1024
#define VBS_PNP_MAX_HYPOTHESES 4096
#define VBS_PNP_FEW_POINTS        1
#define VBS_PNP_NO_HYPOTHESIS     2
int vbs_pnp_ransac(int device, const double* world, int n_points, const double* image, const float* table,
                   const uint8_t* valid, int n_problems, const vbs_camera* cam, const int32_t* samples, int n_hyp,
                   double reproj_px, int32_t* hyp_count, double* hyp_pose, int32_t* status, double* pose,
                   int32_t* inlier_count, uint8_t* inlier_mask, double* errors, int32_t* winner, void* stream);

/* ---- Intrinsic calibration (code/Marker_Calibration/intrinsic_calibration.py) ---------------------------------------------------
 * vbs_calibrate_camera - cv2.calibrateCamera(obj_points, img_points, img_size, None, None) (intrinsic_calibration.py:97-98) for one
 * planar board seen in n_views views, as n_problems problems at once that each use a subset of the views (all of them, each one
 * left out, random subsets) and share the corners.  No handle needed, nothing is allocated: the homographies are an output.
 *   obj [dev] float64 [n_points,2]: the board, Z = 0; 4 <= n_points <= VBS_CHESS_MAX_PATTERN;
 *   img [dev] float64 [n_views,n_points,2]: the corners of every view; 1 <= n_views <= VBS_CALIB_MAX_VIEWS;
 *   view_mask [dev] uint8 [n_problems,n_views] or NULL: problem b uses the views with a non-zero entry (NULL: every problem uses
 *     all views); w, h: the image size (the initial principal point is its centre); max_iter >= 1 (cv2: 30).
 * Every view, once per call: homography by Hartley-normalised normal equations with h33 = 1 (the 8 x 8 elimination of
 * vbs_pnp_ransac), then 5 Gauss-Newton steps on the transfer error.  VOID when a pivot falls below 1e-9 of the largest entry
 * or the corners lie on one line (determinant of their scatter below 1e-9 of the product of its diagonal).
 *   homography [dev] float64 [n_views,9] (NaN where void), view_void [dev] int32 [n_views] (outputs).
 * Every problem: cv2's closed form for a planar target with flags = 0 (cx, cy at the centre; 1 / fx^2, 1 / fy^2 from two rows per
 * view, 2 x 2 normal equations summed in view order; recalled from cvInitIntrinsicParams2D, unverified: DESIGN.md 7), a pose per
 * view from K^-1 H, then Levenberg-Marquardt on the pixel error of every corner of the active views over fx fy cx cy k1 k2 p1 p2
 * k3 and 6 pose parameters per view (left-multiplied rotation update), damping lambda diag from 1e-3, / 10 on an accepted step,
 * x 10 on a rejected one, until max_iter steps were tried or the largest step component falls below 1e-11.
 *   status [dev] int32 [n_problems]: VBS_OK, VBS_CALIB_FEW_VIEWS (fewer than 3 active views, :92) or VBS_CALIB_DEGENERATE (an
 *     active view is void; the closed form is singular or gives a non-positive 1 / f^2; a pose puts the board behind the camera;
 *     no damping up to 1e10 factorises).  A failed problem has NaN outputs and does not touch its neighbours.
 *   K4 [dev] float64 [n_problems,4] = fx fy cx cy; dist [dev] float64 [n_problems,5] = k1 k2 p1 p2 k3 (cv2's order);
 *   R [dev] float64 [n_problems,n_views,9], T [dev] float64 [n_problems,n_views,3]: board to camera, NaN for inactive views;
 *   rms [dev] float64 [n_problems] = sqrt(sum |e|^2 / points), cv2's return value; view_rms [dev] float64 [n_problems,n_views];
 *   std_intrinsics [dev] float64 [n_problems,9] = sqrt(sigma^2 diag S^-1) at the optimum, sigma^2 = sum e^2 / (2 points -
 *     parameters), S = the Schur complement of the pose blocks in J^T J (NaN without degrees of freedom);
 *   iterations [dev] int32 [n_problems]: steps tried (accepted or rejected).
 * Float64, no atomics, sums ordered by the position in the list of active views: two runs give the same bits, and a masked
 * problem gives the bits of the same views passed alone.  Checks before the device is touched: VBS_EINVAL (a null pointer other
 * than view_mask, n_points < 4, n_views, n_problems, w, h or max_iter < 1), VBS_ECAPACITY beyond either cap. */
#define VBS_CALIB_MAX_VIEWS   64
#define VBS_CALIB_FEW_VIEWS    1
#define VBS_CALIB_DEGENERATE   2
int vbs_calibrate_camera(int device, const double* obj, int n_points, const double* img, int n_views, const uint8_t* view_mask,
                         int n_problems, int w, int h, int max_iter, double* homography, int32_t* view_void, int32_t* status,
                         double* K4, double* dist, double* R, double* T, double* rms, double* view_rms, double* std_intrinsics,
                         int32_t* iterations, void* stream);

/* MarkerTracker._marker_center (marker_detection.py:166-249): band = mask AND NOT erode(mask)
 * (maximum/minimum_filter :171-174) -> 4-connected labels (:176) -> centroids (:181); 5x5 open
 * (:195) -> external contours (:196) -> fitEllipse (:208) -> contour/centre matching (:222-243).
 * mask, area_mask [dev] uint8 [n,h,w] dense, two-valued (0 / non-zero).
 * det [dev] float64 [n,max_markers,VBS_DET_COLS], rows in the reference's output order (centroids are
 * integer sums / count in float64, bit-identical to ndimage.center_of_mass; axes and angle are the
 * float32 values cv2.fitEllipse would return, widened);
 * counts [dev] int32 [n] = number of rows, or a negative status for that frame: VBS_ECAPACITY beyond the labelling's
 * limits (30720 runs, max_markers or 512 components), and for a contour so long that its int64 vertex moments could leave
 * 64 bits (vertex count + sum x^2 (w - 1)^2 + sum y^2 (h - 1)^2 >= 9e18 about its first pixel: only frames of several
 * thousand rows hold one). */
int vbs_marker_center(vbs_handle* h, const uint8_t* mask, const uint8_t* area_mask, int n,
                      double* det, int32_t* counts, void* stream);

/* ---- Marker diameter validation (code/Precision_Validation/DiameterValidation.py) ------------------------------------------
 * vbs_measure_markers - main's GaussianBlur (:218) and measure_markers (:113-144) with the statistics of :169-170 / :233-234,
 * for every frame of a batch (frames as for vbs_find_markers; BGR goes through the BGR2GRAY of :211 first; undistortion
 * set on the handle is NOT applied).  GaussianBlur(gray, (5,5), 0) = the fixed kernel (1, 4, 6, 4, 1) / 16 in the fixed-point
 * model of the other blurs (its standing against cv2 itself: restated, unpinned) -> THRESH_BINARY_INV (:115: blur <= threshold,
 * level floor(threshold)) -> external contours (:116; 8-connected components, holes ignored, in findContours' order) ->
 * contourArea (:122), arcLength (:126), circularity (:129), the filters area < min_area (:123), perimeter == 0 (:127),
 * circularity < min_circularity (:130) -> minEnclosingCircle (:134) -> diameter_mm = 2 radius / scale_px_per_mm + offset_mm
 * (:135-138).
 *   rec [dev] float64 [n,max_markers,VBS_DIAM_COLS], one row per surviving contour in the reference's order:
 *     0 cx, 1 cy, 2 radius_px (the EXACT minimum enclosing circle of the pixel centres, float64; cv2 returns float32),
 *     3 diameter_mm, 4 area (= |area2| / 2), 5 perimeter (= n_axis + n_diag sqrt 2 in float64), 6 circularity,
 *     7 n_axis, 8 n_diag (unit / diagonal steps of the full border chain), 9 first pixel (y * width + x),
 *     10 number of support points (1, 2 or 3), 11-16 their (x, y), 17 pixels of the component (holes filled),
 *     18-21 bounding box x0, y0, x1, y1 (inclusive), 22 area2 = the signed shoelace sum over the chain, 23 component id.
 *   counts [dev] int32 [n] = rows, or a negative status; stats [dev] float64 [n,VBS_DIAM_STATS_COLS] = count, mean, std
 *     (np.std, ddof 0), min, max of diameter_mm (NaN at count 0 or a negative status), summed in a fixed order.
 * Capacity: the labelling's (VBS_ECAPACITY beyond 30720 runs, max_markers or 512 components per frame), and a SURVIVING
 * contour whose bounding box exceeds VBS_DIAM_MAX_EXTENT pixels in either direction reports VBS_ECAPACITY for its frame: the
 * circle kernel keeps two candidate points per row of the box in a 4 KB LDS array, coordinates packed into 16 bits each (the
 * exact integer tests themselves would hold for a larger box).  A contour the filters reject - the chessboard of a
 * validation shot - never counts against it.  Six launches per pass (clear, threshold, k_label, measure, circle, statistics;
 * seven for BGR), no allocation (BGR: the gray plane, as above).
 * The call runs in the handle's FIRST pass workspace and overwrites its bit planes, run tables and per-frame statistics:
 * afterwards vbs_frame_stats and vbs_stage_tables describe this call's last pass, not the last tracking pass.
 * vbs_threshold_bits (stage entry for parity tests): the first step alone -> bits [dev] uint64 [n,height,ceil(width/64)],
 * bit x % 64 of word x / 64 = pixel x. */
#define VBS_DIAM_COLS        24
#define VBS_DIAM_STATS_COLS   5
#define VBS_DIAM_MAX_EXTENT 512
int vbs_threshold_bits(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n, int64_t stride_row,
                       double threshold, uint64_t* bits, void* stream);
int vbs_measure_markers(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n, int64_t stride_row,
                        double threshold, double min_area, double min_circularity, double scale_px_per_mm, double offset_mm,
                        double* rec, int32_t* counts, double* stats, void* stream);

/* ---- Chessboard corners (Marker_Calibration/intrinsic_calibration.py:75-81, Precision_Validation/DiameterValidation.py:50) ----
 * vbs_chess_corners - cv2.findChessboardCorners(gray, (pw, ph)) for n gray frames at once, restated (cv2 is not available to
 * this project: DESIGN.md 4.9 and 7 say what is restated and what is recalled).  No handle needed.
 *   gray [dev] uint8, pixel (i, y, x) at gray + i*stride_n + y*stride_row + x (a crop is a pointer offset); BGR frames go
 *   through vbs_bgr2gray first.  1 <= h, w <= 16384; 2 <= pw, ph; pw * ph <= VBS_CHESS_MAX_PATTERN, else VBS_ECAPACITY (a
 *   pattern is never cut short).
 * Response: the integer ChESS response on a 16-sample ring of radius 5, R = 5 (SR - DR) - |5 sum(ring) - 16 L|, for pixels at
 * least 5 from every edge (minus infinity elsewhere).  Candidates: R > 0, >= every response of its 9 x 9 neighbourhood and > those
 * before it in row-major order.  Ordering: the VBS_CHESS_MAX_CANDIDATES strongest by (R desc, y asc, x asc) are the seeds, in
 * that order, and a seed walks only over candidates with 8 R >= its own R.  Its two steps are its nearest neighbour and its
 * nearest neighbour between 60 and 120 degrees of that, at most twice as long; positions p + step are walked with the step
 * re-estimated at every corner, the nearest candidate accepted when 16 d^2 <= |step|^2.  found = 1 only when the maximal
 * lattice through the seed is exactly pw x ph (a larger or an incomplete one: 0); the first seed that succeeds wins.  Integer
 * arithmetic throughout: results do not depend on scheduling.
 *   peaks [dev] int32 [n,pw*ph,2] (x, y): corner (r, c) at r*pw + c, column step x row step > 0 in image axes, and among the
 *     labellings that satisfy this the one whose corner 0 has the smallest (y, x); -1 where found = 0.
 *   corners [dev] float64 [n,pw*ph,2]: the peaks through vbs_corner_subpix with window (2,2), 15 iterations, eps 0.1 - the
 *     refinement findChessboardCorners ends with; NaN where found = 0.
 *   found [dev] int32 [n]; n_candidates [dev] int32 [n]: ALL candidates of the frame, before the cap.
 *   response [dev] int32 [n,h,w] or NULL: the response map (INT32_MIN = minus infinity), for tests; otherwise never written.
 *   workspace [dev]: vbs_chess_workspace(n, h, w) bytes, 8-byte aligned (one 64-bit slot per 5 x 5 cell of every 32 x 16 tile).
 * vbs_corner_subpix - cv2.cornerSubPix(gray, corners, (wx, wy), (zx, zy), (EPS + MAX_ITER, max_iter, eps)) (:80-81) for k
 * corners in each of n frames, in place: Gaussian window exp(-(i/wy)^2) exp(-(j/wx)^2), zeroed inside the zero zone (-1, -1 =
 * none); per iteration a bilinear (2wx+3) x (2wy+3) patch with replicated border, central differences, the sums a, b, c, bb1,
 * bb2, the 2 x 2 solve; stops at max_iter, at |step| <= eps, on a singular system, or when the corner leaves the image; a
 * corner that ends further than the window from its start returns to its start.  1 <= wx, wy <= VBS_CHESS_MAX_WIN, n*k < 2^30.
 * The patch and the window are float32 as in cv2, positions and sums float64 (cv2: float32 positions), one wave per corner,
 * sums reduced over the lanes in a fixed tree: the same bits run to run and whatever the batch.  A non-finite corner is left
 * as it is.  iters [dev] int32 [n,k] or NULL: solves done per corner. */
#define VBS_CHESS_MAX_CANDIDATES 256
#define VBS_CHESS_MAX_PATTERN    256
#define VBS_CHESS_MAX_WIN         15
int64_t vbs_chess_workspace(int n, int h, int w);
int vbs_chess_corners(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row, int pw, int ph,
                      double* corners, int32_t* found, int32_t* peaks, int32_t* n_candidates, int32_t* response,
                      void* workspace, void* stream);
int vbs_corner_subpix(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row,
                      double* corners, int k, int wx, int wy, int zx, int zy, int max_iter, double eps, int32_t* iters,
                      void* stream);

/* MarkerTracker._track_markers (marker_detection.py:349-396): per reference ID the nearest
 * detection (first on ties), dropped when farther than min_dist.  ref_xy [dev] float64 [m_ref,2]
 * = (Ox, Oy) in reference-dict order; table [dev] float32 [n,m_ref,VBS_TABLE_COLS]; XYZ columns
 * are left 0 and VBS_FLAG_XYZ clear. */
int vbs_track(vbs_handle* h, const double* det, const int32_t* counts, int n, const double* ref_xy,
              int m_ref, double min_dist, float* table, void* stream);

/* MarkerAnalysis._undistort_points + _calculate_3d_position (3d_reconstruction.py:185-238) on the
 * tracked rows of `table` (in place: fills X,Y,Z and VBS_FLAG_XYZ).  Rows with
 * major_axis < min_marker_size_px are skipped (load_marker_data :172-176). */
int vbs_solve3d(vbs_handle* h, float* table, int n, int m_ref, const vbs_camera* cam,
                double min_marker_size_px, void* stream);

/* Fused frames -> table: everything above in one call, intermediates kept on the device in
 * float64 / bit-packed form (no uint8 masks are written).  counts may be NULL.  The 3-D solve reads
 * Cx, Cy, major_axis as the float32 values of the row it writes: the table equals vbs_track followed
 * by vbs_solve3d bit for bit. */
int vbs_track_to_3d(vbs_handle* h, const uint8_t* frames, int n, int channels, int64_t stride_n,
                    int64_t stride_row, const double* ref_xy, int m_ref, double min_dist,
                    const vbs_camera* cam, double min_marker_size_px, float* table,
                    double* det, int32_t* counts, void* stream);

/* MarkerAnalysis._track_markers (3d_reconstruction.py:240-316) on a (gathered) table of n
 * consecutive frames: per ID the displacement against the frame where it was LAST SEEN; frames
 * before `first_frame + warmup_frames` are skipped; |d| > max_displacement clears the flag.
 * disp [dev] float32 [n,m_ref,VBS_DISP_COLS]. */
int vbs_displacement(vbs_handle* h, const float* table, int n, int m_ref, int warmup_frames,
                     double min_marker_size_px, double max_displacement, float* disp, void* stream);

/* The same, emitting only frames [frame_begin, frame_end) of a table holding frames [0, n): what a rank of a
 * multi-GPU run calls on the gathered table for its own shard (disp [dev] float32 [frame_end-frame_begin, m_ref, 5]).
 * The look-back for the last-seen frame may reach before frame_begin. */
int vbs_displacement_range(vbs_handle* h, const float* table, int n, int m_ref, int warmup_frames,
                           double min_marker_size_px, double max_displacement, int frame_begin, int frame_end,
                           float* disp, void* stream);

/* The same on float64 tables (same column layout, no handle): what `MarkerAnalysis._track_markers(df)`
 * uses so that the DataFrame interface keeps the reference's float64 results. */
int vbs_displacement_f64(int device, const double* table, int n, int m_ref, int warmup_frames,
                         double min_marker_size_px, double max_displacement, double* disp, void* stream);

/* fit_plane_least_squares (ForceDistribution.py:138-162): per frame Z = aX + bY + c over the rows
 * with VBS_FLAG_XYZ, tilt = atan(sqrt(a^2+b^2)) in degrees.  plane [dev] float32 [n,VBS_PLANE_COLS]. */
int vbs_plane_fit(vbs_handle* h, const float* table, int n, int m_ref, float* plane, void* stream);

/* The deviation field and its plane (ForceDistribution.py: process_marker_data :168-208, visualize_deviations :218-243,
 * :262-268, :274): for every marker with a 3-D point (VBS_FLAG_XYZ) in all four table rows - start / end of the vertical
 * loading, start / end of the tilted one - deviation = (tilt_end - tilt_start) - (vert_end - vert_start) (:196-204); the
 * plane Z = aX + bY + c is fitted over the END POINTS ref + scale * deviation (:229-243; shell_mode 0 = 'plane': Z starts
 * at 0, 1 = 'shell': at the reference Z, :222), tilt = atan(sqrt(a^2 + b^2)); out also carries the mean of the scaled
 * deviation vectors (:263) and the mean magnitude of the deviations (:274).
 *   vert_start .. tilt_end [dev] float32 [m_ref][VBS_TABLE_COLS]: one frame's rows of a table each (same slot order)
 *   ref_xyz [dev] float32 [m_ref][3] reference positions (the embedded MARKER_REF_DATA :29-95 in the reference)
 *   deviation [dev] float32 [m_ref][4] = (1 | 0 common, dX, dY, dZ); out [dev] float32 [VBS_DEVPLANE_COLS] */
int vbs_deviation_plane(vbs_handle* h, const float* vert_start, const float* vert_end, const float* tilt_start,
                        const float* tilt_end, const float* ref_xyz, int m_ref, int shell_mode, double scale,
                        float* deviation, float* out, void* stream);

/* ---- The time axis: per-marker statistics of a tracked sequence, on the device ----------------------------------------
 * What the reference computes from its result sheet with pandas, along time and per marker, from the two dense tensors a
 * sequence ends as.  Float64 accumulation, no atomics: two calls on the same input give the same bits.  Frames are cut into
 * chunks of VBS_SERIES_CHUNK, ALIGNED TO GLOBAL FRAME 0 (frame_begin = the global number of the first frame passed, as
 * vbs_displacement_range's), one thread per (chunk, slot); a slot's chunks are then merged in frame order (Chan, Golub &
 * LeVeque's pairwise update of mean and M2), so nothing is serial in the number of frames.
 *
 * vbs_series_stats - MarkerAnalysis.analyze_displacement (3d_reconstruction.py:332-334 cumulative series, :397-400 the
 * statistics of displacement_statistics.csv): disp [dev] float32 [n,m_ref,VBS_DISP_COLS] as vbs_displacement writes it (col 0
 * says which entries are rows of the reference's DataFrame, col 4 is its `displacement`) -> stats [dev] float64
 * [m_ref,VBS_STATS_COLS] = count, mean, std (ddof = 1), max, total (= the last cumulative value).  count 0: the other four
 * are NaN (the groupby has no such group); count 1: std is NaN (as pandas).  cumulative (may be NULL) [dev] float64 [n,m_ref]:
 * the inclusive running sum per slot; where the flag is 0 the value of the frame before is carried (0 before the first row).
 * Cost: three launches (four with cumulative) and a scratch of vbs_series_chunks * m_ref * (VBS_SERIES_REC_COLS + 1) doubles
 * inside the handle - ALLOCATED AT THE FIRST CALL, sized by that call's n and m_ref (a gathered table is longer than a pass,
 * so max_batch says nothing about it), kept, and grown only when a larger call arrives (hipFree + hipMalloc: synchronises
 * the device; VBS_ENOMEM under stream capture).  A repeated call of the same or a smaller shape allocates nothing.
 * vbs_window_means shares that scratch (n_windows * ceil(longest window / VBS_SERIES_CHUNK) * m_ref * 4 doubles).
 * vbs_series_stats_f64: the same on a float64 disp (as vbs_displacement_f64 writes it), no handle; scratch [dev] = that many
 * doubles, provided by the caller.
 * vbs_series_partial / vbs_series_merge: the two halves, for a sequence whose disp is spread over ranks.  partial: records
 * [dev] float64 [vbs_series_chunks,m_ref,VBS_SERIES_REC_COLS] = count, mean, M2, max, sum of every chunk the frames
 * [frame_begin, frame_begin + n) touch (a chunk cut by the call's first or last frame gives a record of its part).  merge:
 * n_records records IN FRAME ORDER (any mix of whole and cut chunks; records of count 0 are skipped, so padding changes no
 * bit) -> stats as above, and prefix (may be NULL) [dev] float64 [n_records,m_ref] = the sum of the records before each.
 * vbs_series_chunks (host only): the number of records of such a call; VBS_EINVAL for n < 1 or frame_begin < 0. */
#define VBS_SERIES_CHUNK    32
#define VBS_SERIES_REC_COLS 5   /* count, mean, M2 (sum of squared deviations), max, sum */
#define VBS_STATS_COLS      5   /* count, mean, std (ddof = 1), max, total               */
#define VBS_WINDOW_COLS     4   /* count, mean X, mean Y, mean Z                         */
int vbs_series_chunks(int n, int frame_begin);
int vbs_series_stats(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* stats, double* cumulative,
                     void* stream);
int vbs_series_stats_f64(int device, const double* disp, int n, int m_ref, int frame_begin, double* stats, double* cumulative,
                         double* scratch, void* stream);
int vbs_series_partial(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* records, void* stream);
int vbs_series_merge(vbs_handle* h, const double* records, int n_records, int m_ref, double* stats, double* prefix,
                     void* stream);
/* calculate_average_coordinates (LocalAnalysis.py:53-60): for each of n_windows frame windows [a, b] - INCLUSIVE indices into
 * the table's frames, windows = HOST int32 [n_windows][2] - per slot the number of rows with VBS_FLAG_XYZ and the float64 mean
 * of their X, Y, Z (cols 6-8): means [dev] float64 [n_windows,m_ref,VBS_WINDOW_COLS]; NaN means at count 0 (the reference's
 * groupby has no such marker, its inner merge :81 drops it).  A window outside [0, n) or with a > b: VBS_EINVAL. */
int vbs_window_means(vbs_handle* h, const float* table, int n, int m_ref, const int32_t* windows, int n_windows, double* means,
                     void* stream);
/* MarkerDisplacement.py:158-173 (SCALAR mode: the distance of a marker from its own position in frame 0) for every slot and
 * frame at once: out [dev] float64 [n,m_ref,2] = (flag, sqrt(dX^2 + dY^2 + dZ^2) against the slot's row in frame ref_frame);
 * flag = 1 where both rows carry VBS_FLAG_XYZ, else (0, 0).  ref_frame outside [0, n): VBS_EINVAL. */
int vbs_displacement_from_frame(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, double* out, void* stream);

/* ---- The dynamic polishing process (the reference's Figure 11; it ships no code for it): totals, FIR trend, residual --------
 * vbs_axis_displacement - the signed analogue of vbs_displacement_from_frame.  For every frame of [frame_begin, frame_end) of a
 * table holding frames [0, n) (the _range form of the other entries: what a rank calls on the gathered table for its shard) and
 * every slot: axis [dev] float64 [fe-fb, m_ref, VBS_AXIS_COLS] = (1, dX, dY, dZ) with d = (double)X - (double)X_ref (cols 6-8)
 * where this row and the slot's row in ref_frame both carry VBS_FLAG_XYZ, else (0, 0, 0, 0).  slot_mask [dev] uint8 [m_ref]
 * (may be NULL = all): a slot with mask 0 is treated as a slot whose flags are clear.  total [dev] float64 [fe-fb,
 * VBS_TOTAL_COLS] = complete, sum dX, sum dY, sum dZ, count over the slots with flag 1; complete = 1 when count equals the number
 * of selected slots valid in ref_frame and that number is >= 1 (a frame where a marker dropped out is not silently a smaller
 * sum).  THE ORDER OF SUMMATION IS PART OF THE INTERFACE: lane l of 64 adds slots l, l + 64, l + 128, ... in ascending order
 * (other slots add nothing), the 64 lane sums are folded a[i] + a[i + 32], then + 16, + 8, + 4, + 2, + 1.  No atomics.  axis or
 * total may be NULL (not both).  ref_frame outside [0, n), a range outside 0 <= fb <= fe <= n: VBS_EINVAL; fb == fe emits nothing.
 *
 * vbs_fir_series_f64 - a normalised zero-phase FIR along time with gaps, no handle.  rec [dev] float64 [n, s, cols], time-major:
 * col 0 the flag (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values < cols <= 8 (axis and total above are valid
 * inputs as they are: cols 4 resp. 5, n_values 3).  half HOST [n_half] = the centre tap, then the taps at distance 1 .. n_half-1:
 * the filter is w[k] = half[|k|], k = -h .. h, h = n_half - 1, SYMMETRIC BY CONSTRUCTION, which is what makes it zero-phase.
 * THE TAPS TRAVEL AS KERNEL ARGUMENTS (1 KB): the call allocates nothing and reads `half` before it returns.  For every frame
 * f of [frame_begin, frame_end) and every series, in ascending k and skipping (never multiplying by zero) the entries that are
 * invalid or outside [0, n) - they may hold NaN or anything else:
 *     num = sum w[k] x[f+k],   den = sum w[k],   sw = the same ascending sum of ALL w[k] (on the host)
 *     ok = valid[f] && den >= min_coverage * sw
 * out [dev] float64 [fe-fb, s, 1 + 2 n_values] = flag, filtered[n_values], residual[n_values]: flag = valid[f] + 2 ok (0, 1 or
 * 3); where ok, filtered = num / den and residual = x[f] - filtered, otherwise both are 0.  Float64 without contraction; an
 * output depends on its 2h + 1 inputs only - not on the tile (VBS_FIR_TILE frames x 64 series a workgroup, stated for tests of
 * its edges), on the range or on s.  n_half < 1, 2 n_half - 1 > VBS_FIR_MAX_TAPS, min_coverage outside (0, 1], sw <= 0, a bad
 * range, bad cols / n_values: VBS_EINVAL. */
#define VBS_FIR_MAX_TAPS 255   /* full length K = 2*n_half - 1, odd */
#define VBS_FIR_TILE     64    /* frames a workgroup emits (no result depends on it) */
#define VBS_AXIS_COLS    4     /* flag, dX, dY, dZ                                   */
#define VBS_TOTAL_COLS   5     /* complete, sum dX, sum dY, sum dZ, count            */
int vbs_axis_displacement(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, const uint8_t* slot_mask,
                          int frame_begin, int frame_end, double* axis, double* total, void* stream);
int vbs_fir_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half,
                       double min_coverage, int frame_begin, int frame_end, double* out, void* stream);

/* ---- The probe-indentation validation (the reference's Figure 6(b); it ships no code for it): steps, dwells, step error ---------
 * Three entries without a handle on the record layout vbs_fir_series_f64 takes: rec [dev] float64 [n, s, cols], time-major, col 0
 * the flag (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values < cols <= 8.  Float64 without contraction, no atomics;
 * invalid entries are selected out and never multiplied (they may hold NaN).  No result depends on the launch shape, on a tile
 * boundary or on s.  THE DEFINITIONS AND THE ORDER OF EVERY SUM ARE PART OF THE INTERFACE.
 *
 * vbs_step_response_f64 - a step detector: the difference of two one-sided means.  1 <= min_count <= w <= VBS_STEP_MAX_WINDOW.
 * For frame f the left window is the valid frames g of [f-w, f) within [0, n), the right window the valid frames g of [f, f+w)
 * within [0, n); their populations are cl and cr, and ok = cl >= min_count && cr >= min_count.  Per value v each sum starts at
 * 0.0 and adds in ascending g, one add per valid frame: EVERY OUTPUT ADDS ITS OWN WINDOWS (no running sum: it would change the
 * bits and drift).  r_v = SR_v / cr - SL_v / cl;  score = sum of r_v * r_v in ascending v from 0.0.  The score stays squared: no
 * square root enters a decision.  out [dev] float64 [n, s, 2 + n_values] = (ok, score, r_1 .. r_nv), all zero where !ok.
 *
 * vbs_find_steps_f64 - the peaks of that response.  Only columns 0 (ok) and 1 (score) of resp [dev] float64 [n, s, resp_cols]
 * are read, 2 <= resp_cols <= 9; thr2 is the SQUARED threshold, a double computed by the caller (NaN or negative: VBS_EINVAL).
 * Frame f is a step of series i when ok[f], score[f] >= thr2, and for every g of [f-w, f+w] within [0, n), g != f, with ok[g]:
 * score[g] < score[f] when g < f and score[g] <= score[f] when g > f - so the earliest of equal maxima wins.  A NaN score is
 * never a step and never suppresses one.  steps [dev] int32 [s, 1 + max_steps], 1 <= max_steps <= VBS_STEP_MAX_STEPS: column 0
 * the number of steps found - it MAY EXCEED max_steps, which is how the caller sees an overflow: a per-series result, not an
 * error of the call - then the first min(count, max_steps) frames in ascending order, then -1.  The order is ascending by
 * construction (a workgroup walks the frames of its 64 series in order); no atomics decide it.
 *
 * vbs_dwell_stats_f64 - the statistics between the steps.  steps [dev] int32 [steps_rows, 1 + max_steps] as above; steps_rows
 * is s (each series has its own steps) or 1 (one list shared by all series); guard >= 0.  With k = min(count, max_steps)
 * (a negative count reads as 0) and the change frames c_0 < .. < c_{k-1}, dwell j of [0, k] covers [begin, end):
 * begin = j == 0 ? 0 : c_{j-1} + guard, end = j == k ? n : c_j - guard, both clipped to [0, n], then end = max(end, begin).
 * out [dev] float64 [s, max_steps + 1, 3 + 2 n_values] = (begin, end, count, mean_v .., M2_v ..).  One wave per (series, dwell):
 * lane l of 64 adds the valid frames begin + l, begin + l + 64, .. in ascending order from 0.0, the 64 lane sums are folded
 * a[i] + a[i + 32], then + 16, + 8, + 4, + 2, + 1 (the rule of vbs_axis_displacement's totals); mean = S / count; a second pass
 * in the same order gives M2 = sum of (x - mean)^2.  count == 0: mean is NaN and M2 is 0.  Rows j > k are (-1, -1, 0, NaN ..).
 * std = sqrt(M2 / (count - 1)) is the caller's (NaN below two frames).
 * All three: a null pointer, n < 1, s < 1, bad cols / n_values or a limit above broken: VBS_EINVAL, decided before the device
 * is touched. */
#define VBS_STEP_MAX_WINDOW 64
#define VBS_STEP_MAX_STEPS  64
int vbs_step_response_f64(int device, const double* rec, int n, int s, int cols, int n_values, int window, int min_count,
                          double* out, void* stream);
int vbs_find_steps_f64(int device, const double* resp, int n, int s, int resp_cols, int window, double thr2, int max_steps,
                       int32_t* steps, void* stream);
int vbs_dwell_stats_f64(int device, const double* rec, int n, int s, int cols, int n_values, const int32_t* steps, int steps_rows,
                        int max_steps, int guard, double* out, void* stream);

/* ---- Pose misalignment along a recording (ForceDistribution.py's deviation field and plane, for every frame): plane, tilt, trend ----
 * vbs_pose_series - what vbs_deviation_plane gives for four table rows, for every frame of [frame_begin, frame_end) of a table
 * holding frames [0, n), in float64, against a reference state that is given once.
 *   table [dev] float32 [n, m_ref, VBS_TABLE_COLS];  ref_disp [dev] float64 [m_ref, 4] = (flag, dX, dY, dZ): the displacement field
 *   of the reference state (one frame of vbs_axis_displacement's `axis` is a valid input as it is);  ref_xyz [dev] float64
 *   [m_ref, 3] reference positions;  slot_mask [dev] uint8 [m_ref] as vbs_axis_displacement's (may be NULL = all).
 * A slot r is COMMON in frame f when it is selected, ref_disp[r][0] != 0, and its rows in start_frame and in f both carry
 * VBS_FLAG_XYZ.  Where common, per axis (cols 6-8)  d = ((double)X_f - (double)X_start) - ref_disp[r],  the end point is
 * P = (ref_x + scale dX, ref_y + scale dY, (shell_mode ? ref_z : 0.0) + scale dZ)  and  |d| = sqrt(dX dX + dY dY + dZ dZ), added
 * left to right.  Nothing else of a slot is ever read into a sum: the XYZ of rows without the flag and ref_disp rows with flag 0
 * may hold NaN.
 *   deviation [dev] float64 [fe-fb, m_ref, 4] = (1, dX, dY, dZ) where common, else (0, 0, 0, 0)
 *   field [dev] float64 [fe-fb, VBS_POSEFIELD_COLS] = complete, count, the means of scale d and of |d| over the common slots
 *       (zeros at count 0); complete = 1 when count equals the number of selected slots valid in ref_disp and in start_frame and
 *       that number is >= 1.  `field` is always over ALL common slots
 *   pose [dev] float64 [fe-fb, VBS_POSE_COLS] = flag, a, b, c, tilt_deg, azimuth_deg, rms, n_used
 * Any of the three may be NULL (not all).  EVERY SUM FOLLOWS THE RULE OF vbs_axis_displacement, WHICH IS PART OF THE INTERFACE:
 * lane l of 64 adds slots l, l + 64, ... in ascending order (other slots add nothing - selected, never multiplied by zero), the
 * 64 lane sums are folded a[i] + a[i + 32], then + 16, 8, 4, 2, 1.  No atomics, float64 without contraction: no result depends
 * on the launch shape, on the range or on VBS_POSE_GROUP (the frames a workgroup takes: stated for tests of its edges).
 * The plane, with the formulas of vbs_deviation_plane: the means (mx, my, mz) of P; the centred sums xx, xy, yy, xz, yz, recomputed
 * from the table (never from a rounded output); det = xx yy - xy xy; a plane exists iff count >= 3 and |det| > 1e-300;
 * a = (xz yy - yz xy) / det, b = (yz xx - xz xy) / det, c = mz - a mx - b my.  The residual of a slot on the centred coordinates is
 * r = z - (a x + b y), SSR = the sum of r r by the same rule, rms = sqrt(SSR / n_used), tilt_deg = atan(sqrt(a a + b b)) and
 * azimuth_deg = atan2(b, a), both times 57.29577951308232 (the azimuth is the steep direction: where the plane rises).
 * One round of outlier rejection, only when reject_k > 0, a plane exists and SSR > 0: the common slots with
 * r r <= (reject_k reject_k) (SSR / count) are kept (squared: no square root decides).  If fewer are kept than are common and the
 * kept set still gives a plane (kept >= 3, |det| > 1e-300 of its own centred sums), means, sums, plane and SSR are those of the
 * kept set, n_used = kept and flag = 2; otherwise the first plane stands with n_used = count and flag = 1.  flag = 0: no plane;
 * a .. rms are 0 and n_used = count.  A nonzero flag is what vbs_fir_series_f64 reads as valid: `pose` seen as [F, 1, 8] with
 * n_values = 3 is a FIR input (a, b, c; angles are never filtered).
 * start_frame outside [0, n), a range outside 0 <= fb <= fe <= n, reject_k negative or not finite, scale not finite, m_ref < 1,
 * a shell_mode other than 0 / 1: VBS_EINVAL; fb == fe emits nothing.  The call allocates nothing. */
#define VBS_POSE_COLS      8   /* flag, a, b, c, tilt_deg, azimuth_deg, rms, n_used                     */
#define VBS_POSEFIELD_COLS 6   /* complete, count, mean k dX, mean k dY, mean k dZ, mean |d|            */
#define VBS_POSE_GROUP     8   /* frames a workgroup takes, one wave each (no result depends on it)     */
int vbs_pose_series(vbs_handle* h, const float* table, int n, int m_ref, int start_frame, const double* ref_disp,
                    const double* ref_xyz, const uint8_t* slot_mask, int shell_mode, double scale, double reject_k, int frame_begin,
                    int frame_end, double* deviation, double* field, double* pose, void* stream);

/* ---- Contact maps along a recording (the reference's Figure 4(c) stops at arrows on the markers; it ships no code for this) ----
 * The spatial counterpart of vbs_fir_series_f64: a gap-aware, normalised kernel smoother in space, for every frame of a recording
 * in one launch, and the contact patch of every resulting map.  Two entries without a handle.  The operator, the coverage rule
 * and the patch definition are this project's.
 *
 * vbs_field_map_f64 - rec [dev] float64 [n, s, cols], time-major, the record layout vbs_fir_series_f64 takes: col 0 the flag
 * (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values <= 3, n_values < cols <= 8 (one range of
 * vbs_axis_displacement's `axis` and vbs_pose_series's `deviation` are valid inputs as they are).  W [dev] float64 [P, s],
 * row-major: the non-negative weight of slot m at grid point p, computed by the caller (as the FIR's taps are: no exp of the
 * device enters a result).  wsum [dev] float64 [P]: the caller's full row sums.  For frame f of [frame_begin, frame_end) and grid
 * point p, over the VALID slots only:
 *     den = sum W[p,m],   num_v = sum W[p,m] x_v[f,m],   ok = den > 0 && den >= min_coverage * wsum[p]
 * map [dev] float64 [fe-fb, P, 1 + n_values] = (ok, num_v / den ..), all zeros where !ok.  Invalid entries are selected out when
 * they are staged, never multiplied by zero: they may hold NaN or 1e300, and so may every column beyond n_values.
 * The kernel is a float64 matrix product on v_mfma_f64_16x16x4_f64: a tile is 16 grid points x 16 columns = VBS_FIELD_FRAMES
 * frames x (x1, x2, x3, flag as 1.0 / 0.0); padding is selected zeros, never a read past s or P.  No atomics.
 * THE ORDER OF SUMMATION IS NOT PART OF THIS INTERFACE (unlike the entries above): the order inside the matrix instruction is not
 * documented, and nothing rests on it.  What is promised instead:
 *   - exact where the inputs make every order exact: if every product and every partial sum is representable, num and den are
 *     exact and the quotient is the correctly rounded one;
 *   - otherwise, with u = 2^-53, gamma_k = k u / (1 - k u), A = sum W |x_v| and d = sum W over the valid slots:
 *     |value - num / den| <= (2 gamma_(s+6) + 2 u) A / d, for any order of summation, with or without fused multiply-add
 *     (derived in DESIGN 4.14);
 *   - bit-identical under every change of batching: run to run, range by range, a frame alone or at any position of a tile, and
 *     with dead (invalid) slots appended.  No result depends on how many frames a workgroup takes.
 * A null pointer, n, s or P < 1, bad cols / n_values, min_coverage outside (0, 1], a range outside 0 <= fb <= fe <= n:
 * VBS_EINVAL; s > VBS_FIELD_MAX_SLOTS or P > VBS_FIELD_MAX_POINTS: VBS_ECAPACITY; all decided before the device is touched.
 * fb == fe emits nothing.  The call allocates nothing.
 *
 * vbs_patch_stats_f64 - the contact patch of every frame of a map.  map [dev] float64 [F, P, 1 + n_values] as above, grid_xy
 * [dev] float64 [P, 2]; component 0 .. n_values-1, or -1 for the squared norm; sign +1 or -1; thr >= 0, for component -1 the
 * SQUARED threshold, computed by the caller.  A point is COVERED when its flag is nonzero.  Its score is sign * v_component; for
 * component -1 it is v1 v1 + v2 v2 + v3 v3 (the values there are), added left to right.  It is IN THE PATCH when it is covered and
 * score >= thr; a NaN score is never in the patch.
 * patch [dev] float64 [F, VBS_PATCH_COLS] = flag, covered, count, S, cx, cy, peak, peak_index:  S = sum score,
 * cx = (sum score gx) / S, cy = (sum score gy) / S over the patch; peak = the largest score in the patch and peak_index its p,
 * the smallest p among equal maxima.  flag 0: nothing is covered, everything else is 0.  flag 1: covered, but the patch is empty
 * or S <= 0: cx, cy, peak are 0 and peak_index is -1.  flag 2: a patch with a centre.
 * EVERY SUM FOLLOWS THE RULE OF vbs_axis_displacement, WHICH IS PART OF THE INTERFACE: lane l of 64 adds points l, l + 64, ... in
 * ascending order (selected, never multiplied by zero), the 64 lane sums are folded a[i] + a[i + 32], then + 16, 8, 4, 2, 1; the
 * peak folds the same way.  One wave per frame, VBS_PATCH_GROUP frames a workgroup, no result depending on it; float64 without
 * contraction, no atomics.  A null pointer, F or P < 1, n_values outside 1..3, a component outside -1 .. n_values-1, a sign other
 * than +-1, thr NaN or negative: VBS_EINVAL; P > VBS_FIELD_MAX_POINTS: VBS_ECAPACITY; decided before the device is touched. */
#define VBS_FIELD_FRAMES     4       /* frames of a 16-column tile: 4 x (x1, x2, x3, flag)                  */
#define VBS_FIELD_MAX_SLOTS  1024    /* s at most (the cap of max_markers)                                   */
#define VBS_FIELD_MAX_POINTS 65536   /* P at most                                                            */
#define VBS_PATCH_COLS       8       /* flag, covered, count, S, cx, cy, peak, peak_index                    */
#define VBS_PATCH_GROUP      8       /* frames a workgroup takes, one wave each (no result depends on it)    */
int vbs_field_map_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* W, const double* wsum,
                      int P, double min_coverage, int frame_begin, int frame_end, double* map, void* stream);
int vbs_patch_stats_f64(int device, const double* map, int F, int P, int n_values, const double* grid_xy, int component,
                        double sign, double thr, double* patch, void* stream);

/* ---- Displacement spectra along a recording (the reference's Figure 11(b) shows the oscillation; it ships no code for this) ----
 * The bonnet spins and precesses, so every marker's displacement is periodic.  A gap-aware least-squares fit of
 * x ~ c0 + a cos(theta) + b sin(theta) at every frequency of a list the caller chooses (a zoom grid round the spindle line,
 * harmonics), in two entries without a handle: a gap-aware projection of every series onto a basis given by the caller, and a
 * small kernel that turns those projections into fits and peaks.  Operator, conditioning rule and peak rule are this project's
 * (DESIGN 4.15, 7).  A full-band spectrum on the natural grid q / n is an FFT's job; this is the tool for a BAND of Q << n
 * frequencies at arbitrary real values.
 *
 * vbs_project_series_f64 - rec [dev] float64 [n, s, cols], time-major, the record layout vbs_fir_series_f64 takes: col 0 the flag
 * (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values <= 3, n_values < cols <= 8 (one range of vbs_axis_displacement's
 * `axis` or `total`, of vbs_pose_series's `deviation`, or a FIR output's residual columns repacked, are valid inputs).  basis [dev]
 * float64 [R, n], row-major, finite, computed by the caller (as the FIR's taps and the smoother's weights are: no sin / cos of the
 * device enters a result).  For slot i and basis row r, over the VALID frames only:
 *     den = sum basis[r,f],   num_v = sum basis[r,f] x_v[f,i]
 * proj [dev] float64 [s, R, 1 + n_values] = (den, num_1 ..), SERIES-MAJOR: the projections of a series are contiguous, which is
 * what vbs_harmonic_fit_f64 and a user read.  Invalid entries are selected out when they are staged, never multiplied by zero:
 * they may hold NaN or 1e300, and so may every column beyond n_values.  A series with no valid frame gives exact zeros.
 * The kernel is a float64 matrix product on v_mfma_f64_16x16x4_f64 with the frame axis as K: a tile is 16 basis rows x 16
 * columns = VBS_PROJ_SLOTS slots x (x1, x2, x3, flag as 1.0 / 0.0), so the flag column's product IS den; padding (frames >= n
 * inside a chunk, rows >= R, slots >= s, columns >= n_values) is selected zeros, never a read past n, R or s.  No atomics and NO
 * SPLIT OF K ACROSS WORKGROUPS: every output is one accumulator chain over the frames, chunk after chunk of VBS_PROJ_CHUNK in
 * ascending order from frame 0, so a result depends on its own basis row and its own series only.
 * THE ORDER OF SUMMATION IS NOT PART OF THIS INTERFACE, as for vbs_field_map_f64.  What is promised instead:
 *   - exact where the inputs make every order exact: if every product and every partial sum is representable, num and den are
 *     exact;
 *   - otherwise, with u = 2^-53, gamma_k = k u / (1 - k u), over the valid frames:
 *     |num^ - num| <= gamma_(n+6) sum |basis x_v|   and   |den^ - den| <= gamma_(n+6) sum |basis|,
 *     for any order of summation, with or without fused multiply-add (derived in DESIGN 4.15);
 *   - bit-identical run to run, a basis row alone against the same row among R, a series alone against the same series among s,
 *     with dead (invalid) slots appended and with dead frames appended at the end (zero-selected entries add exact zeros).
 * A null pointer, n, s or R < 1, bad cols / n_values: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES, s > VBS_PROJ_MAX_SLOTS or
 * R > VBS_PROJ_MAX_ROWS: VBS_ECAPACITY; a bad argument comes before a capacity; all decided before the device is touched.  The
 * call allocates nothing.
 *
 * vbs_harmonic_fit_f64 - reads a proj [dev] float64 [s, R, 1 + n_values] whose basis had R == 1 + 4 Q rows in this order: row 0
 * all ones; rows 1 + 2q, 2 + 2q the cos and sin of 2 pi nu_q f; rows 1 + 2Q + 2q, 2 + 2Q + 2q the cos and sin of 2 pi (2 nu_q) f.
 * Per slot i, with N = proj[i,0,0] (the number of valid frames, an exact integer), per value v, m = proj[i,0,v] / N, and per bin q:
 *     c1, s1 = den of rows 1+2q, 2+2q        c2, s2 = den of rows 1+2Q+2q, 2+2Q+2q
 *     CC = 0.5 * (N + c2) - (c1 * c1) / N    SS = 0.5 * (N - c2) - (s1 * s1) / N    CS = 0.5 * s2 - (c1 * s1) / N
 *     det = CC * SS - CS * CS                ok = N >= min_count && det > det_min * (N * N)
 *     pc = num_v(row 1+2q) - m * c1          ps = num_v(row 2+2q) - m * s1
 *     a = (pc * SS - ps * CS) / det          b = (ps * CC - pc * CS) / det          p = a * pc + b * ps
 * the floating-mean least-squares fit solved by elimination; p is the drop in the sum of squares; the half-angle identities stand
 * in for sum cos^2, sum sin^2, sum cos sin over the valid frames, which is why the 2 nu rows travel.  EVERY EXPRESSION IS EVALUATED
 * AS WRITTEN, FLOAT64 WITHOUT CONTRACTION, AND THAT IS PART OF THIS INTERFACE; nothing here runs on a matrix instruction.  No
 * square root and no atan2: amplitude hypot(a, b) and phase degrees(atan2(b, a)) (x ~ A cos(theta - phi)) are the caller's, as
 * std is in vbs_dwell_stats_f64.
 * fit (may be NULL) [dev] float64 [s, Q, 1 + 3 n_values] = ok, then (a, b, p) per value; all zeros where !ok.
 * peak (may be NULL; not both) [dev] float64 [s, n_values, VBS_PEAK_COLS] = flag, N, mean, bin, a, b, p: the bin is the ok bin
 * with the largest p; a NaN p never wins and never suppresses; the smallest q wins among equal maxima.  flag 2: a peak.  flag 1:
 * N >= min_count but no ok bin with a non-NaN p: bin -1, a, b, p are 0.  flag 0: N < min_count: mean 0, bin -1, a, b, p 0.
 * One wave per slot, VBS_FIT_GROUP slots a workgroup (no result depends on it); lane l of 64 takes bins l, l + 64, .. ascending,
 * the peak folds 32, 16, 8, 4, 2, 1 with the tie rule, as vbs_patch_stats_f64 folds its peak.
 * min_count < 3, det_min outside [0, 0.25), Q < 1 or above (VBS_PROJ_MAX_ROWS - 1) / 4, s < 1, R != 1 + 4 Q, n_values outside 1..3, a null proj, fit and peak both
 * null: VBS_EINVAL, decided before the device is touched. */
#define VBS_PROJ_SLOTS      4        /* slots of a 16-column tile: 4 x (x1, x2, x3, flag)                    */
#define VBS_PROJ_CHUNK      64       /* frames staged at a time (no result depends on it)                    */
#define VBS_PROJ_ROWS       64       /* basis rows a workgroup takes (no result depends on it)               */
#define VBS_PROJ_WG_SLOTS   16       /* slots a workgroup takes (no result depends on it)                    */
#define VBS_PROJ_MAX_ROWS   8192     /* R at most (Q = 2047 bins)                                            */
#define VBS_PROJ_MAX_FRAMES 1048576  /* n at most                                                            */
#define VBS_PROJ_MAX_SLOTS  1024     /* s at most (the cap of max_markers); the total series has s = 1       */
#define VBS_FIT_GROUP       4        /* slots a workgroup of the fit takes, one wave each                    */
#define VBS_PEAK_COLS       7        /* flag, N, mean, bin, a, b, p                                          */
int vbs_project_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* basis, int R,
                           double* proj, void* stream);
int vbs_harmonic_fit_f64(int device, const double* proj, int s, int R, int n_values, int Q, int min_count, double det_min,
                         double* fit, double* peak, void* stream);

/* ---- Shear, torsion and strain along a recording (the reference's Figure 4(c) stops at arrows; it ships no code for this) ----
 * How a marker's displacement depends on where the marker sits: the affine part of the displacement field of every frame (drag,
 * twist about the normal, dilation, shear, tilt of dZ), what is left once that smooth motion is removed, and the same fit over
 * the neighbourhood of every marker.  Two entries without a handle, on the record layout of vbs_fir_series_f64.  The operator,
 * the conditioning rule, the rejection and `worst` are this project's.
 *
 * vbs_motion_series_f64 - rec [dev] float64 [n, s, cols], 4 <= cols <= 8: col 0 the flag (nonzero = valid), cols 1 .. 3 dX, dY, dZ
 * (vbs_axis_displacement's `axis` and vbs_pose_series's `deviation` are valid inputs as they are).  pos [dev] float64 [s, 2]: the
 * rest position (x, y) of every slot.  slot_mask [dev] uint8 [s] as vbs_axis_displacement's (may be NULL = all).  A slot is USED
 * in frame f when it is selected and its flag is nonzero.  Nothing else of a slot is ever read into a sum: invalid entries,
 * columns >= 4 and the pos of unselected slots may hold NaN or 1e300.
 * EVERY SUM FOLLOWS THE RULE OF vbs_axis_displacement, WHICH IS PART OF THE INTERFACE: lane l of 64 adds slots l, l + 64, ... in
 * ascending order (selected, never multiplied by zero), the 64 lane sums are folded a[i] + a[i + 32], then + 16, 8, 4, 2, 1.
 * Float64 without contraction, no atomics: no result depends on the launch shape, on the range or on VBS_MOTION_GROUP.
 * The fit over the used slots, for k = X, Y, Z: the means mx, my of pos and md_k of d_k; on the centred values x = px - mx,
 * y = py - my, e_k = d_k - md_k the sums xx, xy, yy, xe_k, ye_k, recomputed from rec (never from a rounded output);
 * det = xx yy - xy xy; a fit exists iff count >= 3 and |det| > 1e-300 (the rule of vbs_pose_series);
 *     g_kx = (xe_k yy - ye_k xy) / det     g_ky = (ye_k xx - xe_k xy) / det     t_k = md_k - g_kx mx - g_ky my
 * (left to right: the model's displacement at the origin of pos, as c is in the pose).  The residual of a slot is
 * r_k = e_k - (g_kx x + g_ky y), q = r_X r_X + r_Y r_Y + r_Z r_Z added left to right, SSR_k = the sum of r_k r_k by the rule and
 * SSR = (SSR_X + SSR_Y) + SSR_Z.
 * One round of outlier rejection, exactly as vbs_pose_series: only when reject_k > 0, a fit exists and SSR > 0, the used slots
 * with q <= (reject_k reject_k) (SSR / count) are kept.  If fewer are kept than are used and the kept set gives a fit of its own
 * (kept >= 3, |det| > 1e-300 of its own centred sums), everything is the kept set's, flag = 2 and n_used = kept; otherwise the
 * first fit stands with flag = 1 and n_used = count.  flag = 0: no fit; everything else of the row is 0 (worst: -1) and
 * n_used = count.
 *   grad [dev] float64 [fe-fb, 3, 4] = (flag, t_k, g_kx, g_ky) for k = X, Y, Z: a FIR record as it is (s = 3, cols = 4,
 *       n_values = 3)
 *   strain [dev] float64 [fe-fb, VBS_STRAIN_COLS].  With F = I + the in-plane block, F11 = 1 + g_Xx, F12 = g_Xy, F21 = g_Yx,
 *       F22 = 1 + g_Yy, and DEG = 57.29577951308232:
 *        0 - 2   flag, count, n_used
 *        3       dilation = g_Xx + g_Yy
 *        4       omega = 0.5 (g_Yx - g_Xy), the linearised torsion in radians
 *        5, 6    e1 = 0.5 (g_Xx - g_Yy), e2 = 0.5 (g_Xy + g_Yx)
 *        7       max_shear = sqrt(e1 e1 + e2 e2)
 *        8       shear_deg = 0.5 atan2(e2, e1) DEG
 *        9       rot_deg = atan2(q_, p_) DEG, p_ = F11 + F22, q_ = F21 - F12: the rotation of the polar decomposition, any angle
 *        10, 11  lambda1 = 0.5 (h + w), lambda2 = 0.5 (h - w), h = sqrt(p_ p_ + q_ q_), w = sqrt(a_ a_ + b_ b_), a_ = F11 - F22,
 *                b_ = F12 + F21: the principal stretches
 *        12      tilt_deg = atan(sqrt(g_Zx g_Zx + g_Zy g_Zy)) DEG
 *        13, 14  rms_inplane = sqrt((SSR_X + SSR_Y) / n_used), rms_z = sqrt(SSR_Z / n_used)
 *        15      worst = the slot with the largest q among the slots of the final fit (-1: no fit); the smallest index wins among
 *                equals, a NaN never wins; it folds as vbs_patch_stats_f64's peak
 *   residual [dev] float64 [fe-fb, s, 4] = (1 kept or 2 rejected, r_X, r_Y, r_Z) for every used slot against the FINAL fit's
 *       means and gradient; zeros where the slot is not used or there is no fit.  Both flags are nonzero: a valid rec of
 *       vbs_fir_series_f64, vbs_field_map_f64, vbs_project_series_f64 and the step entries (the non-affine part)
 * Any of the three may be NULL (not all).  A null rec or pos, n or s < 1, cols outside 4 .. 8, reject_k negative or not finite, a
 * range outside 0 <= fb <= fe <= n: VBS_EINVAL; s > VBS_FIELD_MAX_SLOTS: VBS_ECAPACITY; a bad argument comes before a capacity;
 * all decided before the device is touched.  fb == fe emits nothing.  The call allocates nothing.
 *
 * vbs_local_strain_f64 - the same fit around every marker.  rec, pos as above (no mask).  nbr [dev] int32 [s, K],
 * 1 <= K <= VBS_STRAIN_MAX_NBR, computed by the caller: an entry outside [0, s) reads as "no neighbour" and is never an address;
 * duplicates are used as given.  The member list of slot i is i, nbr[i][0], .., nbr[i][K-1], in that order; a member is USED when
 * it is in range and its flag in frame f is nonzero.  THE ORDER IS PART OF THE INTERFACE: one thread adds the used members in
 * LIST order from 0.0, the means first, then the centred sums xx, xy, yy, xe_k, ye_k as above.  Slot i has a result iff i itself
 * is used, cnt >= min_count (3 <= min_count <= K + 1) and det > det_rel (xx yy), 0 <= det_rel < 1: det / (xx yy) is 1 - rho^2, so
 * det_rel refuses neighbourhoods close to a line without depending on the units.  Gradients by the formulas above.
 *   out [dev] float64 [fe-fb, s, VBS_LSTRAIN_COLS] = (cnt, dilation, omega, max_shear, e1, e2, g_Zx, g_Zy), zeros where there is no
 *       result.  cnt is nonzero: `out` with n_values = 3 is a valid rec of vbs_field_map_f64 (maps of local dilation, torsion and
 *       shear), and vbs_patch_stats_f64 with component 2 gives the shear zone
 * No atomics, no contraction: no result depends on the launch shape, on the range or on VBS_LSTRAIN_GROUP.  A null pointer, n or
 * s < 1, cols outside 4 .. 8, K, min_count or det_rel outside the ranges above, a range outside 0 <= fb <= fe <= n: VBS_EINVAL;
 * s > VBS_FIELD_MAX_SLOTS: VBS_ECAPACITY; decided before the device is touched.  fb == fe emits nothing. */
#define VBS_STRAIN_COLS    16  /* flag, count, n_used, dilation, omega, e1, e2, max_shear, shear_deg, rot_deg, lambda1, lambda2,
                                  tilt_deg, rms_inplane, rms_z, worst                                    */
#define VBS_LSTRAIN_COLS   8   /* cnt, dilation, omega, max_shear, e1, e2, g_Zx, g_Zy                    */
#define VBS_MOTION_GROUP   8   /* frames a workgroup takes, one wave each (no result depends on it)     */
#define VBS_LSTRAIN_GROUP  8   /* frames a workgroup takes, one after another (no result depends on it) */
#define VBS_STRAIN_MAX_NBR 12  /* K at most                                                             */
int vbs_motion_series_f64(int device, const double* rec, int n, int s, int cols, const double* pos, const uint8_t* slot_mask,
                          double reject_k, int frame_begin, int frame_end, double* grad, double* strain, double* residual,
                          void* stream);
int vbs_local_strain_f64(int device, const double* rec, int n, int s, int cols, const double* pos, const int32_t* nbr, int K,
                         int min_count, double det_rel, int frame_begin, int frame_end, double* out, void* stream);

/* ---- Despiking a tracked series (the reference has no temporal outlier handling; the operator and its rules are this project's) ----
 * The tracker takes the nearest detection within min_dist for every reference marker: a neighbour taken in a dropout, a merged
 * blob or a bad ellipse puts an isolated jump into one marker's series.  Every analysis above is gap-aware, so a spike only has to
 * become a gap; this entry finds it along time: a gap-aware rolling median with the median absolute deviation (the Hampel
 * identifier).  An order statistic has no order of summation: THE DEFINITIONS BELOW ARE THE INTERFACE, the algorithm is not.
 *
 * vbs_hampel_series_f64 - no handle.  rec [dev] float64 [n, s, cols], time-major, the record layout vbs_fir_series_f64 takes: col 0
 * the flag (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values < cols <= 8.  Invalid entries and the columns past the
 * values may hold NaN or anything else: they are selected out and never enter a comparison.  A VALID value must not be NaN; one
 * that is gives unspecified results in the windows that hold it, in those only, and no fault.
 * For frame f of [frame_begin, frame_end), series i and h = half_window (0 <= h <= VBS_ROBUST_MAX_HALF):
 *   window   the valid frames g of [f-h, f+h] within [0, n), f itself included when it is valid; c = its population
 *   judged   c >= min_count (1 <= min_count <= 2h + 1), whether or not f itself is valid
 *   order    for a value column v the candidates are ordered by (x, g): a before b when x_a < x_b, or x_a == x_b and a < b (so
 *            -0.0 and +0.0 tie and the earlier frame comes first); sorted as q_0 .. q_{c-1},
 *              med_v = q_{(c-1)/2}                      for odd c
 *              med_v = 0.5 q_{c/2-1} + 0.5 q_{c/2}      for even c: two products and one add, no contraction
 *   mad_v    the same statistic of d_g = |x_g - med_v| over the same window
 *   spike    thr = k_sigma * 1.4826, one IEEE product on the host.  Where f is valid and judged: dev_v = |x_{f,v} - med_v|,
 *            spike_v = dev_v > thr * mad_v && dev_v > min_scale; the entry is a spike when any v is.  min_scale is an absolute
 *            floor in the units of the data: a series quantised to a constant has mad = 0, and without the floor every sample
 *            off the median would be a spike
 * out [dev] float64 [fe-fb, s, 2 + 2 n_values] = flag, c, med[n_values], mad[n_values]; flag = valid + 2 judged + 4 spike (0, 1, 2,
 * 3 or 7); med and mad are 0 where the entry is not judged.  Flag 2: the marker is missing in the frame, and the median of its
 * neighbours is the value to fill the gap with.
 * clean [dev] float64 [fe-fb, s, cols] (may be NULL): the rows of rec copied BIT FOR BIT (NaN payloads of invalid cells included)
 * with col 0 set to 0.0 where the entry is a spike: a record vbs_fir_series_f64, vbs_field_map_f64, vbs_project_series_f64, the
 * step entries and vbs_motion_series_f64 take as it is.
 * An output depends on its window only: not on the tile (VBS_ROBUST_TILE frames x 64 series a workgroup, stated for tests of its
 * edges), the range, s or what else is in the batch.  No atomics.  A null rec or out, n or s < 1, bad cols / n_values, half_window
 * outside [0, VBS_ROBUST_MAX_HALF], min_count outside [1, 2h + 1], k_sigma not finite or <= 0, min_scale not finite or < 0, a range
 * outside 0 <= fb <= fe <= n: VBS_EINVAL, decided before the device is touched.  fb == fe emits nothing.  The call allocates
 * nothing. */
#define VBS_ROBUST_MAX_HALF 31   /* window 2h + 1 <= 63 */
#define VBS_ROBUST_TILE     64   /* frames a workgroup emits (no result depends on it) */
int vbs_hampel_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, int half_window, int min_count,
                          double k_sigma, double min_scale, int frame_begin, int frame_end, double* out, double* clean,
                          void* stream);

/* ---- Time-resolved amplitude and phase along a recording (the reference's Figure 11(b) shows the oscillation setting in, bursting
 * and settling; it ships no code for this) ----
 * The fit of vbs_harmonic_fit_f64, x ~ c0 + a cos(theta) + b sin(theta), in a SLIDING WINDOW at one known frequency nu, weighted
 * by a symmetric window w, in two entries without a handle: the weighted sums of every window, then a small kernel that turns them
 * into the fit of every frame.  Operator, window, coverage and conditioning rules are this project's.
 *
 * vbs_window_moments_f64 - rec [dev] float64 [n, s, cols], time-major, the record layout vbs_fir_series_f64 takes: col 0 the flag
 * (nonzero = valid), cols 1 .. n_values the values, 1 <= n_values <= 3, n_values < cols <= 8; the values of VALID entries are
 * finite with finite squares.  carrier [dev] float64 [4, n], row-major, finite, computed by the caller: rows c, s, c2, s2 = cos
 * and sin of 2 pi nu f and of 2 pi (2 nu) f at the GLOBAL frame f (no sin / cos of the device enters a result; any finite carrier
 * is taken).  half HOST [n_half]: the centre weight, then the weights at distance 1 .. h, h = n_half - 1, so w[k] = half[|k|],
 * symmetric by construction, exactly as the FIR's taps travel; 0 <= h <= VBS_ENV_MAX_HALF (2h + 1 <= VBS_FIR_MAX_TAPS), every
 * weight finite and >= 0, the centre > 0.  For every frame f of [frame_begin, frame_end) and every slot i the sums run over the
 * VALID frames j of [f - h, f + h] n [0, n), with w = w[j - f]: M = 5 + 4 n_values sums, in this column order:
 *     W = sum w    C1 = sum w c[j]    S1 = sum w s[j]    C2 = sum w c2[j]    S2 = sum w s2[j]
 *     per value v:   X = sum w x    XC = sum w (x c[j])    XS = sum w (x s[j])    XX = sum w (x x)
 * mom [dev] float64 [frame_end - frame_begin, s, M].  Invalid entries and frames outside [0, n) are selected out when they are
 * staged, never multiplied by zero: they may hold NaN or 1e300, and so may every column beyond n_values.  A window with no valid
 * frame gives exact zeros.  The call allocates nothing.
 * The kernel is a banded float64 matrix product on v_mfma_f64_16x16x4_f64: a tile is 16 output frames x 16 columns of the
 * flattened axis i M + m (the memory layout of mom), K the input frames, A[r][k] = w[k - r - h] inside the band and 0.0 outside
 * (which is why a valid value must be finite with a finite square: 0.0 times it must be 0.0), B the staged, selected terms, the
 * products x c, x s, x x rounded once each when staged.  Frame tiles are aligned to multiples of VBS_ENV_TILE of the GLOBAL frame
 * index, never to frame_begin.  No atomics.
 * THE ORDER OF SUMMATION IS NOT PART OF THIS INTERFACE, as for vbs_field_map_f64 and vbs_project_series_f64.  What is promised:
 *   - exact where the inputs make every order exact: if every product and every partial sum is representable, every sum is exact;
 *   - otherwise, with u = 2^-53, gamma_k = k u / (1 - k u), K = 2h + 1, every sum satisfies
 *         |sum^ - sum| <= gamma_(K+8) sum w |term|      (term = 1, c, s, c2, s2, x, x c, x s, x x; derived in DESIGN 4.18)
 *     for any order of summation, with or without fused multiply-add;
 *   - bit-identical run to run, range by range (any frame_begin, frame_end) against the full call, a series alone against the same
 *     series among s, with dead (invalid) slots appended and with dead frames appended at the end.
 * A null pointer, n or s < 1, bad cols / n_values, n_half < 1 or h > VBS_ENV_MAX_HALF, a negative or non-finite weight, a centre
 * <= 0, a range outside 0 <= fb <= fe <= n: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES or s > VBS_PROJ_MAX_SLOTS: VBS_ECAPACITY; a bad
 * argument comes before a capacity; all decided before the device is touched.  fb == fe emits nothing.
 *
 * vbs_window_fit_f64 - mom [dev] float64 [F, s, M = 5 + 4 n_values] as above; sw = the ascending sum of all 2h + 1 weights
 * (finite, > 0; the caller's, on the host), min_coverage in (0, 1], det_min in [0, 0.25).  Per (frame, slot), then per value:
 *     CC = 0.5 * (W + C2) - (C1 * C1) / W    SS = 0.5 * (W - C2) - (S1 * S1) / W    CS = 0.5 * S2 - (C1 * S1) / W
 *     det = CC * SS - CS * CS                ok = W > 0 && W >= min_coverage * sw && det > det_min * (W * W)
 *     m = X / W     pc = XC - m * C1     ps = XS - m * S1
 *     a = (pc * SS - ps * CS) / det          b = (ps * CC - pc * CS) / det          p = a * pc + b * ps
 *     c0 = m - (a * C1 + b * S1) / W         M2 = XX - m * X
 * the weighted floating-mean fit of vbs_harmonic_fit_f64 with W in the place of N (the half-angle identities hold under weights,
 * which is why c2 and s2 travel); p is the drop in the weighted sum of squares M2.  EVERY EXPRESSION IS EVALUATED AS WRITTEN,
 * FLOAT64 WITHOUT CONTRACTION (min_coverage * sw one product on the host), AND THAT IS PART OF THIS INTERFACE.  A comparison with
 * a NaN is false, so a NaN W or det is not ok.  No square root and no atan2: amplitude and phase are the caller's.  M2 cancels
 * where the mean dwarfs the oscillation: feed residuals.
 * fit [dev] float64 [F, s, 1 + 5 n_values] = ok (1.0 / 0.0), then (a, b, p, c0, M2) per value; all zeros where !ok.  The flag
 * makes fit a record that vbs_field_map_f64, vbs_fir_series_f64 and the step entries take as it is.  One thread per (frame, slot).
 * A null pointer, F or s < 1, n_values outside 1..3, sw not finite or <= 0, min_coverage outside (0, 1], det_min outside [0, 0.25):
 * VBS_EINVAL; F > VBS_PROJ_MAX_FRAMES or s > VBS_PROJ_MAX_SLOTS: VBS_ECAPACITY, after the arguments; before the device is touched. */
#define VBS_ENV_TILE     64      /* frames a workgroup emits (no result depends on it)          */
#define VBS_ENV_MAX_HALF 127     /* h at most: a window of 2h + 1 <= VBS_FIR_MAX_TAPS frames     */
int vbs_window_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* carrier,
                           const double* half, int n_half, int frame_begin, int frame_end, double* mom, void* stream);
int vbs_window_fit_f64(int device, const double* mom, int F, int s, int n_values, double sw, double min_coverage, double det_min,
                       double* fit, void* stream);

/* ---- Marker velocity, acceleration and gap filling along a recording (slip, approach speed, first contact and the direction
 * reversal of Figure 11(b) are statements about rates; the reference ships no code for this) ----
 * A gap-aware weighted local polynomial fit along time - Savitzky-Golay with the gaps selected out, one-sided at the ends of the
 * recording - in two entries without a handle: the moments of every window, then a small kernel that turns them into the fit of
 * every frame.  Its constant term is the smoothed position (the gap filler), its linear term the velocity, its quadratic term the
 * acceleration.  Operator, scaling, fallback rule and every default are this project's.
 *
 * The taps.  h = n_half - 1 in 0 .. VBS_KIN_MAX_HALF, degree d in 0 .. VBS_KIN_MAX_DEGREE, H = the smallest power of two >=
 * max(h, 1), u = delta / H (an exact scaling), w[delta] = half[|delta|] as for vbs_window_moments_f64 (finite, >= 0, centre > 0):
 *     taps[k][delta] = w[delta] * u^k        k = 0 .. 2d, delta = -h .. h
 * u^k by repeated multiplication, every product exact (|delta|^k < 2^42), so a tap is rounded ONCE (`filters.poly_taps`).
 *
 * vbs_poly_moments_f64 - rec [dev] float64 [n, s, cols], the record layout of vbs_fir_series_f64: col 0 the flag (nonzero =
 * valid), cols 1 .. n_values the values, 1 <= n_values <= 3, n_values < cols <= 8; the values of VALID entries are finite with
 * finite squares.  For every frame f of [frame_begin, frame_end) and every slot the sums run over the VALID frames j of
 * [f - h, f + h] n [0, n), delta = j - f: M = (2d + 1) + (d + 2) n_values sums, in this column order:
 *     S_k = sum taps[k][delta]                      k = 0 .. 2d
 *     per value:   X_k = sum taps[k][delta] x_j     k = 0 .. d,     XX = sum taps[0][delta] (x_j x_j)
 * the square rounded once when it is staged, no contraction.  mom [dev] float64 [frame_end - frame_begin, s, M].  Invalid entries
 * and frames outside [0, n) are selected out before anything is computed from them, never multiplied by zero: they may hold NaN
 * or 1e300, and so may every column beyond n_values.  A window with no valid frame gives exact zeros.  The call allocates nothing.
 * The kernel is a banded float64 matrix product on v_mfma_f64_16x16x4_f64 with SEVERAL bands over ONE staged operand: B, staged
 * once per input frame, is (valid, x1, x2, x3) of 4 slots a tile, their squares, and a tile of 16 slots' flags for the orders
 * k > d; each tap row is its own Toeplitz A, A_k[r][j] = taps[k][j - r - h] inside the band and 0.0 outside (which is why a valid
 * value must be finite with a finite square: 0.0 times it must be 0.0), each product into its own accumulator.  Frame tiles are
 * aligned to multiples of VBS_KIN_TILE of the GLOBAL frame index, never to frame_begin.  No atomics.
 * THE ORDER OF SUMMATION IS NOT PART OF THIS INTERFACE, as for vbs_window_moments_f64.  What is promised:
 *   - exact where the inputs make every order exact: if every product and every partial sum is representable, every sum is exact;
 *   - otherwise, with u = 2^-53, gamma_k = k u / (1 - k u), K = 2h + 1, every sum satisfies
 *         |sum^ - sum| <= gamma_(K+8) sum |taps[k][delta] term|      (term = 1, x, x x; derived in DESIGN 4.20)
 *     against the sum of the ROUNDED taps in exact arithmetic, for any order of summation, with or without fused multiply-add;
 *   - bit-identical run to run, range by range (any frame_begin, frame_end) against the full call, a series alone against the same
 *     series among s, with dead (invalid) slots appended and with dead frames appended at the end.
 * A null pointer, n or s < 1, bad cols / n_values, n_half < 1 or h > VBS_KIN_MAX_HALF, degree outside 0 .. VBS_KIN_MAX_DEGREE, a
 * negative or non-finite weight, a centre <= 0, a range outside 0 <= fb <= fe <= n: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES or s >
 * VBS_PROJ_MAX_SLOTS: VBS_ECAPACITY; a bad argument comes before a capacity; all decided before the device is touched.  fb == fe
 * emits nothing.
 *
 * vbs_poly_fit_f64 - mom [dev] float64 [F, s, M] as above for the frames [frame_begin, frame_end) of rec [dev] [n, s, cols] (read
 * for the flag of the centre frame and, with `filled`, for the rows of valid entries); half_window = the h of the moments (it
 * fixes H), thr HOST [d + 1], >= 0 and not NaN (+inf switches an order off: the caller's for k >= 2h + 1, which no window of 2h + 1
 * frames determines): thr[0] = min_coverage * sw (sw the ascending sum of w), thr[k] = piv_rel *
 * piv_full[k] (the pivots of the gap-free full window), each ONE IEEE product formed by the caller.  Per (frame, slot) the normal
 * equations are the Hankel matrix G[a][b] = S_(a+b), factored G = L diag(D) L^T without a square root, column by column:
 *     for j = 0 .. d:
 *         t = S_(2j);        for m = 0 .. j-1 ascending:  t = t - V[j][m] * L[j][m];        D_j = t
 *         for a = j+1 .. d:  t = S_(a+j);  for m = 0 .. j-1 ascending:  t = t - V[a][m] * L[j][m];   V[a][j] = t;  L[a][j] = t / D_j
 * THE DEGREE USED q is the largest q <= d with D_k > thr[k] for ALL k <= q, -1 when there is none; a comparison with a NaN is
 * false.  The leading block of the factorisation is the factorisation of the lower-degree problem, so the fallback is a shorter
 * back substitution: a window across a gap degrades from cubic to line to mean instead of returning a wild curvature.  Per value:
 *     for k = 0 .. d:        t = X_k;  for m = 0 .. k-1 ascending:  t = t - L[k][m] * z_m;    z_k = t;   g_k = z_k / D_k
 *     for k = q down to 0:   t = g_k;  for m = k+1 .. q ascending:  t = t - L[m][k] * c_m;    c_k = t
 *     y0 = c_0     y1 = c_1 / H     y2 = (2 * c_2) / (H * H)     y3 = (6 * c_3) / (H * H * H)       (0 for the orders above q)
 *     rss = XX;    for k = 0 .. q ascending:  rss = rss - z_k * g_k
 * y_k is the k-th derivative of the fitted polynomial at the window's centre in units of frames; g_k = z_k / D_k is the solution of
 * the diagonal system (the "y" of L z = X, D y = z, L^T c = y), so rss is the weighted residual sum of squares of the degree-q
 * fit, reported as computed: it may be a rounding below zero; with q = -1 it is XX.  EVERY EXPRESSION IS EVALUATED AS WRITTEN,
 * FLOAT64 WITHOUT CONTRACTION, AND THAT IS PART OF THIS INTERFACE (a division by H is an exact scaling).
 * fit [dev] float64 [F, s, 2 + (d + 2) n_values] = flag, q, then (y_0 .. y_d, rss) per value;
 *     flag = (centre entry valid) + 2 (q >= 0) + 4 (q == d).
 * filled [dev] float64 [F, s, cols] or NULL, as vbs_hampel_series_f64 writes `clean`: where the centre entry is valid the row of
 * rec bit for bit; where it is missing and q >= fill_degree (0 <= fill_degree <= VBS_KIN_MAX_DEGREE; above d nothing is filled) flag 2.0, the values y0, 0.0 in the columns
 * beyond n_values; otherwise all zeros.  Any flag != 0 is what every other entry reads as valid.  One thread per (frame, slot).
 * A null pointer (filled excepted), n or s < 1, bad cols / n_values / degree / half_window / fill_degree, a thr that is negative
 * or NaN, a range outside 0 <= fb <= fe <= n: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES or s > VBS_PROJ_MAX_SLOTS:
 * VBS_ECAPACITY, after the arguments; before the device is touched. */
#define VBS_KIN_TILE       64    /* frames a workgroup emits (no result depends on it)           */
#define VBS_KIN_MAX_HALF   127   /* h at most: a window of 2h + 1 <= VBS_FIR_MAX_TAPS frames      */
#define VBS_KIN_MAX_DEGREE 3     /* d at most                                                     */
int vbs_poly_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* half, int n_half,
                         int degree, int frame_begin, int frame_end, double* mom, void* stream);
int vbs_poly_fit_f64(int device, const double* mom, const double* rec, int n, int s, int cols, int n_values, int degree,
                     int half_window, const double* thr, int fill_degree, int frame_begin, int frame_end, double* fit,
                     double* filled, void* stream);

/* ---- Principal modes of the displacement field along a recording (the reference ships no code for this; every other analysis
 * here reduces the recording with a model chosen in advance) ----
 * Which spatial patterns of marker displacement a recording consists of, how much of the variance each carries and how each
 * evolves along time: PCA / proper orthogonal decomposition with gaps, in four entries without a handle on the record layout of
 * vbs_fir_series_f64 (rec [dev] float64 [n, s, cols], time-major, col 0 the flag, cols 1 .. n_values the values, 1 <= n_values <= 3,
 * n_values < cols <= 8; invalid entries are selected out when they are read, never multiplied by zero: they and every column
 * beyond n_values may hold NaN or 1e300).  The estimators, the drop rule, the sign rule and `resid` are this project's (DESIGN
 * 4.19, 7).  No call allocates; no atomics, no wait across workgroups.
 *
 * vbs_cross_moments_f64 - shift [dev] float64 [s, n_values] (may be NULL = 0) is subtracted ONCE, rounded, when a valid entry is
 * staged: z = x - shift, AND THAT SUBTRACTION IS PART OF THE INTERFACE; it keeps the later centring free of cancellation, so the
 * caller passes the per-series means.  Per slot the columns are col_0..2 = z_1, z_2, z_3 (a column beyond n_values is 0) and
 * col_3 = the flag as 1.0 / 0.0, all 0 in a frame where the slot is invalid.
 * mom [dev] float64 [s, s, 4, 4]: mom[i, j, v, w] = sum over the frames of col_v(i) col_w(j).  The 3 x 3 corner: the cross sums over
 * the frames where BOTH slots are valid; row or column 3: the sum of one slot's values over the frames where the other is valid
 * too (what pairwise-complete centring needs); [3][3]: the pair count, an exact integer.
 * The kernel is a float64 matrix product on v_mfma_f64_16x16x4_f64 with the frame axis as K, both operands staged from the record;
 * a workgroup takes one pair of tiles of VBS_MOM_WG_SLOTS slots with j-tile >= i-tile and writes the mirror block too:
 * mom[j, i, w, v] HAS THE BITS OF mom[i, j, v, w].  NO SPLIT OF K ACROSS WORKGROUPS: every output is one accumulator chain over the
 * frames, chunk after chunk of VBS_MOM_CHUNK in ascending order from frame 0.
 * THE ORDER OF SUMMATION IS NOT PART OF THIS INTERFACE, as for vbs_project_series_f64.  What is promised instead:
 *   - exact where the inputs make every order exact: if every z, every product and every partial sum is representable;
 *   - otherwise, with u = 2^-53, gamma_k = k u / (1 - k u), over the frames:
 *     |mom^ - mom| <= gamma_(n+6) sum |col_v(i) col_w(j)|   (mom the sums of the ROUNDED z; derived in DESIGN 4.19),
 *     for any order of summation, with or without fused multiply-add;
 *   - bit-identical run to run, a pair of slots alone against the same pair among s, with dead (invalid) slots appended and with
 *     dead frames appended at the end.
 * A null rec or mom, n or s < 1, bad cols / n_values: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES or s > VBS_MOM_MAX_SLOTS: VBS_ECAPACITY; a
 * bad argument comes before a capacity; all decided before the device is touched.
 *
 * vbs_covariance_f64 - mom as above.  cov [dev] float64 [C, C], C = s n_values, c = i n_values + v.  With N = mom[i,j,3,3],
 * S = mom[i,j,v,w], a = mom[i,j,v,3], b = mom[i,j,3,w], for c = (i, v) <= c' = (j, w):
 *     mode 0, pairwise:   cov = (S - (a * b) / N) / (N - 1)
 *     mode 1, filled:     m_i = mom[i,i,v,3] / mom[i,i,3,3],   m_j = mom[j,j,w,3] / mom[j,j,3,3]
 *                         cov = (S - m_i * b - m_j * a + N * (m_i * m_j)) / denom        (left to right)
 * and cov[c', c] is a copy of cov[c, c'].  EVERY EXPRESSION IS EVALUATED AS WRITTEN, FLOAT64 WITHOUT CONTRACTION, AND THAT IS PART OF
 * THIS INTERFACE.  Mode 1 is the Gram matrix of the data with every gap filled by its series' mean, divided by denom (the pipeline
 * passes n - 1): positive semidefinite as long as no pair of unmasked slots falls below min_count (a block zeroed for that
 * breaks the Gram structure; a masked slot, whose whole rows and columns go, does not), biased towards zero by the share of gaps
 * (DESIGN 7).  Mode 0 is unbiased pair by pair and may be INDEFINITE.  ok = N >= min_count (min_count >= 2) and neither slot masked; where !ok the nine cells are exact zeros.
 * slot_mask [dev] uint8 [s] (may be NULL = all): a slot with 0 gives !ok rows and columns.  ok [dev] uint8 [s, s] (may be NULL).
 * One thread per slot pair.  A null mom or cov, s < 1, n_values outside 1..3, mode not 0 or 1, min_count < 2, in mode 1 a denom
 * that is not finite or <= 0: VBS_EINVAL; s > VBS_MOM_MAX_SLOTS: VBS_ECAPACITY, after the arguments; before the device is touched.
 *
 * vbs_leading_modes_f64 - the r <= VBS_MODES_MAX leading eigenpairs of a symmetric A [dev] float64 [C, C] (only what is stated
 * below is read of it; an unsymmetric A gives what the operations give) by orthogonal iteration with a FIXED number of
 * iterations: nothing is tested for convergence, `resid` says what was reached.  The iteration finds the invariant subspace of
 * the LARGEST |lambda|: of an indefinite A (mode 0 above) these may be negative; within the subspace the values come descending.
 * work [dev] float64 [2 C VBS_MODES_MAX], the caller's.  Blocks are [C][VBS_MODES_MAX], r columns used.
 *   start    Q0[c][k] = (double)(int32)h(c VBS_MODES_MAX + k + 1) * 2^-31, h(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13;
 *            x *= 0xc2b2ae35; x ^= x >> 16 on uint32; then `orth`
 *   iterate  `iters` times: Y = A Q (`apply`), Q = orth of Y
 *   apply    one wave per row of A: lane l of 64 adds a[c] * Q[c][k] for c = l, l + 64, .. ascending from 0.0, the 64 sums are
 *            folded a[i] + a[i + 32], then + 16, 8, 4, 2, 1: the order of vbs_axis_displacement
 *   sums     every other sum over the rows c of a block: thread t of 256 adds rows t, t + 256, .. ascending from 0.0, each of the
 *            four waves folds its 64 sums as above, the wave sums are added ((W0 + W1) + W2) + W3
 *   orth     big = the largest of the r squared column norms as they came in.  Twice: for j = 0 .. r-1 ascending: S_k = sum
 *            x_j x_k for k = j .. r-1 (the current columns); the column is DROPPED (zeros, counted in the first round) unless
 *            S_j > tiny * big (first round) or S_j > 0 (second); else nrm = sqrt(S_j), x_j = x_j / nrm, and for k > j
 *            x_k = x_k - (S_k / nrm) * x_j with the new x_j: modified Gram-Schmidt, row-oriented
 *   ritz     Y = A Q once more; T[k][l] = sum Q_k Y_l for k <= l, mirrored; cyclic Jacobi on T, pairs (p, q), p < q, row by row,
 *            VBS_MODES_SWEEPS sweeps: skipped where T[p][q] == 0, else theta = (T[q][q] - T[p][p]) / (2 T[p][q]),
 *            t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; for every k the columns
 *            (T[k][p], T[k][q]) = (c x - s y, s x + c y), then the rows likewise, then the columns of V (from the identity), then
 *            T[p][q] = T[q][p] = 0.  Values = the diagonal, sorted descending, the smaller index first among equals.
 *            u_k[c] = sum over l ascending of Q[c][l] V[l][k], (A u)_k[c] likewise from Y; resid_k = sqrt of the sum (by `sums`) of
 *            ((A u)_k[c] - lambda_k u_k[c])^2.  Every mode's sign makes its entry of largest magnitude positive, the smallest
 *            index among equals.
 * values [dev] float64 [r]; modes [dev] float64 [r, C], orthonormal rows, zeros for a dropped column, whose value 0 and resid 0
 * take the place the descending sort gives a 0: behind the others where every kept value is positive, BETWEEN the positive and
 * the negative ones of an indefinite A - a dropped row is told by its zeros, not by its place;
 * resid [dev] float64 [r] = || A u - lambda u ||_2: THE HONEST CONVERGENCE MEASURE, the fixed `iters` guarantees nothing by itself
 * (the error of a value is at most its resid; the subspace converges like (|lambda_(r+1)| / |lambda_k|)^iters);
 * info [dev] int32 [2] = rank found (r - dropped), columns dropped, of the last orth.  THE ORDER OF EVERY OPERATION IS PART OF THIS
 * INTERFACE.  A null pointer, C < 1, r outside 1 .. min(C, VBS_MODES_MAX), iters outside 0 .. VBS_MODES_MAX_ITERS, tiny outside
 * [0, 1): VBS_EINVAL; C > VBS_MODES_MAX_DIM: VBS_ECAPACITY, after the arguments; before the device is touched.
 *
 * vbs_mode_scores_f64 - rec as above; center [dev] float64 [C] (shift plus mean, the caller's); modes [dev] float64 [r, C].  For
 * every frame f of [frame_begin, frame_end), over the VALID columns c = i n_values + v of the frame, lane l of 64 adding
 * c = l, l + 64, .. ascending from 0.0 and the 64 sums folded 32, 16, 8, 4, 2, 1 (THE ORDER IS PART OF THIS INTERFACE), with
 * d_c = x_c - center_c:   num_k = sum d_c u_k[c]     den_k = sum u_k[c] u_k[c]     e = sum d_c d_c
 * scores [dev] float64 [fe-fb, r, 3] = (1, num_k / den_k, den_k) where den_k >= min_coverage, else (0, 0, den_k): u has unit norm,
 * so den is the share of the mode that was seen, and num / den the least-squares amplitude of the mode over what was seen.  A
 * record with cols 3, n_values 1, s = r that vbs_fir_series_f64, vbs_hampel_series_f64, vbs_project_series_f64,
 * vbs_window_moments_f64 and vbs_step_response_f64 take as it is.  energy (may be NULL) [dev] float64 [fe-fb, 2] = the number of
 * valid columns, e.  One wave per frame, VBS_SCORE_GROUP frames a workgroup (no result depends on it).  A null rec, center, modes
 * or scores, n or s < 1, bad cols / n_values, r outside 1 .. VBS_MODES_MAX, min_coverage outside (0, 1], a range outside
 * 0 <= fb <= fe <= n: VBS_EINVAL; n > VBS_PROJ_MAX_FRAMES or s > VBS_MOM_MAX_SLOTS: VBS_ECAPACITY, after the arguments; before the
 * device is touched.  fb == fe emits nothing. */
#define VBS_MOM_CHUNK       32       /* frames staged at a time (no result depends on it)                    */
#define VBS_MOM_WG_SLOTS    16       /* slots of a tile; a workgroup takes a pair of tiles (no result depends on it) */
#define VBS_MOM_MAX_SLOTS   1024     /* s at most                                                            */
#define VBS_MODES_MAX       16       /* r at most                                                            */
#define VBS_MODES_MAX_DIM   3072     /* C at most                                                            */
#define VBS_MODES_SWEEPS    10       /* Jacobi sweeps of the Ritz step                                       */
#define VBS_MODES_MAX_ITERS 4096     /* iters at most                                                        */
#define VBS_SCORE_GROUP     8        /* frames a workgroup of the scores takes, one wave each                */
int vbs_cross_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* shift, double* mom,
                          void* stream);
int vbs_covariance_f64(int device, const double* mom, int s, int n_values, int mode, int min_count, double denom,
                       const uint8_t* slot_mask, double* cov, uint8_t* ok, void* stream);
int vbs_leading_modes_f64(int device, const double* A, int C, int r, int iters, double tiny, double* work, double* values,
                          double* modes, double* resid, int32_t* info, void* stream);
int vbs_mode_scores_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* center,
                        const double* modes, int r, double min_coverage, int frame_begin, int frame_end, double* scores,
                        double* energy, void* stream);

/* vbs_retrack - re-track a recording from its detections, ALONG TIME (ours: the reference tracks every frame alone, against
 * the first-frame positions, and lets two IDs take one detection - vbs_track is that rule and stays what it is).  Handle-free.
 *   det [dev] float64 [n,max_det,VBS_DET_COLS] and counts [dev] int32 [n] as vbs_track_to_3d writes them; ref_xy [dev] float64
 *   [m_ref,2]; state_in [dev] float64 [m_ref,VBS_RETRACK_STATE_COLS] = px, py, vx, vy, age, seen per slot, or NULL for the
 *   initial state p = ref_xy, v = 0, age = 0, seen = 0.
 * THE RULE.  For frame f, in frame order, per slot j, all in float64 without contraction; every expression and tie-break
 * below is part of the interface:
 *   1. prediction   k = age + 1,  qx = px + vx*k,  qy = py + vy*k.
 *   2. counts[f] < 0: the frame is unusable, every slot is unmatched and info[f].used = 0.  Else cnt = min(counts[f], max_det);
 *      no row of det at or beyond cnt is used.
 *   3. candidates   a detection with a non-finite x or y is never one.  dx = qx - x_i, dy = qy - y_i, d2 = dx*dx + dy*dy; the
 *      pair (j, i) is a candidate iff d2 <= gate*gate and, when max_travel is finite, (x_i - ox)*(x_i - ox) + (y_i - oy)*(y_i -
 *      oy) <= max_travel*max_travel with (ox, oy) = ref_xy[j].
 *   4. one-to-one   sort the candidate pairs by the key (d2, j, i) ascending and walk them: a pair is taken iff neither its slot
 *      nor its detection has been taken.  (The kernel runs the equivalent rounds: every free slot names its best free candidate
 *      by (d2, i), every free detection its best free slot by (d2, j) among ALL free slots that hold it as a candidate, mutual
 *      pairs are fixed, until no free slot has a free candidate.)
 *   5. update       matched to i with seen == 1: ux = (x_i - px)/k, vx <- vx + vel_gain*(ux - vx), the same for y; with seen
 *      == 0 the velocity stays as it is.  Either way p <- (x_i, y_i), age <- 0, seen <- 1.  Unmatched: age <- age + 1, and
 *      v <- 0 once age > max_coast.
 * Defaults of the shim: gate 10, max_travel +inf, vel_gain 0.5, max_coast 5.
 * Outputs, each may be NULL (all of assign, table and state_out NULL: VBS_EINVAL):
 *   assign [dev] int32 [n,m_ref]     the detection index, or -1
 *   table [dev] float32 [n,m_ref,VBS_TABLE_COLS]  rows exactly as vbs_track writes them: VBS_FLAG_TRACKED, columns 1-5 the
 *                                    detection cast once to float32, column 9 the index, X Y Z zero; vbs_solve3d fills it in place
 *   dist2 [dev] float64 [n,m_ref]    d2 of the accepted pair, or -1
 *   info [dev] int32 [n,VBS_RETRACK_INFO_COLS] = used, matched, with_candidate (slots with >= 1 candidate), contested (slots
 *                                    with a candidate whose outcome is not their own best candidate by (d2, i); a slot left
 *                                    unmatched counts)
 *   state_out [dev] float64 [m_ref,VBS_RETRACK_STATE_COLS]: frames [0, k) and then [k, n) from that state give what [0, n) gives.
 *   workspace [dev], 8-byte aligned, of vbs_retrack_workspace bytes for the same n, m_ref, max_det (the cell grid of every
 *   frame, and the assignment when `assign` is NULL); the call allocates nothing.
 * A null det, counts, ref_xy or workspace, n < 0, m_ref < 1, max_det < 1, a NaN or negative gate, vel_gain outside [0, 1] or
 * max_coast < 0: VBS_EINVAL; m_ref or max_det above VBS_RETRACK_MAX: VBS_ECAPACITY, after the arguments; both before a device is
 * selected.  Results do not depend on the path a frame takes: the cell lists need a gate <= 4095 and cell coordinates below
 * 2^30, any other frame (or slot) scans every detection. */
#define VBS_RETRACK_MAX        1024  /* m_ref and max_det at most                                             */
#define VBS_RETRACK_STATE_COLS 6     /* px, py, vx, vy, age, seen                                             */
#define VBS_RETRACK_INFO_COLS  4     /* used, matched, with_candidate, contested                              */
int64_t vbs_retrack_workspace(int n, int m_ref, int max_det);
int vbs_retrack(int device, const double* det, const int32_t* counts, int n, int max_det, const double* ref_xy, int m_ref,
                const double* state_in, double gate, double max_travel, double vel_gain, int max_coast, int32_t* assign,
                float* table, double* dist2, int32_t* info, double* state_out, void* workspace, void* stream);

/* Uncertainty of the 3-D solve (ours: the reference states its precision as two figures).  Handle-free; float64 without
 * contraction, + - * / sqrt only, every sum in a stated order: an output depends on its inputs only, never on the launch shape
 * or on the range it was asked in, and tests/helpers/uncert_oracle.py restates every expression bit for bit.
 * THE MODEL is what vbs_solve3d computes for a row: cv2.undistortPoints' five fixed-point iterations (skipped when every
 * distortion coefficient is 0) followed by the closed-form solve, as a function of the observation o = (Cx, Cy, major) - table
 * columns 1 .. 3 read as (double)float32 - and of the camera vector of VBS_UNCERT_CAM = 16 entries
 *     fx, fy, cx, cy, k1, k2, p1, p2, k3, w0, w1, w2, T0, T1, T2, dmm
 * where w is a small rotation on the camera side, R_wc' = exp([w]x) R_wc at w = 0: dX/dw_i = R_wc' (pc x e_i), pc = P_cam - T.
 * It is differentiated by forward mode through the iterations AS EXECUTED (not the implicit-function derivative of the
 * converged inverse); f_avg, dmm / f_avg and f_avg^2, float32 in the solve, are differentiated as the smooth float64 expressions
 * while the primal values the tangents multiply are the solve's own.  First order only.
 * A table row is USABLE where it carries VBS_FLAG_XYZ, major >= min_marker_size_px and the recomputed solve succeeds.
 *
 * vbs_uncert_points - uvd [dev] float64 [n,3] = (Cx, Cy, major) -> xyz [dev] float64 [n,3] and ok [dev] int32 [n], bit for bit
 *   what vbs_calculate_3d gives for vbs_undistort_points of the same points; j_obs [dev] float64 [n,3,3] = dX_r / do_k and j_cam
 *   [dev] float64 [n,3,VBS_UNCERT_CAM] = dX_r / dtheta_k, zeros where ok is 0.
 * vbs_uncert_cov - table [dev] float32 [n,m_ref,VBS_TABLE_COLS].  obs_cov [HOST] float64 [obs_rows,6], obs_rows 1 or m_ref (one
 *   per slot): the symmetric covariance of (Cx, Cy, major) as uu, uv, ud, vv, vd, dd.  cam_factor [HOST] float64 [16,q], 0 <= q
 *   <= 16 (may be NULL at q = 0): Sigma_theta = L L'.  Column c of L is pushed through the model as ONE direction, g_c = J_cam
 *   L[:,c], so a covariance is a sum of squares - positive semidefinite by construction - and J_cam is never formed for a table.
 *   cov [dev] float64 [fe-fb,m_ref,VBS_UNCERT_COV_COLS] = flag (1 = usable), xx, xy, xz, yy, yz, zz of
 *     Sigma_X = J_obs Sigma_o J_obs' + sum_c g_c g_c'           (M = J_obs Sigma_o, then M J_obs', every entry three products added
 *   from the left; then c ascending), zeros where the row is not usable.  May be NULL.
 *   dcov [dev] float64 [fe-fb,m_ref,VBS_UNCERT_DCOV_COLS], may be NULL; needs 0 <= ref_frame < n (with dcov NULL ref_frame must
 *   be -1).  For a row usable in its frame AND in ref_frame: flag 1, the six entries of
 *     Sigma_D = (J_obs,f Sigma_o J_obs,f' + J_obs,0 Sigma_o J_obs,0') + sum_c (g_c,f - g_c,0)(g_c,f - g_c,0)'
 *   and t2 = D' Sigma_D^-1 D with D = table columns 6 .. 8 of the row minus the reference row's, as vbs_axis_displacement forms
 *   it.  The inverse is an LDL' without square roots: d1 = xx, l21 = xy / d1, l31 = xz / d1, d2 = yy - l21 xy, w = yz - l21 xz,
 *   l32 = w / d2, d3 = (zz - l31 xz) - l32 w; z1 = D0, z2 = D1 - l21 z1, z3 = (D2 - l31 z1) - l32 z2; t2 = (z1 z1 / d1 + z2 z2 /
 *   d2) + z3 z3 / d3.  t2 is valid - flag 3 - only where d1, d2 and d3 each exceed piv_rel * ((xx + yy) + zz); else t2 = 0.  The
 *   pixel noise of the two frames is taken as uncorrelated.  The reference row's parts are computed once per slot.
 * vbs_uncert_total - the variance of vbs_axis_displacement's `total`.  A slot counts where slot_mask ([dev] uint8 [m_ref] or
 *   NULL) selects it, the row of ref_frame is usable (want) and the frame's row is.  total [dev] float64
 *   [fe-fb,VBS_UNCERT_TOTAL_COLS] = count, complete (want >= 1 and count == want), var_x, var_y, var_z, cam_x, cam_y, cam_z:
 *     cam_k = sum_c (sum_r (g_c,f,r - g_c,0,r)_k)^2   the camera's share: coherent over the markers, it grows as count^2
 *     var_k = sum_r (J_obs Sigma_o J_obs')_kk,f,r + (..)_kk,0,r  [each slot's pair added first]  + cam_k
 *   Every sum over r: lane l of a wave adds slots l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1 (lane i takes i + off),
 *   as vbs_axis_displacement.  One wave per frame, VBS_UNCERT_GROUP frames a workgroup (no result depends on it).
 * vbs_pixel_noise - out [dev] float64 [m_ref,VBS_NOISE_COLS] = count, mean Cx, Cy, major, then uu, uv, ud, vv, vd, dd: the sample
 *   covariance (ddof 1) of (Cx, Cy, major) over the rows of [frame_begin, frame_end) with VBS_FLAG_TRACKED, two passes (sums ->
 *   means = sum / count; centred products / (count - 1)), frames in order.  count 0: zeros; count 1: the means and zeros.
 * work [dev] float64 [m_ref * VBS_UNCERT_WORK_COLS]: the reference rows and the staged obs_cov; the calls allocate nothing.
 * VBS_EINVAL, before a device is selected and with nothing written: a null pointer (but the optional ones), n or m_ref < 1,
 * obs_rows neither 1 nor m_ref, q outside [0, 16], a non-finite obs_cov or cam_factor, a NaN min_marker_size_px, piv_rel not
 * finite or < 0, ref_frame outside [0, n) where it is needed, frames outside 0 <= frame_begin <= frame_end <= n. */
#define VBS_UNCERT_CAM        16    /* entries of the camera vector                                          */
#define VBS_UNCERT_COV_COLS   7     /* flag, xx, xy, xz, yy, yz, zz                                          */
#define VBS_UNCERT_DCOV_COLS  8     /* flag, xx, xy, xz, yy, yz, zz, t2                                      */
#define VBS_UNCERT_TOTAL_COLS 8     /* count, complete, var_x, var_y, var_z, cam_x, cam_y, cam_z             */
#define VBS_UNCERT_GROUP      4     /* frames a workgroup of the total takes, one wave each                  */
#define VBS_UNCERT_REF_COLS   55    /* a reference row: usable, its six observation entries, g [16][3]       */
#define VBS_UNCERT_WORK_COLS  61    /* VBS_UNCERT_REF_COLS + 6                                               */
#define VBS_NOISE_COLS        10    /* count, three means, six covariance entries                            */
int vbs_uncert_points(int device, const double* uvd, int n, const vbs_camera* cam, double* xyz, double* j_obs, double* j_cam,
                      int32_t* ok, void* stream);
int vbs_uncert_cov(int device, const float* table, int n, int m_ref, const vbs_camera* cam, const double* obs_cov, int obs_rows,
                   const double* cam_factor, int q, int ref_frame, double min_marker_size_px, double piv_rel, int frame_begin,
                   int frame_end, double* work, double* cov, double* dcov, void* stream);
int vbs_uncert_total(int device, const float* table, int n, int m_ref, const vbs_camera* cam, const double* obs_cov, int obs_rows,
                     const double* cam_factor, int q, int ref_frame, const uint8_t* slot_mask, double min_marker_size_px,
                     int frame_begin, int frame_end, double* work, double* total, void* stream);
int vbs_pixel_noise(int device, const float* table, int n, int m_ref, int frame_begin, int frame_end, double* out, void* stream);

/* Uncertainty of the pose misalignment (ours): the first-order covariance of the plane vbs_pose_series fits, of its tilt and
 * azimuth, and the test "is the plane tilted at all".  Handle-free; float64 without contraction, + - * / only in everything but
 * the optional `pose` columns tilt_deg, azimuth_deg and rms; no atomics; every sum over slots follows the rule of
 * vbs_axis_displacement (lane l of 64 adds slots l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1).  No result depends
 * on the launch shape, on the frame range or on VBS_POSECOV_GROUP (the frames a workgroup takes, one wave each);
 * tests/helpers/posecov_oracle.py restates every expression bit for bit.
 * vbs_pose_cov - table, start_frame, ref_disp, ref_xyz, slot_mask, shell_mode, scale, reject_k and the frame range exactly as
 *   vbs_pose_series takes them; cam, obs_cov [HOST] [obs_rows,6], cam_factor [HOST] [16,q], min_marker_size_px and piv_rel exactly
 *   as vbs_uncert_total and vbs_uncert_cov take them.  ref_rows [dev] float32 [2,m_ref,VBS_TABLE_COLS] or NULL: the rows of the
 *   reference session at the two frames whose difference ref_disp is, ref_start first and ref_end second; with NULL the reference
 *   state is taken as exact.  work [dev] float64 [m_ref * VBS_UNCERT_WORK_COLS]; the call allocates nothing.
 * THE MODEL.  The deviation of a slot is d = (X_f - X_start) - (X_re - X_rs): up to four solves with ONE camera.  Once per slot, with
 *   p = J_obs Sigma_o J_obs' and g_c = J_cam L[:,c] of a row as vbs_uncert_cov forms them (Sigma_o is the slot's for every row):
 *     fixed_usable = the row of start_frame is USABLE (the rule above) and, with ref_rows, both of its rows are
 *     S_fix = p_start, with ref_rows (p_start + p_re) + p_rs                      six entries
 *     g_fix,c = g_c,start, with ref_rows (g_c,start + g_c,re) - g_c,rs            (a shift of T cancels to exactly zero)
 *   For frame f the covariance of a slot's end point from pixel noise is C = ss (p_f + S_fix) entry by entry, ss = scale scale, and
 *   its direction for column c is u = scale (g_c,f - g_fix,c); the pixel noise of different rows is taken as uncorrelated.
 * THE PLANE is recomputed exactly as vbs_pose_series states it: the common rule, means, centred sums, det, a, b, c, SSR, the one
 *   round of rejection decided by the first plane.  pose [dev] float64 [fe-fb,VBS_POSE_COLS] (may be NULL) is that entry's `pose`:
 *   flag, a, b, c and n_used bit for bit.  The USED set is the kept set where the pose flag is 2, the common set otherwise; the
 *   selection is taken as given (not differentiated).  mx, my, mz, xx, xy, yy, det and n_used below are those of the used set.
 * THE LINEARISATION.  A used slot has the centred coordinates x = Px - mx, y = Py - my, z = Pz - mz and r = z - (a x + b y).  Its
 *   influence matrix K [3,3] has, for k = 0, 1, 2 and (dx, dy, dz) the unit vector e_k (as the constants 1.0 and 0.0), the column
 *     e = (dz - a dx) - b dy;   h1 = x e + r dx;   h2 = y e + r dy
 *     K[0][k] = (h1 yy - h2 xy) / det;   K[1][k] = (h2 xx - h1 xy) / det;   K[2][k] = (e / n_used - K[0][k] mx) - K[1][k] my
 * THE SUMS, over the used slots that are fixed_usable and usable in f (n_unusable counts the used slots that are not):
 *     Sigma_obs = sum_r K C K'     aa, ab, ac, bb, bc, cc: M = K C, then M K', every entry three products added from the left (the
 *                                  product of vbs_uncert_cov with K for J_obs and C for Sigma_o); six sums
 *     v_c = sum_r K u              row i = (K[i][0] u0 + K[i][1] u1) + K[i][2] u2; three sums per column
 *     Sigma_cam = sum_c v_c v_c'   c ascending, each entry acc + v_i v_j;   Sigma = Sigma_obs + Sigma_cam entry by entry
 *   With rho2 = a a + b b, w = 1.0 + rho2, k2 = 57.29577951308232 * 57.29577951308232, ab2 = (2.0 a) b:
 *     var_tilt    = (k2 ((a a Saa + ab2 Sab) + b b Sbb)) / (rho2 (w w))             in degrees squared; both 0 unless rho2 > 0
 *     var_azimuth = (k2 ((b b Saa - ab2 Sab) + a a Sbb)) / (rho2 rho2)
 *   t2 = (a, b) Sigma_ab^-1 (a, b)' through an LDL' without square roots: d1 = Saa, l = Sab / d1, d2 = Sbb - l Sab, z1 = a,
 *   z2 = b - l a, t2 = z1 z1 / d1 + z2 z2 / d2; valid only where d1 and d2 each exceed piv_rel (Saa + Sbb), else 0.  A tilt is
 *   >= 0 and not Gaussian near 0: t2 (two degrees of freedom), not tilt / sigma_tilt, is the decision.
 *   pcov [dev] float64 [fe-fb,VBS_POSECOV_COLS] (may be NULL, not both) = flag, n_unusable, the six entries of Sigma, the six of
 *   Sigma_cam, var_tilt, var_azimuth, t2.  flag is a bit set: 1 = a plane exists and n_unusable = 0 - only then is any column
 *   but n_unusable nonzero; 2 = t2 is valid; 4 = rho2 > 0, the angle variances are valid.  A nonzero flag keeps pcov readable as
 *   a FIR record.  Nothing of a slot that is not common is read into a value, and of a row nothing but what its flag allows:
 *   such cells may hold NaN.
 * VBS_EINVAL, before a device is selected and with nothing written: what vbs_pose_series and vbs_uncert_total refuse (a null
 *   table, ref_disp, ref_xyz, cam, obs_cov or work, n or m_ref < 1, start_frame outside [0, n), a shell_mode other than 0 / 1, a
 *   scale or reject_k that is not finite, reject_k < 0, obs_rows neither 1 nor m_ref, q outside [0, 16], a non-finite obs_cov or
 *   cam_factor, a NaN min_marker_size_px, piv_rel not finite or < 0, frames outside 0 <= frame_begin <= frame_end <= n), and pose
 *   and pcov both NULL.  frame_begin == frame_end emits nothing. */
#define VBS_POSECOV_COLS  17    /* flag, n_unusable, Sigma [6], Sigma_cam [6], var_tilt, var_azimuth, t2 */
#define VBS_POSECOV_GROUP 4     /* frames a workgroup takes, one wave each (no result depends on it)     */
int vbs_pose_cov(int device, const float* table, int n, int m_ref, int start_frame, const double* ref_disp, const double* ref_xyz,
                 const uint8_t* slot_mask, int shell_mode, double scale, double reject_k, const vbs_camera* cam,
                 const double* obs_cov, int obs_rows, const double* cam_factor, int q, double min_marker_size_px, double piv_rel,
                 const float* ref_rows, int frame_begin, int frame_end, double* work, double* pose, double* pcov, void* stream);

/* Indentation shape along a recording (ours: the reference ships no code for this): a second-order fit in SPACE, per frame, to the
 * end points vbs_pose_series fits its plane to - where the bowl the plane leaves behind has its apex, how deep it is below the
 * plane, how strongly and in which direction it is curved.  Handle-free; float64 without contraction, + - * / only in everything
 * but the columns rms_plane, rms, k1, k2 and dir_deg; no atomics; every sum over slots follows the rule of vbs_axis_displacement
 * (lane l of 64 adds slots l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1).  No result depends on the launch shape, on
 * the frame range or on VBS_SHAPE_GROUP (the frames a workgroup takes, one wave each); tests/helpers/shape_oracle.py restates every
 * expression bit for bit.  The call allocates nothing.
 * vbs_shape_series - table, start_frame, ref_disp, ref_xyz, slot_mask, shell_mode, scale and the frame range exactly as
 *   vbs_pose_series takes them: the COMMON rule, the deviation d and the end point P are that entry's, bit for bit.  Nothing of a
 *   slot that is not common is read into a value: such cells may hold NaN.  length > 0 scales x and y (a length of the marker
 *   field, so that the monomials are of order 1); the results do not carry it.
 * THE FIT of a set of slots (the common set; then once its kept slots): count, the means mx, my, mz of P (sum / count); per slot
 *     u = (Px - mx) / length,  v = (Py - my) / length,  w = Pz - mz
 *     u2 = u u, uv = u v, v2 = v v;  u3 = u2 u, u2v = u2 v, uv2 = u v2, v3 = v2 v;  u4 = u2 u2, u3v = u3 v, u2v2 = u2 v2, uv3 = u v3,
 *     v4 = v2 v2
 *   the 14 sums of u, v, u2, uv, v2, u3, u2v, uv2, v3, u4, u3v, u2v2, uv3, v4 (the first two kept as computed, not taken as zero) and
 *   the 6 sums of w, u w, v w, u2 w, uv w, v2 w.  (The sum of w w has no reader - residuals are explicit - and is not formed.)  With
 *   the basis phi = (1, u, v, u2, uv, v2) the normal matrix is N_ij = sum phi_i phi_j read from those sums, N_00 = count as a
 *   double, and the right-hand side g_i = sum phi_i w.  With count < 3 nothing is summed and the degree is 0.
 *   LDL' without square roots and without pivoting, column j = 0 .. 5 in basis order, every inner sum subtracted from the left with
 *   k ascending:
 *     d_j = N_jj - sum_{k<j} L_jk c_jk;      for i > j:  c_ij = N_ij - sum_{k<j} L_jk c_ik,   L_ij = c_ij / d_j
 *   (the 3 x 3 of vbs_uncert_cov continued: d_1 = N11 - L10 c10, c21 = N21 - L10 c20, d_2 = (N22 - L20 c20) - L21 c21, ..).  Pivot j
 *   PASSES when d_j > piv_rel N_jj; the factorisation stops at the first that does not.  Its leading 3 x 3 is the factorisation of
 *   the plane's normal equations, so one factorisation serves both degrees.  Forward: z_i = g_i - sum_{k<i} L_ik z_k, y_i = z_i / d_i.
 *   DEGREE 2 when count >= min_count and all six pivots pass: beta_5 = y_5, beta_i = y_i - sum_{k>i} L_ki beta_k (k ascending).
 *   DEGREE 1 when the first three pass: gamma_2 = y_2, gamma_1 = y_1 - L_21 gamma_2, gamma_0 = (y_0 - L_10 gamma_1) - L_20 gamma_2;
 *   gamma is computed where degree 2 exists as well.  DEGREE 0 otherwise.  This degree-1 fit is the same least-squares plane as
 *   vbs_pose_series's but NOT its bits (that entry solves the centred 2 x 2 in closed form); the two agree to rounding.
 *   Residuals are explicit, never from the moment identity:
 *     r1 = w - ((gamma_0 + gamma_1 u) + gamma_2 v)
 *     r2 = w - (((((beta_0 + beta_1 u) + beta_2 v) + beta_3 u2) + beta_4 uv) + beta_5 v2)
 *   SSR1 = sum r1 r1 and, at degree 2, SSR2 = sum r2 r2 by the same rule.
 * ONE ROUND OF REJECTION, as vbs_pose_series words it: only when reject_k > 0, the first fit has a degree >= 1 and the SSR of that
 *   degree is > 0.  Kept are the common slots with r r <= (reject_k reject_k) (SSR / count), r the first fit's residual of that
 *   degree.  If fewer are kept than are common and the kept set, fitted by the same rules, reaches the first fit's degree (degree 2:
 *   kept >= min_count and six pivots; degree 1: kept >= 3 and three pivots), every quantity is that of the kept set at THAT degree
 *   and n_used = kept; otherwise the first fit stands and n_used = count.
 *   shape [dev] float64 [fe-fb,VBS_SHAPE_COLS] (may be NULL), zeros where the degree does not allow a column:
 *     0 degree  1 count  2 n_used  3-5 mx, my, mz of the used set (where count >= 1)
 *     6 c0 = mz + beta_0               7 a = beta_1 / length            8 b = beta_2 / length        (at degree 1 from gamma)
 *     9 p = ((2.0 beta_3) / length) / length   10 q = (beta_4 / length) / length   11 r = ((2.0 beta_5) / length) / length
 *     12 rms_plane = sqrt(SSR1 / n_used)       13 rms = sqrt(SSR2 / n_used) at degree 2
 *     14 H = (p + r) / 2.0    15 K = p r - q q    16, 17 k1 = H + s, k2 = H - s with hd = (p - r) / 2.0, s = sqrt(hd hd + q q)
 *     18 dir_deg = (0.5 atan2(2.0 q, p - r)) 57.29577951308232, the direction of k1
 *     19 apex (1 = valid)     20-22 apex_x = mx + xi, apex_y = my + eta, apex_z = c0 + (a xi + b eta) / 2.0
 *     23 depth = apex_z - (mz + ((gamma_0 + (gamma_1 xi) / length) + (gamma_2 eta) / length)): the quadric below the plane there
 *   so that z ~ c0 + a x + b y + (p x x + 2 q x y + r y y) / 2 in x = Px - mx, y = Py - my.  The apex is the stationary point by
 *   Cramer, xi = (q b - r a) / K, eta = (q a - p b) / K, valid only at degree 2 where |K| > apex_rel ((p p + 2.0 (q q)) + r r) and
 *   xi xi + eta eta <= (max_apex length) (max_apex length): squared comparisons, no root decides.  A nonzero degree keeps a row
 *   readable as a FIR record.  Columns 12, 13, 16, 17, 18 pass through sqrt or atan2 (held to 4 ulp); every other column is exact.
 *   coef [dev] float64 [fe-fb,2,4] (may be NULL) = (degree, c0, a, b), (degree == 2 ? 1 : 0, p, q, r): seen as [F, s = 2, cols = 4]
 *     with n_values = 3 a vbs_fir_series_f64 record as it is (trends are taken from filtered coefficients, never from filtered
 *     curvatures or angles).
 *   residual [dev] float64 [fe-fb,m_ref,2] (may be NULL) = (1, r) of the standing fit's degree for every used slot where that degree
 *     is >= 1, (0, 0) elsewhere: a vbs_field_map_f64 record as it is - the map of what no smooth surface explains.
 * VBS_EINVAL, before a device is selected and with nothing written: what vbs_pose_series refuses (a null table, ref_disp or
 *   ref_xyz, n or m_ref < 1, start_frame outside [0, n), a shell_mode other than 0 / 1, a scale or reject_k that is not finite,
 *   reject_k < 0, frames outside 0 <= frame_begin <= frame_end <= n), length not finite or <= 0, min_count < 6, piv_rel, apex_rel or
 *   max_apex not finite or < 0, and all three outputs NULL.  frame_begin == frame_end emits nothing. */
#define VBS_SHAPE_COLS  24      /* degree, count, n_used, means [3], c0, a, b, p, q, r, two rms, H, K, k1, k2, dir, apex [4], depth */
#define VBS_SHAPE_GROUP 4       /* frames a workgroup takes, one wave each (no result depends on it)     */
int vbs_shape_series(int device, const float* table, int n, int m_ref, int start_frame, const double* ref_disp, const double* ref_xyz,
                     const uint8_t* slot_mask, int shell_mode, double scale, double length, double reject_k, int min_count,
                     double piv_rel, double apex_rel, double max_apex, int frame_begin, int frame_end, double* shape, double* coef,
                     double* residual, void* stream);

/* Rigid motion along a recording (ours: the reference ships no code for this): how the markers moved AS A BODY and what is left
 * once that motion is removed.  Per frame the rotation R, the translation t and optionally the scale s with  P ~ s R Q + t  in the
 * least-squares sense, Q a point set given once (`source`: a frame of a table, or a layout) and P the frame's 3-D points, by Horn's
 * closed form: the unit quaternion of R is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix N built from the
 * nine products sum q p'.  That form always returns a proper rotation (no determinant fix) and is well defined on a planar cloud.
 * Handle-free; float64 without contraction; + - * / and sqrt only in everything but columns 26 - 31; no atomics, no LDS, no
 * barrier; every sum over slots follows the rule of vbs_axis_displacement (lane l of 64 adds slots l, l + 64, .. ascending, then
 * the fold 32, 16, 8, 4, 2, 1).  No result depends on the launch shape, on the frame range or on VBS_RIGID_GROUP (the frames a
 * workgroup takes, one wave each); tests/helpers/rigid_oracle.py restates every expression bit for bit.  The call allocates nothing.
 * vbs_rigid_series - table [dev] float32 [n,m_ref,VBS_TABLE_COLS]; source [dev] float64 [m_ref,4] = (flag, X, Y, Z); slot_mask [dev]
 *   uint8 [m_ref] or NULL (all).  A slot is COMMON in frame f when it is selected, source[r][0] != 0 and its row in f carries
 *   VBS_FLAG_XYZ; then Q = source[r][1..3] and P = (double) of the row's columns 6 - 8.  Nothing else of a slot is read into a
 *   value: such cells may hold NaN, 1e30 or 1e300.
 * THE FIT of a set of slots (the common set; then once its kept slots):
 *   Sweep 1: count, qm = (sum Q) / count and pm = (sum P) / count per component.  With count < 3 nothing more is summed: no fit.
 *   Sweep 2: per slot q = Q - qm, p = P - pm per component; the nine sums H_ij = sum q_i p_j (i the SOURCE component, j the frame's:
 *     Hxy = sum qx py), Sqq = sum ((qx qx + qy qy) + qz qz) and Spp = sum ((px px + py py) + pz pz).
 *   N, symmetric (the lower triangle mirrors the upper):
 *     N00 = (Hxx + Hyy) + Hzz   N11 = (Hxx - Hyy) - Hzz   N22 = (Hyy - Hxx) - Hzz   N33 = (Hzz - Hxx) - Hyy
 *     N01 = Hyz - Hzy   N02 = Hzx - Hxz   N03 = Hxy - Hyx   N12 = Hxy + Hyx   N13 = Hzx + Hxz   N23 = Hyz + Hzy
 *   Jacobi: T = N, V = I, VBS_RIGID_SWEEPS sweeps of the cyclic method exactly as vbs_modes' Ritz step states it: pairs (p, q), p < q,
 *     row by row - (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) -; a pair with T[p][q] == 0 is skipped; else
 *       theta = (T[q][q] - T[p][p]) / (2.0 T[p][q])
 *       tt = (theta < 0 ? -1.0 : 1.0) / (|theta| + sqrt(theta theta + 1.0))      cs = 1.0 / sqrt(tt tt + 1.0)      sn = tt cs
 *     then for k = 0 .. 3 the columns  (T[k][p], T[k][q]) <- (cs T[k][p] - sn T[k][q], sn T[k][p] + cs T[k][q])  from the old pair,
 *     then the rows  (T[p][k], T[q][k]) <- (cs T[p][k] - sn T[q][k], sn T[p][k] + cs T[q][k]),  then V's columns as T's columns,
 *     then T[p][q] = T[q][p] = 0.  theta theta may overflow to +inf: then tt = +-0, cs = 1, sn = +-0 and the rotation is the
 *     identity (IEEE, the same on every side).
 *   Eigenvector: k = the index of the largest T[k][k], the smaller index among equals; d2 = the largest T[i][i] over i != k.  With
 *     v = V[:, k]:  nn = ((v0 v0 + v1 v1) + v2 v2) + v3 v3,  (w, x, y, z) = v / sqrt(nn)  (each component divided by the root);  all
 *     four are negated when w < 0, or when w == 0 and the first nonzero of x, y, z is negative.
 *   Gap: gap = (T[k][k] - d2) / (Sqq + Spp), formed where Sqq + Spp > 0 (else 0).  A fit EXISTS iff count >= 3, Sqq + Spp > 0 and
 *     gap > gap_rel; otherwise the two sets do not fix a rotation (collinear or coincident points).
 *   Rotation:  R00 = 1.0 - 2.0 (y y + z z)   R01 = 2.0 (x y - w z)         R02 = 2.0 (x z + w y)
 *              R10 = 2.0 (x y + w z)         R11 = 1.0 - 2.0 (x x + z z)   R12 = 2.0 (y z - w x)
 *              R20 = 2.0 (x z - w y)         R21 = 2.0 (y z + w x)         R22 = 1.0 - 2.0 (x x + y y)
 *   Scale: s = 1.0 exactly unless with_scale is set and Sqq > 0; then s = D / Sqq with D = sum_j sum_i R[j][i] H[i][j] added from
 *     the left, j outer and i inner:  D = (((R00 Hxx + R01 Hyx) + R02 Hzx) + R10 Hxy) + R11 Hyy ... + R22 Hzz  (= sum (R q) . p).
 *   Translation: t_i = pm_i - s ((R_i0 qm_x + R_i1 qm_y) + R_i2 qm_z).
 *   Residual of a slot, explicit and never from a moment identity:  e_i = P_i - (s ((R_i0 Qx + R_i1 Qy) + R_i2 Qz) + t_i).
 *   Sweep 3: SSR = sum ((ex ex + ey ey) + ez ez) and, over the same slots, SS0 = the same sum of d = P - Q per component.
 * ONE ROUND OF REJECTION, as vbs_pose_series words it: only when reject_k > 0, a fit exists and SSR > 0.  Kept are the common slots
 *   with (ex ex + ey ey) + ez ez <= (reject_k reject_k) (SSR / count), e the first fit's residual: a squared comparison, no root
 *   decides.  If fewer are kept than are common and the kept set, fitted by the same rules, gives a fit, every quantity is the kept
 *   set's, n_used = kept and flag = 2; otherwise the first fit stands with n_used = count and flag = 1.
 *   rigid [dev] float64 [fe-fb,VBS_RIGID_COLS] (may be NULL):
 *     0 flag (0 none, 1 fit, 2 refit on the kept set)   1 count   2 n_used   3-5 qm   6-8 pm   9-12 w, x, y, z   13-21 R row-major
 *     22-24 t   25 s   26 rms = sqrt(SSR / n_used)   27 rms0 = sqrt(SS0 / n_used)
 *     28 angle_deg = (2.0 atan2(sqrt((x x + y y) + z z), w)) 57.29577951308232
 *     29 tilt_deg = atan2(sqrt(R02 R02 + R12 R12), R22) 57.29577951308232: the lean of the rotated normal R (0, 0, 1)
 *     30 azimuth_deg = atan2(R12, R02) 57.29577951308232: where it leans to
 *     31 twist_deg = (2.0 atan2(z, w)) 57.29577951308232: the twist about z of the swing-twist split
 *     32 gap
 *     At flag 0 the row holds zeros but count, n_used = count, qm and pm where count >= 1, and gap where it was formed.  Columns
 *     26 - 31 pass through a root or an arc tangent last (held to 4 ulp); every other column is exact.
 *   coef [dev] float64 [fe-fb,4,4] (may be NULL) = (flag, R row i) for i = 0, 1, 2, then (flag, t): seen as [F, s = 4, cols = 4] with
 *     n_values = 3 a vbs_fir_series_f64 record as it is (trends are taken from filtered matrices, brought back to rotations on the
 *     host, never from filtered angles or quaternions).
 *   residual [dev] float64 [fe-fb,m_ref,4] (may be NULL) = (1, ex, ey, ez) for every used slot of a frame with a fit, zeros
 *     elsewhere: a record vbs_field_map_f64, vbs_fir_series_f64, vbs_hampel_series_f64, vbs_cross_moments_f64 and the step entries
 *     take as it is, with n_values = 3.
 * VBS_EINVAL, before a device is selected and with nothing written: a null table or source, n or m_ref < 1, frames outside
 *   0 <= frame_begin <= frame_end <= n, with_scale other than 0 / 1, reject_k or gap_rel not finite or < 0, all three outputs NULL.
 *   frame_begin == frame_end emits nothing. */
#define VBS_RIGID_COLS   33     /* flag, count, n_used, qm [3], pm [3], quaternion [4], R [9], t [3], s, rms, rms0, 4 angles, gap */
#define VBS_RIGID_GROUP  4      /* frames a workgroup takes, one wave each (no result depends on it)     */
#define VBS_RIGID_SWEEPS 8      /* Jacobi sweeps: one more than the 7 after which every host case is diagonal in bits */
int vbs_rigid_series(int device, const float* table, int n, int m_ref, const double* source, const uint8_t* slot_mask,
                     int with_scale, double reject_k, double gap_rel, int frame_begin, int frame_end,
                     double* rigid, double* coef, double* residual, void* stream);

/* Noise-weighted rigid motion along a recording (ours): the maximum-likelihood pose of a frame under the covariance of every 3-D
 * point, the covariance of that pose, chi^2 and the Mahalanobis distance of every marker.  The model is
 *     P_i ~ R (Q_i - qm) + c        with        S_i = Sigma_P,i + R Sigma_Q,i R'   (the second term only with source_cov),
 * qm the source centroid of the start record - a pivot that decorrelates rotation and centre - and no scale (s = 1).  The pose is
 * started at the one vbs_rigid_series left and improved by a FIXED number of Gauss-Newton steps on x = (omega, dc), the rotation
 * updated as R <- exp([omega]x) R through the quaternion (1, omega / 2) / |.|: no sine or cosine appears, and the fixed point is
 * the exponential map's because g = 0 there.  Handle-free; float64 without contraction; + - * / and sqrt only in everything but
 * columns 31 - 34; no atomics, no LDS, no barrier; every sum over slots follows the rule of vbs_axis_displacement (lane l of 64 adds
 * slots l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1).  No result depends on the launch shape, on the frame range or on
 * VBS_RIGID_ML_GROUP (the frames a workgroup takes, one wave each); tests/helpers/rigid_ml_oracle.py restates every expression bit
 * for bit.  The call allocates nothing.
 * vbs_rigid_ml_series - table [dev] float32 [n,m_ref,VBS_TABLE_COLS] and source [dev] float64 [m_ref,4] as vbs_rigid_series took
 *   them.  Per-frame inputs that cover exactly the frames [frame_begin, frame_end), index 0 = frame_begin: cov [dev] float64
 *   [fe-fb,m_ref,VBS_UNCERT_COV_COLS] as vbs_uncert_cov writes it; rigid [dev] float64 [fe-fb,VBS_RIGID_COLS] and residual [dev]
 *   float64 [fe-fb,m_ref,4] as vbs_rigid_series wrote them for this table and source.  source_cov [dev] float64
 *   [m_ref,VBS_UNCERT_COV_COLS] in cov's format, or NULL: an exact source (a layout).  iters in [1, VBS_RIGID_ML_MAX_ITERS].
 *   A frame HAS A START where rigid[f][0] != 0; of such a row columns 3 - 5 (qm), 9 - 12 (the quaternion q) and 22 - 24 (t) are read
 *   and nothing else; of a row without a start nothing else is read.  R is formed from q by vbs_rigid_series's nine expressions (so
 *   the start's R is the record's to the bit) and c_i = ((R_i0 qm_x + R_i1 qm_y) + R_i2 qm_z) + t_i.
 *   A slot is BEGUN in frame f where residual[f][r][0] != 0 (the set vbs_rigid_series let stand, its rejection included; this
 *   entry rejects nothing itself) and USED in a sweep where it is begun, cov[f][r][0] != 0, source_cov is NULL or source_cov[r][0]
 *   != 0, and all three pivots of S pass (below).  Nothing else of a slot that fails one of the flags is read into a value.
 * THE SWEEP at a pose (q, R, c), per used slot (every 3-term sum is (a + b) + c from the left):
 *     d = Q - qm per component;   y_i = (R_i0 d_x + R_i1 d_y) + R_i2 d_z;   e_i = P_i - (y_i + c_i),  P the (double) of columns 6 - 8
 *     S = Sigma_P (xx xy xz yy yz zz);  with source_cov  T_ij = (R_i0 G_0j + R_i1 G_1j) + R_i2 G_2j  (G = Sigma_Q) and, for i <= j,
 *       S_ij = S_ij + ((T_i0 R_j0 + T_i1 R_j1) + T_i2 R_j2), mirrored
 *     S = L D L' by vbs_shape_series's LDL' (pivot j passes iff d_j > piv_rel S_jj; d_1 = S11 - L10 c10, ..); W = S^-1 column by
 *       column: for j = 0, 1, 2 the forward substitution z_0 = b_0, z_1 = b_1 - L10 z_0, z_2 = (b_2 - L20 z_0) - L21 z_1, y_k = z_k
 *       / d_k of the unit vector b = e_j, then x_2 = y_2, x_1 = y_1 - L21 x_2, x_0 = (y_0 - L10 x_1) - L20 x_2; W_ij = W_ji = x_i for
 *       i <= j (the upper triangle of the columns is the one kept)
 *     u_i = (W_i0 e_x + W_i1 e_y) + W_i2 e_z;   dist = (e_x u_x + e_y u_y) + e_z u_z            (the slot's Mahalanobis distance^2)
 *     M = W B with B = -[y]x, the rotation block of J = [B | I]:
 *       M_i0 = W_i2 y_y - W_i1 y_z     M_i1 = W_i0 y_z - W_i2 y_x     M_i2 = W_i1 y_x - W_i0 y_y
 *     N = B' M, upper:  N_0b = M_2b y_y - M_1b y_z  (b = 0, 1, 2)    N_1b = M_0b y_z - M_2b y_x  (b = 1, 2)    N_22 = M_12 y_x - M_02 y_y
 *     g_0 = u_z y_y - u_y y_z    g_1 = u_x y_z - u_z y_x    g_2 = u_y y_x - u_x y_y    g_3..5 = u
 *   28 sums over the used slots: N [6], M [9], W [6] (xx xy xz yy yz zz), g [6], chi^2 = sum dist; and two counts, begun and used.
 *   A, symmetric 6 x 6 over (omega, c):  A[a][b] = N_ab (a <= b < 3),  A[a][3+i] = M_ia,  A[3+i][3+j] = W_ij.
 * THE ITERATION: sweep k = 0 .. iters.  After a sweep with used >= 3, A = L D L' by the same LDL' at N = 6 with all six pivots
 *   required.  For k < iters the step follows: x = A^-1 g (forward, then back substitution),
 *     h = 0.5 omega per component;  hn = sqrt(((1.0 + h_x h_x) + h_y h_y) + h_z h_z);  a = (1.0 / hn, h_x / hn, h_y / hn, h_z / hn)
 *     q <- a (x) q, Hamilton's product with b = q:   w = ((a_w b_w - a_x b_x) - a_y b_y) - a_z b_z
 *       x = ((a_w b_x + a_x b_w) + a_y b_z) - a_z b_y    y = ((a_w b_y - a_x b_z) + a_y b_w) + a_z b_x    z = ((a_w b_z + a_x b_y) - a_y b_x) + a_z b_w
 *     each divided by sqrt(((w w + x x) + y y) + z z), then vbs_rigid_series's sign rule;  R from q;  c <- c + dc per component
 *     step_rot = the largest of |omega_x|, |omega_y|, |omega_z| and step_c likewise of dc, by comparisons
 *   For k = iters the sweep was at the final pose: its chi^2, its counts and its A are reported; the covariance is A^-1 column by
 *   column (unit vector j through the forward and the back substitution), entry (i, j), i <= j, taken from column j.  flag = 2.
 *   A frame STOPS at flag 1 where a sweep has used < 3 or a pivot of A fails, in any sweep, the last included: the pose is set back
 *   to the start, ONE more sweep runs there, chi2 = chi2_start = its sum, n_used its count, the steps are 0, the covariance is 0 and
 *   column 3 holds the steps taken before the stop.
 *   ml [dev] float64 [fe-fb,VBS_RIGID_ML_COLS] (may be NULL):
 *     0 flag (0 no start, 1 the start only, 2 the weighted fit)   1 n_start (begun)   2 n_used   3 steps taken   4-7 w, x, y, z
 *     8-16 R row-major   17-19 t_i = c_i - ((R_i0 qm_x + R_i1 qm_y) + R_i2 qm_z)   20-22 c   23-25 qm   26 chi2   27 dof = 3 n_used - 6
 *     28 chi2_start: sweep 0's sum, the Horn pose under the same weights   29 step_rot, 30 step_c of the LAST step: what was reached
 *     31 angle_deg, 32 tilt_deg, 33 azimuth_deg, 34 twist_deg by vbs_rigid_series's four expressions (held to 4 ulp)
 *     With n = R z = (R02, R12, R22), Sg = the rotation block of the covariance and G the x, y rows of -[n]x (dn = omega x n):
 *       a_j = n_z Sg_1j - n_y Sg_2j (j = 0, 1, 2)    b_j = n_x Sg_2j - n_z Sg_0j (j = 0, 2)
 *     35 nxx = a_1 n_z - a_2 n_y   36 nxy = a_2 n_x - a_0 n_z   37 nyy = b_2 n_x - b_0 n_z            (Sigma_n = G Sg G', mm-free, rad^2)
 *     38 t2_tilt = (n_x n_x) / nxx + (z2 z2) / d2 with l = nxy / nxx, d2 = nyy - l nxy, z2 = n_y - l n_x, where nxx > 0 and d2 >
 *        piv_rel nyy, else 0: (n_x, n_y) Sigma_n^-1 (n_x, n_y)'.  A tilt is >= 0 and not Gaussian near 0, so t2_tilt decides whether
 *        a frame is tilted, not tilt / sigma (as vbs_pose_cov argues).
 *     39 var_twist = (n_x v_x + n_y v_y) + n_z v_z with v_i = (Sg_i0 n_x + Sg_i1 n_y) + Sg_i2 n_z
 *     Columns 35 - 39 are 0 but at flag 2.  At flag 0 the row holds zeros.
 *   pcov [dev] float64 [fe-fb,VBS_RIGID_ML_PCOV_COLS] (may be NULL) = flag (1 at ml's flag 2, else 0 and zeros), then the 21 upper
 *     entries of the covariance of (omega, c) row by row, in rad^2, rad mm and mm^2.  c is the image of qm; the covariance of t, or of
 *     the image of any other point, follows on the host (rigid.move_centre).
 *   coef [dev] float64 [fe-fb,4,4] (may be NULL) = (flag, R row i), (flag, t) with ml's flag: vbs_rigid_series's FIR record.
 *   mahal [dev] float64 [fe-fb,m_ref,3] (may be NULL) = (1, dist at the final pose, dist at the start) for every slot used in the
 *     last sweep, zeros elsewhere (a slot used at the start only holds zeros); at flag 1 both columns hold the start's.  A record
 *     vbs_field_map_f64, vbs_fir_series_f64, vbs_hampel_series_f64 and vbs_patch_stats_f64 take as it is, with n_values = 2.
 * VBS_EINVAL, before a device is selected and with nothing written: a null table, source, cov, rigid or residual, n or m_ref < 1,
 *   frames outside 0 <= frame_begin <= frame_end <= n, iters outside [1, VBS_RIGID_ML_MAX_ITERS], piv_rel not finite or < 0, all four
 *   outputs NULL.  frame_begin == frame_end emits nothing. */
#define VBS_RIGID_ML_COLS      40   /* flag, n_start, n_used, steps, q [4], R [9], t [3], c [3], qm [3], chi2, dof, chi2_start, 2 steps, 4 angles, Sigma_n [3], t2_tilt, var_twist */
#define VBS_RIGID_ML_PCOV_COLS 22   /* flag, the 21 upper entries of the covariance of (omega, c)            */
#define VBS_RIGID_ML_GROUP     4    /* frames a workgroup takes, one wave each (no result depends on it)     */
#define VBS_RIGID_ML_MAX_ITERS 16   /* Gauss-Newton steps a call may ask for                                 */
int vbs_rigid_ml_series(int device, const float* table, int n, int m_ref, const double* source, const double* cov, const double* rigid,
                        const double* residual, const double* source_cov, int iters, double piv_rel, int frame_begin, int frame_end,
                        double* ml, double* pcov, double* coef, double* mahal, void* stream);

/* Bonnet contact geometry along a recording (ours: the reference ships no code for this): the bonnet is a spherical cap, and a
 * workpiece cuts it by a plane.  Per frame the sphere the markers lie on - fitted, or GIVEN and held -, the CONTACT (the markers that
 * lie inside that sphere by more than contact_depth), the plane through the contact markers alone, and from the two the contact
 * normal, the tool offset, the spot radius and the spot centre.  Handle-free; float64 without contraction; + - * / and sqrt only in
 * everything but columns 24 and 25; no atomics, no LDS, no barrier; every sum over slots follows the rule of vbs_axis_displacement
 * (lane l of 64 adds slots l, l + 64, .. ascending, then the fold 32, 16, 8, 4, 2, 1).  No result depends on the launch shape, on the
 * frame range or on VBS_SPHERE_GROUP (the frames a workgroup takes, one wave each); tests/helpers/sphere_oracle.py restates every
 * expression bit for bit.  The call allocates nothing.
 * vbs_sphere_series - table [dev] float32 [n,m_ref,VBS_TABLE_COLS]; sphere_in [HOST] double [4] = (Cx, Cy, Cz, R) or NULL (fit per
 *   frame); fit_mask [dev] uint8 [m_ref] or NULL (all): the slots the sphere is fitted to, or held against; slot_mask [dev] uint8
 *   [m_ref] or NULL (all): the slots analysed; source [dev] float64 [m_ref,4] = (flag, X, Y, Z) as vbs_rigid_series takes it, or NULL.
 *   A slot is USED (for the fit, for the analysis) when its mask selects it and its row carries VBS_FLAG_XYZ; then P = (double) of
 *   the row's columns 6 - 8.  Nothing else of a row is read into a value, and nothing of a source row whose flag is 0: such cells
 *   may hold NaN, 1e30 or 1e300.  With d = P - C per component, r2 = (dx dx + dy dy) + dz dz and rho = sqrt(r2) - R.
 * THE FIT of a set of slots (sphere_in == NULL; the used fit_mask slots, then once its kept slots):
 *   Sweep 1: count and pm = (sum P) / count per component.  With count < 4 nothing more is summed: no sphere.
 *   Sweep 2: per slot u = P - pm per component and s = (ux ux + uy uy) + uz uz; the 13 sums
 *     Sx, Sy, Sz of u;  Sxx, Sxy, Sxz, Syy, Syz, Szz of the products u_i u_j;  Ss of s;  Sxs, Sys, Szs of u_i s
 *   (the first three kept as computed, not taken as zero); with count as a double they are the 14 sums of the normal equations of
 *   [ux uy uz 1] beta = s in that basis order: N00 = Sxx, N10 = Sxy, N20 = Sxz, N30 = Sx, N11 = Syy, N21 = Syz, N31 = Sy,
 *   N22 = Szz, N32 = Sz, N33 = count, g = (Sxs, Sys, Szs, Ss).
 *   LDL' without square roots and without pivoting exactly as vbs_shape_series states it, j = 0 .. 3:
 *     d_j = N_jj - sum_{k<j} L_jk c_jk;      for i > j:  c_ij = N_ij - sum_{k<j} L_jk c_ik,   L_ij = c_ij / d_j
 *   every inner sum subtracted from the left with k ascending; pivot j PASSES when d_j > piv_rel N_jj and all four must pass.
 *   Forward z_i = g_i - sum_{k<i} L_ik z_k, y_i = z_i / d_i; back beta_3 = y_3, beta_i = y_i - sum_{k>i} L_ki beta_k (k ascending).
 *   c = beta_i / 2.0 (i < 3), kappa = beta_3, C = pm + c per component, R2 = kappa + ((cx cx + cy cy) + cz cz).  A sphere EXISTS iff
 *   count >= 4, four pivots pass and R2 > 0; then R = sqrt(R2).
 *   Sweep 3: SSR = sum rho rho.
 * ONE ROUND OF REJECTION, as vbs_pose_series words it: only when reject_k > 0, a sphere exists and SSR > 0.  Kept are the fit slots
 *   with rho rho <= (reject_k reject_k) (SSR / count), rho the first sphere's: a squared comparison.  If fewer are kept than were
 *   fitted and the kept set, fitted by the same rules, gives a sphere, every quantity is the kept set's, n_fit_used = kept and
 *   rejected = 1; otherwise the first sphere stands with n_fit_used = n_fit and rejected = 0.
 * THE SPHERE GIVEN (sphere_in != NULL): C and R as they are; a sphere always exists; n_fit = n_fit_used = the used fit_mask slots,
 *   SSR = sum rho rho over them (it tells whether the held sphere still fits the rim); piv_rel and reject_k are not read.
 * THE CONTACT, with a sphere: Rc = R - contact_depth.  The contact set is the used slot_mask slots with r2 < Rc Rc, and is empty
 *   unless Rc > 0: squared, no root decides membership.  n_contact; the centroid cm = (sum P) / n_contact per component; per contact
 *   slot the depth R - sqrt(r2) (= -rho); depth_sum by the rule, depth_mean = depth_sum / n_contact, depth_max = R - sqrt(r2min),
 *   r2min the smallest r2 of the set, `deepest` its slot, the smaller slot among equals.
 *   With n_contact >= 3: q = P - cm per component and the six sums Axx, Axy, Axz, Ayy, Ayz, Azz of q_i q_j; tr = (Axx + Ayy) + Azz.
 *   With tr > 0: T = the symmetric 3 x 3 of those sums, V = I, VBS_SPHERE_SWEEPS sweeps of the cyclic Jacobi exactly as vbs_modes'
 *   Ritz step and vbs_rigid_series state it (theta, tt, cs, sn; columns, rows, V's columns, both entries set to 0; a pair with
 *   T[p][q] == 0 is skipped), pairs (0,1) (0,2) (1,2).  k = the index of the SMALLEST T[k][k], the smaller index among equals;
 *   lmin = T[k][k], lmid = the smaller of the other two diagonal entries; gap = (lmid - lmin) / tr.  With v = V[:, k]:
 *   n = v / sqrt((v0 v0 + v1 v1) + v2 v2) (each component divided by the root), dist = (nx (Cx - cmx) + ny (Cy - cmy)) + nz (Cz - cmz);
 *   where dist < 0 all three components of n and dist are negated: n points from the contact towards the centre of the sphere.
 *   A plane EXISTS iff n_contact >= 3, tr > 0, gap > gap_rel and dist > 0 (collinear or coincident contact slots fix no plane).
 * FLAG: 0 no sphere; 1 a sphere and no contact slot; 2 contact without a plane (depths reported, plane columns zero); 3 a plane.
 *   sphere [dev] float64 [fe-fb,VBS_SPHERE_COLS] (may be NULL), zeros where the flag does not allow a column:
 *     0 flag   1 n_fit   2 n_fit_used   3 rejected   4-6 C   7 R   8 rms_fit = sqrt(SSR / n_fit_used) (0 where n_fit_used == 0)
 *     9 n_used (the used slot_mask slots, at every flag)   10 n_contact   11-13 cm   14 depth_sum   15 depth_mean   16 depth_max
 *     17 deepest (-1 without a contact slot)   18-20 n   21 dist   22 offset = R - dist
 *     23 spot_radius = sqrt(max(R R - dist dist, 0))
 *     24 tilt_deg = atan2(sqrt(nx nx + ny ny), nz) 57.29577951308232     25 azimuth_deg = atan2(ny, nx) 57.29577951308232
 *     26-28 the spot centre C - dist n per component   29 plane_rms = sqrt(max(lmin, 0) / n_contact)
 *     30 gap (wherever it was formed: n_contact >= 3 and tr > 0)
 *     Columns 8, 23, 24, 25 and 29 pass through a root or an arc tangent last (held to 4 ulp); every other column is exact.
 *   radial [dev] float64 [fe-fb,m_ref,2] (may be NULL) = (1, rho) for every used slot_mask slot of a frame with a sphere, zeros
 *     elsewhere: a record vbs_field_map_f64, vbs_fir_series_f64, vbs_hampel_series_f64 and the step entries take as it is, with
 *     n_values = 1.
 *   decomp [dev] float64 [fe-fb,m_ref,4] (may be NULL; needs source) = (1, d_n, d_mer, d_az) for every used slot_mask slot of a frame
 *     with a sphere whose source flag is != 0 and whose Q = source[r][1..3] is not the centre; zeros elsewhere.  D = P - Q per
 *     component is resolved in the shell's own frame at Q:  w = Q - C, wn = sqrt((wx wx + wy wy) + wz wz), h = w / wn (the normal);
 *     h2 = hx hx + hy hy; where h2 == 0 exactly e_az = (0, 1, 0) and e_mer = (1, 0, 0); else hh = sqrt(h2),
 *     e_az = (-hy / hh, hx / hh, 0) and e_mer = e_az x h = (az_y hz, -(az_x hz), az_x hy - az_y hx).
 *     d_n = (Dx hx + Dy hy) + Dz hz,  d_mer = (Dx mer_x + Dy mer_y) + Dz mer_z,  d_az = Dx az_x + Dy az_y.  A record with n_values = 3.
 * VBS_EINVAL, before a device is selected and with nothing written: a null table, n or m_ref < 1, frames outside
 *   0 <= frame_begin <= frame_end <= n, contact_depth not finite or <= 0, piv_rel, gap_rel or reject_k not finite or < 0, a sphere_in
 *   with a non-finite entry or R <= 0, decomp without source, all three outputs NULL.  frame_begin == frame_end emits nothing. */
#define VBS_SPHERE_COLS   31    /* flag, n_fit, n_fit_used, rejected, C [3], R, rms_fit, n_used, n_contact, cm [3], 3 depths, deepest,
                                   n [3], dist, offset, spot_radius, tilt, azimuth, spot centre [3], plane_rms, gap */
#define VBS_SPHERE_GROUP  4     /* frames a workgroup takes, one wave each (no result depends on it)     */
#define VBS_SPHERE_SWEEPS 6     /* Jacobi sweeps: one more than the 5 after which every host case is diagonal in bits */
int vbs_sphere_series(int device, const float* table, int n, int m_ref, const double* sphere_in, const uint8_t* fit_mask,
                      const uint8_t* slot_mask, const double* source, double contact_depth, double piv_rel, double gap_rel,
                      double reject_k, int frame_begin, int frame_end, double* sphere, double* radial, double* decomp, void* stream);

/* vbs_refine_markers - centre, area, diameter and axes of every tracked marker measured from the grey levels themselves (ours:
 * the reference has no grey-level measurement; table column 3 is the axis of an ellipse fitted to a thresholded contour).
 * Handle-free, opt-in; vbs_track, vbs_track_to_3d and every other output stay what they are.
 *   gray [dev] uint8 [n,h,w] with strides (a crop view is fine): the frames the detector saw (after vbs_undistort_frames where
 *   that is set).  table [dev] float32 [n,m_ref,VBS_TABLE_COLS] as vbs_track writes it.
 * THE RULE, per table row.  Everything up to the six sums is integer, so nothing depends on an order of summation; a handful of
 * float64 operations without contraction follow.  Every expression and tie-break below is part of the interface.
 *   Setup.  flags = (int)row[0] where 0 <= row[0] < 2^24, else 0.  Cx, Cy, major = the float32 columns 1, 2, 3 widened to double.
 *   1. Geometry.  r = 0.5 major;  x0 = (int)floor(Cx + 0.5), y0 likewise;  R = (int)ceil(ring_f r) + 1;  c2 = floor((core_f r)
 *      (core_f r)), g2 = floor((disc_f r) (disc_f r)), R2 = R R;  d2 = dx dx + dy dy with the integer offsets from (x0, y0).
 *      Core = {d2 <= c2}, disc = {d2 <= g2}, ring = {g2 < d2 <= R2}.
 *   2. Status (rec column 0), the first match wins:
 *        1  not tracked (flags without VBS_FLAG_TRACKED)
 *        2  Cx, Cy or major not finite, major < 2, or |Cx| or |Cy| >= 2^30
 *        3  ceil(ring_f r) + 1 > VBS_REFINE_MAX_R (decided in float64, before the conversion): the window is never truncated
 *        4  the square [x0 - R, x0 + R] x [y0 - R, y0 + R] is not wholly inside the frame: no pixel outside the frame is read
 *        5  low contrast: C8 < 8 min_contrast
 *        6  degenerate: S0 <= 0, or not l2 > 0
 *        7  moved: shift > max_shift_f r
 *        0  refined
 *      A row with status 1 .. 4 costs no pixel load.
 *   3. Levels.  A pixel's level is v, with polarity 1 (bright markers) 255 - v.  For a set of pixels with the level histogram H
 *      and `total` pixels, q(num) is the smallest level whose cumulative count times 4 is >= total num, and
 *        T8(set) = (8 sum{v H[v] : q(1) <= v <= q(3)}) / sum{H[v] : q(1) <= v <= q(3)}        integer division
 *      the mean of the two middle quarters in eighths of a level (whole bins: every pixel AT q(1) or q(3) counts).  B8 = T8(ring),
 *      D8 = T8(core), C8 = B8 - D8.  The ring is trimmed so that a neighbour's edge or a highlight in it does not move the
 *      background level.
 *   4. Sums over the disc, int64:  wgt = min(max(B8 - 8 v, 0), C8);  S0 = sum wgt, Sx = sum wgt dx, Sy = sum wgt dy, Sxx = sum wgt
 *      dx dx, Sxy = sum wgt dx dy, Syy = sum wgt dy dy.
 *   5. Float64, PI = 3.14159265358979323846:
 *        A = (double)S0 / (double)C8;   d_area = 2.0 sqrt(A / PI)                              [status 6 if S0 <= 0]
 *        cx = (double)x0 + (double)Sx / (double)S0, cy likewise;   shift = hypot(cx - Cx, cy - Cy)
 *        mxx = (double)(Sxx S0 - Sx Sx) / ((double)S0 (double)S0), mxy from Sxy S0 - Sx Sy, myy from Syy S0 - Sy Sy (the
 *        numerators are int64)
 *        t = 0.5 (mxx + myy);  hd = 0.5 (mxx - myy);  q = sqrt(hd hd + mxy mxy);  l1 = t + q;  l2 = t - q     [status 6 unless l2 > 0]
 *        k = sqrt(sqrt(l1 / l2));  major' = d_area k;  minor' = d_area / k
 *        angle = (0.5 atan2(2.0 mxy, mxx - myy)) 180.0 / PI + 180.0
 *        edge_var = sqrt(l1 l2) - A / (4.0 PI)
 *      Blur inflates the moments but conserves the integral: the SIZE comes from the area, only the axis ratio and the direction
 *      come from the moments.  edge_var is the excess of the second moment over a sharp ellipse's, about sigma^2 of the optics: a
 *      focus measure.  The angle is table column 5's convention - cv2.fitEllipse's angle plus 90 where its first axis is the shorter
 *      (marker_detection.py:217; k_finalize keeps the shorter axis first, so always): the direction of the MAJOR axis in degrees
 *      from +x towards +y (y down), modulo 180, in [90, 270) there and in (90, 270] here.
 * Outputs, each may be NULL (all three NULL: VBS_EINVAL):
 *   rec [dev] float64 [n,m_ref,VBS_REFINE_COLS] = status, cx, cy, major', minor', angle, d_area, A, B8 / 8.0, D8 / 8.0, edge_var,
 *     shift.  Status 0 and 7: every column.  Status 5: columns 8, 9.  Status 6 with S0 <= 0: columns 6 .. 9; with S0 > 0 also 1, 2
 *     and 11.  Every other cell after column 0 is 0.
 *   sums [dev] int64 [n,m_ref,VBS_REFINE_SUM_COLS] = B8, D8, S0, Sx, Sy, Sxx, Sxy, Syy.  Status 1 .. 4: zeros; status 5: B8, D8.
 *   table_out [dev] float32 [n,m_ref,VBS_TABLE_COLS]: every row has VBS_FLAG_XYZ clear, X, Y, Z = 0 and column 9 (det_index) as it
 *     came, so vbs_solve3d runs on it as on vbs_track's output.  Status 0: flags = VBS_FLAG_TRACKED, columns 1 .. 5 = cx, cy,
 *     major', minor', angle, each cast to float32 once.  Any other status: a gap (columns 0 .. 8 zero) - or, with keep_unrefined
 *     and a status >= 2, the input row's columns 0 .. 5 with VBS_FLAG_XYZ cleared.  The gap is the default: a series that mixes
 *     two estimators with a systematic offset carries steps.
 * Defaults of the shim: core_f 0.5, disc_f 1.5, ring_f 2.0, min_contrast 16, max_shift_f 1.0, polarity 0, keep_unrefined 0.
 * VBS_EINVAL, before a device is selected: a null gray or table, n < 0, m_ref < 1, n m_ref >= 2^30, h or w outside 1 .. 16384,
 * stride_row < w, parameters that are not finite or not 0 < core_f <= disc_f <= ring_f <= 64, min_contrast outside [0.125, 255]
 * (so C8 >= 1 wherever it divides), max_shift_f < 0, polarity or keep_unrefined other than 0 / 1.
 * The bound behind the int64 products at R = VBS_REFINE_MAX_R: a window holds at most 127 x 127 pixels of weight <= 8 x 255 =
 * 2040 and |dx|, |dy| <= 63, so S0 <= 2040 x 16129 < 2^25, |Sx| <= 63 S0 < 2^31 and Sxx <= 3969 S0 < 2^37: Sxx S0 < 2^62 and
 * Sx Sx < 2^62 (tests/test_refine_host.py proves it with Python integers for the all-saturated window). */
#define VBS_REFINE_COLS     12   /* status, cx, cy, major', minor', angle, d_area, A, B8/8, D8/8, edge_var, shift */
#define VBS_REFINE_SUM_COLS 8    /* B8, D8, S0, Sx, Sy, Sxx, Sxy, Syy                                            */
#define VBS_REFINE_MAX_R    63   /* the window is at most 127 x 127: two columns a lane                          */
#define VBS_REFINE_WAVES    4    /* table rows a workgroup takes, one wave each (no result depends on it)        */
#define VBS_REFINE_NOT_TRACKED  1
#define VBS_REFINE_BAD_ROW      2
#define VBS_REFINE_TOO_LARGE    3
#define VBS_REFINE_AT_BORDER    4
#define VBS_REFINE_LOW_CONTRAST 5
#define VBS_REFINE_DEGENERATE   6
#define VBS_REFINE_MOVED        7
int vbs_refine_markers(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row,
                       const float* table, int m_ref, double core_f, double disc_f, double ring_f, double min_contrast,
                       double max_shift_f, int polarity, int keep_unrefined, double* rec, int64_t* sums, float* table_out,
                       void* stream);

/* Frame-0 identity assignment on the device — `MarkerTracker._process_first_frame`
 * (marker_detection.py:275-347; inlined again at tracking.py:106-178): the marker nearest the mean is (0,0), the
 * others' radii are clustered into `num_layers` rings (exact 1-D k-means, the deterministic stand-in for the
 * reference's unseeded KMeans) and each ring is ordered by angle from the member nearest angle 0.
 *   det [dev]     float64 [*count][VBS_DET_COLS] rows of frame 0 as vbs_marker_center / vbs_track_to_3d write them
 *   count [dev]   int32[1] number of rows (a device status s < 0 comes back as m_out = 1000 s)
 *   id_mode       0 = "as_written" (the published `(layer,-1)` key collision: 1 + num_layers IDs), 1 = "full"
 *   ids [dev]     int32 [cap][2] (layer, index) in the reference dict's order; ref_xy [dev] float64 [cap][2] (Ox, Oy):
 *                 the table vbs_track / vbs_track_to_3d take as `ref_xy`
 *   m_out [dev]   int32[1] number of IDs; -1 = no markers ("No markers detected in first frame!"), -2 = cap too small,
 *                 -3 = *count > VBS_IDS_MAX_MARKERS (the kernel keeps every marker in LDS; nothing is truncated)
 * Limits: 1 <= num_layers <= VBS_IDS_MAX_LAYERS, else VBS_EINVAL, decided on the host before any launch (like a null
 * pointer, cap < 1 or another id_mode).  *count lives on the device, so its limit is the kernel's: with m_out < 0 neither
 * `ids` nor `ref_xy` is written.  Only rows < *count and columns 0, 1 (cx, cy) of `det` are read.  With fewer than
 * num_layers + 1 markers every marker but the centre is its own layer (k = max(1, min(num_layers, *count - 1))). */
#define VBS_IDS_MAX_MARKERS 1024
#define VBS_IDS_MAX_LAYERS  16
int vbs_assign_ids(vbs_handle* h, const double* det, const int32_t* count, int num_layers, int id_mode,
                   int32_t* ids, double* ref_xy, int cap, int32_t* m_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VBS_H */
