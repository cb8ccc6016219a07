// C-ABI of include/vbs.h, the analyses along a FIR record: the entries that take a device index instead of a handle.  Every entry
// answers in the same order: VBS_EINVAL for a bad argument, VBS_ECAPACITY for a shape above a kernel's limit - both without
// touching a device - then it selects the device and launches on `stream`.
#include <cmath>
#include "common.h"

// ---- the predicates the entries share ----------------------------------------------------------------------------------------------
// a record [n, s, cols]: the flag and 1 .. 7 value columns, of which the entry takes the first n_values <= most (7 = all there are)
static inline bool record_ok(int n, int s, int cols, int n_values, int most) {
    return n >= 1 && s >= 1 && cols >= 2 && cols <= 8 && n_values >= 1 && n_values <= most && n_values < cols;
}
static inline bool slots_fit_grid(int s) { return s <= 65535 * 64; }   // (the entries with a grid row per 64 slots and no limit of their own)
static inline bool range_ok(int frame_begin, int frame_end, int n) { return frame_begin >= 0 && frame_end <= n && frame_begin <= frame_end; }
static inline bool coverage_ok(double min_coverage) { return min_coverage > 0.0 && min_coverage <= 1.0; }   // (a NaN fails it)
// the half of a symmetric window, read on the host: finite weights >= 0, the centre > 0
static inline bool half_taps_ok(const double* half, int n_half) {
    for (int i = 0; i < n_half; ++i)
        if (!std::isfinite(half[i]) || !(half[i] >= 0.0)) return false;
    return half[0] > 0.0;
}
static inline int launched() { return hipGetLastError() == hipSuccess ? VBS_OK : VBS_EHIP; }

// ---- the dynamic polishing process (k_filter.hip) ----------------------------------------------------------------------------------
extern "C" int vbs_fir_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* half,
                                  int n_half, double min_coverage, int frame_begin, int frame_end, double* out, void* stream) {
    if (!rec || !half || !out || !record_ok(n, s, cols, n_values, 7) || !slots_fit_grid(s) || n_half < 1 ||
        2 * (int64_t)n_half - 1 > VBS_FIR_MAX_TAPS || !coverage_ok(min_coverage) || !range_ok(frame_begin, frame_end, n))
        return VBS_EINVAL;
    double sw = 0.0;                                     // ascending over k = -h .. h, as the kernel adds den
    for (int k = -(n_half - 1); k <= n_half - 1; ++k) sw = sw + half[k < 0 ? -k : k];
    if (!(sw > 0.0)) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_fir_series(rec, n, s, cols, n_values, half, n_half, min_coverage * sw, frame_begin, frame_end, out,
                          (hipStream_t)stream);
    return launched();
}

// ---- despiking a tracked series (k_robust.hip) ----------------------------------------------------------------------------------
extern "C" int vbs_hampel_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, int half_window,
                                     int min_count, double k_sigma, double min_scale, int frame_begin, int frame_end, double* out,
                                     double* clean, void* stream) {
    if (!rec || !out || !record_ok(n, s, cols, n_values, 7) || !slots_fit_grid(s) || half_window < 0 ||
        half_window > VBS_ROBUST_MAX_HALF || min_count < 1 || min_count > 2 * half_window + 1 || !std::isfinite(k_sigma) ||
        !(k_sigma > 0.0) || !std::isfinite(min_scale) || !(min_scale >= 0.0) || !range_ok(frame_begin, frame_end, n))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_hampel_series(rec, n, s, cols, n_values, half_window, min_count, k_sigma * 1.4826, min_scale, frame_begin, frame_end,
                             out, clean, (hipStream_t)stream);
    return launched();
}

// ---- time-resolved amplitude and phase along a recording (k_envelope.hip) -------------------------------------------------------
extern "C" int vbs_window_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* carrier,
                                      const double* half, int n_half, int frame_begin, int frame_end, double* mom, void* stream) {
    if (!rec || !carrier || !half || !mom || !record_ok(n, s, cols, n_values, 3) || n_half < 1 || n_half - 1 > VBS_ENV_MAX_HALF ||
        !range_ok(frame_begin, frame_end, n) || !half_taps_ok(half, n_half))
        return VBS_EINVAL;
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_PROJ_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_window_moments(rec, n, s, cols, n_values, carrier, half, n_half, frame_begin, frame_end, mom, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_window_fit_f64(int device, const double* mom, int F, int s, int n_values, double sw, double min_coverage,
                                  double det_min, double* fit, void* stream) {
    if (!mom || !fit || F < 1 || s < 1 || n_values < 1 || n_values > 3 || !std::isfinite(sw) || !(sw > 0.0) ||
        !coverage_ok(min_coverage) || !(det_min >= 0.0 && det_min < 0.25))
        return VBS_EINVAL;
    if (F > VBS_PROJ_MAX_FRAMES || s > VBS_PROJ_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_window_fit(mom, F, s, n_values, min_coverage * sw, det_min, fit, (hipStream_t)stream);
    return launched();
}

// ---- marker velocity, acceleration and gap filling (k_kinematics.hip) ------------------------------------------------------------
extern "C" int vbs_poly_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* half,
                                    int n_half, int degree, int frame_begin, int frame_end, double* mom, void* stream) {
    if (!rec || !half || !mom || !record_ok(n, s, cols, n_values, 3) || n_half < 1 || n_half - 1 > VBS_KIN_MAX_HALF || degree < 0 ||
        degree > VBS_KIN_MAX_DEGREE || !range_ok(frame_begin, frame_end, n) || !half_taps_ok(half, n_half))
        return VBS_EINVAL;
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_PROJ_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_poly_moments(rec, n, s, cols, n_values, half, n_half, degree, frame_begin, frame_end, mom, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_poly_fit_f64(int device, const double* mom, const double* rec, int n, int s, int cols, int n_values, int degree,
                                int half_window, const double* thr, int fill_degree, int frame_begin, int frame_end, double* fit,
                                double* filled, void* stream) {
    if (!mom || !rec || !thr || !fit || !record_ok(n, s, cols, n_values, 3) || degree < 0 || degree > VBS_KIN_MAX_DEGREE ||
        half_window < 0 || half_window > VBS_KIN_MAX_HALF || fill_degree < 0 || fill_degree > VBS_KIN_MAX_DEGREE ||
        !range_ok(frame_begin, frame_end, n))
        return VBS_EINVAL;
    for (int k = 0; k <= degree; ++k)
        if (!(thr[k] >= 0.0)) return VBS_EINVAL;                     // (a NaN fails it; +inf switches the order off)
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_PROJ_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_poly_fit(mom, rec, s, cols, n_values, degree, half_window, thr, fill_degree, frame_begin, frame_end, fit, filled,
                        (hipStream_t)stream);
    return launched();
}

// ---- principal modes of the displacement field (k_modes.hip) ----------------------------------------------------------------------
extern "C" int vbs_cross_moments_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* shift,
                                     double* mom, void* stream) {
    if (!rec || !mom || !record_ok(n, s, cols, n_values, 3)) return VBS_EINVAL;
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_MOM_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_cross_moments(rec, n, s, cols, n_values, shift, mom, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_covariance_f64(int device, const double* mom, int s, int n_values, int mode, int min_count, double denom,
                                  const uint8_t* slot_mask, double* cov, uint8_t* ok, void* stream) {
    if (!mom || !cov || s < 1 || n_values < 1 || n_values > 3 || (mode != 0 && mode != 1) || min_count < 2 ||
        (mode == 1 && (!std::isfinite(denom) || !(denom > 0.0))))
        return VBS_EINVAL;
    if (s > VBS_MOM_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_covariance(mom, s, n_values, mode, min_count, denom, slot_mask, cov, ok, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_leading_modes_f64(int device, const double* A, int C, int r, int iters, double tiny, double* work, double* values,
                                     double* modes, double* resid, int32_t* info, void* stream) {
    if (!A || !work || !values || !modes || !resid || !info || C < 1 || r < 1 || r > VBS_MODES_MAX || r > C || iters < 0 ||
        iters > VBS_MODES_MAX_ITERS || !(tiny >= 0.0 && tiny < 1.0))
        return VBS_EINVAL;
    if (C > VBS_MODES_MAX_DIM) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_leading_modes(A, C, r, iters, tiny, work, values, modes, resid, info, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_mode_scores_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* center,
                                   const double* modes, int r, double min_coverage, int frame_begin, int frame_end, double* scores,
                                   double* energy, void* stream) {
    if (!rec || !center || !modes || !scores || !record_ok(n, s, cols, n_values, 3) || r < 1 || r > VBS_MODES_MAX ||
        !coverage_ok(min_coverage) || !range_ok(frame_begin, frame_end, n))
        return VBS_EINVAL;
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_MOM_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_mode_scores(rec, s, cols, n_values, center, modes, r, min_coverage, frame_begin, frame_end, scores, energy,
                           (hipStream_t)stream);
    return launched();
}

// ---- contact maps along a recording (k_field.hip) -------------------------------------------------------------------------------
extern "C" int vbs_field_map_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* W,
                                 const double* wsum, int P, double min_coverage, int frame_begin, int frame_end, double* map,
                                 void* stream) {
    if (!rec || !W || !wsum || !map || !record_ok(n, s, cols, n_values, 3) || P < 1 || !coverage_ok(min_coverage) ||
        !range_ok(frame_begin, frame_end, n))
        return VBS_EINVAL;
    if (s > VBS_FIELD_MAX_SLOTS || P > VBS_FIELD_MAX_POINTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin) {
        const int rc = launch_field_map(rec, s, cols, n_values, W, wsum, P, min_coverage, frame_begin, frame_end, map,
                                        (hipStream_t)stream);
        if (rc != VBS_OK) { (void)hipGetLastError(); return rc; }
    }
    return launched();
}

extern "C" int vbs_patch_stats_f64(int device, const double* map, int F, int P, int n_values, const double* grid_xy, int component,
                                   double sign, double thr, double* patch, void* stream) {
    if (!map || !grid_xy || !patch || F < 1 || P < 1 || n_values < 1 || n_values > 3 || component < -1 || component >= n_values ||
        !(sign == 1.0 || sign == -1.0) || !(thr >= 0.0))
        return VBS_EINVAL;
    if (P > VBS_FIELD_MAX_POINTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_patch_stats(map, F, P, n_values, grid_xy, component, sign, thr, patch, (hipStream_t)stream);
    return launched();
}

// ---- displacement spectra along a recording (k_spectrum.hip) --------------------------------------------------------------------
extern "C" int vbs_project_series_f64(int device, const double* rec, int n, int s, int cols, int n_values, const double* basis,
                                      int R, double* proj, void* stream) {
    if (!rec || !basis || !proj || !record_ok(n, s, cols, n_values, 3) || R < 1) return VBS_EINVAL;
    if (n > VBS_PROJ_MAX_FRAMES || s > VBS_PROJ_MAX_SLOTS || R > VBS_PROJ_MAX_ROWS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_project_series(rec, n, s, cols, n_values, basis, R, proj, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_harmonic_fit_f64(int device, const double* proj, int s, int R, int n_values, int Q, int min_count,
                                    double det_min, double* fit, double* peak, void* stream) {
    if (!proj || (!fit && !peak) || s < 1 || Q < 1 || Q > (VBS_PROJ_MAX_ROWS - 1) / 4 || R != 1 + 4 * Q || n_values < 1 ||
        n_values > 3 || min_count < 3 || !(det_min >= 0.0 && det_min < 0.25))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_harmonic_fit(proj, s, R, n_values, Q, min_count, det_min, fit, peak, (hipStream_t)stream);
    return launched();
}

// ---- shear, torsion and strain along a recording (k_motion.hip): the record's values are dX, dY, dZ, so cols >= 4 ----------------
extern "C" int vbs_motion_series_f64(int device, const double* rec, int n, int s, int cols, const double* pos,
                                     const uint8_t* slot_mask, double reject_k, int frame_begin, int frame_end, double* grad,
                                     double* strain, double* residual, void* stream) {
    if (!rec || !pos || !record_ok(n, s, cols, 3, 3) || !range_ok(frame_begin, frame_end, n) || (!grad && !strain && !residual) ||
        !std::isfinite(reject_k) || reject_k < 0.0)
        return VBS_EINVAL;
    if (s > VBS_FIELD_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_motion_series(rec, s, cols, pos, slot_mask, reject_k, frame_begin, frame_end, grad, strain, residual,
                             (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_local_strain_f64(int device, const double* rec, int n, int s, int cols, const double* pos, const int32_t* nbr,
                                    int K, int min_count, double det_rel, int frame_begin, int frame_end, double* out,
                                    void* stream) {
    if (!rec || !pos || !nbr || !out || !record_ok(n, s, cols, 3, 3) || !range_ok(frame_begin, frame_end, n) || K < 1 ||
        K > VBS_STRAIN_MAX_NBR || min_count < 3 || min_count > K + 1 || !(det_rel >= 0.0 && det_rel < 1.0))
        return VBS_EINVAL;
    if (s > VBS_FIELD_MAX_SLOTS) return VBS_ECAPACITY;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_local_strain(rec, s, cols, pos, nbr, K, min_count, det_rel, frame_begin, frame_end, out, (hipStream_t)stream);
    return launched();
}

// ---- the probe-indentation validation (k_steps.hip) ---------------------------------------------------------------------------
extern "C" int vbs_step_response_f64(int device, const double* rec, int n, int s, int cols, int n_values, int window,
                                     int min_count, double* out, void* stream) {
    if (!rec || !out || !record_ok(n, s, cols, n_values, 7) || !slots_fit_grid(s) || window > VBS_STEP_MAX_WINDOW ||
        min_count < 1 || min_count > window)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_step_response(rec, n, s, cols, n_values, window, min_count, out, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_find_steps_f64(int device, const double* resp, int n, int s, int resp_cols, int window, double thr2,
                                  int max_steps, int32_t* steps, void* stream) {
    if (!resp || !steps || n < 1 || s < 1 || !slots_fit_grid(s) || resp_cols < 2 || resp_cols > 9 || window < 1 ||
        window > VBS_STEP_MAX_WINDOW || !(thr2 >= 0.0) || max_steps < 1 || max_steps > VBS_STEP_MAX_STEPS)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_find_steps(resp, n, s, resp_cols, window, thr2, max_steps, steps, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_dwell_stats_f64(int device, const double* rec, int n, int s, int cols, int n_values, const int32_t* steps,
                                   int steps_rows, int max_steps, int guard, double* out, void* stream) {
    if (!rec || !steps || !out || !record_ok(n, s, cols, n_values, 7) || !slots_fit_grid(s) || (steps_rows != s && steps_rows != 1) ||
        max_steps < 1 || max_steps > VBS_STEP_MAX_STEPS || guard < 0)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_dwell_stats(rec, n, s, cols, n_values, steps, steps_rows, max_steps, guard, out, (hipStream_t)stream);
    return launched();
}

// ---- uncertainty of the 3-D solve (k_uncert.hip) -------------------------------------------------------------------------------
extern "C" int vbs_uncert_points(int device, const double* uvd, int n, const vbs_camera* cam, double* xyz, double* j_obs,
                                 double* j_cam, int32_t* ok, void* stream) {
    if (!uvd || !cam || !xyz || !j_obs || !j_cam || !ok || n < 0) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n) launch_uncert_points(uvd, n, *cam, xyz, j_obs, j_cam, ok, (hipStream_t)stream);
    return launched();
}

// what vbs_uncert_cov and vbs_uncert_total share: the table, the two covariances (read on the host), the gate
static inline bool uncert_ok(const float* table, int n, int m, const vbs_camera* cam, const double* obs_cov, int obs_rows,
                             const double* cam_factor, int q, double min_size, int frame_begin, int frame_end, const double* work) {
    if (!table || !cam || !obs_cov || !work || n < 1 || m < 1 || !slots_fit_grid(m) || (obs_rows != 1 && obs_rows != m) || q < 0 ||
        q > VBS_UNCERT_CAM || (q > 0 && !cam_factor) || std::isnan(min_size) || !range_ok(frame_begin, frame_end, n))
        return false;
    for (int64_t i = 0; i < (int64_t)obs_rows * 6; ++i)
        if (!std::isfinite(obs_cov[i])) return false;
    for (int i = 0; i < VBS_UNCERT_CAM * q; ++i)
        if (!std::isfinite(cam_factor[i])) return false;
    return true;
}
// the observation covariance behind the reference rows of `work`; the copy has left the host array when this returns
static inline double* uncert_stage_obs(const double* obs_cov, int obs_rows, int m, double* work, void* stream) {
    double* obs = work + (int64_t)m * VBS_UNCERT_REF_COLS;
    if (hipMemcpyAsync(obs, obs_cov, sizeof(double) * 6 * (size_t)obs_rows, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
        return nullptr;
    return obs;
}

extern "C" int vbs_uncert_cov(int device, const float* table, int n, int m_ref, const vbs_camera* cam, const double* obs_cov,
                              int obs_rows, const double* cam_factor, int q, int ref_frame, double min_marker_size_px, double piv_rel,
                              int frame_begin, int frame_end, double* work, double* cov, double* dcov, void* stream) {
    if (!uncert_ok(table, n, m_ref, cam, obs_cov, obs_rows, cam_factor, q, min_marker_size_px, frame_begin, frame_end, work) ||
        (!cov && !dcov) || (dcov ? (ref_frame < 0 || ref_frame >= n) : ref_frame != -1) || !std::isfinite(piv_rel) || piv_rel < 0.0)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin) {
        double* obs = uncert_stage_obs(obs_cov, obs_rows, m_ref, work, stream);
        if (!obs) { (void)hipGetLastError(); return VBS_EHIP; }
        launch_uncert_cov(table, m_ref, *cam, obs, obs_rows, cam_factor, q, ref_frame, min_marker_size_px, piv_rel, frame_begin,
                          frame_end, work, cov, dcov, (hipStream_t)stream);
    }
    return launched();
}

extern "C" int vbs_uncert_total(int device, const float* table, int n, int m_ref, const vbs_camera* cam, const double* obs_cov,
                                int obs_rows, const double* cam_factor, int q, int ref_frame, const uint8_t* slot_mask,
                                double min_marker_size_px, int frame_begin, int frame_end, double* work, double* total, void* stream) {
    if (!uncert_ok(table, n, m_ref, cam, obs_cov, obs_rows, cam_factor, q, min_marker_size_px, frame_begin, frame_end, work) ||
        !total || ref_frame < 0 || ref_frame >= n)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin) {
        double* obs = uncert_stage_obs(obs_cov, obs_rows, m_ref, work, stream);
        if (!obs) { (void)hipGetLastError(); return VBS_EHIP; }
        launch_uncert_total(table, m_ref, *cam, obs, obs_rows, cam_factor, q, ref_frame, slot_mask, min_marker_size_px, frame_begin,
                            frame_end, work, total, (hipStream_t)stream);
    }
    return launched();
}

// ---- uncertainty of the pose misalignment (k_posecov.hip) ------------------------------------------------------------------------
extern "C" int vbs_pose_cov(int device, const float* table, int n, int m_ref, int start_frame, const double* ref_disp,
                            const double* ref_xyz, const uint8_t* slot_mask, int shell_mode, double scale, double reject_k,
                            const vbs_camera* cam, const double* obs_cov, int obs_rows, const double* cam_factor, int q,
                            double min_marker_size_px, double piv_rel, const float* ref_rows, int frame_begin, int frame_end,
                            double* work, double* pose, double* pcov, void* stream) {
    if (!uncert_ok(table, n, m_ref, cam, obs_cov, obs_rows, cam_factor, q, min_marker_size_px, frame_begin, frame_end, work) ||
        !ref_disp || !ref_xyz || (!pose && !pcov) || start_frame < 0 || start_frame >= n || (shell_mode != 0 && shell_mode != 1) ||
        !std::isfinite(scale) || !std::isfinite(reject_k) || reject_k < 0.0 || !std::isfinite(piv_rel) || piv_rel < 0.0)
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin) {
        double* obs = uncert_stage_obs(obs_cov, obs_rows, m_ref, work, stream);
        if (!obs) { (void)hipGetLastError(); return VBS_EHIP; }
        launch_pose_cov(table, m_ref, start_frame, ref_disp, ref_xyz, slot_mask, shell_mode, scale, reject_k, *cam, obs, obs_rows,
                        cam_factor, q, min_marker_size_px, piv_rel, ref_rows, frame_begin, frame_end, work, pose, pcov,
                        (hipStream_t)stream);
    }
    return launched();
}

// ---- indentation shape along a recording (k_shape.hip) --------------------------------------------------------------------------
static inline bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

extern "C" int vbs_shape_series(int device, const float* table, int n, int m_ref, int start_frame, const double* ref_disp,
                                const double* ref_xyz, const uint8_t* slot_mask, int shell_mode, double scale, double length,
                                double reject_k, int min_count, double piv_rel, double apex_rel, double max_apex, int frame_begin,
                                int frame_end, double* shape, double* coef, double* residual, void* stream) {
    if (!table || !ref_disp || !ref_xyz || (!shape && !coef && !residual) || n < 1 || m_ref < 1 || !slots_fit_grid(m_ref) ||
        start_frame < 0 || start_frame >= n || !range_ok(frame_begin, frame_end, n) || (shell_mode != 0 && shell_mode != 1) ||
        !std::isfinite(scale) || !finite_nonneg(reject_k) || !std::isfinite(length) || !(length > 0.0) || min_count < 6 ||
        !finite_nonneg(piv_rel) || !finite_nonneg(apex_rel) || !finite_nonneg(max_apex))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_shape_series(table, m_ref, start_frame, ref_disp, ref_xyz, slot_mask, shell_mode, scale, length, reject_k, min_count,
                            piv_rel, apex_rel, max_apex, frame_begin, frame_end, shape, coef, residual, (hipStream_t)stream);
    return launched();
}

// ---- rigid motion along a recording (k_rigid.hip) --------------------------------------------------------------------------------
extern "C" int vbs_rigid_series(int device, const float* table, int n, int m_ref, const double* source, const uint8_t* slot_mask,
                                int with_scale, double reject_k, double gap_rel, int frame_begin, int frame_end, double* rigid,
                                double* coef, double* residual, void* stream) {
    if (!table || !source || n < 1 || m_ref < 1 || !slots_fit_grid(m_ref) || !range_ok(frame_begin, frame_end, n) ||
        (with_scale != 0 && with_scale != 1) || !finite_nonneg(reject_k) || !finite_nonneg(gap_rel) || (!rigid && !coef && !residual))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_rigid_series(table, m_ref, source, slot_mask, with_scale, reject_k, gap_rel, frame_begin, frame_end, rigid, coef,
                            residual, (hipStream_t)stream);
    return launched();
}

// ---- noise-weighted rigid motion along a recording (k_rigid_ml.hip) -----------------------------------------------------------------
extern "C" int vbs_rigid_ml_series(int device, const float* table, int n, int m_ref, const double* source, const double* cov,
                                   const double* rigid, const double* residual, const double* source_cov, int iters, double piv_rel,
                                   int frame_begin, int frame_end, double* ml, double* pcov, double* coef, double* mahal,
                                   void* stream) {
    if (!table || !source || !cov || !rigid || !residual || n < 1 || m_ref < 1 || !slots_fit_grid(m_ref) ||
        !range_ok(frame_begin, frame_end, n) || iters < 1 || iters > VBS_RIGID_ML_MAX_ITERS || !finite_nonneg(piv_rel) ||
        (!ml && !pcov && !coef && !mahal))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_rigid_ml_series(table, m_ref, source, cov, rigid, residual, source_cov, iters, piv_rel, frame_begin, frame_end, ml,
                               pcov, coef, mahal, (hipStream_t)stream);
    return launched();
}

// ---- bonnet contact geometry along a recording (k_sphere.hip) ------------------------------------------------------------------------
extern "C" int vbs_sphere_series(int device, const float* table, int n, int m_ref, const double* sphere_in, const uint8_t* fit_mask,
                                 const uint8_t* slot_mask, const double* source, double contact_depth, double piv_rel, double gap_rel,
                                 double reject_k, int frame_begin, int frame_end, double* sphere, double* radial, double* decomp,
                                 void* stream) {
    if (!table || n < 1 || m_ref < 1 || !slots_fit_grid(m_ref) || !range_ok(frame_begin, frame_end, n) ||
        !(std::isfinite(contact_depth) && contact_depth > 0.0) || !finite_nonneg(piv_rel) || !finite_nonneg(gap_rel) ||
        !finite_nonneg(reject_k) || (decomp && !source) || (!sphere && !radial && !decomp))
        return VBS_EINVAL;
    if (sphere_in && !(std::isfinite(sphere_in[0]) && std::isfinite(sphere_in[1]) && std::isfinite(sphere_in[2]) &&
                       std::isfinite(sphere_in[3]) && sphere_in[3] > 0.0))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (frame_end > frame_begin)
        launch_sphere_series(table, m_ref, sphere_in, fit_mask, slot_mask, source, contact_depth, piv_rel, gap_rel, reject_k,
                             frame_begin, frame_end, sphere, radial, decomp, (hipStream_t)stream);
    return launched();
}

extern "C" int vbs_pixel_noise(int device, const float* table, int n, int m_ref, int frame_begin, int frame_end, double* out,
                               void* stream) {
    if (!table || !out || n < 1 || m_ref < 1 || !slots_fit_grid(m_ref) || !range_ok(frame_begin, frame_end, n)) return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    launch_pixel_noise(table, m_ref, frame_begin, frame_end, out, (hipStream_t)stream);
    return launched();
}

// ---- grey-level refinement of tracked markers (k_refine.hip) ---------------------------------------------------------------------
extern "C" int vbs_refine_markers(int device, const uint8_t* gray, int n, int h, int w, int64_t stride_n, int64_t stride_row,
                                  const float* table, int m_ref, double core_f, double disc_f, double ring_f, double min_contrast,
                                  double max_shift_f, int polarity, int keep_unrefined, double* rec, int64_t* sums,
                                  float* table_out, void* stream) {
    if (!gray || !table || (!rec && !sums && !table_out) || n < 0 || m_ref < 1 || (int64_t)n * m_ref >= (1 << 30) || h < 1 || w < 1 ||
        h > 16384 || w > 16384 || stride_row < w || !std::isfinite(core_f) || !std::isfinite(disc_f) || !std::isfinite(ring_f) ||
        !(core_f > 0.0) || !(core_f <= disc_f) || !(disc_f <= ring_f) || !(ring_f <= 64.0) || !(min_contrast >= 0.125) ||
        !(min_contrast <= 255.0) || !std::isfinite(max_shift_f) || !(max_shift_f >= 0.0) || (polarity != 0 && polarity != 1) ||
        (keep_unrefined != 0 && keep_unrefined != 1))
        return VBS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return VBS_EHIP;
    if (n)
        launch_refine(gray, n, h, w, stride_n, stride_row, table, m_ref, core_f, disc_f, ring_f, min_contrast, max_shift_f, polarity,
                      keep_unrefined, rec, (i64*)sums, table_out, (hipStream_t)stream);
    return launched();
}
