"""ctypes binding of csrc/libvbs.so (C-ABI: include/vbs.h).  No fallback: a missing library raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvbs.so")

VBS_OK, VBS_EINVAL, VBS_ECAPACITY, VBS_EHIP, VBS_ENOMEM, VBS_EINTERNAL = 0, -1, -2, -3, -4, -5
DET_COLS, TABLE_COLS, DISP_COLS, PLANE_COLS, DEVPLANE_COLS = 6, 10, 5, 5, 9
FLAG_TRACKED, FLAG_XYZ = 1, 2
JPEG_BLOCK_BITS_MAX, JPEG_HEADER_BYTES = 1660, 623
MJPEG_SCAN_ALIGN, MJPEG_SCAN_GUARD, MJPEG_HUFF_SET_BYTES, MJPEG_SUBSEQ_BITS, MJPEG_SHORT = 16, 16, 8928, 1024, 1
SERIES_CHUNK, SERIES_REC_COLS, STATS_COLS, WINDOW_COLS = 32, 5, 5, 4
FIR_MAX_TAPS, FIR_TILE, AXIS_COLS, TOTAL_COLS = 255, 64, 4, 5
STEP_MAX_WINDOW, STEP_MAX_STEPS = 64, 64
POSE_COLS, POSEFIELD_COLS, POSE_GROUP = 8, 6, 8
FIELD_FRAMES, FIELD_MAX_SLOTS, FIELD_MAX_POINTS, PATCH_COLS, PATCH_GROUP = 4, 1024, 65536, 8, 8
PROJ_SLOTS, PROJ_CHUNK, PROJ_ROWS, PROJ_WG_SLOTS, PROJ_MAX_ROWS, PROJ_MAX_FRAMES, PROJ_MAX_SLOTS = 4, 64, 64, 16, 8192, 1048576, 1024
FIT_GROUP, PEAK_COLS = 4, 7
ENV_TILE, ENV_MAX_HALF = 64, 127
KIN_TILE, KIN_MAX_HALF, KIN_MAX_DEGREE = 64, 127, 3
MOM_CHUNK, MOM_WG_SLOTS, MOM_MAX_SLOTS = 32, 16, 1024
MODES_MAX, MODES_MAX_DIM, MODES_SWEEPS, MODES_MAX_ITERS, SCORE_GROUP = 16, 3072, 10, 4096, 8
STRAIN_COLS, LSTRAIN_COLS, MOTION_GROUP, LSTRAIN_GROUP, STRAIN_MAX_NBR = 16, 8, 8, 8, 12
ROBUST_MAX_HALF, ROBUST_TILE = 31, 64
DIAM_COLS, DIAM_STATS_COLS, DIAM_MAX_EXTENT = 24, 5, 512
PNP_SAMPLE, PNP_MAX_POINTS, PNP_MAX_HYPOTHESES, PNP_FEW_POINTS, PNP_NO_HYPOTHESIS = 6, 1024, 4096, 1, 2
CHESS_MAX_CANDIDATES, CHESS_MAX_PATTERN, CHESS_MAX_WIN = 256, 256, 15
CALIB_MAX_VIEWS, CALIB_FEW_VIEWS, CALIB_DEGENERATE = 64, 1, 2
IDS_MAX_MARKERS, IDS_MAX_LAYERS = 1024, 16
RETRACK_MAX, RETRACK_STATE_COLS, RETRACK_INFO_COLS = 1024, 6, 4
UNCERT_CAM, UNCERT_COV_COLS, UNCERT_DCOV_COLS, UNCERT_TOTAL_COLS, UNCERT_GROUP = 16, 7, 8, 8, 4
UNCERT_REF_COLS, UNCERT_WORK_COLS, NOISE_COLS = 55, 61, 10
POSECOV_COLS, POSECOV_GROUP = 17, 4
SHAPE_COLS, SHAPE_GROUP = 24, 4
RIGID_COLS, RIGID_GROUP, RIGID_SWEEPS = 33, 4, 8
RIGID_ML_COLS, RIGID_ML_PCOV_COLS, RIGID_ML_GROUP, RIGID_ML_MAX_ITERS = 40, 22, 4, 16
SPHERE_COLS, SPHERE_GROUP, SPHERE_SWEEPS = 31, 4, 6
REFINE_COLS, REFINE_SUM_COLS, REFINE_MAX_R, REFINE_WAVES = 12, 8, 63, 4
REFINE_NOT_TRACKED, REFINE_BAD_ROW, REFINE_TOO_LARGE, REFINE_AT_BORDER, REFINE_LOW_CONTRAST, REFINE_DEGENERATE, REFINE_MOVED = 1, 2, 3, 4, 5, 6, 7
OPT_GRAY_COEFFS, OPT_FORCE_SEQ_MATCH, OPT_NCC_MARGIN, OPT_STAGE_IMPL, OPT_BLUR_IMPL, OPT_PASS_STREAMS, OPT_LATENCY_FRAMES = 1, 2, 4, 5, 6, 7, 8

# every symbol include/vbs.h declares (tests check the export list against the header)
SYMBOLS = ("vbs_create", "vbs_destroy", "vbs_last_error", "vbs_version", "vbs_contour_lut",
           "vbs_gaussian_taps_q8", "vbs_ncc_template", "vbs_ncc_trim_guard", "vbs_stage_box_geom", "vbs_set_undistort", "vbs_undistort_frames", "vbs_find_markers", "vbs_ncc_map", "vbs_normxcorr2",
           "vbs_profile", "vbs_profile_read", "vbs_frame_stats", "vbs_undistort_points", "vbs_calculate_3d", "vbs_marker_center",
           "vbs_track", "vbs_solve3d", "vbs_track_to_3d", "vbs_displacement", "vbs_displacement_range", "vbs_displacement_f64",
           "vbs_plane_fit", "vbs_assign_ids", "vbs_set_option", "vbs_bgr2gray", "vbs_ncc_counters", "vbs_normxcorr2_general",
           "vbs_stage_tables", "vbs_ellipse_table", "vbs_deviation_plane", "vbs_format_csv", "vbs_mjpeg_probe", "vbs_mjpeg_entropy_batch",
           "vbs_mjpeg_reconstruct", "vbs_jpeg_encode_workspace", "vbs_jpeg_encode", "vbs_draw_tracking",
           "vbs_series_chunks", "vbs_series_stats", "vbs_series_stats_f64", "vbs_series_partial", "vbs_series_merge",
           "vbs_window_means", "vbs_displacement_from_frame", "vbs_mjpeg_scan_batch", "vbs_mjpeg_huffman_device",
           "vbs_step_lut", "vbs_threshold_bits", "vbs_measure_markers", "vbs_pnp_ransac",
           "vbs_chess_workspace", "vbs_chess_corners", "vbs_corner_subpix", "vbs_calibrate_camera",
           "vbs_retrack_workspace", "vbs_retrack",
           "vbs_uncert_points", "vbs_uncert_cov", "vbs_uncert_total", "vbs_pixel_noise", "vbs_pose_cov", "vbs_shape_series", "vbs_rigid_series", "vbs_rigid_ml_series", "vbs_sphere_series", "vbs_refine_markers",
           "vbs_axis_displacement", "vbs_fir_series_f64",
           "vbs_step_response_f64", "vbs_find_steps_f64", "vbs_dwell_stats_f64", "vbs_pose_series",
           "vbs_field_map_f64", "vbs_patch_stats_f64", "vbs_project_series_f64", "vbs_harmonic_fit_f64", "vbs_window_moments_f64", "vbs_window_fit_f64",
           "vbs_poly_moments_f64", "vbs_poly_fit_f64",
           "vbs_motion_series_f64", "vbs_local_strain_f64", "vbs_hampel_series_f64",
           "vbs_cross_moments_f64", "vbs_covariance_f64", "vbs_leading_modes_f64", "vbs_mode_scores_f64")


class Camera(C.Structure):
    """vbs_camera: float32 fields exactly as `MarkerAnalysis.load_parameters` stores them."""
    _fields_ = [("K", C.c_float * 9), ("dist", C.c_float * 5), ("R", C.c_float * 9),
                ("T", C.c_float * 3), ("marker_diameter_mm", C.c_float)]


class VbsError(RuntimeError):
    pass


def status_text(status: int, max_markers: int = 0) -> str:
    """What a negative per-frame status in `counts[]` means (include/vbs.h)."""
    if status == VBS_ECAPACITY:
        return ("the frame exceeds the device workspace (more than 30720 runs in a mask, more than "
                f"{max_markers or 'max_markers'} band components, more than about 512 contours, or a contour thousands of rows "
                "long whose vertex moments would leave 64 bits)")
    if status == VBS_EINTERNAL:
        return ("a kernel's internal hand-shake timed out: the frame's result is not to be trusted (bounded wait expired; "
                "see VBS_EINTERNAL in include/vbs.h)")
    return "unexpected device status"


_lib = None


def lib():
    """Load libvbs.so once.  Raises (never falls back) when the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VbsError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                       f"g.build()'` (hipcc, gfx950). There is no CPU fallback.")
    # torch first: it brings its own HIP runtime (libamdhip64 of the same soname), and the library must bind to THAT copy.
    # Loaded the other way round - this library before torch - the process holds two runtimes and the second one to
    # initialise fails (hipSetDevice: seen with `python __graft_entry__.py --smoke`, where build() loads the library first).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double
    cam_p = C.POINTER(Camera)
    sig = {
        "vbs_create": (i32, [i32, i32, i32, i32, i32, C.POINTER(vp)]),
        "vbs_destroy": (i32, [vp]),
        "vbs_last_error": (C.c_char_p, [vp]),
        "vbs_version": (i32, []),
        "vbs_contour_lut": (i32, [vp]),
        "vbs_gaussian_taps_q8": (i32, [i32, f64, vp]),
        "vbs_ncc_template": (i32, [i32, f64, vp, vp]),
        "vbs_ncc_trim_guard": (i32, [i32, f64, i32, i32, f64, vp]),
        "vbs_stage_box_geom": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "vbs_set_undistort": (i32, [vp, vp, vp, i32, vp, vp]),
        "vbs_undistort_frames": (i32, [vp, vp, i32, i32, i64, i64, vp, vp]),
        "vbs_find_markers": (i32, [vp, vp, i32, i32, i64, i64, vp, vp, vp]),
        "vbs_ncc_map": (i32, [vp, vp, i32, i32, i64, i64, vp, vp]),
        "vbs_normxcorr2": (i32, [vp, vp, i32, vp, vp, vp]),
        "vbs_profile": (i32, [vp, i32]),
        "vbs_profile_read": (i32, [vp, vp, i32]),
        "vbs_frame_stats": (i32, [vp, vp, i32]),
        "vbs_undistort_points": (i32, [i32, vp, i32, cam_p, vp, vp]),
        "vbs_calculate_3d": (i32, [i32, vp, i32, cam_p, vp, vp, vp]),
        "vbs_marker_center": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "vbs_track": (i32, [vp, vp, vp, i32, vp, i32, f64, vp, vp]),
        "vbs_solve3d": (i32, [vp, vp, i32, i32, cam_p, f64, vp]),
        "vbs_track_to_3d": (i32, [vp, vp, i32, i32, i64, i64, vp, i32, f64, cam_p, f64, vp, vp, vp, vp]),
        "vbs_displacement": (i32, [vp, vp, i32, i32, i32, f64, f64, vp, vp]),
        "vbs_displacement_range": (i32, [vp, vp, i32, i32, i32, f64, f64, i32, i32, vp, vp]),
        "vbs_displacement_f64": (i32, [i32, vp, i32, i32, i32, f64, f64, vp, vp]),
        "vbs_plane_fit": (i32, [vp, vp, i32, i32, vp, vp]),
        "vbs_assign_ids": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp]),
        "vbs_set_option": (i32, [vp, i32, i32]),
        "vbs_bgr2gray": (i32, [vp, vp, i32, i64, i64, vp, vp]),
        "vbs_ncc_counters": (i32, [vp, vp, i32]),
        "vbs_normxcorr2_general": (i32, [i32, vp, i32, i32, vp, i32, i32, i32, vp, vp]),
        "vbs_stage_tables": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "vbs_ellipse_table": (i32, [vp, i32, vp]),
        "vbs_deviation_plane": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f64, vp, vp, vp]),
        "vbs_format_csv": (i64, [vp, vp, vp, vp, i32, i64, vp, i64, i32]),
        "vbs_mjpeg_probe": (i32, [vp, i64, vp]),
        "vbs_mjpeg_entropy_batch": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32]),
        "vbs_mjpeg_reconstruct": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, i64, i64, vp]),
        "vbs_mjpeg_scan_batch": (i32, [vp, i64, vp, vp, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32]),
        "vbs_mjpeg_huffman_device": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]),
        "vbs_jpeg_encode_workspace": (i32, [i32, i32, i32, vp, vp, vp]),
        "vbs_jpeg_encode": (i32, [vp, i32, i32, i32, i64, i64, i32, vp, i64, vp, i64, vp, vp, vp]),
        "vbs_draw_tracking": (i32, [vp, i32, i32, i32, i64, i64, vp, i32, vp, vp, i32, vp, vp, vp]),
        "vbs_series_chunks": (i32, [i32, i32]),
        "vbs_series_stats": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "vbs_series_stats_f64": (i32, [i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "vbs_series_partial": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "vbs_series_merge": (i32, [vp, vp, i32, i32, vp, vp, vp]),
        "vbs_window_means": (i32, [vp, vp, i32, i32, vp, i32, vp, vp]),
        "vbs_displacement_from_frame": (i32, [vp, vp, i32, i32, i32, vp, vp]),
        "vbs_axis_displacement": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp, vp]),
        "vbs_fir_series_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, f64, i32, i32, vp, vp]),
        "vbs_step_response_f64": (i32, [i32, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "vbs_find_steps_f64": (i32, [i32, vp, i32, i32, i32, i32, f64, i32, vp, vp]),
        "vbs_dwell_stats_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp]),
        "vbs_pose_series": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, i32, f64, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_field_map_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, vp, i32, f64, i32, i32, vp, vp]),
        "vbs_patch_stats_f64": (i32, [i32, vp, i32, i32, i32, vp, i32, f64, f64, vp, vp]),
        "vbs_project_series_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, vp, vp]),
        "vbs_harmonic_fit_f64": (i32, [i32, vp, i32, i32, i32, i32, i32, f64, vp, vp, vp]),
        "vbs_window_moments_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
        "vbs_window_fit_f64": (i32, [i32, vp, i32, i32, i32, f64, f64, f64, vp, vp]),
        "vbs_poly_moments_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp]),
        "vbs_poly_fit_f64": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp]),
        "vbs_motion_series_f64": (i32, [i32, vp, i32, i32, i32, vp, vp, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_local_strain_f64": (i32, [i32, vp, i32, i32, i32, vp, vp, i32, i32, f64, i32, i32, vp, vp]),
        "vbs_hampel_series_f64": (i32, [i32, vp, i32, i32, i32, i32, i32, i32, f64, f64, i32, i32, vp, vp, vp]),
        "vbs_cross_moments_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, vp, vp]),
        "vbs_covariance_f64": (i32, [i32, vp, i32, i32, i32, i32, f64, vp, vp, vp, vp]),
        "vbs_leading_modes_f64": (i32, [i32, vp, i32, i32, i32, f64, vp, vp, vp, vp, vp, vp]),
        "vbs_mode_scores_f64": (i32, [i32, vp, i32, i32, i32, i32, vp, vp, i32, f64, i32, i32, vp, vp, vp]),
        "vbs_step_lut": (i32, [vp]),
        "vbs_threshold_bits": (i32, [vp, vp, i32, i32, i64, i64, f64, vp, vp]),
        "vbs_measure_markers": (i32, [vp, vp, i32, i32, i64, i64, f64, f64, f64, f64, f64, vp, vp, vp, vp]),
        "vbs_pnp_ransac": (i32, [i32, vp, i32, vp, vp, vp, i32, cam_p, vp, i32, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "vbs_chess_workspace": (i64, [i32, i32, i32]),
        "vbs_chess_corners": (i32, [i32, vp, i32, i32, i32, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vbs_corner_subpix": (i32, [i32, vp, i32, i32, i32, i64, i64, vp, i32, i32, i32, i32, i32, i32, f64, vp, vp]),
        "vbs_calibrate_camera": (i32, [i32, vp, i32, vp, i32, vp, i32, i32, i32, i32] + [vp] * 12),
        "vbs_retrack_workspace": (i64, [i32, i32, i32]),
        "vbs_retrack": (i32, [i32, vp, vp, i32, i32, vp, i32, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vbs_uncert_points": (i32, [i32, vp, i32, cam_p, vp, vp, vp, vp, vp]),
        "vbs_uncert_cov": (i32, [i32, vp, i32, i32, cam_p, vp, i32, vp, i32, i32, f64, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_uncert_total": (i32, [i32, vp, i32, i32, cam_p, vp, i32, vp, i32, i32, vp, f64, i32, i32, vp, vp, vp]),
        "vbs_pixel_noise": (i32, [i32, vp, i32, i32, i32, i32, vp, vp]),
        "vbs_pose_cov": (i32, [i32, vp, i32, i32, i32, vp, vp, vp, i32, f64, f64, cam_p, vp, i32, vp, i32, f64, f64, vp, i32, i32, vp, vp, vp,
                               vp]),
        "vbs_shape_series": (i32, [i32, vp, i32, i32, i32, vp, vp, vp, i32, f64, f64, f64, i32, f64, f64, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_rigid_series": (i32, [i32, vp, i32, i32, vp, vp, i32, f64, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_rigid_ml_series": (i32, [i32, vp, i32, i32, vp, vp, vp, vp, vp, i32, f64, i32, i32, vp, vp, vp, vp, vp]),
        "vbs_sphere_series": (i32, [i32, vp, i32, i32, vp, vp, vp, vp, f64, f64, f64, f64, i32, i32, vp, vp, vp, vp]),
        "vbs_refine_markers": (i32, [i32, vp, i32, i32, i32, i64, i64, vp, i32, f64, f64, f64, f64, f64, i32, i32, vp, vp, vp, vp]),
    }
    for name in SYMBOLS:
        fn = getattr(L, name)            # AttributeError here = stale library
        fn.restype, fn.argtypes = sig[name]
    _lib = L
    return L


def make_camera(K, dist, R, T, marker_diameter_mm=2.0) -> Camera:
    import numpy as np
    cam = Camera()
    cam.K[:] = np.asarray(K, dtype=np.float32).reshape(9).tolist()
    d = np.zeros(5, dtype=np.float32)
    dd = np.asarray(dist, dtype=np.float32).ravel()[:5]
    d[:dd.size] = dd
    cam.dist[:] = d.tolist()
    cam.R[:] = np.asarray(R, dtype=np.float32).reshape(9).tolist()
    cam.T[:] = np.asarray(T, dtype=np.float32).reshape(3).tolist()
    cam.marker_diameter_mm = float(marker_diameter_mm)
    return cam
