"""Thin torch-facing wrapper over the C-ABI: tensors are buffers, all compute is in libvbs.so.

One `Engine` = one `vbs_handle` = one (device, frame size).  Every method enqueues on the current
torch stream of the engine's device and returns device tensors (no synchronisation except where a
host value is needed to raise the reference's exceptions).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .analysis import _device, _frame_range, _ptr
from .analysis import (KIN_PIV_REL, covariance_f64, cross_moments_f64, dwell_stats_f64, field_map_f64, find_steps_f64,  # noqa: F401
                       fir_series_f64, hampel_series_f64, harmonic_fit_f64, kin_thresholds, leading_modes_f64, local_strain_f64,
                       mode_scores_f64, motion_series_f64, n_kin_sums, patch_stats_f64, poly_fit_f64, poly_moments_f64,
                       project_series_f64, step_response_f64, taps_sum, window_fit_f64, window_moments_f64)
from .analysis import pixel_noise, pose_cov, rigid_ml_series, rigid_series, shape_series, solve3d_cov, solve3d_jacobian, sphere_series  # noqa: F401
# the wrappers' argument checkers, under the names the host tests have held them to since before they moved
from .analysis import (_covariance_args, _envelope_args, _envelope_fit_args, _field_args, _fit_args, _kin_args,  # noqa: F401
                       _kin_fit_args, _lstrain_args, _modes_args, _moments_args, _motion_args, _patch_args, _project_args,
                       _posecov_args, _rigid_args, _rigid_ml_args, _robust_args, _scores_args, _shape_args, _sphere_args, _uncert_args)


class Engine:
    def __init__(self, height: int, width: int, max_markers: int = 512, max_batch: int = 16,
                 device: int | torch.device | None = None):
        if not torch.cuda.is_available():
            raise L.VbsError("no GPU visible: vbs_amd has no CPU path (the oracle lives in oracle/ and "
                             "is test-only)")
        self.lib = L.lib()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index or 0)
        self.H, self.W = int(height), int(width)
        self.max_markers, self.max_batch = int(max_markers), int(max_batch)
        self.pass_streams = 2                           # the library's default for VBS_OPT_PASS_STREAMS (see set_option)
        h = C.c_void_p()
        rc = self.lib.vbs_create(self.device.index, self.H, self.W, self.max_markers, self.max_batch,
                                 C.byref(h))
        self._h = h
        if rc != L.VBS_OK:
            msg = self.lib.vbs_last_error(h).decode() if h else "vbs_create failed"
            if h:
                self.lib.vbs_destroy(h)
                self._h = None
            raise (ValueError if rc == L.VBS_EINVAL else L.VbsError)(f"vbs_create: {msg} (status {rc})")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vbs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc == L.VBS_OK:
            return
        msg = self.lib.vbs_last_error(self._h).decode()
        raise (ValueError if rc == L.VBS_EINVAL else L.VbsError)(f"{what}: {msg} (status {rc})")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _frames(self, frames: torch.Tensor):
        """uint8 device tensor [N,H,W] or [N,H,W,3] (a crop view is fine) -> (ptr, n, ch, strides)."""
        if frames.dtype != torch.uint8 or frames.device != self.device:
            raise ValueError("frames must be a uint8 tensor on the engine's device")
        if frames.dim() == 2 or (frames.dim() == 3 and frames.shape[-1] == 3 and frames.shape[0] == self.H
                                 and frames.shape[1] == self.W):
            frames = frames.unsqueeze(0)
        ch = 1
        if frames.dim() == 4:
            ch = frames.shape[3]
            if ch not in (1, 3) or frames.stride(3) != 1 or frames.stride(2) != ch:
                raise ValueError("frames must be [N,H,W] or channel-last [N,H,W,3] with unit pixel stride")
        elif frames.dim() != 3 or frames.stride(2) != 1:
            raise ValueError("frames must be [N,H,W] or [N,H,W,3] with unit pixel stride")
        if frames.shape[1] != self.H or frames.shape[2] != self.W:
            raise ValueError(f"engine was built for {self.H}x{self.W}, got {tuple(frames.shape[1:3])}")
        return frames, frames.shape[0], ch, frames.stride(0), frames.stride(1)

    # ---- a2 / f3 ----------------------------------------------------------------------------
    def set_undistort(self, K=None, dist=None):
        """Enable (K, dist given) or disable (K None) frame undistortion; returns the new camera matrix [3,3]."""
        if K is None:
            self._check(self.lib.vbs_set_undistort(self._h, None, None, 0, None, self._stream()), "vbs_set_undistort")
            return None
        Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))
        dd = np.ascontiguousarray(np.asarray([] if dist is None else dist, dtype=np.float64).ravel()[:5])
        newK = np.zeros(9, dtype=np.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_set_undistort(self._h, Kd.ctypes.data_as(C.c_void_p),
                                                   dd.ctypes.data_as(C.c_void_p) if dd.size else None, int(dd.size),
                                                   newK.ctypes.data_as(C.c_void_p), self._stream()), "vbs_set_undistort")
        return newK.reshape(3, 3)

    def undistort_frames(self, frames):
        frames, n, ch, sn, sr = self._frames(frames)
        shape = (n, self.H, self.W) + ((ch,) if frames.dim() == 4 else ())
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_undistort_frames(self._h, _ptr(frames), n, ch, sn, sr, _ptr(out), self._stream()),
                        "vbs_undistort_frames")
        return out

    # ---- a3-a8 -------------------------------------------------------------------------------
    def bgr2gray(self, frames):
        """cv2.cvtColor(BGR2GRAY) of [N,H,W,3] frames -> uint8 [N,H,W] (coefficient set: OPT_GRAY_COEFFS)."""
        frames, n, ch, sn, sr = self._frames(frames)
        if ch != 3:
            raise ValueError("bgr2gray needs 3-channel frames")
        out = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_bgr2gray(self._h, _ptr(frames), n, sn, sr, _ptr(out), self._stream()), "vbs_bgr2gray")
        return out

    def find_markers(self, frames):
        frames, n, ch, sn, sr = self._frames(frames)
        mask = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=self.device)
        area = torch.empty_like(mask)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_find_markers(self._h, _ptr(frames), n, ch, sn, sr, _ptr(mask), _ptr(area),
                                                  self._stream()), "vbs_find_markers")
        return mask, area

    def ncc_map(self, frames):
        frames, n, ch, sn, sr = self._frames(frames)
        out = torch.empty((n, self.H, self.W), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_ncc_map(self._h, _ptr(frames), n, ch, sn, sr, _ptr(out), self._stream()),
                        "vbs_ncc_map")
        return out

    def normxcorr2(self, area_mask, want_mask=False):
        """NCC of a two-valued uint8 area_mask [n,H,W] with the branch template -> float64 map."""
        if area_mask.dim() == 2:
            area_mask = area_mask.unsqueeze(0)
        if area_mask.dtype != torch.uint8 or area_mask.device != self.device or not area_mask.is_contiguous() \
                or tuple(area_mask.shape[1:]) != (self.H, self.W):
            raise ValueError("area_mask must be a contiguous uint8 [n,H,W] tensor on the engine's device")
        n = area_mask.shape[0]
        out = torch.empty((n, self.H, self.W), dtype=torch.float64, device=self.device)
        mask = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=self.device) if want_mask else None
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_normxcorr2(self._h, _ptr(area_mask), n, _ptr(out), _ptr(mask),
                                                self._stream()), "vbs_normxcorr2")
        return (out, mask) if want_mask else out

    def set_option(self, option: int, value: int):
        """`vbs_set_option`: L.OPT_GRAY_COEFFS (15 | 14), test hooks L.OPT_FORCE_SEQ_MATCH,
        L.OPT_NCC_MARGIN (units of 1e-6), L.OPT_STAGE_IMPL / L.OPT_BLUR_IMPL (0 | 1), L.OPT_PASS_STREAMS (1 | 2),
        L.OPT_LATENCY_FRAMES (0 .. 32: passes of at most that many frames take the several-workgroups-per-frame labelling kernel).
        (The NCC kernel's skipping of empty windows has no option: the handle decides it once, `vbs_ncc_trim_guard`.)"""
        self._check(self.lib.vbs_set_option(self._h, int(option), int(value)), "vbs_set_option")
        if int(option) == L.OPT_PASS_STREAMS:
            self.pass_streams = int(value)

    def profile(self, enable: bool):
        self._check(self.lib.vbs_profile(self._h, 1 if enable else 0), "vbs_profile")

    def profile_read(self):
        """{kernel: (launches, total_ms)} from the HIP events recorded since profile(True)."""
        buf = C.create_string_buffer(8192)
        self._check(self.lib.vbs_profile_read(self._h, buf, len(buf)), "vbs_profile_read")
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out

    def frame_stats(self, n):
        out = np.zeros((n, 8), dtype=np.uint32)
        self._check(self.lib.vbs_frame_stats(self._h, out.ctypes.data_as(C.c_void_p), n), "vbs_frame_stats")
        return out

    def stage_tables(self, n):
        """Host copies of the labelling kernels' per-component tables for the first n frames of the last internal pass
        (`vbs_stage_tables`, diagnostic): dict of ncomp [n,2], band_sums [n,M,4], area_first [n,M], area_sums [n,M,16],
        probe [n,M,4], slow [n]."""
        M = self.max_markers
        t = {"ncomp": np.zeros((n, 2), np.uint32), "band_sums": np.zeros((n, M, 4), np.uint64),
             "area_first": np.zeros((n, M), np.uint32), "area_sums": np.zeros((n, M, 16), np.int64),
             "probe": np.zeros((n, M, 4), np.uint16), "slow": np.zeros((n,), np.uint32)}
        self._check(self.lib.vbs_stage_tables(self._h, n, *(t[k].ctypes.data_as(C.c_void_p) for k in
                                                            ("ncomp", "band_sums", "area_first", "area_sums", "probe", "slow"))),
                    "vbs_stage_tables")
        return t

    def ellipse_table(self, n):
        """Host copy of the ellipse table of the first n frames of the last internal pass (`vbs_ellipse_table`, diagnostic):
        float64 [n,M,8] = cx, cy, w, h, angle, contour vertices, fitted (0 | 1), spare; rows in `stage_tables` order."""
        out = np.zeros((n, self.max_markers, 8), dtype=np.float64)
        self._check(self.lib.vbs_ellipse_table(self._h, n, out.ctypes.data_as(C.c_void_p)), "vbs_ellipse_table")
        return out

    def ncc_counters(self, reset=False):
        """{ambiguous, exact, frames} over every detection pass since the last reset (`vbs_ncc_counters`)."""
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.vbs_ncc_counters(self._h, out.ctypes.data_as(C.c_void_p), 1 if reset else 0),
                    "vbs_ncc_counters")
        return {"ambiguous": int(out[0]), "exact": int(out[1]), "frames": int(out[2])}

    # ---- a9-a13 ------------------------------------------------------------------------------
    def marker_center(self, mask, area_mask):
        for t in (mask, area_mask):
            if t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous():
                raise ValueError("mask / area_mask must be contiguous uint8 tensors on the engine's device")
        if mask.dim() == 2:
            mask, area_mask = mask.unsqueeze(0), area_mask.unsqueeze(0)
        n = mask.shape[0]
        if tuple(mask.shape[1:]) != (self.H, self.W) or mask.shape != area_mask.shape:
            raise ValueError("mask shape mismatch")
        det = torch.zeros((n, self.max_markers, L.DET_COLS), dtype=torch.float64, device=self.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_marker_center(self._h, _ptr(mask), _ptr(area_mask), n, _ptr(det),
                                                   _ptr(counts), self._stream()), "vbs_marker_center")
        return det, counts

    # ---- a15 ---------------------------------------------------------------------------------
    # ---- diameter validation (Precision_Validation/DiameterValidation.py) ------------------------
    def threshold_bits(self, frames, threshold):
        """The first step of `measure_markers` alone: GaussianBlur 5x5 + THRESH_BINARY_INV as bit-packed masks, int64 tensor
        [n, H, ceil(W / 64)] (the words are unsigned; bit x % 64 of word x // 64 = pixel x)."""
        frames, n, ch, sn, sr = self._frames(frames)
        bits = torch.zeros((n, self.H, (self.W + 63) // 64), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_threshold_bits(self._h, _ptr(frames), n, ch, sn, sr, float(threshold), _ptr(bits),
                                                    self._stream()), "vbs_threshold_bits")
        return bits

    def measure_markers(self, frames, threshold, scale, min_area=100, min_circularity=0.85, offset_mm=0.0):
        """`measure_markers` (DiameterValidation.py:113-144, after the blur of :218) for every frame of a batch: records
        [n, max_markers, DIAM_COLS] float64 (include/vbs.h lists the columns), counts [n] int32 (rows per frame, or a negative
        status), stats [n, 5] float64 (count, mean, np.std, min, max of diameter_mm).  Device tensors, no synchronisation."""
        frames, n, ch, sn, sr = self._frames(frames)
        rec = torch.zeros((n, self.max_markers, L.DIAM_COLS), dtype=torch.float64, device=self.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=self.device)
        stats = torch.zeros((n, L.DIAM_STATS_COLS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_measure_markers(self._h, _ptr(frames), n, ch, sn, sr, float(threshold), float(min_area),
                                                     float(min_circularity), float(scale), float(offset_mm), _ptr(rec),
                                                     _ptr(counts), _ptr(stats), self._stream()), "vbs_measure_markers")
        return rec, counts, stats

    # ---- chessboard corners (Marker_Calibration/intrinsic_calibration.py, DiameterValidation.calculate_scale) ----
    def _gray_batch(self, frames):
        """uint8 [H,W] | [H,W,3] | [N,H,W] | [N,H,W,3], array or tensor, strided views included -> gray device tensor [N,H,W]
        with unit pixel stride (BGR through k_gray)."""
        f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.asarray(frames))
        if f.dtype != torch.uint8:
            raise ValueError("frames must be uint8")
        if f.dim() == 2 or (f.dim() == 3 and f.shape[-1] == 3 and tuple(f.shape[:2]) == (self.H, self.W)):
            f = f.unsqueeze(0)
        f = f.to(self.device)
        if f.stride(-1) != 1 or (f.dim() == 4 and f.stride(2) != 3):
            f = f.contiguous()
        f, n, ch, _, _ = self._frames(f)
        return self.bgr2gray(f) if ch == 3 else f

    def find_chessboard_corners(self, frames, pattern_size, want_response=False):
        """`cv2.findChessboardCorners(gray, pattern_size)` for every frame of a batch (`vbs_chess_corners`; include/vbs.h says
        what is restated): (found int32 [n], corners float64 [n, pw*ph, 2], peaks int32 [n, pw*ph, 2], n_candidates int32 [n])
        as device tensors, and the int32 response map [n, H, W] as a fifth with `want_response`.  corners are NaN and peaks -1
        where found is 0.  No synchronisation."""
        pw, ph = int(pattern_size[0]), int(pattern_size[1])
        g = self._gray_batch(frames)
        n = g.shape[0]
        k = max(pw * ph, 0)
        corners = torch.empty((n, k, 2), dtype=torch.float64, device=self.device)
        peaks = torch.empty((n, k, 2), dtype=torch.int32, device=self.device)
        found = torch.empty((n,), dtype=torch.int32, device=self.device)
        ncand = torch.empty((n,), dtype=torch.int32, device=self.device)
        resp = torch.empty((n, self.H, self.W), dtype=torch.int32, device=self.device) if want_response else None
        nbytes = int(self.lib.vbs_chess_workspace(n, self.H, self.W))
        if nbytes < 0:
            raise ValueError(f"vbs_chess_workspace: frames of {self.H} x {self.W} are outside 1..16384 pixels a side (status {nbytes})")
        ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.vbs_chess_corners(self.device.index, _ptr(g), n, self.H, self.W, g.stride(0), g.stride(1), pw, ph,
                                            _ptr(corners), _ptr(found), _ptr(peaks), _ptr(ncand), _ptr(resp), _ptr(ws),
                                            self._stream())
        if rc == L.VBS_ECAPACITY:
            raise L.VbsError(f"vbs_chess_corners: a pattern of {pw} x {ph} corners exceeds VBS_CHESS_MAX_PATTERN = "
                             f"{L.CHESS_MAX_PATTERN} (status {rc})")
        if rc != L.VBS_OK:
            raise (ValueError if rc == L.VBS_EINVAL else L.VbsError)(f"vbs_chess_corners: bad argument or HIP error (status {rc})")
        return (found, corners, peaks, ncand) + ((resp,) if want_response else ())

    def corner_subpix(self, frames, corners, win=(11, 11), zero_zone=(-1, -1), max_iter=30, eps=1e-3, want_iters=False):
        """`cv2.cornerSubPix(gray, corners, win, zero_zone, (EPS + MAX_ITER, max_iter, eps))` for k corners in each frame of a
        batch (`vbs_corner_subpix`): corners [n, k, 2] ([k, 2] or cv2's [k, 1, 2] for one frame), array or tensor -> a NEW float64
        device tensor [n, k, 2]; with `want_iters` also the solves done per corner, int32 [n, k]."""
        g = self._gray_batch(frames)
        n = g.shape[0]
        c = corners if isinstance(corners, torch.Tensor) else torch.from_numpy(np.asarray(corners))
        c = c.to(device=self.device, dtype=torch.float64).reshape(n, -1, 2).contiguous().clone()
        k = c.shape[1]
        iters = torch.zeros((n, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.vbs_corner_subpix(self.device.index, _ptr(g), n, self.H, self.W, g.stride(0), g.stride(1), _ptr(c), k,
                                            int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), int(max_iter),
                                            float(eps), _ptr(iters), self._stream())
        if rc != L.VBS_OK:
            raise (ValueError if rc == L.VBS_EINVAL else L.VbsError)(
                f"vbs_corner_subpix: bad argument (window half-sizes 1..{L.CHESS_MAX_WIN}) or HIP error (status {rc})")
        return (c, iters) if want_iters else c

    # ---- grey-level refinement of the tracked markers (k_refine.hip; the rule: include/vbs.h) ----
    def refine_markers(self, frames, table, want=("rec", "sums", "table"), **params):
        """Centre, area, diameter and axes of every tracked row of `table` measured from the grey levels of `frames`
        (`vbs_refine_markers`): threshold-free, normalised by each marker's own local contrast.  frames: gray or BGR (BGR goes
        through k_gray), uint8 tensor or array, [n,H,W(,3)] or one frame, strided crops included.  They must be THE FRAMES THE
        DETECTOR SAW: after `undistort_frames` when undistortion is set on the engine, and the crop the table's coordinates
        refer to.  table float32 [n, m, 10] as `track` / `track_to_3d` return it (not modified).  `params`: core_f, disc_f,
        ring_f, min_contrast, max_shift_f, polarity, keep_unrefined (`refine.DEFAULTS`), and `passes` (default 1): the rule
        assumes a start within a pixel or two of the truth - its disc is 1.5 x the START's radius - which the detector's
        diameter is not at low contrast; with passes = k the rule runs k times, each pass starting from the rows the pass
        before wrote (a row it could not refine keeps its start until the last pass, which applies `keep_unrefined`); `rec` and
        `sums` are the last pass's, so `shift` is the last pass's step.
        Returns (rec float64 [n, m, 12], sums int64 [n, m, 8], table float32 [n, m, 10]) as device tensors - None for those
        not in `want`; the returned table is `track`'s format with X, Y, Z unset, for `solve3d`.  No synchronisation."""
        from .refine import params as _params
        p = _params(True, **params)
        passes = p.pop("passes", 1)
        unknown = sorted(set(want) - {"rec", "sums", "table"})
        if unknown or not want:
            raise ValueError(f"refine_markers: want is a non-empty subset of rec, sums, table (got {list(want)})")
        g = self._gray_batch(frames)
        n = g.shape[0]
        t = table if isinstance(table, torch.Tensor) else torch.from_numpy(np.asarray(table, dtype=np.float32))
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[0] != n or t.shape[2] != L.TABLE_COLS or t.shape[1] < 1:
            raise ValueError(f"table must be [n = {n}, m >= 1, {L.TABLE_COLS}] for these frames")
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        m = t.shape[1]
        rec = torch.empty((n, m, L.REFINE_COLS), dtype=torch.float64, device=self.device) if "rec" in want else None
        sums = torch.empty((n, m, L.REFINE_SUM_COLS), dtype=torch.int64, device=self.device) if "sums" in want else None
        out = torch.empty((n, m, L.TABLE_COLS), dtype=torch.float32, device=self.device) if "table" in want else None
        mid = torch.empty_like(t) if passes > 1 else None
        with torch.cuda.device(self.device):
            for k in range(passes):
                last = k == passes - 1
                rc = self.lib.vbs_refine_markers(self.device.index, _ptr(g), n, self.H, self.W, g.stride(0), g.stride(1), _ptr(t), m,
                                                 p["core_f"], p["disc_f"], p["ring_f"], p["min_contrast"], p["max_shift_f"],
                                                 p["polarity"], p["keep_unrefined"] if last else 1, _ptr(rec) if last else None,
                                                 _ptr(sums) if last else None, _ptr(out) if last else _ptr(mid), self._stream())
                if rc != L.VBS_OK:
                    raise (ValueError if rc == L.VBS_EINVAL else L.VbsError)(
                        f"vbs_refine_markers: bad argument or HIP error (status {rc})")
                if not last:
                    t, mid = mid, (torch.empty_like(t) if k == 0 else t)      # (never write into the caller's table)
        return rec, sums, out

    def track(self, det, counts, ref_xy, min_dist=20.0):
        ref = torch.as_tensor(ref_xy, dtype=torch.float64, device=self.device).contiguous().reshape(-1, 2)
        if det.dtype != torch.float64 or not det.is_contiguous() or det.device != self.device or det.dim() != 3 \
                or tuple(det.shape[1:]) != (self.max_markers, L.DET_COLS):
            raise ValueError(f"det must be a contiguous float64 tensor [n, {self.max_markers}, {L.DET_COLS}] on the "
                             "engine's device")
        if counts.dtype != torch.int32 or counts.device != self.device or not counts.is_contiguous() \
                or counts.numel() != det.shape[0]:
            raise ValueError("counts must be a contiguous int32 tensor [n] on the engine's device")
        n, m = det.shape[0], ref.shape[0]
        table = torch.empty((n, m, L.TABLE_COLS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_track(self._h, _ptr(det), _ptr(counts), n, _ptr(ref), m, float(min_dist),
                                           _ptr(table), self._stream()), "vbs_track")
        return table

    # ---- a19-a20 -----------------------------------------------------------------------------
    def solve3d(self, table, cam: L.Camera, min_marker_size_px=5.0):
        n, m = table.shape[0], table.shape[1]
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_solve3d(self._h, _ptr(table), n, m, C.byref(cam), float(min_marker_size_px),
                                             self._stream()), "vbs_solve3d")
        return table

    # ---- fused ---------------------------------------------------------------------------------
    def track_to_3d(self, frames, ref_xy=None, min_dist=20.0, cam: L.Camera | None = None,
                    min_marker_size_px=5.0, want_det=False):
        frames, n, ch, sn, sr = self._frames(frames)
        table = ref = None
        m = 0
        if ref_xy is not None:
            ref = torch.as_tensor(ref_xy, dtype=torch.float64, device=self.device).contiguous().reshape(-1, 2)
            m = ref.shape[0]
            table = torch.empty((n, m, L.TABLE_COLS), dtype=torch.float32, device=self.device)
        det = torch.zeros((n, self.max_markers, L.DET_COLS), dtype=torch.float64,
                          device=self.device) if want_det else None
        counts = torch.zeros((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_track_to_3d(
                self._h, _ptr(frames), n, ch, sn, sr, _ptr(ref), m, float(min_dist),
                C.byref(cam) if cam is not None else None, float(min_marker_size_px), _ptr(table), _ptr(det),
                _ptr(counts), self._stream()), "vbs_track_to_3d")
        return table, det, counts

    # ---- the annotated video (`_draw_tracking`, marker_detection.py:398-427) ----------------------
    def draw_tracking(self, frames, det, table, ref_xy):
        """The reference's `_draw_tracking` on every tracked slot of every frame, in slot order: frames uint8 [n,H,W,3] BGR
        on the device (a crop view is fine; not modified), det [n,max_markers,6] float64 / table [n,m,10] float32 as
        `track_to_3d(..., want_det=True)` returns them, ref_xy [m,2] -> a new dense uint8 [n,H,W,3] tensor."""
        frames, n, ch, sn, sr = self._frames(frames)
        if ch != 3 or frames.dim() != 4:
            raise ValueError("draw_tracking needs BGR frames [n,H,W,3] (the reference only draws on colour frames)")
        ref = torch.as_tensor(ref_xy, dtype=torch.float64, device=self.device).contiguous().reshape(-1, 2)
        m = ref.shape[0]
        if (det.dtype != torch.float64 or det.dim() != 3 or det.shape[0] < n or det.shape[2] != L.DET_COLS
                or not det.is_contiguous() or det.device != self.device):
            raise ValueError("det must be a contiguous float64 device tensor [n,max_markers,6]")
        if (table.dtype != torch.float32 or tuple(table.shape) != (n, m, L.TABLE_COLS) or not table.is_contiguous()
                or table.device != self.device):
            raise ValueError("table must be a contiguous float32 device tensor [n,m_ref,10] matching ref_xy")
        need = n * self.H * self.W
        if getattr(self, "_lastw", None) is None or self._lastw.numel() < need:
            self._lastw = torch.empty(need, dtype=torch.int32, device=self.device)
        out = torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_draw_tracking(_ptr(frames), n, self.H, self.W, sn, sr, _ptr(det), det.shape[1],
                                                   _ptr(table), _ptr(ref), m, _ptr(self._lastw), _ptr(out), self._stream()),
                        "vbs_draw_tracking")
        return out

    # ---- a21, f1 -------------------------------------------------------------------------------
    def displacement(self, table, warmup_frames=100, min_marker_size_px=5.0, max_displacement=50.0,
                     frame_range=None):
        """Last-seen displacement of `table` [n,m,10]; `frame_range=(a, b)` emits only frames [a, b)."""
        table = table.contiguous()
        n, m = table.shape[0], table.shape[1]
        a, b = (0, n) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
        if not (0 <= a <= b <= n):
            raise ValueError(f"frame_range {frame_range} outside the table's {n} frames")
        disp = torch.empty((b - a, m, L.DISP_COLS), dtype=torch.float32, device=self.device)
        if a == b:                                       # (a rank whose shard is empty: nothing to emit, no null pointer to pass)
            return disp
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_displacement_range(self._h, _ptr(table), n, m, int(warmup_frames),
                                                        float(min_marker_size_px), float(max_displacement), a, b,
                                                        _ptr(disp), self._stream()), "vbs_displacement")
        return disp

    def plane_fit(self, table):
        table = table.contiguous()
        n, m = table.shape[0], table.shape[1]
        plane = torch.empty((n, L.PLANE_COLS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_plane_fit(self._h, _ptr(table), n, m, _ptr(plane), self._stream()),
                        "vbs_plane_fit")
        return plane


    def deviation_plane(self, vert_start, vert_end, tilt_start, tilt_end, ref_xyz, mode="plane", scale=1.0):
        """Deviation field between a tilted and a vertical loading and the plane through its end points
        (`ForceDistribution.py:168-208,218-243`): four table rows [M,10] (one frame each), reference positions [M,3];
        returns (deviation [M,4] = (common, dX, dY, dZ), out [9] = (n, a, b, c, tilt_deg, mean k dX, k dY, k dZ, mean |d|))."""
        if mode not in ("plane", "shell"):
            raise ValueError("mode must be 'plane' or 'shell'")
        rows = [t.to(device=self.device, dtype=torch.float32).contiguous() for t in (vert_start, vert_end, tilt_start, tilt_end)]
        m = rows[0].shape[0]
        if any(tuple(t.shape) != (m, L.TABLE_COLS) for t in rows):
            raise ValueError(f"table rows must be [M, {L.TABLE_COLS}]")
        ref = torch.as_tensor(np.asarray(ref_xyz, dtype=np.float32).reshape(-1, 3), device=self.device).contiguous()
        if ref.shape[0] != m:
            raise ValueError("ref_xyz must hold one position per table slot")
        dev = torch.empty((m, 4), dtype=torch.float32, device=self.device)
        out = torch.empty((L.DEVPLANE_COLS,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_deviation_plane(self._h, *(_ptr(t) for t in rows), _ptr(ref), m,
                                                     1 if mode == "shell" else 0, float(scale), _ptr(dev), _ptr(out),
                                                     self._stream()), "vbs_deviation_plane")
        return dev, out

    # ---- the time axis: per-marker statistics of a tracked sequence (k_series.hip) ---------------------------------
    def _disp32(self, disp):
        if disp.dtype != torch.float32 or disp.device != self.device or disp.dim() != 3 or disp.shape[2] != L.DISP_COLS:
            raise ValueError(f"disp must be a float32 tensor [n, m, {L.DISP_COLS}] on the engine's device")
        if disp.shape[0] < 1 or disp.shape[1] < 1:
            raise ValueError("disp holds no frames (n <= 0) or no slots")
        return disp.contiguous()

    def _table32(self, table):
        if table.dtype != torch.float32 or table.device != self.device or table.dim() != 3 or table.shape[2] != L.TABLE_COLS:
            raise ValueError(f"table must be a float32 tensor [n, m, {L.TABLE_COLS}] on the engine's device")
        if table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("table holds no frames (n <= 0) or no slots")
        return table.contiguous()

    def series_stats(self, disp, frame_begin=0, cumulative=False):
        """`analyze_displacement`'s numbers (`3d_reconstruction.py:332-334, 397-400`) from disp [n,m,5]: float64 stats [m,5] =
        count, mean, std (ddof 1), max, total per slot (NaN where pandas has none), and with `cumulative=True` also the running
        sum [n,m] float64.  `frame_begin`: global number of disp's first frame (chunks are aligned to global frame 0)."""
        disp = self._disp32(disp)
        n, m = disp.shape[0], disp.shape[1]
        stats = torch.empty((m, L.STATS_COLS), dtype=torch.float64, device=self.device)
        cum = torch.empty((n, m), dtype=torch.float64, device=self.device) if cumulative else None
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_series_stats(self._h, _ptr(disp), n, m, int(frame_begin), _ptr(stats), _ptr(cum),
                                                  self._stream()), "vbs_series_stats")
        return (stats, cum) if cumulative else stats

    def series_partial(self, disp, frame_begin=0):
        """The per-chunk records [chunks, m, 5] (count, mean, M2, max, sum) of this block of frames (`vbs_series_partial`)."""
        disp = self._disp32(disp)
        n, m = disp.shape[0], disp.shape[1]
        k = self.lib.vbs_series_chunks(n, int(frame_begin))
        if k < 0:
            raise ValueError(f"series_partial: frame_begin {frame_begin} / {n} frames out of range")
        rec = torch.empty((k, m, L.SERIES_REC_COLS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_series_partial(self._h, _ptr(disp), n, m, int(frame_begin), _ptr(rec), self._stream()),
                        "vbs_series_partial")
        return rec

    def series_merge(self, records):
        """Records [k, m, 5] in frame order -> stats [m, 5] (`vbs_series_merge`)."""
        if records.dtype != torch.float64 or records.device != self.device or records.dim() != 3 \
                or records.shape[2] != L.SERIES_REC_COLS or records.shape[0] < 1 or records.shape[1] < 1:
            raise ValueError(f"records must be a float64 tensor [k >= 1, m, {L.SERIES_REC_COLS}] on the engine's device")
        records = records.contiguous()
        m = records.shape[1]
        stats = torch.empty((m, L.STATS_COLS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_series_merge(self._h, _ptr(records), records.shape[0], m, _ptr(stats), None,
                                                  self._stream()), "vbs_series_merge")
        return stats

    def window_means(self, table, windows):
        """`calculate_average_coordinates` (`LocalAnalysis.py:53-60`): for every inclusive frame window (a, b) of `windows`
        the per-slot count and float64 mean X, Y, Z over the rows with a 3-D point -> [W, m, 4] (NaN means at count 0)."""
        table = self._table32(table)
        n, m = table.shape[0], table.shape[1]
        w = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
        if w.shape[0] < 1 or (w < -2**31).any() or (w >= 2**31).any():
            raise ValueError("windows must be a non-empty list of (first, last) frame indices")
        w = w.astype(np.int32)
        means = torch.empty((w.shape[0], m, L.WINDOW_COLS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_window_means(self._h, _ptr(table), n, m, w.ctypes.data_as(C.c_void_p), w.shape[0],
                                                  _ptr(means), self._stream()), "vbs_window_means")
        return means

    def displacement_from_frame(self, table, ref_frame=0):
        """`MarkerDisplacement.py:158-173` for every slot: [n, m, 2] float64 = (flag, distance from the slot's position in frame
        `ref_frame`); flag 1 where both rows hold a 3-D point."""
        table = self._table32(table)
        n, m = table.shape[0], table.shape[1]
        out = torch.empty((n, m, 2), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_displacement_from_frame(self._h, _ptr(table), n, m, int(ref_frame), _ptr(out),
                                                             self._stream()), "vbs_displacement_from_frame")
        return out

    def axis_displacement(self, table, ref_frame=0, slots=None, frame_range=None):
        """The signed displacement of every slot from its position in frame `ref_frame` and its sum over the slots
        (`vbs_axis_displacement`): `(axis, total)` = float64 [b-a, m, 4] (flag, dX, dY, dZ) and [b-a, 5] (complete, sum dX, sum dY,
        sum dZ, count).  `slots` (indices) selects markers as `window_displacement` does: the others count as not seen.
        `frame_range=(a, b)` emits only frames [a, b) of the table."""
        table = self._table32(table)
        n, m = table.shape[0], table.shape[1]
        a, b = (0, n) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
        if not (0 <= a <= b <= n):
            raise ValueError(f"frame_range {frame_range} outside the table's {n} frames")
        if not (0 <= int(ref_frame) < n):
            raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
        mask = None
        if slots is not None:
            idx = np.asarray(slots, dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= m):
                raise ValueError(f"slots outside the table's {m} slots")
            mask = torch.zeros((m,), dtype=torch.uint8, device=self.device)
            mask[torch.as_tensor(idx, device=self.device)] = 1
        axis = torch.empty((b - a, m, L.AXIS_COLS), dtype=torch.float64, device=self.device)
        total = torch.empty((b - a, L.TOTAL_COLS), dtype=torch.float64, device=self.device)
        if a == b:
            return axis, total
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_axis_displacement(self._h, _ptr(table), n, m, int(ref_frame), _ptr(mask), a, b, _ptr(axis),
                                                       _ptr(total), self._stream()), "vbs_axis_displacement")
        return axis, total

    def pose_series(self, table, ref_disp, ref_xyz, start_frame=0, mode="plane", scale=1.0, slots=None, reject_k=0.0,
                    frame_range=None):
        """Pose misalignment for every frame of a recording (`vbs_pose_series`): the deviation of the displacement field against
        frame `start_frame` from the reference state's field `ref_disp` [m, 4] (flag, dX, dY, dZ: one frame of
        `axis_displacement`'s `axis`), the plane through reference position + scale * deviation (`ref_xyz` [m, 3]; `mode` as
        `deviation_plane`), its tilt, steep direction and residual.  Returns float64 device tensors `(deviation, field, pose)` =
        [b-a, m, 4] (common, dX, dY, dZ), [b-a, 6] (complete, count, mean scaled dX, dY, dZ, mean |d|) and [b-a, 8] (flag, a, b,
        c, tilt_deg, azimuth_deg, rms, n_used; flag 0 = no plane, 1 = the plane of all common slots, 2 = refitted after one round
        of rejection at `reject_k` times the rms residual; `reject_k = 0`: no rejection).  `slots` selects markers as `axis_displacement` does; `frame_range=(a, b)` emits only
        frames [a, b) of the table."""
        table = self._table32(table)
        n, m = table.shape[0], table.shape[1]
        a, b, shell = _pose_args(n, m, start_frame, mode, scale, slots, reject_k, frame_range)
        rd = torch.as_tensor(ref_disp, dtype=torch.float64, device=self.device).contiguous()
        rx = torch.as_tensor(ref_xyz, dtype=torch.float64, device=self.device).contiguous()
        if tuple(rd.shape) != (m, L.AXIS_COLS) or tuple(rx.shape) != (m, 3):
            raise ValueError(f"ref_disp must be [{m}, {L.AXIS_COLS}] and ref_xyz [{m}, 3]: one row per table slot")
        mask = None
        if slots is not None:
            mask = torch.zeros((m,), dtype=torch.uint8, device=self.device)
            mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=self.device)] = 1
        deviation = torch.empty((b - a, m, 4), dtype=torch.float64, device=self.device)
        field = torch.empty((b - a, L.POSEFIELD_COLS), dtype=torch.float64, device=self.device)
        pose = torch.empty((b - a, L.POSE_COLS), dtype=torch.float64, device=self.device)
        if a == b:
            return deviation, field, pose
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_pose_series(self._h, _ptr(table), n, m, int(start_frame), _ptr(rd), _ptr(rx), _ptr(mask), shell,
                                                 float(scale), float(reject_k), a, b, _ptr(deviation), _ptr(field), _ptr(pose),
                                                 self._stream()), "vbs_pose_series")
        return deviation, field, pose

    # ---- a14 / f4 ------------------------------------------------------------------------------
    def assign_ids(self, det, counts, num_layers=5, id_mode="as_written"):
        """Frame-0 identities on the device: (ids int32 [M,2], ref_xy float64 [M,2]) as device tensors, in the
        reference dict's order.  `det` / `counts` are frame 0's rows of `marker_center` / `track_to_3d(want_det=True)`."""
        if id_mode not in ("as_written", "full"):
            raise ValueError(f"id_mode must be 'as_written' or 'full', got {id_mode!r}")
        if int(num_layers) > L.IDS_MAX_LAYERS:
            raise ValueError(f"vbs_assign_ids: num_layers {int(num_layers)} above the kernel's {L.IDS_MAX_LAYERS} "
                             "(VBS_IDS_MAX_LAYERS); ids.assign_ids on the host has no such limit")
        det0 = (det[0] if det.dim() == 3 else det).contiguous()
        cnt0 = counts.reshape(-1)[:1].contiguous()
        cap = det0.shape[0] + 1
        ids = torch.zeros((cap, 2), dtype=torch.int32, device=self.device)
        xy = torch.zeros((cap, 2), dtype=torch.float64, device=self.device)
        m = torch.zeros((1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.vbs_assign_ids(self._h, _ptr(det0), _ptr(cnt0), int(num_layers),
                                                1 if id_mode == "full" else 0, _ptr(ids), _ptr(xy), cap, _ptr(m),
                                                self._stream()), "vbs_assign_ids")
        mm = int(m.item())
        if mm == -1:
            raise ValueError("No markers detected in first frame!")
        if mm <= -1000:
            raise L.VbsError(f"device status {mm // 1000} in frame 0")
        if mm == -3:
            raise L.VbsError(f"vbs_assign_ids: more than {L.IDS_MAX_MARKERS} markers in frame 0 (VBS_IDS_MAX_MARKERS); "
                             "nothing was assigned")
        if mm < 0:
            raise L.VbsError(f"vbs_assign_ids: device status {mm}")
        return ids[:mm], xy[:mm]


def _dev_f64(x, dev, cols):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float64).reshape(-1, cols).contiguous()
    return torch.as_tensor(np.asarray(x, dtype=np.float64).reshape(-1, cols), device=dev).contiguous()


def undistort_points(points, cam: L.Camera, device=None):
    """float64 [n,2] -> [n,2] on the GPU (`MarkerAnalysis._undistort_points`)."""
    dev = _device(device)
    p = _dev_f64(points, dev, 2)
    out = torch.empty_like(p)
    rc = L.lib().vbs_undistort_points(dev.index, _ptr(p), p.shape[0], C.byref(cam), _ptr(out),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_undistort_points failed ({rc})")
    return out


def pnp_samples(n: int, iterations: int = 1000, seed: int = 0) -> np.ndarray:
    """The sample table of `pnp_ransac`: int32 [iterations, 6], per hypothesis 6 distinct indices out of n, drawn from
    `np.random.default_rng(seed)`.  Fewer than 6 points: every row is -1 (void)."""
    n, iterations = int(n), int(iterations)
    if n < 1 or not 1 <= iterations <= L.PNP_MAX_HYPOTHESES:
        raise ValueError(f"pnp_samples: n >= 1 and 1 <= iterations <= {L.PNP_MAX_HYPOTHESES}")
    out = np.full((iterations, L.PNP_SAMPLE), -1, dtype=np.int32)
    if n >= L.PNP_SAMPLE:
        rng = np.random.default_rng(seed)
        for h in range(iterations):
            out[h] = rng.choice(n, size=L.PNP_SAMPLE, replace=False)
    return out


def pnp_ransac(world, image_or_table, cam: L.Camera, iterations: int = 1000, reproj_px: float = 8.0, seed: int = 0, valid=None,
               device=None, samples=None):
    """`calibrate_camera_extrinsics` (`extrinsic_calibration.py:81-123`) for a batch of problems on the GPU (`vbs_pnp_ransac`).
    world [N,3]; image_or_table: float64 [B,N,2] (or [N,2]) pixel positions, or a float32 tracker table [B,N,10] (Cx, Cy of the
    rows with FLAG_TRACKED); valid: optional [B,N] mask.  Returns a dict of device tensors: status [B], R [B,3,3], T [B,3],
    inlier_count [B], inlier_mask [B,N] uint8, mean_error [B], inlier_rms [B], winner [B], and per hypothesis hyp_count [B,H],
    hyp_pose [B,H,12]; `samples` (int32 [H,6], default `pnp_samples(N, iterations, seed)`) is returned as given."""
    dev = _device(device)
    w = _dev_f64(world, dev, 3)
    n = w.shape[0]
    x = image_or_table if isinstance(image_or_table, torch.Tensor) else torch.as_tensor(np.asarray(image_or_table))
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3 or x.shape[1] != n or x.shape[2] not in (2, L.TABLE_COLS):
        raise ValueError(f"image_or_table must be [B, {n}, 2] or [B, {n}, {L.TABLE_COLS}]")
    is_table = x.shape[2] == L.TABLE_COLS
    x = x.to(device=dev, dtype=torch.float32 if is_table else torch.float64).contiguous()
    b = x.shape[0]
    v = None
    if valid is not None:
        v = torch.as_tensor(valid, device=dev).reshape(b, n).ne(0).to(torch.uint8).contiguous()
    smp = pnp_samples(n, iterations, seed) if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    if smp.ndim != 2 or smp.shape[1] != L.PNP_SAMPLE:
        raise ValueError(f"samples must be [H, {L.PNP_SAMPLE}]")
    smp_d = torch.as_tensor(smp, device=dev)
    nh = smp.shape[0]
    out = {"hyp_count": torch.empty((b, nh), dtype=torch.int32, device=dev),
           "hyp_pose": torch.empty((b, nh, 12), dtype=torch.float64, device=dev),
           "status": torch.empty((b,), dtype=torch.int32, device=dev),
           "inlier_count": torch.empty((b,), dtype=torch.int32, device=dev),
           "inlier_mask": torch.empty((b, n), dtype=torch.uint8, device=dev),
           "winner": torch.empty((b,), dtype=torch.int32, device=dev)}
    pose = torch.empty((b, 12), dtype=torch.float64, device=dev)
    errors = torch.empty((b, 2), dtype=torch.float64, device=dev)
    rc = L.lib().vbs_pnp_ransac(dev.index, _ptr(w), n, _ptr(None if is_table else x), _ptr(x if is_table else None), _ptr(v), b,
                                C.byref(cam), _ptr(smp_d), nh, float(reproj_px), _ptr(out["hyp_count"]), _ptr(out["hyp_pose"]),
                                _ptr(out["status"]), _ptr(pose), _ptr(out["inlier_count"]), _ptr(out["inlier_mask"]),
                                _ptr(errors), _ptr(out["winner"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError(f"vbs_pnp_ransac: bad argument (at most {L.PNP_MAX_POINTS} points and {L.PNP_MAX_HYPOTHESES} "
                         "hypotheses, positive focal lengths, reproj_px >= 0)")
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_pnp_ransac failed ({rc})")
    out.update(R=pose[:, :9].reshape(b, 3, 3), T=pose[:, 9:], mean_error=errors[:, 0], inlier_rms=errors[:, 1], samples=smp)
    return out


def _board_and_corners(obj_points, img_points, dev):
    """cv2's list-of-arrays layout, stacked arrays or device tensors -> (board [N,2], corners [V,N,2]) float64 on `dev`."""
    if isinstance(img_points, torch.Tensor):
        img = img_points.to(device=dev, dtype=torch.float64)
    else:
        img = torch.as_tensor(np.stack([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in img_points]), device=dev)
    if img.dim() == 4 and img.shape[2] == 1:
        img = img[:, :, 0]
    if img.dim() != 3 or img.shape[2] != 2:
        raise ValueError("img_points must be V arrays of [N,1,2] or [N,2] corners")
    if isinstance(obj_points, torch.Tensor):
        obj = obj_points.to(device=dev, dtype=torch.float64)
    elif isinstance(obj_points, np.ndarray) and obj_points.ndim == 2:
        obj = torch.as_tensor(obj_points.astype(np.float64), device=dev)
    else:
        views = [np.asarray(o, dtype=np.float64).reshape(len(o), -1) for o in obj_points]
        if len(views) != img.shape[0] or any(o.shape != views[0].shape or not np.array_equal(o, views[0]) for o in views):
            raise ValueError("obj_points must hold the same board once per view")
        obj = torch.as_tensor(views[0], device=dev)
    if obj.dim() == 3:
        if obj.shape[0] != img.shape[0] or not bool((obj == obj[:1]).all()):
            raise ValueError("obj_points must hold the same board once per view")
        obj = obj[0]
    if obj.dim() != 2 or obj.shape[1] not in (2, 3) or obj.shape[0] != img.shape[1]:
        raise ValueError(f"obj_points must be [{img.shape[1]},3] (or [.,2]) board points")
    if obj.shape[1] == 3:
        if bool((obj[:, 2] != 0).any()):
            raise ValueError("obj_points must be one planar board with Z = 0")
        obj = obj[:, :2]
    return obj.contiguous(), img.contiguous()


def calibrate_camera_points(obj_points, img_points, img_size, view_mask=None, max_iter: int = 30, device=None):
    """`cv2.calibrateCamera(obj_points, img_points, img_size, None, None)` (`intrinsic_calibration.py:97-98`) on the GPU
    (`vbs_calibrate_camera`) for one planar board, as a batch of problems over subsets of its views.
    obj_points: cv2's list of [N,3] float32 arrays - which must all be the same board with Z = 0 - or one [N,3] / [N,2] array;
    img_points: a list of [N,1,2] / [N,2] corners per view, or a stacked array / device tensor [V,N,2]; img_size = (width, height);
    view_mask: optional [B,V] (or [V]) - problem b uses the views with a non-zero entry; None = one problem over all views.
    Returns a dict of device tensors: status [B], K4 [B,4], dist [B,5], R [B,V,3,3], T [B,V,3], rms [B], view_rms [B,V],
    std_intrinsics [B,9], iterations [B], and per view homography [V,3,3], view_void [V]."""
    dev = _device(device)
    obj, img = _board_and_corners(obj_points, img_points, dev)
    nv, n = img.shape[0], img.shape[1]
    if nv > L.CALIB_MAX_VIEWS or n > L.CHESS_MAX_PATTERN:
        raise L.VbsError(f"vbs_calibrate_camera: {nv} views of {n} points exceed VBS_CALIB_MAX_VIEWS = {L.CALIB_MAX_VIEWS} or "
                         f"VBS_CHESS_MAX_PATTERN = {L.CHESS_MAX_PATTERN}")
    m = None
    if view_mask is not None:
        m = torch.as_tensor(view_mask, device=dev).reshape(-1, nv).ne(0).to(torch.uint8).contiguous()
    b = 1 if m is None else m.shape[0]
    f64, i32 = torch.float64, torch.int32
    out = {"status": torch.empty((b,), dtype=i32, device=dev), "K4": torch.empty((b, 4), dtype=f64, device=dev),
           "dist": torch.empty((b, 5), dtype=f64, device=dev), "R": torch.empty((b, nv, 3, 3), dtype=f64, device=dev),
           "T": torch.empty((b, nv, 3), dtype=f64, device=dev), "rms": torch.empty((b,), dtype=f64, device=dev),
           "view_rms": torch.empty((b, nv), dtype=f64, device=dev), "std_intrinsics": torch.empty((b, 9), dtype=f64, device=dev),
           "iterations": torch.empty((b,), dtype=i32, device=dev), "homography": torch.empty((nv, 3, 3), dtype=f64, device=dev),
           "view_void": torch.empty((nv,), dtype=i32, device=dev)}
    rc = L.lib().vbs_calibrate_camera(dev.index, _ptr(obj), n, _ptr(img), nv, _ptr(m), b, int(img_size[0]), int(img_size[1]),
                                      int(max_iter), _ptr(out["homography"]), _ptr(out["view_void"]), _ptr(out["status"]),
                                      _ptr(out["K4"]), _ptr(out["dist"]), _ptr(out["R"]), _ptr(out["T"]), _ptr(out["rms"]),
                                      _ptr(out["view_rms"]), _ptr(out["std_intrinsics"]), _ptr(out["iterations"]),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError("vbs_calibrate_camera: bad argument (at least 4 points, 1 view and 1 problem, positive image size and max_iter)")
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_calibrate_camera failed ({rc})")
    return out


def normxcorr2_general(template, image, mode="same", device=None):
    """`_normxcorr2` for arbitrary operands: float64 map of the mode's size on the GPU (`vbs_normxcorr2_general`)."""
    dev = _device(device)
    modes = {"full": 0, "same": 1, "valid": 2}
    if mode not in modes:
        raise ValueError("acceptable mode flags are 'valid', 'same', or 'full'")        # scipy's message
    t = torch.as_tensor(np.asarray(template, dtype=np.float64), device=dev).contiguous()
    im = torch.as_tensor(np.asarray(image, dtype=np.float64), device=dev).contiguous()
    if t.dim() != 2 or im.dim() != 2:
        raise ValueError("template and image must be 2-D")
    (th, tw), (h, w) = t.shape, im.shape
    if tw > 256:
        raise NotImplementedError("vbs_normxcorr2_general holds template rows of at most 256 samples")
    oh, ow = {0: (h + th - 1, w + tw - 1), 1: (h, w), 2: (h - th + 1, w - tw + 1)}[modes[mode]]
    if oh < 1 or ow < 1:
        raise ValueError("For 'valid' mode, one must be at least as large as the other in every dimension")
    out = torch.empty((oh, ow), dtype=torch.float64, device=dev)
    rc = L.lib().vbs_normxcorr2_general(dev.index, _ptr(t), th, tw, _ptr(im), h, w, modes[mode], _ptr(out),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_normxcorr2_general failed ({rc})")
    return out


def calculate_3d(uvd, cam: L.Camera, device=None):
    """float64 [n,3] (u, v, diameter_px) -> (xyz float64 [n,3], ok int32 [n]) on the GPU."""
    dev = _device(device)
    p = _dev_f64(uvd, dev, 3)
    xyz = torch.empty_like(p)
    ok = torch.empty((p.shape[0],), dtype=torch.int32, device=dev)
    rc = L.lib().vbs_calculate_3d(dev.index, _ptr(p), p.shape[0], C.byref(cam), _ptr(xyz), _ptr(ok),
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError("Focal lengths must be positive")
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_calculate_3d failed ({rc})")
    return xyz, ok


def displacement_f64(table64, warmup_frames=0, min_marker_size_px=0.0, max_displacement=50.0, device=None):
    """float64 table [n,m,10] (host or device) -> disp float64 [n,m,5] on the GPU (`vbs_displacement_f64`)."""
    dev = _device(device)
    t = torch.as_tensor(table64, dtype=torch.float64, device=dev).contiguous()
    n, m = t.shape[0], t.shape[1]
    disp = torch.empty((n, m, L.DISP_COLS), dtype=torch.float64, device=dev)
    rc = L.lib().vbs_displacement_f64(dev.index, _ptr(t), n, m, int(warmup_frames), float(min_marker_size_px),
                                      float(max_displacement), _ptr(disp),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_displacement_f64 failed ({rc})")
    return disp


def series_stats_f64(disp64, frame_begin=0, cumulative=False, device=None):
    """float64 disp [n,m,5] (host or device, as `displacement_f64` returns it) -> stats float64 [m,5] (and the running sum
    [n,m]) on the GPU (`vbs_series_stats_f64`)."""
    dev = _device(device)
    d = torch.as_tensor(disp64, dtype=torch.float64, device=dev).contiguous()
    if d.dim() != 3 or d.shape[2] != L.DISP_COLS or d.shape[0] < 1 or d.shape[1] < 1:
        raise ValueError(f"disp must be [n >= 1, m >= 1, {L.DISP_COLS}]")
    n, m = d.shape[0], d.shape[1]
    k = L.lib().vbs_series_chunks(n, int(frame_begin))
    if k < 0:
        raise ValueError(f"series_stats_f64: frame_begin {frame_begin} / {n} frames out of range")
    scratch = torch.empty((k * m * (L.SERIES_REC_COLS + 1),), dtype=torch.float64, device=dev)
    stats = torch.empty((m, L.STATS_COLS), dtype=torch.float64, device=dev)
    cum = torch.empty((n, m), dtype=torch.float64, device=dev) if cumulative else None
    with torch.cuda.device(dev):
        rc = L.lib().vbs_series_stats_f64(dev.index, _ptr(d), n, m, int(frame_begin), _ptr(stats), _ptr(cum), _ptr(scratch),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError("vbs_series_stats_f64: bad argument")
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_series_stats_f64 failed ({rc})")
    return (stats, cum) if cumulative else stats


def _pose_args(n, m, start_frame, mode, scale, slots, reject_k, frame_range):
    """`Engine.pose_series`'s argument checks (no device needed): -> (a, b, shell_mode) or ValueError."""
    if mode not in ("plane", "shell"):
        raise ValueError("mode must be 'plane' or 'shell'")
    a, b = _frame_range(frame_range, n, "the table's")
    if not (0 <= int(start_frame) < n):
        raise ValueError(f"start_frame {start_frame} outside the table's {n} frames")
    if not np.isfinite(float(scale)):
        raise ValueError(f"scale {scale} is not finite")
    if not (np.isfinite(float(reject_k)) and float(reject_k) >= 0.0):
        raise ValueError(f"reject_k {reject_k} must be finite and >= 0 (0 = no rejection)")
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= m):
            raise ValueError(f"slots outside the table's {m} slots")
    return a, b, 1 if mode == "shell" else 0


# ---- re-tracking a recording along time (k_retrack.hip) ---------------------------------------------------------------------------
def _retrack_args(n, m, max_det, gate, max_travel, vel_gain, max_coast, want):
    """`retrack`'s argument checks (no device needed): -> (gate, max_travel, vel_gain, max_coast, want) or ValueError."""
    from .retrack import OUTPUTS
    if n < 0 or m < 1 or max_det < 1:
        raise ValueError("det must be [n >= 0, max_det >= 1, 6] and ref_xy [m >= 1, 2]")
    if m > L.RETRACK_MAX or max_det > L.RETRACK_MAX:
        raise ValueError(f"at most {L.RETRACK_MAX} slots and {L.RETRACK_MAX} detections per frame (VBS_RETRACK_MAX)")
    g = float(gate)
    if not g >= 0.0:
        raise ValueError(f"gate {gate} must be >= 0")
    mt = float(max_travel)
    if np.isnan(mt):
        raise ValueError("max_travel must not be NaN (inf = no limit)")
    vg = float(vel_gain)
    if not 0.0 <= vg <= 1.0:
        raise ValueError(f"vel_gain {vel_gain} must lie in [0, 1]")
    mc = int(max_coast)
    if mc != max_coast or mc < 0:
        raise ValueError(f"max_coast {max_coast} must be an integer >= 0")
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in OUTPUTS]
    if unknown:
        raise ValueError(f"want: unknown outputs {unknown} (known: {', '.join(OUTPUTS)})")
    return g, mt, vg, mc, want


def retrack(det, counts, ref_xy, gate=10.0, max_travel=float("inf"), vel_gain=0.5, max_coast=5, state=None,
            want=("assign", "table", "dist2", "info"), device=None):
    """Re-track a recording from its detections along time (`vbs_retrack`; the rule: include/vbs.h): per slot a position and a
    velocity, a gate of `gate` px around the prediction, every detection given to at most one slot.  det float64 [n, max_det, 6]
    and counts int32 [n] as `Engine.track_to_3d(..., want_det=True)` returns them, ref_xy [m, 2] (arrays or tensors); `state`
    [m, 6] as an earlier call returned it, None = `retrack.initial_state(ref_xy)`.  Returns a dict of device tensors: those of
    `want` - assign int32 [n, m] (detection index or -1), table float32 [n, m, 10] (rows as `Engine.track` writes them, ready
    for `Engine.solve3d`), dist2 float64 [n, m], info int32 [n, 4] = used, matched, with_candidate, contested - and always
    `state` float64 [m, 6]: frames [0, k) and then [k, n) with that state give what [0, n) gives."""
    if device is None and isinstance(det, torch.Tensor) and det.is_cuda:
        device = det.device.index
    dev = _device(device)
    d = torch.as_tensor(det, dtype=torch.float64, device=dev).contiguous()
    if d.dim() != 3 or d.shape[2] != L.DET_COLS:
        raise ValueError(f"det must be [n, max_det, {L.DET_COLS}]")
    c = torch.as_tensor(counts, device=dev).to(torch.int32).contiguous().reshape(-1)
    if c.numel() != d.shape[0]:
        raise ValueError(f"counts must be [n = {d.shape[0]}]")
    ref = _dev_f64(ref_xy, dev, 2)
    n, max_det, m = d.shape[0], d.shape[1], ref.shape[0]
    g, mt, vg, mc, want = _retrack_args(n, m, max_det, gate, max_travel, vel_gain, max_coast, want)
    st = None
    if state is not None:
        st = torch.as_tensor(state, dtype=torch.float64, device=dev).contiguous()
        if tuple(st.shape) != (m, L.RETRACK_STATE_COLS):
            raise ValueError(f"state must be [m = {m}, {L.RETRACK_STATE_COLS}]")
    kinds = {"assign": ((n, m), torch.int32), "table": ((n, m, L.TABLE_COLS), torch.float32), "dist2": ((n, m), torch.float64),
             "info": ((n, L.RETRACK_INFO_COLS), torch.int32)}
    out = {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=dev) for k in want}
    if n == 0:                                           # no frame: the state as it came (an empty tensor has no address to pass)
        from .retrack import initial_state
        out["state"] = st.clone() if st is not None else initial_state(ref)
        return out
    out["state"] = torch.empty((m, L.RETRACK_STATE_COLS), dtype=torch.float64, device=dev)
    lib = L.lib()
    ws = torch.empty((int(lib.vbs_retrack_workspace(n, m, max_det)) + 7) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.vbs_retrack(dev.index, _ptr(d), _ptr(c), n, max_det, _ptr(ref), m, _ptr(st), g, mt, vg, mc, _ptr(out.get("assign")),
                             _ptr(out.get("table")), _ptr(out.get("dist2")), _ptr(out.get("info")), _ptr(out["state"]), _ptr(ws),
                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError("vbs_retrack: bad argument (gate >= 0, vel_gain in [0, 1], max_coast >= 0)")
    if rc != L.VBS_OK:
        raise L.VbsError(f"vbs_retrack failed ({rc})")
    return out
