"""The analyses along a FIR record (float64 [n, s, cols]: a flag and up to seven value columns per frame and slot): handle-free
wrappers over the `vbs_*_f64` entries of csrc/api_analysis.hip.  Every wrapper takes host or device data, enqueues on the current
torch stream of its device and returns device tensors.  It raises in one order: no GPU, a wrong rank, what its `_*_args` checker
refuses (pure functions that need no device), then the entry's status.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

_REC = "rec must be [n >= 1, s >= 1, cols]"


# ---- what every wrapper does: the device, the operands, the shared argument rules, the call ---------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host_ptr(a):
    """A contiguous float64 host array the entry reads before it launches (half taps, thresholds)."""
    return a.ctypes.data_as(C.c_void_p)


def _device(device):
    if not torch.cuda.is_available():
        raise L.VbsError("no GPU visible: vbs_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device() if device is None else device)


def _f64(x, dev, dims=None, what=None, nonempty=0):
    """x (host or device) as a contiguous float64 tensor on `dev`; ValueError(what) unless it has `dims` dimensions, the first
    `nonempty` of them not empty."""
    t = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    if dims is not None and (t.dim() != dims or any(k < 1 for k in t.shape[:nonempty])):
        raise ValueError(what)
    return t


def _record_shape(n, s, cols):
    if n < 1 or s < 1 or not (2 <= cols <= 8):
        raise ValueError("rec must be [n >= 1, s >= 1, 2 <= cols <= 8]")


def _frame_range(frame_range, n, what="the"):
    """The frames [a, b) of `frame_range`, all `n` by default."""
    a, b = (0, n) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
    if not (0 <= a <= b <= n):
        raise ValueError(f"frame_range {frame_range} outside {what} {n} frames")
    return a, b


def _n_values(cols, n_values, most):
    """`n_values`, by default every value column and at most `most` of them, inside the bounds its entry has.  `most` None (the
    filter and the step entries, which take all seven): the host checks the lower bound only and the entry the upper one."""
    if n_values is not None:
        nv = int(n_values)
    else:
        nv = cols - 1 if most is None else min(cols - 1, most)
    if most is None:
        if nv < 1:
            raise ValueError("n_values must be >= 1")
    elif not (1 <= nv <= most and nv < cols):
        raise ValueError(f"n_values must be {'1 .. 3' if most == 3 else '>= 1'} and below cols")
    return nv


def _coverage(min_coverage):
    mc = float(min_coverage)
    if not (0.0 < mc <= 1.0):
        raise ValueError("min_coverage must lie in (0, 1]")
    return mc


def _capacity(entry, limits):
    """limits: (what, got, the limit's name in _lib) - the shapes `entry` would answer VBS_ECAPACITY to."""
    for what, got, name in limits:
        if got > getattr(L, name):
            raise L.VbsError(f"{entry}: {got} {what} exceed VBS_{name} = {getattr(L, name)} (status {L.VBS_ECAPACITY})")


def _call(entry, hint, dev, *args, capacity=None):
    """`entry(dev.index, *args, the current stream of dev)` with `dev` current; its status as an exception: VBS_EINVAL -> ValueError
    with `hint`, VBS_ECAPACITY -> VbsError with `capacity` where the entry has such a text, anything else but VBS_OK -> VbsError."""
    with torch.cuda.device(dev):
        rc = getattr(L.lib(), entry)(dev.index, *args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == L.VBS_EINVAL:
        raise ValueError(f"{entry}: bad argument ({hint})")
    if rc == L.VBS_ECAPACITY and capacity is not None:
        raise L.VbsError(f"{entry}: {capacity} (status {rc})")
    if rc != L.VBS_OK:
        raise L.VbsError(f"{entry} failed ({rc})")


# ---- the dynamic polishing process (k_filter.hip): a zero-phase FIR along time ------------------------------------------------------
def fir_series_f64(rec, taps, n_values=None, min_coverage=0.5, frame_range=None, device=None):
    """A normalised zero-phase FIR along time with gaps (`vbs_fir_series_f64`).  rec float64 [n, s, cols] (host or device): col 0
    the flag (nonzero = valid), cols 1 .. n_values the values (default cols - 1).  `taps`: the FULL odd-length array, refused
    unless |w[k] - w[K-1-k]| <= 1e-12 max|w|; the means of its pairs are what is used (`filters.half_taps`), so the filter is
    exactly symmetric.  Returns float64 [b-a, s, 1 + 2 n_values] = flag (0, 1 = valid, 3 = valid and filtered), filtered,
    residual for the frames [a, b) of `frame_range` (default all); an output does not depend on the range it was asked in."""
    from .filters import half_taps
    dev = _device(device)
    half = np.ascontiguousarray(half_taps(taps), dtype=np.float64)
    r = _f64(rec, dev, 3, _REC, nonempty=2)
    n, s, cols = r.shape
    a, b = _frame_range(frame_range, n)
    nv = _n_values(cols, n_values, None)
    out = torch.empty((b - a, s, 1 + 2 * nv), dtype=torch.float64, device=dev)
    if a == b:
        return out
    _call("vbs_fir_series_f64", f"at most {L.FIR_MAX_TAPS} taps with a positive sum, min_coverage in (0, 1], 1 <= n_values < cols <= 8",
          dev, _ptr(r), n, s, cols, nv, _host_ptr(half), half.size, float(min_coverage), a, b, _ptr(out))
    return out


# ---- despiking a tracked series (k_robust.hip): rolling median, MAD, the Hampel rule ---------------------------------------------
def _robust_args(n, s, cols, half_window, k_sigma, min_scale, min_count, n_values, frame_range):
    """`hampel_series_f64`'s argument checks (no device needed): -> (a, b, n_values, h, min_count) or ValueError."""
    _record_shape(n, s, cols)
    nv = _n_values(cols, n_values, 7)
    h = int(half_window)
    if h != half_window or not (0 <= h <= L.ROBUST_MAX_HALF):
        raise ValueError(f"half_window must be an integer in [0, {L.ROBUST_MAX_HALF}] (VBS_ROBUST_MAX_HALF)")
    mc = h + 1 if min_count is None else int(min_count)
    if (min_count is not None and mc != min_count) or not (1 <= mc <= 2 * h + 1):
        raise ValueError(f"min_count must be an integer in [1, 2 half_window + 1 = {2 * h + 1}]")
    if not (np.isfinite(float(k_sigma)) and float(k_sigma) > 0.0):
        raise ValueError(f"k_sigma {k_sigma} must be finite and > 0")
    if not (np.isfinite(float(min_scale)) and float(min_scale) >= 0.0):
        raise ValueError(f"min_scale {min_scale} must be finite and >= 0")
    a, b = _frame_range(frame_range, n)
    return a, b, nv, h, mc


def hampel_series_f64(rec, half_window, k_sigma=3.0, min_scale=0.0, min_count=None, n_values=None, frame_range=None,
                      want_clean=True, device=None):
    """A gap-aware rolling median and median absolute deviation along time with the Hampel rule (`vbs_hampel_series_f64`).  rec
    float64 [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols 1 .. n_values the values (default cols - 1).  The
    window of frame f is the valid frames of [f - h, f + h], h = `half_window` <= VBS_ROBUST_MAX_HALF; an entry is judged when the
    window holds at least `min_count` (default h + 1) of them, and a valid judged entry is a spike when for any value
    |x - med| > k_sigma * 1.4826 * mad and > `min_scale` (an absolute floor in the units of the data).  Returns (out, clean) for
    the frames [a, b) of `frame_range` (default all): out float64 [b-a, s, 2 + 2 n_values] = flag (valid + 2 judged + 4 spike),
    the population of the window, med, mad - flag 2 is a missing entry whose median is the value to fill the gap with; clean
    float64 [b-a, s, cols] = those rows of rec bit for bit with the flag of every spike set to 0 (None when `want_clean` is
    false).  An output does not depend on the range it was asked in."""
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC)
    n, s, cols = r.shape
    a, b, nv, h, mc = _robust_args(n, s, cols, half_window, k_sigma, min_scale, min_count, n_values, frame_range)
    out = torch.empty((b - a, s, 2 + 2 * nv), dtype=torch.float64, device=dev)
    clean = torch.empty((b - a, s, cols), dtype=torch.float64, device=dev) if want_clean else None
    if a == b:
        return out, clean
    _call("vbs_hampel_series_f64", f"half_window in [0, {L.ROBUST_MAX_HALF}], min_count in [1, 2 half_window + 1], k_sigma finite "
          "and > 0, min_scale finite and >= 0, 1 <= n_values < cols <= 8",
          dev, _ptr(r), n, s, cols, nv, h, mc, float(k_sigma), float(min_scale), a, b, _ptr(out), _ptr(clean))
    return out, clean


# ---- contact maps along a recording (k_field.hip): the smoother in space, the contact patch ------------------------------------
def _field_args(n, s, cols, P, w_shape, wsum_shape, min_coverage, n_values, frame_range):
    """`field_map_f64`'s argument checks (no device needed): -> (a, b, n_values) or ValueError."""
    _record_shape(n, s, cols)
    if tuple(w_shape) != (P, s) or P < 1:
        raise ValueError(f"W must be [P >= 1, {s}]: one weight per grid point and slot of rec")
    if wsum_shape is not None and tuple(wsum_shape) != (P,):
        raise ValueError(f"wsum must be [{P}]")
    nv = _n_values(cols, n_values, 3)
    _coverage(min_coverage)
    a, b = _frame_range(frame_range, n)
    _capacity("vbs_field_map_f64", (("slots", s, "FIELD_MAX_SLOTS"), ("grid points", P, "FIELD_MAX_POINTS")))
    return a, b, nv


def field_map_f64(rec, W, wsum=None, min_coverage=0.5, n_values=None, frame_range=None, device=None):
    """A normalised kernel smoother in space with gaps (`vbs_field_map_f64`), every frame in one launch.  rec float64
    [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols 1 .. n_values the values (default min(cols - 1, 3)).
    W float64 [P, s]: non-negative weights of slot m at grid point p (`fields.gaussian_weights`); wsum [P] its full row sums
    (default `fields.row_sums(W)`, on the host).  Returns float64 [b-a, P, 1 + n_values] = ok, the weighted mean of every value
    over the valid slots, for the frames [a, b) of `frame_range` (default all): ok where the valid weight is positive and at
    least min_coverage * wsum, zeros elsewhere.  An output does not depend on the range it was asked in."""
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC)
    if wsum is None:
        from .fields import row_sums
        wsum = row_sums(W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else W)
    w, ws = _f64(W, dev), _f64(wsum, dev)
    n, s, cols = r.shape
    P = w.shape[0] if w.dim() == 2 else 0
    a, b, nv = _field_args(n, s, cols, P, w.shape, ws.shape, min_coverage, n_values, frame_range)
    out = torch.empty((b - a, P, 1 + nv), dtype=torch.float64, device=dev)
    if a == b:
        return out
    _call("vbs_field_map_f64", "min_coverage in (0, 1], 1 <= n_values <= 3, n_values < cols <= 8",
          dev, _ptr(r), n, s, cols, nv, _ptr(w), _ptr(ws), P, float(min_coverage), a, b, _ptr(out),
          capacity=f"more than VBS_FIELD_MAX_SLOTS = {L.FIELD_MAX_SLOTS} slots or VBS_FIELD_MAX_POINTS = {L.FIELD_MAX_POINTS} grid points")
    return out


def _patch_args(F, P, oc, grid_shape, component, sign, threshold):
    """`patch_stats_f64`'s argument checks (no device needed): -> (n_values, component, sign, thr as the entry takes it)."""
    nv = oc - 1
    if F < 0 or P < 1 or not (1 <= nv <= 3):
        raise ValueError("map must be [F, P >= 1, 2 .. 4]")
    if tuple(grid_shape) != (P, 2):
        raise ValueError(f"grid_xy must be [{P}, 2]")
    c = int(component)
    if not (-1 <= c < nv):
        raise ValueError(f"component must be 0 .. {nv - 1}, or -1 for the squared norm")
    if float(sign) not in (1.0, -1.0):
        raise ValueError("sign must be +1 or -1")
    thr = float(threshold)
    if not (thr >= 0.0):
        raise ValueError("threshold must be >= 0")
    _capacity("vbs_patch_stats_f64", (("grid points", P, "FIELD_MAX_POINTS"),))
    return nv, c, float(sign), thr * thr if c < 0 else thr


def patch_stats_f64(map, grid_xy, component=2, sign=1.0, threshold=0.0, device=None):
    """The contact patch of every frame of a map (`vbs_patch_stats_f64`).  map float64 [F, P, 1 + n_values] as `field_map_f64`
    returns it, grid_xy float64 [P, 2].  The score of a covered point is sign * value[component], or for component -1 the squared
    norm of its values; the patch is the covered points whose score reaches `threshold` (for component -1 `threshold` is a length:
    its square is what is compared).  Returns float64 [F, 8] = flag (0 nothing covered, 1 no patch, 2 a patch with a centre),
    covered, count, sum of the scores, score-weighted centre cx, cy, peak score, index of the peak (the first of equal ones)."""
    dev = _device(device)
    m, g = _f64(map, dev, 3, "map must be [F, P, 1 + n_values]"), _f64(grid_xy, dev)
    F, P, oc = m.shape
    nv, c, sg, thr = _patch_args(F, P, oc, g.shape, component, sign, threshold)
    out = torch.empty((F, L.PATCH_COLS), dtype=torch.float64, device=dev)
    if F == 0:
        return out
    _call("vbs_patch_stats_f64", "component -1 .. n_values-1, sign +-1, threshold >= 0",
          dev, _ptr(m), F, P, nv, _ptr(g), c, sg, thr, _ptr(out),
          capacity=f"more than VBS_FIELD_MAX_POINTS = {L.FIELD_MAX_POINTS} grid points")
    return out


# ---- displacement spectra along a recording (k_spectrum.hip): the projection onto a basis, the harmonic fit ------------------------
def _project_args(n, s, cols, basis_shape, n_values):
    """`project_series_f64`'s argument checks (no device needed): -> (R, n_values) or ValueError."""
    _record_shape(n, s, cols)
    bs = tuple(basis_shape)
    if len(bs) != 2 or bs[0] < 1 or bs[1] != n:
        raise ValueError(f"basis must be [R >= 1, {n}]: one value per basis row and frame of rec")
    nv = _n_values(cols, n_values, 3)
    _capacity("vbs_project_series_f64", (("frames", n, "PROJ_MAX_FRAMES"), ("slots", s, "PROJ_MAX_SLOTS"),
                                         ("basis rows", bs[0], "PROJ_MAX_ROWS")))
    return int(bs[0]), nv


def project_series_f64(rec, basis, n_values=None, device=None):
    """The gap-aware projection of every series onto a basis (`vbs_project_series_f64`), a float64 matrix product over the time
    axis.  rec float64 [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols 1 .. n_values the values (default
    min(cols - 1, 3)).  basis float64 [R, n], finite (`spectra.harmonic_basis`).  Returns float64 [s, R, 1 + n_values] = den, num
    per value: the sums of basis[r, f] and of basis[r, f] * x_v[f, i] over the valid frames of slot i."""
    dev = _device(device)
    r, b = _f64(rec, dev, 3, _REC), _f64(basis, dev)
    n, s, cols = r.shape
    R, nv = _project_args(n, s, cols, b.shape, n_values)
    out = torch.empty((s, R, 1 + nv), dtype=torch.float64, device=dev)
    _call("vbs_project_series_f64", "1 <= n_values <= 3, n_values < cols <= 8", dev, _ptr(r), n, s, cols, nv, _ptr(b), R, _ptr(out))
    return out


def _fit_args(s, R, oc, Q, min_count, det_min):
    """`harmonic_fit_f64`'s argument checks (no device needed): -> (n_values, min_count, det_min) or ValueError."""
    nv, Q, mc, dm = int(oc) - 1, int(Q), int(min_count), float(det_min)
    if s < 1 or not (1 <= nv <= 3):
        raise ValueError("proj must be [s >= 1, R, 2 .. 4]")
    if Q < 1 or Q > (L.PROJ_MAX_ROWS - 1) // 4 or R != 1 + 4 * Q:
        raise ValueError(f"proj has {R} basis rows: harmonic_fit_f64 needs 1 + 4 Q = {1 + 4 * Q} in the order of "
                         f"spectra.harmonic_basis, 1 <= Q <= {(L.PROJ_MAX_ROWS - 1) // 4}")
    if mc < 3:
        raise ValueError("min_count must be >= 3 (a mean, a cosine and a sine)")
    if not (0.0 <= dm < 0.25):
        raise ValueError("det_min must lie in [0, 0.25)")
    return nv, mc, dm


def harmonic_fit_f64(proj, Q, min_count=8, det_min=1e-3, want_fit=True, want_peak=True, device=None):
    """The floating-mean least-squares fit x ~ c0 + a cos + b sin at every frequency of a `spectra.harmonic_basis`
    (`vbs_harmonic_fit_f64`).  proj float64 [s, 1 + 4 Q, 1 + n_values] as `project_series_f64` returns it for that basis.  A bin is
    ok where the series has at least `min_count` valid frames and the determinant of its normal equations exceeds `det_min` N^2
    (N^2 / 4 is what a whole number of periods without gaps gives).  Returns `(fit, peak)`: fit float64 [s, Q, 1 + 3 n_values] =
    ok, then a, b and the power p (the drop in the sum of squares) per value, zeros where not ok; peak float64 [s, n_values, 7] =
    flag (0 too few frames, 1 no ok bin, 2 a peak), N, mean, bin, a, b, p of the ok bin with the largest p (the first of equal
    ones).  Amplitude and phase: `spectra.amplitude_phase(a, b)`.  `want_fit` / `want_peak` False: None in its place."""
    dev = _device(device)
    p = _f64(proj, dev, 3, "proj must be [s, 1 + 4 Q, 1 + n_values]")
    if not (want_fit or want_peak):
        raise ValueError("at least one of fit and peak")
    s, R, oc = p.shape
    nv, mc, dm = _fit_args(s, R, oc, Q, min_count, det_min)
    fit = torch.empty((s, int(Q), 1 + 3 * nv), dtype=torch.float64, device=dev) if want_fit else None
    peak = torch.empty((s, nv, L.PEAK_COLS), dtype=torch.float64, device=dev) if want_peak else None
    _call("vbs_harmonic_fit_f64", "R == 1 + 4 Q, min_count >= 3, det_min in [0, 0.25)",
          dev, _ptr(p), s, R, nv, int(Q), mc, dm, _ptr(fit), _ptr(peak))
    return fit, peak


# ---- shear, torsion and strain along a recording (k_motion.hip): the global affine fit, the fit around every marker -----------------
_MOTION_WANT = ("grad", "strain", "residual")


def _motion_shape(n, s, cols, pos_shape, frame_range):
    if n < 1 or s < 1 or not (4 <= cols <= 8):
        raise ValueError("rec must be [n >= 1, s >= 1, 4 <= cols <= 8]: flag, dX, dY, dZ")
    if tuple(pos_shape) != (s, 2):
        raise ValueError(f"pos must be [{s}, 2]: the rest position of every slot of rec")
    return _frame_range(frame_range, n)


def _motion_args(n, s, cols, pos_shape, slots, reject_k, frame_range, want):
    """`motion_series_f64`'s argument checks (no device needed): -> (a, b, want as a tuple) or ValueError / VbsError."""
    a, b = _motion_shape(n, s, cols, pos_shape, frame_range)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _MOTION_WANT for w in want):
        raise ValueError(f"want must name at least one of {_MOTION_WANT}")
    if not (np.isfinite(float(reject_k)) and float(reject_k) >= 0.0):
        raise ValueError(f"reject_k {reject_k} must be finite and >= 0 (0 = no rejection)")
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= s):
            raise ValueError(f"slots outside the record's {s} slots")
    _capacity("vbs_motion_series_f64", (("slots", s, "FIELD_MAX_SLOTS"),))
    return a, b, want


def motion_series_f64(rec, pos, slots=None, reject_k=0.0, frame_range=None, want=_MOTION_WANT, device=None):
    """The affine fit of the displacement field of every frame (`vbs_motion_series_f64`): d_k ~ t_k + g_kx x + g_ky y over the
    used slots, its invariants and what it leaves.  rec float64 [n, s, cols >= 4] (host or device): col 0 the flag (nonzero =
    valid), cols 1 .. 3 dX, dY, dZ (`Engine.axis_displacement`'s `axis` as it is); pos float64 [s, 2] the rest positions; `slots`
    selects markers as `axis_displacement` does; `reject_k > 0`: one round of rejection at reject_k times the rms residual.
    Returns a dict of float64 device tensors for the frames [a, b) of `frame_range`, with the keys of `want`: `grad` [b-a, 3, 4] =
    flag (0 no fit, 1, 2 = refitted), t_k, g_kx, g_ky for k = X, Y, Z (a FIR record); `strain` [b-a, 16] = flag, count, n_used,
    dilation, omega, e1, e2, max_shear, shear_deg, rot_deg, lambda1, lambda2, tilt_deg, rms_inplane, rms_z, worst; `residual`
    [b-a, s, 4] = (1 kept | 2 rejected, r_X, r_Y, r_Z), zeros where not used: a record for every other series entry."""
    dev = _device(device)
    r, p = _f64(rec, dev, 3, _REC), _f64(pos, dev)
    n, s, cols = r.shape
    a, b, want = _motion_args(n, s, cols, p.shape, slots, reject_k, frame_range, want)
    mask = None
    if slots is not None:
        mask = torch.zeros((s,), dtype=torch.uint8, device=dev)
        mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=dev)] = 1
    shapes = {"grad": (b - a, 3, 4), "strain": (b - a, L.STRAIN_COLS), "residual": (b - a, s, 4)}
    out = {w: torch.empty(shapes[w], dtype=torch.float64, device=dev) for w in want}
    if a == b:
        return out
    _call("vbs_motion_series_f64", "4 <= cols <= 8, reject_k finite and >= 0, at least one output",
          dev, _ptr(r), n, s, cols, _ptr(p), _ptr(mask), float(reject_k), a, b, _ptr(out.get("grad")), _ptr(out.get("strain")),
          _ptr(out.get("residual")))
    return out


def _lstrain_args(n, s, cols, pos_shape, nbr_shape, min_count, det_rel, frame_range):
    """`local_strain_f64`'s argument checks (no device needed): -> (a, b, K) or ValueError / VbsError."""
    a, b = _motion_shape(n, s, cols, pos_shape, frame_range)
    ns = tuple(nbr_shape)
    if len(ns) != 2 or ns[0] != s or not (1 <= ns[1] <= L.STRAIN_MAX_NBR):
        raise ValueError(f"nbr must be [{s}, 1 <= K <= {L.STRAIN_MAX_NBR}] (`strain.neighbour_lists`)")
    K = int(ns[1])
    if not (3 <= int(min_count) <= K + 1):
        raise ValueError(f"min_count must lie in 3 .. K + 1 = {K + 1}")
    if not (0.0 <= float(det_rel) < 1.0):
        raise ValueError("det_rel must lie in [0, 1)")
    _capacity("vbs_local_strain_f64", (("slots", s, "FIELD_MAX_SLOTS"),))
    return a, b, K


def local_strain_f64(rec, pos, nbr, min_count=4, det_rel=0.01, frame_range=None, device=None):
    """The affine fit around every marker (`vbs_local_strain_f64`).  rec, pos as `motion_series_f64`; nbr int32 [s, K] from
    `strain.neighbour_lists` (an entry outside [0, s) = no neighbour).  Slot i has a result in a frame where it is valid itself,
    at least `min_count` of i and its neighbours are, and these do not lie close to a line (1 - rho^2 > det_rel).  Returns float64
    [b-a, s, 8] = cnt, dilation, omega, max_shear, e1, e2, g_Zx, g_Zy (zeros where there is no result): with n_values = 3 a
    record `field_map_f64` turns into maps of local dilation, torsion and shear."""
    dev = _device(device)
    r, p = _f64(rec, dev, 3, _REC), _f64(pos, dev)
    nb = torch.as_tensor(nbr, device=dev).to(torch.int32).contiguous()
    n, s, cols = r.shape
    a, b, K = _lstrain_args(n, s, cols, p.shape, nb.shape, min_count, det_rel, frame_range)
    out = torch.empty((b - a, s, L.LSTRAIN_COLS), dtype=torch.float64, device=dev)
    if a == b:
        return out
    _call("vbs_local_strain_f64", "4 <= cols <= 8, 1 <= K <= 12, 3 <= min_count <= K + 1, 0 <= det_rel < 1",
          dev, _ptr(r), n, s, cols, _ptr(p), _ptr(nb), K, int(min_count), float(det_rel), a, b, _ptr(out))
    return out


# ---- time-resolved amplitude and phase (k_envelope.hip): the sums of a sliding window at one frequency, the fit of every window ----
def taps_sum(half):
    """The ascending sum of all 2h + 1 weights w[k] = half[|k|], k = -h .. h: `sw` of `vbs_window_fit_f64`, as the FIR adds its own."""
    half = np.asarray(half, dtype=np.float64)
    sw = np.float64(0.0)
    for k in range(-(half.size - 1), half.size):
        sw = sw + half[abs(k)]
    return float(sw)


def _envelope_args(n, s, cols, carrier_shape, half, n_values, frame_range):
    """`window_moments_f64`'s argument checks (no device needed): -> (n_values, a, b) or ValueError."""
    _record_shape(n, s, cols)
    if tuple(carrier_shape) != (4, n):
        raise ValueError(f"carrier must be [4, {n}]: cos, sin of 2 pi nu f and of 2 pi (2 nu) f at every frame of rec (spectra.carrier)")
    nv = _n_values(cols, n_values, 3)
    half = np.asarray(half, dtype=np.float64)
    if half.ndim != 1 or half.size < 1 or half.size - 1 > L.ENV_MAX_HALF:
        raise ValueError(f"the window must have 1 .. {2 * L.ENV_MAX_HALF + 1} taps (half_window <= VBS_ENV_MAX_HALF = {L.ENV_MAX_HALF})")
    if not np.isfinite(half).all() or (half < 0.0).any() or not half[0] > 0.0:
        raise ValueError("the window's weights must be finite and >= 0, the centre > 0")
    a, b = _frame_range(frame_range, n)
    _capacity("vbs_window_moments_f64", (("frames", n, "PROJ_MAX_FRAMES"), ("slots", s, "PROJ_MAX_SLOTS")))
    return nv, a, b


def window_moments_f64(rec, carrier, taps, n_values=None, frame_range=None, device=None):
    """The weighted sums of a sliding window at one frequency for every frame and series (`vbs_window_moments_f64`), a banded
    float64 matrix product over the time axis.  rec float64 [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols
    1 .. n_values the values (default min(cols - 1, 3)).  carrier float64 [4, n], finite (`spectra.carrier(n, nu)`).  `taps`: the
    FULL odd-length symmetric window (`spectra.window_taps`), through `filters.half_taps` as `fir_series_f64` takes its own; at
    most 2 * 127 + 1 weights, each >= 0, the centre > 0.  Returns float64 [b-a, s, 5 + 4 n_values] = W, C1, S1, C2, S2, then X, XC,
    XS, XX per value, over the valid frames of [f - h, f + h], for the frames [a, b) of `frame_range` (default all); an output
    does not depend on the range it was asked in."""
    from .filters import half_taps
    dev = _device(device)
    half = np.ascontiguousarray(half_taps(taps), dtype=np.float64)
    r, c = _f64(rec, dev, 3, _REC), _f64(carrier, dev)
    n, s, cols = r.shape
    nv, a, b = _envelope_args(n, s, cols, c.shape, half, n_values, frame_range)
    out = torch.empty((b - a, s, 5 + 4 * nv), dtype=torch.float64, device=dev)
    if a == b:
        return out
    _call("vbs_window_moments_f64", "1 <= n_values <= 3, n_values < cols <= 8, finite weights >= 0",
          dev, _ptr(r), n, s, cols, nv, _ptr(c), _host_ptr(half), half.size, a, b, _ptr(out))
    return out


def _envelope_fit_args(F, s, M, taps_sum, min_coverage, det_min):
    """`window_fit_f64`'s argument checks (no device needed): -> (n_values, sw, min_coverage, det_min) or ValueError."""
    nv = (int(M) - 5) // 4
    if F < 1 or s < 1 or int(M) != 5 + 4 * nv or not (1 <= nv <= 3):
        raise ValueError("mom must be [F >= 1, s >= 1, 9 | 13 | 17]")
    sw, dm = float(taps_sum), float(det_min)
    if not (np.isfinite(sw) and sw > 0.0):
        raise ValueError("taps_sum must be finite and > 0 (engine.taps_sum of the window's half taps)")
    mc = _coverage(min_coverage)
    if not (0.0 <= dm < 0.25):
        raise ValueError("det_min must lie in [0, 0.25)")
    _capacity("vbs_window_fit_f64", (("frames", F, "PROJ_MAX_FRAMES"), ("slots", s, "PROJ_MAX_SLOTS")))
    return nv, sw, mc, dm


def window_fit_f64(mom, taps_sum, min_coverage=0.5, det_min=1e-3, device=None):
    """The weighted floating-mean fit x ~ c0 + a cos + b sin of every window (`vbs_window_fit_f64`).  mom float64
    [F, s, 5 + 4 n_values] as `window_moments_f64` returns it; `taps_sum` the ascending sum of the window's weights
    (`engine.taps_sum(filters.half_taps(taps))`).  A window is ok where W > 0, W >= `min_coverage` x taps_sum and the determinant
    of its normal equations exceeds `det_min` W^2 (W^2 / 4 is what a whole number of periods without gaps gives).  Returns float64
    [F, s, 1 + 5 n_values] = ok, then a, b, the power p, c0 and the weighted sum of squared deviations M2 per value; zeros where
    not ok.  Amplitude and phase: `spectra.amplitude_phase(a, b)`."""
    dev = _device(device)
    m = _f64(mom, dev, 3, "mom must be [F, s, 5 + 4 n_values]")
    F, s, M = m.shape
    nv, sw, mc, dm = _envelope_fit_args(F, s, M, taps_sum, min_coverage, det_min)
    out = torch.empty((F, s, 1 + 5 * nv), dtype=torch.float64, device=dev)
    _call("vbs_window_fit_f64", "taps_sum > 0, min_coverage in (0, 1], det_min in [0, 0.25)",
          dev, _ptr(m), F, s, nv, sw, mc, dm, _ptr(out))
    return out


# ---- principal modes of the displacement field (k_modes.hip): cross moments, covariance, leading eigenpairs, scores -----------------
def _moments_args(n, s, cols, shift_shape, n_values):
    """`cross_moments_f64`'s argument checks (no device needed): -> n_values or ValueError / VbsError."""
    _record_shape(n, s, cols)
    nv = _n_values(cols, n_values, 3)
    if shift_shape is not None and tuple(shift_shape) != (s, nv):
        raise ValueError(f"shift must be [{s}, {nv}]: one value per slot and value column")
    _capacity("vbs_cross_moments_f64", (("frames", n, "PROJ_MAX_FRAMES"), ("slots", s, "MOM_MAX_SLOTS")))
    return nv


def cross_moments_f64(rec, shift=None, n_values=None, device=None):
    """The cross moments of all pairs of series (`vbs_cross_moments_f64`), a symmetric float64 matrix product over the time axis.
    rec float64 [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols 1 .. n_values the values (default
    min(cols - 1, 3)).  `shift` float64 [s, n_values] (default none) is subtracted from every valid value first: pass the series'
    means.  Returns float64 [s, s, 4, 4]: [i, j, v, w] the sum over the frames of col_v(i) col_w(j), the columns of a slot being its
    shifted values (0 beyond n_values) and its flag as 1.0 / 0.0, all 0 where the slot is invalid - so [.., 3, 3] is the number
    of frames where both slots are valid and row / column 3 the sums pairwise-complete centring needs."""
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC)
    sh = None if shift is None else _f64(shift, dev)
    n, s, cols = r.shape
    nv = _moments_args(n, s, cols, None if sh is None else sh.shape, n_values)
    out = torch.empty((s, s, 4, 4), dtype=torch.float64, device=dev)
    _call("vbs_cross_moments_f64", "1 <= n_values <= 3, n_values < cols <= 8", dev, _ptr(r), n, s, cols, nv, _ptr(sh), _ptr(out))
    return out


_COV_MODES = {"pairwise": 0, "filled": 1, 0: 0, 1: 1}


def _covariance_args(mom_shape, n_values, mode, min_count, denom, mask_shape):
    """`covariance_f64`'s argument checks (no device needed): -> (s, n_values, mode, min_count, denom) or ValueError / VbsError."""
    ms = tuple(mom_shape)
    if len(ms) != 4 or ms[0] < 1 or ms[0] != ms[1] or ms[2:] != (4, 4):
        raise ValueError("mom must be [s >= 1, s, 4, 4] (`cross_moments_f64`)")
    nv = int(n_values)
    if not (1 <= nv <= 3):
        raise ValueError("n_values must be 1 .. 3")
    if mode not in _COV_MODES:
        raise ValueError("mode must be 'pairwise' (0) or 'filled' (1)")
    m, mc = _COV_MODES[mode], int(min_count)
    if mc < 2:
        raise ValueError("min_count must be >= 2")
    d = 1.0 if denom is None else float(denom)
    if m == 1 and (denom is None or not (np.isfinite(d) and d > 0.0)):
        raise ValueError("mode 'filled' needs a finite denom > 0 (n - 1)")
    if mask_shape is not None and tuple(mask_shape) != (ms[0],):
        raise ValueError(f"slot_mask must be [{ms[0]}]")
    _capacity("vbs_covariance_f64", (("slots", ms[0], "MOM_MAX_SLOTS"),))
    return ms[0], nv, m, mc, d


def covariance_f64(mom, n_values, mode="filled", min_count=2, denom=None, slot_mask=None, want_ok=False, device=None):
    """The covariance of all pairs of value columns from their cross moments (`vbs_covariance_f64`).  mom float64 [s, s, 4, 4] as
    `cross_moments_f64` returns it.  mode 'pairwise': every pair over the frames where both are valid, unbiased, possibly
    indefinite; 'filled': the Gram matrix of the data with gaps filled by the series' means over `denom` (n - 1), positive
    semidefinite while no pair falls below `min_count`.  A pair with fewer than `min_count` common frames, or with a slot whose `slot_mask` (uint8 [s]) is 0, gives exact
    zeros.  Returns float64 [C, C], C = s n_values, column c = i n_values + v; with `want_ok` also the uint8 [s, s] pair flags."""
    dev = _device(device)
    m = _f64(mom, dev)
    mk = None if slot_mask is None else torch.as_tensor(slot_mask, device=dev).to(torch.uint8).contiguous()
    s, nv, md, mc, d = _covariance_args(m.shape, n_values, mode, min_count, denom, None if mk is None else mk.shape)
    cov = torch.empty((s * nv, s * nv), dtype=torch.float64, device=dev)
    ok = torch.empty((s, s), dtype=torch.uint8, device=dev) if want_ok else None
    _call("vbs_covariance_f64", "mode 0 or 1, min_count >= 2, denom > 0",
          dev, _ptr(m), s, nv, md, mc, d, _ptr(mk), _ptr(cov), _ptr(ok))
    return (cov, ok) if want_ok else cov


def _modes_args(a_shape, r, iters, tiny):
    """`leading_modes_f64`'s argument checks (no device needed): -> (C, r, iters, tiny) or ValueError / VbsError."""
    sh = tuple(a_shape)
    if len(sh) != 2 or sh[0] < 1 or sh[0] != sh[1]:
        raise ValueError("A must be [C >= 1, C], symmetric")
    Cn, r, it, tn = sh[0], int(r), int(iters), float(tiny)
    if not (1 <= r <= min(Cn, L.MODES_MAX)):
        raise ValueError(f"n_modes must lie in 1 .. min(C, VBS_MODES_MAX = {L.MODES_MAX})")
    if not (0 <= it <= L.MODES_MAX_ITERS):
        raise ValueError(f"iters must lie in 0 .. {L.MODES_MAX_ITERS}")
    if not (0.0 <= tn < 1.0):
        raise ValueError("tiny must lie in [0, 1)")
    _capacity("vbs_leading_modes_f64", (("columns", Cn, "MODES_MAX_DIM"),))
    return Cn, r, it, tn


def leading_modes_f64(A, n_modes, iters=48, tiny=1e-24, work=None, device=None):
    """The `n_modes` <= 16 leading eigenpairs of a symmetric float64 [C, C] matrix (`vbs_leading_modes_f64`) by orthogonal
    iteration from a fixed start block with a FIXED number of iterations: deterministic, nothing is tested for convergence, and
    `resid` says what was reached.  The iteration finds the largest |lambda| (an indefinite A may give negative values); the
    values come descending.  A column whose squared norm falls below `tiny` times the largest is dropped (a rank-deficient A).
    `work`: an optional float64 device tensor of 2 * C * 16 elements to reuse.  Returns `(values [r], modes [r, C], resid [r],
    info int32 [2] = rank found, columns dropped)`: every mode has unit norm and its entry of largest magnitude positive."""
    dev = _device(device)
    a = _f64(A, dev)
    Cn, r, it, tn = _modes_args(a.shape, n_modes, iters, tiny)
    if work is None:
        work = torch.empty((2 * Cn * L.MODES_MAX,), dtype=torch.float64, device=dev)
    elif work.dtype != torch.float64 or work.device != dev or not work.is_contiguous() or work.numel() < 2 * Cn * L.MODES_MAX:
        raise ValueError(f"work must be a contiguous float64 tensor of 2 * C * {L.MODES_MAX} elements on {dev}")
    values = torch.empty((r,), dtype=torch.float64, device=dev)
    modes = torch.empty((r, Cn), dtype=torch.float64, device=dev)
    resid = torch.empty((r,), dtype=torch.float64, device=dev)
    info = torch.empty((2,), dtype=torch.int32, device=dev)
    _call("vbs_leading_modes_f64", "1 <= r <= min(C, 16), iters >= 0, 0 <= tiny < 1",
          dev, _ptr(a), Cn, r, it, tn, _ptr(work), _ptr(values), _ptr(modes), _ptr(resid), _ptr(info))
    return values, modes, resid, info


def _scores_args(n, s, cols, center_shape, modes_shape, n_values, min_coverage, frame_range):
    """`mode_scores_f64`'s argument checks (no device needed): -> (n_values, r, min_coverage, a, b) or ValueError / VbsError."""
    nv = _moments_args(n, s, cols, None, n_values)
    Cn = s * nv
    ms = tuple(modes_shape)
    if len(ms) != 2 or not (1 <= ms[0] <= L.MODES_MAX) or ms[1] != Cn:
        raise ValueError(f"modes must be [1 .. {L.MODES_MAX}, {Cn}] (`leading_modes_f64`)")
    if tuple(center_shape) != (Cn,):
        raise ValueError(f"center must be [{Cn}]: one value per value column of rec")
    mc = _coverage(min_coverage)
    a, b = _frame_range(frame_range, n)
    return nv, int(ms[0]), mc, a, b


def mode_scores_f64(rec, center, modes, n_values=None, min_coverage=0.5, frame_range=None, want_energy=True, device=None):
    """The score of every mode in every frame (`vbs_mode_scores_f64`): the least-squares amplitude of the mode over the columns
    that are valid in the frame.  rec float64 [n, s, cols]; center float64 [s n_values] (what the covariance was centred on);
    modes float64 [r, s n_values], unit norm.  Returns `(scores, energy)` for the frames [a, b) of `frame_range`: scores float64
    [b-a, r, 3] = flag, score, den - den the share of the mode that was seen, flag 1 where it reaches `min_coverage`, else
    (0, 0, den) - a record every series entry takes (cols 3, n_values 1, s = r); energy float64 [b-a, 2] = the number of valid
    columns and the sum of their squared centred values (None without `want_energy`)."""
    dev = _device(device)
    r_, c, m = _f64(rec, dev, 3, _REC), _f64(center, dev), _f64(modes, dev)
    n, s, cols = r_.shape
    nv, r, mc, a, b = _scores_args(n, s, cols, c.shape, m.shape, n_values, min_coverage, frame_range)
    scores = torch.empty((b - a, r, 3), dtype=torch.float64, device=dev)
    energy = torch.empty((b - a, 2), dtype=torch.float64, device=dev) if want_energy else None
    if a == b:
        return scores, energy
    _call("vbs_mode_scores_f64", "1 <= n_values <= 3, n_values < cols <= 8, min_coverage in (0, 1]",
          dev, _ptr(r_), n, s, cols, nv, _ptr(c), _ptr(m), r, mc, a, b, _ptr(scores), _ptr(energy))
    return scores, energy


# ---- marker velocity, acceleration and gap filling (k_kinematics.hip): the moments of a local polynomial fit, the fit -------------
KIN_PIV_REL = 5e-3             # the default `piv_rel`: a gap-free one-sided window keeps its full degree (DESIGN 4.20's table)


def n_kin_sums(degree, n_values):
    """M of `poly_moments_f64`: (2d + 1) + (d + 2) n_values."""
    return 2 * int(degree) + 1 + (int(degree) + 2) * int(n_values)


def _kin_args(n, s, cols, half_window, degree, window, n_values, frame_range):
    """`poly_moments_f64`'s argument checks (no device needed): -> (h, d, n_values, a, b) or ValueError."""
    _record_shape(n, s, cols)
    nv = _n_values(cols, n_values, 3)
    h, d = int(half_window), int(degree)
    if h != half_window or not (0 <= h <= L.KIN_MAX_HALF):
        raise ValueError(f"half_window must be an integer in 0 .. VBS_KIN_MAX_HALF = {L.KIN_MAX_HALF}")
    if d != degree or not (0 <= d <= L.KIN_MAX_DEGREE):
        raise ValueError(f"degree must be an integer in 0 .. VBS_KIN_MAX_DEGREE = {L.KIN_MAX_DEGREE}")
    if isinstance(window, str) and window not in ("hann", "rect"):
        raise ValueError('window must be "hann", "rect" or 2 half_window + 1 weights')
    a, b = _frame_range(frame_range, n)
    _capacity("vbs_poly_moments_f64", (("frames", n, "PROJ_MAX_FRAMES"), ("slots", s, "PROJ_MAX_SLOTS")))
    return h, d, nv, a, b


def poly_moments_f64(rec, half_window, degree, window="hann", n_values=None, frame_range=None, device=None):
    """The moments of a gap-aware weighted local polynomial fit along time for every frame and series (`vbs_poly_moments_f64`,
    DESIGN 4.20): several banded float64 matrix products over one staged operand.  rec float64 [n, s, cols] (host or device): col
    0 the flag (nonzero = valid), cols 1 .. n_values the values (default min(cols - 1, 3)).  The window is
    `filters.poly_window(half_window, window)` ("hann", "rect" or 2h + 1 symmetric weights), the tap rows `filters.poly_taps(half_window, degree, window)`.  Returns float64
    [b-a, s, (2d + 1) + (d + 2) n_values] = S_0 .. S_2d, then X_0 .. X_d, XX per value, over the valid frames of [f - h, f + h], for
    the frames [a, b) of `frame_range` (default all); an output does not depend on the range it was asked in."""
    from .filters import half_taps, poly_window
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC)
    n, s, cols = r.shape
    h, d, nv, a, b = _kin_args(n, s, cols, half_window, degree, window, n_values, frame_range)
    half = np.ascontiguousarray(half_taps(poly_window(h, window)), dtype=np.float64)
    out = torch.empty((b - a, s, n_kin_sums(d, nv)), dtype=torch.float64, device=dev)
    if a == b:
        return out
    _call("vbs_poly_moments_f64", "1 <= n_values <= 3, n_values < cols <= 8, 0 <= degree <= 3",
          dev, _ptr(r), n, s, cols, nv, _host_ptr(half), half.size, d, a, b, _ptr(out))
    return out


def kin_thresholds(sw, piv_full, min_coverage=0.5, piv_rel=KIN_PIV_REL, half_window=None):
    """thr [d + 1] of `vbs_poly_fit_f64`: thr[0] = min_coverage * sw, thr[k] = piv_rel * piv_full[k], one IEEE product each; with
    `half_window`, +inf for the orders k >= 2h + 1, which a window of 2h + 1 frames cannot determine (their full pivot is zero up
    to rounding, and a rounding is not a pivot)."""
    piv = np.asarray(piv_full, dtype=np.float64)
    thr = np.float64(piv_rel) * piv
    thr[0] = np.float64(min_coverage) * np.float64(sw)
    if half_window is not None:
        thr[2 * int(half_window) + 1:] = np.inf
    return thr


_KIN_PIVOTS = {}               # (h, d, window name) -> (sw, piv_full) of `filters.poly_taps`


def _kin_fit_args(F, s, M, n, cols, half_window, degree, window, n_values, min_coverage, piv_rel, fill_degree, frame_range):
    """`poly_fit_f64`'s argument checks (no device needed): -> (h, d, n_values, thr [d + 1], fill_degree, a, b) or ValueError."""
    from .filters import poly_taps
    h, d, nv, a, b = _kin_args(n, s, cols, half_window, degree, window, n_values, frame_range)
    if (int(F), int(M)) != (b - a, n_kin_sums(d, nv)):
        raise ValueError(f"mom must be [{b - a}, {s}, {n_kin_sums(d, nv)}]: the moments of the frames {a}:{b} at degree {d} "
                         f"and {nv} values")
    mc, pr = _coverage(min_coverage), float(piv_rel)
    if not (0.0 <= pr < 1.0):
        raise ValueError("piv_rel must lie in [0, 1)")
    fd = int(fill_degree)
    if fd != fill_degree or not (0 <= fd <= L.KIN_MAX_DEGREE):
        raise ValueError(f"fill_degree must be an integer in 0 .. {L.KIN_MAX_DEGREE} (above `degree` nothing is filled)")
    if isinstance(window, str):
        if (h, d, window) not in _KIN_PIVOTS:                    # (host loops over the window: formed once per design)
            _KIN_PIVOTS[(h, d, window)] = poly_taps(h, d, window)[1:]
        sw, piv = _KIN_PIVOTS[(h, d, window)]
    else:
        _, sw, piv = poly_taps(h, d, window)
    return h, d, nv, kin_thresholds(sw, piv, mc, pr, h), fd, a, b


def poly_fit_f64(mom, rec, half_window, degree, window="hann", n_values=None, min_coverage=0.5, piv_rel=KIN_PIV_REL,
                 fill_degree=1, want_filled=False, frame_range=None, device=None):
    """The local polynomial fit of every window with its fallback in degree (`vbs_poly_fit_f64`).  mom float64
    [b-a, s, M] as `poly_moments_f64(rec, half_window, degree, window, n_values, frame_range)` returns it, rec the record itself.
    A window keeps the largest degree q <= d whose pivots D_0 .. D_q all exceed their thresholds: D_0 = S_0 > `min_coverage` x the
    window's sum, D_k > `piv_rel` x the pivot of the gap-free full window.  Returns `fit` float64 [b-a, s, 2 + (d + 2) n_values] =
    flag (centre valid + 2 (q >= 0) + 4 (q == d)), q, then per value the derivatives y_0 .. y_d at the centre in units of frames
    (0 above q) and the weighted residual sum of squares; with `want_filled` (fit, filled): `filled` float64 [b-a, s, cols], the
    valid rows of rec bit for bit, flag 2.0 and y_0 where the entry is missing and q >= `fill_degree`, zeros otherwise -
    a record every other entry of this module takes as it is."""
    dev = _device(device)
    m, r = _f64(mom, dev), _f64(rec, dev)
    if m.dim() != 3 or r.dim() != 3 or m.shape[1] != r.shape[1]:
        raise ValueError("mom must be [F, s, M] and rec [n, s, cols] with the same s")
    F, s, M = m.shape
    n, _, cols = r.shape
    h, d, nv, thr, fd, a, b = _kin_fit_args(F, s, M, n, cols, half_window, degree, window, n_values, min_coverage, piv_rel,
                                            fill_degree, frame_range)
    fit = torch.empty((F, s, 2 + (d + 2) * nv), dtype=torch.float64, device=dev)
    filled = torch.empty((F, s, cols), dtype=torch.float64, device=dev) if want_filled else None
    if F:
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        _call("vbs_poly_fit_f64", "thresholds >= 0, 0 <= fill_degree <= 3",
              dev, _ptr(m), _ptr(r), n, s, cols, nv, d, h, _host_ptr(thr), fd, a, b, _ptr(fit), _ptr(filled))
    return (fit, filled) if want_filled else fit


# ---- the probe-indentation validation (k_steps.hip): steps, dwells ---------------------------------------------------------------
def step_response_f64(rec, window, n_values=None, min_count=None, device=None):
    """A step detector along time with gaps (`vbs_step_response_f64`): per frame the mean of the valid frames of [f, f+window)
    minus that of [f-window, f).  rec float64 [n, s, cols] (host or device): col 0 the flag (nonzero = valid), cols 1 .. n_values
    the values (default cols - 1).  `min_count` (default (window + 1) // 2): the valid frames each side needs.  Returns float64
    [n, s, 2 + n_values] = ok, score (the SQUARED norm of the difference), the difference per value; zero where not ok."""
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC, nonempty=2)
    n, s, cols = r.shape
    nv = _n_values(cols, n_values, None)
    w = int(window)
    mc = (w + 1) // 2 if min_count is None else int(min_count)
    out = torch.empty((n, s, 2 + nv), dtype=torch.float64, device=dev)
    _call("vbs_step_response_f64", f"1 <= min_count <= window <= {L.STEP_MAX_WINDOW}, 1 <= n_values < cols <= 8",
          dev, _ptr(r), n, s, cols, nv, w, mc, _ptr(out))
    return out


def find_steps_f64(resp, window, threshold, max_steps=L.STEP_MAX_STEPS, device=None):
    """The peaks of a step response (`vbs_find_steps_f64`): frame f is a step where it is ok, its score reaches `threshold`
    squared and no ok frame within `window` on either side has a larger score (of equal ones the earliest wins).  resp float64
    [n, s, >= 2] as `step_response_f64` returns it.  Returns int32 [s, 1 + max_steps]: the number of steps found (more than
    `max_steps` = an overflow of that series), the first `max_steps` of them in ascending order, then -1."""
    dev = _device(device)
    r = _f64(resp, dev, 3, "resp must be [n >= 1, s >= 1, cols >= 2]", nonempty=2)
    n, s, cols = r.shape
    ms = int(max_steps)
    steps = torch.empty((s, 1 + max(ms, 0)), dtype=torch.int32, device=dev)
    thr = float(threshold)
    _call("vbs_find_steps_f64", f"1 <= window <= {L.STEP_MAX_WINDOW}, threshold >= 0, 1 <= max_steps <= {L.STEP_MAX_STEPS}, "
          "2 <= cols <= 9", dev, _ptr(r), n, s, cols, int(window), thr * thr, ms, _ptr(steps))
    return steps


def dwell_stats_f64(rec, steps, guard, n_values=None, device=None):
    """The statistics of the dwells between steps (`vbs_dwell_stats_f64`).  rec float64 [n, s, cols] as `step_response_f64`
    takes it; steps int32 [s or 1, 1 + max_steps] as `find_steps_f64` returns it (one row: the list is shared by all series);
    `guard`: frames left out on either side of a step.  Returns float64 [s, max_steps + 1, 3 + 2 n_values] = begin, end, count,
    mean per value, M2 per value (sum of squared deviations; std = sqrt(M2 / (count - 1))); rows past the last dwell are
    (-1, -1, 0, NaN ...)."""
    dev = _device(device)
    r = _f64(rec, dev, 3, _REC, nonempty=2)
    n, s, cols = r.shape
    nv = _n_values(cols, n_values, None)
    st = torch.as_tensor(steps, dtype=torch.int32, device=dev).contiguous()
    if st.dim() != 2 or st.shape[1] < 2:
        raise ValueError("steps must be [s or 1, 1 + max_steps]")
    ms = st.shape[1] - 1
    out = torch.empty((s, ms + 1, 3 + 2 * nv), dtype=torch.float64, device=dev)
    _call("vbs_dwell_stats_f64", f"steps rows = s or 1, 1 <= max_steps <= {L.STEP_MAX_STEPS}, guard >= 0, 1 <= n_values < cols <= 8",
          dev, _ptr(r), n, s, cols, nv, _ptr(st), st.shape[0], ms, int(guard), _ptr(out))
    return out


# ---- uncertainty of the 3-D solve (k_uncert.hip): Jacobians by forward mode, covariances, the pixel noise of a still segment -------
_TABLE = "table must be float32 [n >= 1, m >= 1, 10]"


def _f32_table(table, dev):
    t = torch.as_tensor(table, dtype=torch.float32, device=dev).contiguous()
    if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 1 or t.shape[2] != L.TABLE_COLS:
        raise ValueError(_TABLE)
    return t


def solve3d_jacobian(uvd, cam, device=None):
    """The 3-D solve of points with its Jacobians (`vbs_uncert_points`).  uvd float64 [n, 3] = (Cx, Cy, major) as a table row holds
    them, BEFORE undistortion; cam an `_lib.Camera`.  Returns `(xyz [n, 3], J_obs [n, 3, 3], J_cam [n, 3, 16], ok int32 [n])`: xyz
    and ok bit for bit `calculate_3d(undistort_points(..))`, J_obs = dX / d(Cx, Cy, major), J_cam = dX / d(fx, fy, cx, cy, k1, k2,
    p1, p2, k3, w0, w1, w2, T0, T1, T2, dmm) by forward mode through the five undistortion iterations as executed; zeros where ok
    is 0."""
    dev = _device(device)
    p = _f64(uvd, dev, 2, "uvd must be [n, 3]")
    if p.shape[1] != 3:
        raise ValueError("uvd must be [n, 3]")
    n = p.shape[0]
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    jo = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
    jc = torch.empty((n, 3, L.UNCERT_CAM), dtype=torch.float64, device=dev)
    ok = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return xyz, jo, jc, ok
    _call("vbs_uncert_points", "uvd [n, 3]", dev, _ptr(p), n, C.byref(cam), _ptr(xyz), _ptr(jo), _ptr(jc), _ptr(ok))
    return xyz, jo, jc, ok


def _uncert_args(n, m, obs_cov, cam_factor, ref_frame, slots, min_marker_size_px, piv_rel, frame_range):
    """`solve3d_cov`'s argument checks (no device needed): -> (obs [1 or m, 6], L [16, q], ref_frame or -1, a, b) or ValueError."""
    obs = np.ascontiguousarray(obs_cov, dtype=np.float64)
    if obs.shape == (3, 3):
        if not np.array_equal(obs, obs.T):
            raise ValueError("obs_cov as a 3 x 3 matrix must be symmetric")
        obs = obs[np.triu_indices(3)]
    if obs.shape == (6,):
        obs = obs.reshape(1, 6)
    if obs.shape not in ((1, 6), (m, 6)):
        raise ValueError(f"obs_cov must be [6] or [{m}, 6] = uu, uv, ud, vv, vd, dd of (Cx, Cy, major), or one symmetric 3 x 3")
    if not np.isfinite(obs).all():
        raise ValueError("obs_cov must be finite")
    Lf = np.zeros((L.UNCERT_CAM, 0)) if cam_factor is None else np.ascontiguousarray(cam_factor, dtype=np.float64)
    if Lf.ndim != 2 or Lf.shape[0] != L.UNCERT_CAM or Lf.shape[1] > L.UNCERT_CAM:
        raise ValueError(f"cam_factor must be [{L.UNCERT_CAM}, q <= {L.UNCERT_CAM}] (`uncertainty.camera_factor`)")
    if not np.isfinite(Lf).all():
        raise ValueError("cam_factor must be finite")
    rf = -1 if ref_frame is None else int(ref_frame)
    if ref_frame is not None and not (0 <= rf < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= m):
            raise ValueError(f"slots outside the table's {m} slots")
    if np.isnan(float(min_marker_size_px)):
        raise ValueError("min_marker_size_px must be a number")
    if not (np.isfinite(float(piv_rel)) and float(piv_rel) >= 0.0):
        raise ValueError("piv_rel must be finite and >= 0")
    a, b = _frame_range(frame_range, n)
    return np.ascontiguousarray(obs), np.ascontiguousarray(Lf), rf, a, b


def solve3d_cov(table, cam, obs_cov, cam_factor=None, ref_frame=None, slots=None, min_marker_size_px=5.0, piv_rel=1e-12,
                frame_range=None, device=None):
    """The covariance of every 3-D point of a table, of its displacement from `ref_frame` and of the frame's total displacement
    (`vbs_uncert_cov`, `vbs_uncert_total`).  table float32 [n, m, 10]; cam an `_lib.Camera`; obs_cov the covariance of
    (Cx, Cy, major) as [6] = uu, uv, ud, vv, vd, dd, one per slot [m, 6], or a symmetric 3 x 3 (`uncertainty.obs_cov`); cam_factor
    [16, q] with Sigma_theta = L L' (`uncertainty.camera_factor`; None = an exact camera).  Returns a dict of float64 device tensors
    for the frames [a, b) of `frame_range`: `cov` [b-a, m, 7] = flag, xx, xy, xz, yy, yz, zz of Sigma_X; with a `ref_frame` also
    `dcov` [b-a, m, 8] = flag (1 both rows usable, 3 = t2 valid), Sigma_D, t2 = D' Sigma_D^-1 D, and `total` [b-a, 8] = count,
    complete, var_x, var_y, var_z of `axis_displacement`'s total over `slots`, then the coherent camera share of each variance;
    without one both are None.  A row is usable where it carries the XYZ flag, major >= min_marker_size_px and the solve succeeds."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    obs, Lf, rf, a, b = _uncert_args(n, m, obs_cov, cam_factor, ref_frame, slots, min_marker_size_px, piv_rel, frame_range)
    q = Lf.shape[1]
    cov = torch.empty((b - a, m, L.UNCERT_COV_COLS), dtype=torch.float64, device=dev)
    dcov = torch.empty((b - a, m, L.UNCERT_DCOV_COLS), dtype=torch.float64, device=dev) if rf >= 0 else None
    total = torch.empty((b - a, L.UNCERT_TOTAL_COLS), dtype=torch.float64, device=dev) if rf >= 0 else None
    out = {"cov": cov, "dcov": dcov, "total": total}
    if a == b:
        return out
    work = torch.empty((m * L.UNCERT_WORK_COLS,), dtype=torch.float64, device=dev)
    hint = "obs_cov finite [1 or m, 6], cam_factor finite [16, q <= 16], ref_frame inside the table, piv_rel >= 0"
    _call("vbs_uncert_cov", hint, dev, _ptr(t), n, m, C.byref(cam), _host_ptr(obs), obs.shape[0], _host_ptr(Lf), q, rf,
          float(min_marker_size_px), float(piv_rel), a, b, _ptr(work), _ptr(cov), _ptr(dcov))
    if rf >= 0:
        mask = None
        if slots is not None:
            mask = torch.zeros((m,), dtype=torch.uint8, device=dev)
            mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=dev)] = 1
        _call("vbs_uncert_total", hint, dev, _ptr(t), n, m, C.byref(cam), _host_ptr(obs), obs.shape[0], _host_ptr(Lf), q, rf,
              _ptr(mask), float(min_marker_size_px), a, b, _ptr(work), _ptr(total))
    return out


# ---- uncertainty of the pose misalignment (k_posecov.hip): the covariance of the plane, of its angles, and t2 -------------------------
def _posecov_args(n, m, obs_cov, cam_factor, start_frame, mode, scale, slots, reject_k, min_marker_size_px, piv_rel, frame_range,
                  ref_disp_shape, ref_xyz_shape, ref_rows_shape=None, want=("pose", "pcov")):
    """`pose_cov`'s argument checks (no device needed): what `vbs_pose_series` and `vbs_uncert_total` refuse, in the wrappers' words
    -> (obs [1 or m, 6], L [16, q], a, b, shell_mode, want) or ValueError."""
    if n < 1 or m < 1:
        raise ValueError(_TABLE)
    if mode not in ("plane", "shell"):
        raise ValueError("mode must be 'plane' or 'shell'")
    if int(start_frame) != start_frame or not (0 <= int(start_frame) < n):
        raise ValueError(f"start_frame {start_frame} outside the table's {n} frames")
    if not np.isfinite(float(scale)):
        raise ValueError(f"scale {scale} is not finite")
    if not (np.isfinite(float(reject_k)) and float(reject_k) >= 0.0):
        raise ValueError(f"reject_k {reject_k} must be finite and >= 0 (0 = no rejection)")
    if tuple(ref_disp_shape) != (m, L.AXIS_COLS) or tuple(ref_xyz_shape) != (m, 3):
        raise ValueError(f"ref_disp must be [{m}, {L.AXIS_COLS}] and ref_xyz [{m}, 3]: one row per table slot")
    if ref_rows_shape is not None and tuple(ref_rows_shape) != (2, m, L.TABLE_COLS):
        raise ValueError(f"ref_rows must be [2, {m}, {L.TABLE_COLS}]: the reference session's rows at ref_start and at ref_end")
    want = tuple(want)
    if not want or any(w not in ("pose", "pcov") for w in want):
        raise ValueError("want must name at least one of 'pose' and 'pcov'")
    obs, Lf, _, a, b = _uncert_args(n, m, obs_cov, cam_factor, None, slots, min_marker_size_px, piv_rel, frame_range)
    return obs, Lf, a, b, 1 if mode == "shell" else 0, want


def pose_cov(table, ref_disp, ref_xyz, cam, obs_cov, cam_factor=None, ref_rows=None, start_frame=0, mode="plane", scale=1.0,
             slots=None, reject_k=0.0, min_marker_size_px=5.0, piv_rel=1e-12, frame_range=None, want=("pose", "pcov"), device=None):
    """The first-order covariance of the plane `Engine.pose_series` fits, of its tilt and azimuth, and the test "is the plane tilted
    at all" (`vbs_pose_cov`).  table, ref_disp, ref_xyz, start_frame, mode, scale, slots, reject_k and frame_range as
    `Engine.pose_series` takes them; cam, obs_cov, cam_factor, min_marker_size_px and piv_rel as `solve3d_cov` does.  ref_rows
    float32 [2, m, 10]: the reference session's rows at the two frames whose difference `ref_disp` is (ref_start first); None takes
    the reference state as exact.  Returns float64 device tensors `(pose, pcov)` for the frames [a, b) (None for one `want` leaves
    out): pose [b-a, 8] as `Engine.pose_series`; pcov [b-a, 17] = flag (bit 1: a plane exists and every used slot is usable - only
    then is any other column but n_unusable nonzero; bit 2: t2 valid; bit 4: the angle variances are valid), n_unusable, then aa,
    ab, ac, bb, bc, cc of Sigma, the same six of the camera's share Sigma_cam, var_tilt and var_azimuth in degrees squared, and
    t2 = (a, b) Sigma_ab^-1 (a, b)'."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    rd = torch.as_tensor(ref_disp, dtype=torch.float64, device=dev).contiguous()
    rx = torch.as_tensor(ref_xyz, dtype=torch.float64, device=dev).contiguous()
    rr = None if ref_rows is None else torch.as_tensor(ref_rows, dtype=torch.float32, device=dev).contiguous()
    obs, Lf, a, b, shell, want = _posecov_args(n, m, obs_cov, cam_factor, start_frame, mode, scale, slots, reject_k, min_marker_size_px,
                                               piv_rel, frame_range, rd.shape, rx.shape, None if rr is None else rr.shape, want)
    pose = torch.empty((b - a, L.POSE_COLS), dtype=torch.float64, device=dev) if "pose" in want else None
    pcov = torch.empty((b - a, L.POSECOV_COLS), dtype=torch.float64, device=dev) if "pcov" in want else None
    if a == b:
        return pose, pcov
    mask = None
    if slots is not None:
        mask = torch.zeros((m,), dtype=torch.uint8, device=dev)
        mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=dev)] = 1
    work = torch.empty((m * L.UNCERT_WORK_COLS,), dtype=torch.float64, device=dev)
    hint = ("start_frame inside the table, scale and reject_k finite, reject_k >= 0, obs_cov finite [1 or m, 6], cam_factor finite "
            "[16, q <= 16], piv_rel >= 0")
    _call("vbs_pose_cov", hint, dev, _ptr(t), n, m, int(start_frame), _ptr(rd), _ptr(rx), _ptr(mask), shell, float(scale),
          float(reject_k), C.byref(cam), _host_ptr(obs), obs.shape[0], _host_ptr(Lf), Lf.shape[1], float(min_marker_size_px),
          float(piv_rel), _ptr(rr), a, b, _ptr(work), _ptr(pose), _ptr(pcov))
    return pose, pcov


# ---- indentation shape along a recording (k_shape.hip): the quadric of every frame, its apex, depth and curvatures ---------------------
_SHAPE_WANT = ("shape", "coef", "residual")


def _shape_args(n, m, start_frame, mode, scale, length, slots, reject_k, min_count, piv_rel, apex_rel, max_apex, frame_range,
                ref_disp_shape, ref_xyz_shape, want=_SHAPE_WANT):
    """`shape_series`'s argument checks (no device needed): what `vbs_shape_series` refuses, in the wrappers' words
    -> (a, b, shell_mode, min_count, want) or ValueError."""
    if n < 1 or m < 1:
        raise ValueError(_TABLE)
    if mode not in ("plane", "shell"):
        raise ValueError("mode must be 'plane' or 'shell'")
    if int(start_frame) != start_frame or not (0 <= int(start_frame) < n):
        raise ValueError(f"start_frame {start_frame} outside the table's {n} frames")
    if not np.isfinite(float(scale)):
        raise ValueError(f"scale {scale} is not finite")
    if not (np.isfinite(float(reject_k)) and float(reject_k) >= 0.0):
        raise ValueError(f"reject_k {reject_k} must be finite and >= 0 (0 = no rejection)")
    if tuple(ref_disp_shape) != (m, L.AXIS_COLS) or tuple(ref_xyz_shape) != (m, 3):
        raise ValueError(f"ref_disp must be [{m}, {L.AXIS_COLS}] and ref_xyz [{m}, 3]: one row per table slot")
    if not (np.isfinite(float(length)) and float(length) > 0.0):
        raise ValueError(f"length {length} must be finite and > 0")
    if int(min_count) != min_count or int(min_count) < 6:
        raise ValueError("min_count must be an integer >= 6 (a quadric has six coefficients)")
    for name, v in (("piv_rel", piv_rel), ("apex_rel", apex_rel), ("max_apex", max_apex)):
        if not (np.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} {v} must be finite and >= 0")
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= m):
            raise ValueError(f"slots outside the table's {m} slots")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _SHAPE_WANT for w in want):
        raise ValueError(f"want must name at least one of {_SHAPE_WANT}")
    a, b = _frame_range(frame_range, n)
    return a, b, 1 if mode == "shell" else 0, int(min_count), want


def shape_series(table, ref_disp, ref_xyz, start_frame=0, mode="plane", scale=1.0, length=None, slots=None, reject_k=0.0,
                 min_count=9, piv_rel=1e-10, apex_rel=1e-6, max_apex=2.0, frame_range=None, want=_SHAPE_WANT, device=None):
    """The quadric through the end points of every frame (`vbs_shape_series`): z ~ c0 + a x + b y + (p x x + 2 q x y +
    r y y) / 2 around the means of the used slots, with the fallback to the plane of the same factorisation and to nothing.  table,
    ref_disp, ref_xyz, start_frame, mode, scale, slots, reject_k and frame_range as `Engine.pose_series` takes them.  `length`
    scales x and y inside the fit (default `shapes.default_length(ref_xyz, slots)`, the rms radius of the selected reference
    positions; the results do not carry it).  Degree 2 needs `min_count` common slots (>= 6) and six pivots above `piv_rel` times
    their diagonal, degree 1 three; the apex is valid where |K| > `apex_rel` (p^2 + 2 q^2 + r^2) and it lies within `max_apex`
    lengths of the mean.  The defaults are this project's.  Returns a dict of float64 device tensors for the frames [a, b), with
    the keys of `want`: `shape` [b-a, 24] = degree, count, n_used, mx, my, mz, c0, a, b, p, q, r, rms_plane, rms, H, K, k1, k2,
    dir_deg, apex, apex_x, apex_y, apex_z, depth; `coef` [b-a, 2, 4] = (degree, c0, a, b), (degree == 2, p, q, r), a FIR record
    with n_values 3; `residual` [b-a, m, 2] = (1, r) for every used slot of a frame with a fit, a `field_map_f64` record."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    rd = torch.as_tensor(ref_disp, dtype=torch.float64, device=dev).contiguous()
    rx = torch.as_tensor(ref_xyz, dtype=torch.float64, device=dev).contiguous()
    if length is None and tuple(rx.shape) == (m, 3):
        from .shapes import default_length
        length = default_length(rx.cpu().numpy(), slots)
    a, b, shell, mc, want = _shape_args(n, m, start_frame, mode, scale, length, slots, reject_k, min_count, piv_rel, apex_rel, max_apex,
                                        frame_range, rd.shape, rx.shape, want)
    shapes = {"shape": (b - a, L.SHAPE_COLS), "coef": (b - a, 2, 4), "residual": (b - a, m, 2)}
    out = {w: torch.empty(shapes[w], dtype=torch.float64, device=dev) for w in want}
    if a == b:
        return out
    mask = None
    if slots is not None:
        mask = torch.zeros((m,), dtype=torch.uint8, device=dev)
        mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=dev)] = 1
    _call("vbs_shape_series", "start_frame inside the table, scale and reject_k finite, reject_k >= 0, length > 0, min_count >= 6, "
          "piv_rel, apex_rel and max_apex finite and >= 0, at least one output",
          dev, _ptr(t), n, m, int(start_frame), _ptr(rd), _ptr(rx), _ptr(mask), shell, float(scale), float(length), float(reject_k),
          mc, float(piv_rel), float(apex_rel), float(max_apex), a, b, _ptr(out.get("shape")), _ptr(out.get("coef")),
          _ptr(out.get("residual")))
    return out


# ---- rigid motion along a recording (k_rigid.hip): rotation, translation and scale of every frame, the residual per marker ------------
_RIGID_WANT = ("rigid", "coef", "residual")


def _rigid_args(n, m, source_shape, slots, with_scale, reject_k, gap_rel, frame_range, want=_RIGID_WANT):
    """`rigid_series`'s argument checks (no device needed): what `vbs_rigid_series` refuses, in the order the entry checks, in the
    wrappers' words -> (a, b, with_scale 0 / 1, want) or ValueError."""
    if n < 1 or m < 1:
        raise ValueError(_TABLE)
    if tuple(source_shape) != (m, 4):
        raise ValueError(f"source must be [{m}, 4] = (flag, X, Y, Z): one row per table slot")
    a, b = _frame_range(frame_range, n)
    if not isinstance(with_scale, (bool, np.bool_)) and with_scale not in (0, 1):
        raise ValueError("with_scale must be False / True")
    for name, v in (("reject_k", reject_k), ("gap_rel", gap_rel)):
        if not (np.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} {v} must be finite and >= 0")
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= m):
            raise ValueError(f"slots outside the table's {m} slots")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _RIGID_WANT for w in want):
        raise ValueError(f"want must name at least one of {_RIGID_WANT}")
    return a, b, int(bool(with_scale)), want


def rigid_series(table, source, slots=None, with_scale=False, reject_k=0.0, gap_rel=1e-6, frame_range=None, want=_RIGID_WANT,
                 device=None):
    """How the markers of every frame moved as a body against `source` (`vbs_rigid_series`): the rotation R, the
    translation t and, with `with_scale`, the scale s of  P ~ s R Q + t  by Horn's quaternion form, and what that motion leaves per
    marker.  table float32 [n, m, 10]; source float64 [m, 4] = (flag, X, Y, Z), the point set the frames are registered TO
    (`rigid.source_from_table`, `rigid.source_from_layout`); `slots` selects; `reject_k` > 0 asks for one round of rejection at
    reject_k times the rms; a fit exists where three or more slots are common and the two largest eigenvalues differ by more than
    `gap_rel` of Sqq + Spp.  The defaults are this project's.  Returns a dict of float64 device tensors for the frames [a, b), with
    the keys of `want`: `rigid` [b-a, 33] = flag, count, n_used, qm [3], pm [3], w, x, y, z, R [9] row-major, t [3], s, rms, rms0,
    angle_deg, tilt_deg, azimuth_deg, twist_deg, gap; `coef` [b-a, 4, 4] = (flag, R row i), (flag, t), a FIR record with n_values
    3; `residual` [b-a, m, 4] = (1, ex, ey, ez) for every used slot of a frame with a fit, a record with n_values 3."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    src = torch.as_tensor(source, dtype=torch.float64, device=dev).contiguous()
    a, b, ws, want = _rigid_args(n, m, src.shape, slots, with_scale, reject_k, gap_rel, frame_range, want)
    shapes = {"rigid": (b - a, L.RIGID_COLS), "coef": (b - a, 4, 4), "residual": (b - a, m, 4)}
    out = {w: torch.empty(shapes[w], dtype=torch.float64, device=dev) for w in want}
    if a == b:
        return out
    mask = None
    if slots is not None:
        mask = torch.zeros((m,), dtype=torch.uint8, device=dev)
        mask[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=dev)] = 1
    _call("vbs_rigid_series", "with_scale 0 / 1, reject_k and gap_rel finite and >= 0, at least one output",
          dev, _ptr(t), n, m, _ptr(src), _ptr(mask), ws, float(reject_k), float(gap_rel), a, b, _ptr(out.get("rigid")),
          _ptr(out.get("coef")), _ptr(out.get("residual")))
    return out


# ---- noise-weighted rigid motion (k_rigid_ml.hip): the ML pose from rigid_series's start, its covariance, chi^2, distances ------------
_RIGID_ML_WANT = ("ml", "pcov", "coef", "mahal")


def _rigid_ml_args(n, m, source_shape, cov_shape, rigid_shape, residual_shape, source_cov_shape, iters, piv_rel, frame_range,
                   want=_RIGID_ML_WANT):
    """`rigid_ml_series`'s argument checks (no device needed): what `vbs_rigid_ml_series` refuses, in the order the entry checks, and
    the shapes of the per-frame inputs, in the wrappers' words -> (a, b, iters, want) or ValueError."""
    if n < 1 or m < 1:
        raise ValueError(_TABLE)
    if tuple(source_shape) != (m, 4):
        raise ValueError(f"source must be [{m}, 4] = (flag, X, Y, Z): one row per table slot")
    a, b = _frame_range(frame_range, n)
    for name, shape, expect in (("cov", cov_shape, (b - a, m, L.UNCERT_COV_COLS)), ("rigid", rigid_shape, (b - a, L.RIGID_COLS)),
                                ("residual", residual_shape, (b - a, m, 4))):
        if tuple(shape) != expect:
            raise ValueError(f"{name} must be {list(expect)}: one row per frame of [{a}, {b}), as its entry wrote it for that range")
    if source_cov_shape is not None and tuple(source_cov_shape) != (m, L.UNCERT_COV_COLS):
        raise ValueError(f"source_cov must be [{m}, {L.UNCERT_COV_COLS}] = (flag, xx, xy, xz, yy, yz, zz), or None")
    if isinstance(iters, (bool, np.bool_)) or int(iters) != iters or not (1 <= int(iters) <= L.RIGID_ML_MAX_ITERS):
        raise ValueError(f"iters {iters} must be an integer in [1, {L.RIGID_ML_MAX_ITERS}]")
    if not (np.isfinite(float(piv_rel)) and float(piv_rel) >= 0.0):
        raise ValueError(f"piv_rel {piv_rel} must be finite and >= 0")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _RIGID_ML_WANT for w in want):
        raise ValueError(f"want must name at least one of {_RIGID_ML_WANT}")
    return a, b, int(iters), want


def rigid_ml_series(table, source, cov, rigid, residual, source_cov=None, iters=8, piv_rel=1e-12, frame_range=None,
                    want=_RIGID_ML_WANT, device=None):
    """The noise-weighted rigid motion of every frame (`vbs_rigid_ml_series`): the maximum-likelihood pose of
    P ~ R (Q - qm) + c  under the covariance of every 3-D point, from the pose `rigid_series` left, by `iters` Gauss-Newton steps;
    the covariance of that pose; chi^2; the Mahalanobis distance of every marker.  table and source as `rigid_series` took them;
    `cov` [b-a, m, 7] as `solve3d_cov` writes it, `rigid` [b-a, 33] and `residual` [b-a, m, 4] as `rigid_series(with_scale=False)`
    wrote them, all three for exactly the frames [a, b) of `frame_range`; `source_cov` [m, 7] in cov's format where the source is
    itself measured (a frame of a table), None for an exact one (a layout).  Returns a dict of float64 device tensors with the keys
    of `want`: `ml` [b-a, 40] = flag (0 no start, 1 the start only, 2 the weighted fit), n_start, n_used, steps, w, x, y, z, R [9],
    t [3], c [3], qm [3], chi2, dof, chi2_start, step_rot, step_c, angle_deg, tilt_deg, azimuth_deg, twist_deg, nxx, nxy, nyy, t2_tilt,
    var_twist; `pcov` [b-a, 22] = flag, the 21 upper entries of the covariance of (omega, c); `coef` [b-a, 4, 4], the FIR record of
    `rigid_series` from the weighted pose; `mahal` [b-a, m, 3] = (1, distance^2 at the final pose, at the start), a record with
    n_values 2.  `rigid.pose_sigma`, `rigid.move_centre` and `rigid.consistent` read them."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    f64 = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()   # noqa: E731
    src, cv, rg, rs, sc = f64(source), f64(cov), f64(rigid), f64(residual), f64(source_cov)
    a, b, iters, want = _rigid_ml_args(n, m, src.shape, cv.shape, rg.shape, rs.shape, None if sc is None else sc.shape, iters, piv_rel,
                                       frame_range, want)
    shapes = {"ml": (b - a, L.RIGID_ML_COLS), "pcov": (b - a, L.RIGID_ML_PCOV_COLS), "coef": (b - a, 4, 4), "mahal": (b - a, m, 3)}
    out = {w: torch.empty(shapes[w], dtype=torch.float64, device=dev) for w in want}
    if a == b:
        return out
    _call("vbs_rigid_ml_series", "iters in [1, 16], piv_rel finite and >= 0, at least one output",
          dev, _ptr(t), n, m, _ptr(src), _ptr(cv), _ptr(rg), _ptr(rs), _ptr(sc), iters, float(piv_rel), a, b, _ptr(out.get("ml")),
          _ptr(out.get("pcov")), _ptr(out.get("coef")), _ptr(out.get("mahal")))
    return out


# ---- bonnet contact geometry along a recording (k_sphere.hip): the sphere, the contact set, its plane, the two records ----------------
_SPHERE_WANT = ("sphere", "radial", "decomp")


def _mask_idx(slots, m, name):
    if slots is None:
        return None
    idx = np.asarray(slots, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= m):
        raise ValueError(f"{name} outside the table's {m} slots")
    return idx


def _sphere_args(n, m, sphere, source_shape, fit_slots, slots, contact_depth, piv_rel, gap_rel, reject_k, frame_range, want=None):
    """`sphere_series`'s argument checks (no device needed): what `vbs_sphere_series` refuses, in the wrappers' words ->
    (a, b, sphere as float64 [4] or None, want) or ValueError.  `want` None: `sphere` and `radial`, and `decomp` with a source."""
    if n < 1 or m < 1:
        raise ValueError(_TABLE)
    a, b = _frame_range(frame_range, n)
    if not (np.isfinite(float(contact_depth)) and float(contact_depth) > 0.0):
        raise ValueError(f"contact_depth {contact_depth} must be finite and > 0")
    for name, v in (("piv_rel", piv_rel), ("gap_rel", gap_rel), ("reject_k", reject_k)):
        if not (np.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} {v} must be finite and >= 0")
    sph = None
    if sphere is not None:
        sph = np.ascontiguousarray(np.asarray(sphere, dtype=np.float64).reshape(-1))
        if sph.shape != (4,) or not np.isfinite(sph).all() or not sph[3] > 0.0:
            raise ValueError("sphere must be (Cx, Cy, Cz, R), finite, with R > 0")
    if source_shape is not None and tuple(source_shape) != (m, 4):
        raise ValueError(f"source must be [{m}, 4] = (flag, X, Y, Z): one row per table slot")
    _mask_idx(fit_slots, m, "fit_slots")
    _mask_idx(slots, m, "slots")
    if want is None:
        want = _SPHERE_WANT if source_shape is not None else _SPHERE_WANT[:2]
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in _SPHERE_WANT for w in want):
        raise ValueError(f"want must name at least one of {_SPHERE_WANT}")
    if "decomp" in want and source_shape is None:
        raise ValueError("decomp needs `source` [M, 4]: the positions the displacement is taken from")
    return a, b, sph, want


def sphere_series(table, sphere=None, fit_slots=None, slots=None, source=None, contact_depth=0.1, piv_rel=1e-9, gap_rel=1e-3,
                  reject_k=0.0, frame_range=None, want=None, device=None):
    """The bonnet's contact geometry of every frame (`vbs_sphere_series`): the sphere the markers lie on - fitted per
    frame over `fit_slots` when `sphere` is None, else `sphere` = (Cx, Cy, Cz, R) given and HELD (what a loaded recording needs: a
    per-frame fit over a pressed cap is wrong) -, the contact set (the `slots` that lie inside the sphere by more than
    `contact_depth`), the plane through those alone and from the two the contact normal, the offset, the spot radius and the spot
    centre.  table float32 [n, m, 10]; `source` float64 [m, 4] = (flag, X, Y, Z) as `rigid_series` takes it, needed for `decomp`
    only; `reject_k` > 0 asks for one round of rejection in the per-frame fit; a plane exists where three or more contact slots
    spread by more than `gap_rel` of their scatter's trace in two directions.  The defaults are this project's.  Returns a dict of
    float64 device tensors for the frames [a, b), with the keys of `want` (default: `sphere`, `radial`, and `decomp` with a source):
    `sphere` [b-a, 31] (the columns of `vbs_amd.sphere`), `radial` [b-a, m, 2] = (flag, rho), a record with n_values 1, `decomp`
    [b-a, m, 4] = (flag, d_n, d_mer, d_az), the displacement from `source` in the shell's own frame, a record with n_values 3."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    src = None if source is None else torch.as_tensor(source, dtype=torch.float64, device=dev).contiguous()
    a, b, sph, want = _sphere_args(n, m, sphere, None if src is None else src.shape, fit_slots, slots, contact_depth, piv_rel, gap_rel,
                                   reject_k, frame_range, want)
    shapes = {"sphere": (b - a, L.SPHERE_COLS), "radial": (b - a, m, 2), "decomp": (b - a, m, 4)}
    out = {w: torch.empty(shapes[w], dtype=torch.float64, device=dev) for w in want}
    if a == b:
        return out

    def mask_of(sl):
        if sl is None:
            return None
        mk = torch.zeros((m,), dtype=torch.uint8, device=dev)
        mk[torch.as_tensor(np.asarray(sl, dtype=np.int64).reshape(-1), device=dev)] = 1
        return mk
    fm, sm = mask_of(fit_slots), mask_of(slots)
    _call("vbs_sphere_series", "contact_depth > 0, piv_rel, gap_rel and reject_k finite and >= 0, a finite sphere with R > 0, decomp "
          "only with a source, at least one output",
          dev, _ptr(t), n, m, _host_ptr(sph) if sph is not None else C.c_void_p(0), _ptr(fm), _ptr(sm), _ptr(src),
          float(contact_depth), float(piv_rel), float(gap_rel), float(reject_k), a, b, _ptr(out.get("sphere")), _ptr(out.get("radial")),
          _ptr(out.get("decomp")))
    return out


def pixel_noise(table, frame_range=None, device=None):
    """The scatter of the observation over a still segment (`vbs_pixel_noise`): table float32 [n, m, 10] -> float64 [m, 10] = count,
    mean Cx, Cy, major, then uu, uv, ud, vv, vd, dd, the sample covariance (ddof 1) over the tracked rows of the frames [a, b) of
    `frame_range` - columns 4 .. 9 are an `obs_cov` per slot for `solve3d_cov`.  count 0: zeros; count 1: the means and zeros."""
    dev = _device(device)
    t = _f32_table(table, dev)
    n, m, _ = t.shape
    a, b = _frame_range(frame_range, n)
    out = torch.empty((m, L.NOISE_COLS), dtype=torch.float64, device=dev)
    _call("vbs_pixel_noise", "0 <= frame_begin <= frame_end <= n", dev, _ptr(t), n, m, a, b, _ptr(out))
    return out
