"""Grey-level refinement of tracked markers (`vbs_refine_markers`, csrc/k_refine.hip): the pieces that need no device.  The rule
itself - levels, weights, sums, the float64 tail - is stated in include/vbs.h; `Engine.refine_markers` runs it,
`pipeline.refine_table` wraps it."""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L

DEFAULTS = {"core_f": 0.5, "disc_f": 1.5, "ring_f": 2.0, "min_contrast": 16.0, "max_shift_f": 1.0, "polarity": 0,
            "keep_unrefined": 0}
MAX_PASSES = 8                      # `passes` of `Engine.refine_markers`: a host-side repetition, no parameter of the entry
STATUS_NAMES = {0: "refined", L.REFINE_NOT_TRACKED: "not_tracked", L.REFINE_BAD_ROW: "bad_row", L.REFINE_TOO_LARGE: "too_large",
                L.REFINE_AT_BORDER: "at_border", L.REFINE_LOW_CONTRAST: "low_contrast", L.REFINE_DEGENERATE: "degenerate",
                L.REFINE_MOVED: "moved"}
REC_COLUMNS = ("status", "cx", "cy", "major", "minor", "angle", "d_area", "area", "background", "dark", "edge_var", "shift")
SUM_COLUMNS = ("B8", "D8", "S0", "Sx", "Sy", "Sxx", "Sxy", "Syy")


def params(config=True, **overrides):
    """The `"refine"` key of a tracker's config, or keyword arguments -> None (absent, None, False: no refinement) or the checked
    parameters: `True` is the defaults, a dict overrides some of them.  ValueError for what `vbs_refine_markers` refuses.  The
    key `passes` (1 .. MAX_PASSES, default 1; see `Engine.refine_markers`) is kept only where it was given."""
    if config is None or config is False:
        return None
    if config is True:
        config = {}
    if not isinstance(config, dict):
        raise ValueError("config['refine'] must be True, False, None or a dict of " + ", ".join(DEFAULTS))
    p = {**config, **overrides}
    passes = p.pop("passes", None)
    if passes is not None and (not isinstance(passes, int) or isinstance(passes, bool) or not 1 <= passes <= MAX_PASSES):
        raise ValueError(f"refine: passes is an integer in 1 .. {MAX_PASSES}")
    unknown = sorted(set(p) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"refine: unknown keys {unknown} (known: {', '.join(DEFAULTS)})")
    p = {**DEFAULTS, **p}
    for k in ("core_f", "disc_f", "ring_f", "min_contrast", "max_shift_f"):
        p[k] = float(p[k])
        if not math.isfinite(p[k]):
            raise ValueError(f"refine: {k} must be finite")
    if not 0.0 < p["core_f"] <= p["disc_f"] <= p["ring_f"] <= 64.0:
        raise ValueError("refine: 0 < core_f <= disc_f <= ring_f <= 64")
    if not 0.125 <= p["min_contrast"] <= 255.0:
        raise ValueError("refine: min_contrast in [0.125, 255] levels")
    if p["max_shift_f"] < 0.0:
        raise ValueError("refine: max_shift_f >= 0")
    for k in ("polarity", "keep_unrefined"):
        if p[k] not in (0, 1, False, True):
            raise ValueError(f"refine: {k} is 0 or 1")
        p[k] = int(p[k])
    if passes is not None:
        p["passes"] = passes
    return p


def window(major, ring_f=2.0, core_f=0.5, disc_f=1.5):
    """The geometry of a row of diameter `major` (read as float32, as the kernel reads it): dict of R (the window is 2 R + 1 a
    side), c2, g2, R2, the pixel counts of core, disc and ring, and `fits` = R <= VBS_REFINE_MAX_R."""
    r = 0.5 * float(np.float32(major))
    R = int(math.ceil(ring_f * r)) + 1
    c2, g2 = int(math.floor((core_f * r) * (core_f * r))), int(math.floor((disc_f * r) * (disc_f * r)))
    d = np.arange(-R, R + 1, dtype=np.int64)
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    return {"R": R, "c2": c2, "g2": g2, "R2": R * R, "core": int((d2 <= c2).sum()), "disc": int((d2 <= g2).sum()),
            "ring": int(((d2 > g2) & (d2 <= R * R)).sum()), "fits": R <= L.REFINE_MAX_R}


def max_major(ring_f=2.0):
    """The largest diameter whose window fits: ceil(ring_f major / 2) + 1 <= VBS_REFINE_MAX_R."""
    return 2.0 * (L.REFINE_MAX_R - 1) / float(ring_f)


def report(rec, table_in, disc_f=DEFAULTS["disc_f"]):
    """What a refinement did, from `rec` [n, m, VBS_REFINE_COLS] and the table it started from (arrays or tensors):
    `status_per_frame` int64 [n, 8] and `status_per_slot` int64 [m, 8] - the count of every status 0 .. 7; per slot, over its
    refined rows, `dmajor_mean`, `dmajor_std` (major' - major) and `shift_mean`, `shift_std` (NaN where a slot has none; std with
    ddof 0); `never_refined`, the slots without a refined row; `edge_var_median` over all refined rows (NaN without any);
    `uncovered` bool [n, m] and `uncovered_per_slot` int64 [m]: refined rows whose disc - `disc_f` x the START's radius - does not
    reach a pixel beyond the refined radius, major' / 2 + 1 > disc_f major / 2.  Such a row has status 0 and is still short: the
    area was cut off by the disc (a binary diameter far too small, as at low contrast).  Refine again with `passes` > 1."""
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)     # noqa: E731
    rec, tab = host(rec), host(table_in)
    if rec.ndim != 3 or rec.shape[2] != L.REFINE_COLS or tab.shape[:2] != rec.shape[:2] or tab.shape[2] != L.TABLE_COLS:
        raise ValueError(f"rec must be [n, m, {L.REFINE_COLS}] and the table [n, m, {L.TABLE_COLS}]")
    n, m = rec.shape[:2]
    status = rec[..., 0].astype(np.int64)
    per_frame = np.stack([(status == s).sum(axis=1) for s in range(8)], axis=1).astype(np.int64).reshape(n, 8)
    per_slot = np.stack([(status == s).sum(axis=0) for s in range(8)], axis=1).astype(np.int64).reshape(m, 8)
    ok = status == 0
    cnt = ok.sum(axis=0)
    dmaj = np.where(ok, rec[..., 3] - tab[..., 3].astype(np.float64), 0.0)
    shift = np.where(ok, rec[..., 11], 0.0)

    def mean_std(x):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = x.sum(axis=0) / cnt
            var = np.where(ok, (x - mean) ** 2, 0.0).sum(axis=0) / cnt
        return mean, np.sqrt(var)

    uncovered = ok & (0.5 * rec[..., 3] + 1.0 > float(disc_f) * 0.5 * tab[..., 3].astype(np.float64))
    dm, ds = mean_std(dmaj)
    sm, ss = mean_std(shift)
    return {"status_per_frame": per_frame, "status_per_slot": per_slot, "dmajor_mean": dm, "dmajor_std": ds, "shift_mean": sm,
            "shift_std": ss, "never_refined": np.flatnonzero(cnt == 0), "uncovered": uncovered,
            "uncovered_per_slot": uncovered.sum(axis=0).astype(np.int64),
            "edge_var_median": float(np.median(rec[..., 10][ok])) if ok.any() else float("nan"), "status_names": dict(STATUS_NAMES)}
