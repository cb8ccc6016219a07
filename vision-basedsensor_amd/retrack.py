"""Re-tracking a recording along time (`vbs_retrack`, csrc/k_retrack.hip): the pieces that need no device.  The rule itself -
prediction, gate, one-to-one match - is stated in include/vbs.h; `engine.retrack` runs it, `pipeline.retrack_table` wraps it."""
from __future__ import annotations

import numpy as np

from . import _lib as L

DEFAULTS = {"gate": 10.0, "max_travel": float("inf"), "vel_gain": 0.5, "max_coast": 5}
OUTPUTS = ("assign", "table", "dist2", "info")


def initial_state(ref_xy):
    """The state before the first frame, float64 [m, VBS_RETRACK_STATE_COLS] = px, py, vx, vy, age, seen: every slot at its
    reference position, at rest, never seen.  A tensor gives a tensor on its device, anything else a NumPy array."""
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None and isinstance(ref_xy, torch.Tensor):
        ref = ref_xy.to(torch.float64).reshape(-1, 2)
        st = torch.zeros((ref.shape[0], L.RETRACK_STATE_COLS), dtype=torch.float64, device=ref.device)
        st[:, 0:2] = ref
        return st
    ref = np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    st = np.zeros((ref.shape[0], L.RETRACK_STATE_COLS), dtype=np.float64)
    st[:, 0:2] = ref
    return st


def params(config):
    """The `"retrack"` key of a tracker's config -> None (absent, None, False: the per-frame rule) or the parameters: `True`
    is the defaults, a dict overrides some of them."""
    if config is None or config is False:
        return None
    if config is True:
        return dict(DEFAULTS)
    if not isinstance(config, dict):
        raise ValueError("config['retrack'] must be True, False, None or a dict of " + ", ".join(DEFAULTS))
    unknown = sorted(set(config) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"config['retrack']: unknown keys {unknown} (known: {', '.join(DEFAULTS)})")
    return {**DEFAULTS, **config}


def compare_tables(a, b):
    """What two tables [n, m, VBS_TABLE_COLS] of the same detections say, per frame: `same` - the rows both have with one
    det_index, `only_a` / `only_b` - the rows one of them has alone, `differ` - the rows both have with different det_index.
    -> dict of int64 [n] arrays, and `total` with the four sums."""
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)     # noqa: E731
    a, b = host(a), host(b)
    if a.ndim != 3 or a.shape[2] != L.TABLE_COLS or a.shape != b.shape:
        raise ValueError(f"both tables must be [n, m, {L.TABLE_COLS}] of one shape")
    ta = (a[..., 0].astype(np.int64) & L.FLAG_TRACKED) != 0
    tb = (b[..., 0].astype(np.int64) & L.FLAG_TRACKED) != 0
    eq = a[..., 9] == b[..., 9]
    out = {"same": (ta & tb & eq).sum(axis=1), "only_a": (ta & ~tb).sum(axis=1), "only_b": (~ta & tb).sum(axis=1),
           "differ": (ta & tb & ~eq).sum(axis=1)}
    out = {k: v.astype(np.int64) for k, v in out.items()}
    out["total"] = {k: int(v.sum()) for k, v in out.items()}
    return out
