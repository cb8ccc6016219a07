"""Host helpers of the modal analysis (NumPy only): what the eigenvalues explain, the modes as a record the field
entries take, and the slots that move with nobody."""
from __future__ import annotations

import numpy as np


def explained(values, cov):
    """The share of the trace of `cov` [C, C] every eigenvalue of `values` [r] carries, and the running sum of the shares:
    -> (share [r], cumulative [r]).  NaN where the trace is not positive.  Of an indefinite matrix (the pairwise estimator) a share
    may be negative and the shares of all C values still sum to one."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("cov must be [C, C]")
    tr = float(np.trace(cov))
    share = values / tr if tr > 0.0 else np.full(values.shape, np.nan)
    return share, np.cumsum(share)


def mode_record(modes, s, n_values, valid=None):
    """The modes [r, s n_values] as a record float64 [r, s, 1 + n_values] = flag, the mode's entries of the slot: what
    `field_map_f64` and `patch_stats_f64` take, one "frame" a mode - a map of every mode on the grid and where it is centred.  The
    flag is 1, or `valid` [s] (nonzero = the slot takes part)."""
    s, nv = int(s), int(n_values)
    modes = np.asarray(modes, dtype=np.float64)
    if modes.ndim != 2 or modes.shape[1] != s * nv or nv < 1:
        raise ValueError(f"modes must be [r, {s * nv}]")
    rec = np.empty((modes.shape[0], s, 1 + nv))
    flag = np.ones(s) if valid is None else (np.asarray(valid).reshape(-1) != 0).astype(np.float64)
    if flag.shape != (s,):
        raise ValueError(f"valid must be [{s}]")
    rec[..., 0] = flag
    rec[..., 1:] = modes.reshape(modes.shape[0], s, nv)
    return rec


def loner_slots(cov, modes, values, n_values=3):
    """The share of every slot's variance that lies OUTSIDE the leading subspace: 1 - sum_k lambda_k |u_k[slot]|^2 / var[slot],
    var the sum of the slot's diagonal entries of `cov`; NaN where var is not positive.  A marker whose series correlates with
    nobody keeps its variance to itself and comes out near one: the spatial counterpart of a spike.  -> (share [s], the slots in
    descending order of share, NaN last)."""
    cov = np.asarray(cov, dtype=np.float64)
    modes = np.asarray(modes, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    nv = int(n_values)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] % nv or modes.shape != (values.size, cov.shape[0]):
        raise ValueError("cov must be [C, C], modes [r, C], values [r], C a multiple of n_values")
    s = cov.shape[0] // nv
    var = np.diag(cov).reshape(s, nv).sum(axis=1)
    inside = (values[:, None, None] * modes.reshape(-1, s, nv) ** 2).sum(axis=(0, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(var > 0.0, 1.0 - inside / var, np.nan)
    order = np.argsort(-np.nan_to_num(share, nan=-np.inf), kind="stable")
    return share, order
