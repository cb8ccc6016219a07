"""CPU restatement (pandas / NumPy, float64) of the reference's analysis layer on the package's dense tensors - what the
GPU tests of the time-axis kernels compare against.  `tests/test_analysis_host.py` pins it to `tests/golden/analysis.npz`,
which `tests/golden/make_analysis_golden.py` made by running the reference's own statements:

  series_stats         MarkerAnalysis.analyze_displacement, 3d_reconstruction.py:332-334 (cumulative) and :397-400 (statistics)
  window_means         LocalAnalysis.calculate_average_coordinates, LocalAnalysis.py:53-60
  window_displacement  LocalAnalysis.py:81-93 (inner merge, difference vectors, norms) and the mean norm of :94
  disp_from_frame      MarkerDisplacement.py:161-173 (SCALAR mode)

Inputs are the float32 tensors promoted to float64; every function goes through the DataFrame the reference would hold
(one row per flagged entry) and returns dense arrays with NaN where the reference has no row / no group.

The tolerances the tests use are derived, not tuned (u = 2^-53; any order of summing n float64 terms errs by at most
(n - 1) u sum|x| to first order, device and oracle each use some order):
  count, max, flags                        exact
  total, cumulative entries, window sums   |dev - ref| <= n 2^-52 sum|x|        (n, sum|x| over the terms of that value)
  means                                    that bound / count + 2^-52 |mean|     (the division)
  std                                      relative n kappa 2^-52, kappa = sqrt(1 + mean^2 / var_pop): the condition number
                                           of the variance (Chan, Golub & LeVeque 1983: updating and pairwise algorithms are
                                           bounded by n kappa u on the variance; the root halves it, two sides double it)
  distances, difference vectors, norms     1e-12 relative (the project's tolerance for float64 point interfaces)
"""
import numpy as np
import pandas as pd

FLAG_XYZ = 2
EPS = 2.0 ** -52
REL_POINT = 1e-12


def disp_rows(disp, ids=None):
    """The reference's `results_df` (the columns the analysis uses) from disp [n, m, 5]: one row per flagged entry."""
    d = np.asarray(disp, dtype=np.float64)
    f, s = np.nonzero(d[..., 0] != 0)
    if ids is None:
        ids = np.stack([np.arange(d.shape[1]), np.zeros(d.shape[1], dtype=np.int64)], axis=1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    return pd.DataFrame({"frameno": f.astype(np.int64), "row": ids[s, 0], "col": ids[s, 1], "slot": s.astype(np.int64),
                         "displacement": d[f, s, 4]})


def series_stats(disp, ids=None):
    """(stats [m, 5] = count, mean, std (ddof 1), max, last cumulative value; cumulative [n, m] with the value carried over
    the entries that are no rows, 0 before the first; rows [n, m] bool = which entries are rows)."""
    d = np.asarray(disp, dtype=np.float64)
    n, m = d.shape[:2]
    df = disp_rows(d, ids)
    stats = np.full((m, 5), np.nan)
    stats[:, 0] = 0
    cum = np.zeros((n, m))
    rows = d[..., 0] != 0
    if len(df):
        df = df.sort_values(["row", "col", "frameno"])
        df["cumulative_displacement"] = df.groupby(["row", "col"])["displacement"].cumsum()
        g = df.groupby("slot").agg({"displacement": ["count", "mean", "std", "max"], "cumulative_displacement": "last"})
        stats[g.index.to_numpy()] = g.to_numpy(dtype=np.float64)
        dense = np.full((n, m), np.nan)
        dense[df["frameno"].to_numpy(), df["slot"].to_numpy()] = df["cumulative_displacement"].to_numpy()
        cum = pd.DataFrame(dense).ffill().fillna(0.0).to_numpy()
    return stats, cum, rows


def marker_rows(table, marker_id=None, frame_offset=0):
    """The L4 sheet `frameno, marker_id, Xw, Yw, Zw` from table [n, m, 10]: one row per entry with a 3-D point."""
    t = np.asarray(table, dtype=np.float64)
    f, s = np.nonzero((t[..., 0].astype(np.int64) & FLAG_XYZ) != 0)
    mid = np.arange(t.shape[1]) if marker_id is None else np.asarray(marker_id)
    return pd.DataFrame({"frameno": f + frame_offset, "marker_id": mid[s], "slot": s, "Xw": t[f, s, 6], "Yw": t[f, s, 7],
                         "Zw": t[f, s, 8]})


def window_means(table, windows):
    """[W, m, 4] = count, mean X, Y, Z per slot over the inclusive frame windows (NaN means where the slot has no row)."""
    t = np.asarray(table, dtype=np.float64)
    df = marker_rows(t)
    out = np.full((len(windows), t.shape[1], 4), np.nan)
    out[:, :, 0] = 0
    for w, (a, b) in enumerate(windows):
        sub = df[(df["frameno"] >= a) & (df["frameno"] <= b)]
        if len(sub):
            g = sub.groupby("slot")[["Xw", "Yw", "Zw"]]
            avg, cnt = g.mean(), g.size()
            out[w, avg.index.to_numpy(), 1:] = avg.to_numpy()
            out[w, cnt.index.to_numpy(), 0] = cnt.to_numpy()
    return out


def window_sums_abs(table, windows):
    """[W, m, 3]: sum |X|, |Y|, |Z| over the rows of each window (what the bound on a window mean is made of)."""
    t = np.asarray(table, dtype=np.float64)
    ok = (t[..., 0].astype(np.int64) & FLAG_XYZ) != 0
    out = np.zeros((len(windows), t.shape[1], 3))
    for w, (a, b) in enumerate(windows):
        out[w] = (np.abs(t[a:b + 1, :, 6:9]) * ok[a:b + 1, :, None]).sum(axis=0)
    return out


def window_displacement(table, start, end, slots=None):
    """dict(slots [K], start_xyz, end_xyz [K, 3], d [K, 4] = dX, dY, dZ, |d|, mean): the inner join of the two windows."""
    wm = window_means(table, [start, end])
    common = (wm[0, :, 0] > 0) & (wm[1, :, 0] > 0)
    if slots is not None:
        pick = np.zeros_like(common)
        pick[np.asarray(slots, dtype=np.int64)] = True
        common &= pick
    idx = np.nonzero(common)[0]
    d = wm[1, idx, 1:] - wm[0, idx, 1:]
    mag = np.linalg.norm(d, axis=1)
    return {"slots": idx, "start_xyz": wm[0, idx, 1:], "end_xyz": wm[1, idx, 1:], "d": np.concatenate([d, mag[:, None]], axis=1),
            "mean": np.mean(mag) if len(idx) else np.nan}


def disp_from_frame(table, ref_frame=0):
    """[n, m, 2] = (flag, distance from the slot's position in frame `ref_frame`); flag = both rows hold a 3-D point."""
    t = np.asarray(table, dtype=np.float64)
    ok = (t[..., 0].astype(np.int64) & FLAG_XYZ) != 0
    flag = ok & ok[ref_frame][None, :]
    r = t[ref_frame]
    dist = np.sqrt((t[..., 6] - r[None, :, 6]) ** 2 + (t[..., 7] - r[None, :, 7]) ** 2 + (t[..., 8] - r[None, :, 8]) ** 2)
    return np.stack([flag.astype(np.float64), np.where(flag, dist, 0.0)], axis=2)


# ---- the bounds ---------------------------------------------------------------------------------------------------------
def check_stats(got_stats, want, disp, what=""):
    """Two statistics tables [m, 5] of the same disp (`want` = the reference side) against each other, to the derived bounds."""
    d = np.asarray(disp, dtype=np.float64)
    rows = d[..., 0] != 0
    got_stats, want = np.asarray(got_stats), np.asarray(want)
    sabs = np.where(rows, np.abs(d[..., 4]), 0.0).sum(axis=0)
    n = want[:, 0]
    assert np.array_equal(n, rows.sum(axis=0)), f"{what}: the reference side's counts are not the flags'"
    assert np.array_equal(got_stats[:, 0], n), f"{what}: counts differ"
    assert np.array_equal(np.isnan(got_stats), np.isnan(want)), f"{what}: NaN pattern differs"
    assert np.array_equal(got_stats[:, 3], want[:, 3], equal_nan=True), f"{what}: max differs"
    has = n > 0
    if not has.any():
        return
    tot_bound = n * EPS * sabs
    err = np.abs(got_stats[has, 4] - want[has, 4])
    assert (err <= tot_bound[has]).all(), f"{what}: total off by {err.max()} (bound {tot_bound[has][err.argmax()]})"
    mean_bound = tot_bound[has] / n[has] + EPS * np.abs(want[has, 1])
    err = np.abs(got_stats[has, 1] - want[has, 1])
    assert (err <= mean_bound).all(), f"{what}: mean off by {(err / mean_bound).max()} of its bound"
    two = n > 1
    if two.any():
        var_pop = want[two, 2] ** 2 * (n[two] - 1) / n[two]
        with np.errstate(divide="ignore"):
            kappa = np.sqrt(1.0 + want[two, 1] ** 2 / var_pop)
        rel = np.abs(got_stats[two, 2] - want[two, 2]) / np.where(want[two, 2] > 0, want[two, 2], 1.0)
        bound = n[two] * kappa * EPS
        fin = np.isfinite(kappa)                      # var 0 (all values equal): both sides must give exactly 0
        assert (rel[fin] <= bound[fin]).all(), f"{what}: std off by {(rel[fin] / bound[fin]).max()} of its bound"
        assert (got_stats[two, 2][~fin] == 0).all(), f"{what}: std of a constant series is not 0"


def check_series(got_stats, got_cum, disp, ids=None, what=""):
    """Device (or any other) statistics / cumulative series against this oracle on the same disp, to the derived bounds."""
    d = np.asarray(disp, dtype=np.float64)
    want, wcum, rows = series_stats(d, ids)
    check_stats(got_stats, want, d, what)
    if got_cum is not None:
        got_cum, got_stats = np.asarray(got_cum), np.asarray(got_stats)
        x = np.where(rows, np.abs(d[..., 4]), 0.0)
        bound = np.cumsum(rows, axis=0) * EPS * np.cumsum(x, axis=0)
        err = np.abs(got_cum - wcum)
        assert (err <= bound).all(), f"{what}: cumulative series off by {err.max()}"
        last = np.where(want[:, 0] > 0, got_cum[-1], np.nan)
        assert np.array_equal(last, got_stats[:, 4], equal_nan=True), f"{what}: total is not the last cumulative value"


def stats_from_frame(df, ids, counts):
    """The reference's statistics frame (index (row, col), columns displacement mean / std / max, cumulative_displacement
    last) -> the dense [m, 5] layout, NaN rows for the slots it does not hold; `counts` [m] fills column 0."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    slot = {tuple(k): i for i, k in enumerate(ids.tolist())}
    out = np.full((len(ids), 5), np.nan)
    out[:, 0] = 0
    vals = df.to_numpy(dtype=np.float64)
    for key, v in zip(df.index.tolist(), vals):
        i = slot[(int(key[0]), int(key[1]))]
        out[i, 0] = counts[i]
        out[i, 1:] = v
    return out


def check_window_means(got, table, windows, what=""):
    t = np.asarray(table, dtype=np.float64)
    want = window_means(t, windows)
    sabs = window_sums_abs(t, windows)
    got = np.asarray(got)
    assert np.array_equal(got[..., 0], want[..., 0]), f"{what}: window counts differ"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    n = want[..., 0:1]
    has = (n > 0)[..., 0]
    bound = (n * EPS * sabs)[has] / n[has] + EPS * np.abs(want[..., 1:][has])
    err = np.abs(got[..., 1:][has] - want[..., 1:][has])
    assert (err <= bound).all(), f"{what}: window mean off by {(err / np.maximum(bound, 1e-300)).max()} of its bound"


def check_disp_from_frame(got, table, ref_frame, what=""):
    want = disp_from_frame(table, ref_frame)
    got = np.asarray(got)
    assert np.array_equal(got[..., 0], want[..., 0]), f"{what}: flags differ"
    assert (np.abs(got[..., 1] - want[..., 1]) <= REL_POINT * np.abs(want[..., 1])).all(), f"{what}: distances differ"
