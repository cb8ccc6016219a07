"""NumPy/Python restatement of the despiking entry (`include/vbs.h`: vbs_hampel_series_f64), which the device is held to BIT FOR
BIT.  An order statistic has no order of summation, so the restatement is the definition itself and shares no algorithm with the
kernel: per (frame, series, value) the window's candidates are put in (x, g) order by Python's `sorted` on pairs, the median is
read at its rank (two products and one add for an even count - Python floats are IEEE doubles and nothing contracts them), the
MAD is the same statistic of |x_g - med|, and the spike test is the stated comparisons with thr = k_sigma * 1.4826."""
import numpy as np


def _middle(q):
    """q sorted, len >= 1 -> the statistic of the interface."""
    c = len(q)
    if c & 1:
        return q[(c - 1) // 2]
    return 0.5 * q[c // 2 - 1] + 0.5 * q[c // 2]


def hampel(rec, n_values, half_window, k_sigma=3.0, min_scale=0.0, min_count=None, frame_range=None):
    """-> (out [b-a, s, 2 + 2 nv], clean [b-a, s, cols]) exactly as vbs_hampel_series_f64 states them."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    n, s, cols = rec.shape
    nv, h = int(n_values), int(half_window)
    mc = h + 1 if min_count is None else int(min_count)
    a, b = (0, n) if frame_range is None else frame_range
    thr = float(k_sigma) * 1.4826
    floor = float(min_scale)
    valid = rec[..., 0] != 0
    out = np.zeros((b - a, s, 2 + 2 * nv))
    clean = rec[a:b].copy()
    for i in range(s):
        x = rec[:, i, 1:1 + nv].tolist()
        ok = valid[:, i].tolist()
        for f in range(a, b):
            gs = [g for g in range(max(0, f - h), min(n, f + h + 1)) if ok[g]]
            c = len(gs)
            judged = c >= mc
            spike = False
            o = out[f - a, i]
            o[1] = c
            if judged:
                for v in range(nv):
                    q = [p[0] for p in sorted((x[g][v], g) for g in gs)]
                    med = _middle(q)
                    mad = _middle(sorted(abs(x[g][v] - med) for g in gs))
                    o[2 + v], o[2 + nv + v] = med, mad
                    if ok[f]:
                        dev = abs(x[f][v] - med)
                        spike = spike or (dev > thr * mad and dev > floor)
            o[0] = (1.0 if ok[f] else 0.0) + (2.0 if judged else 0.0) + (4.0 if spike else 0.0)
            if spike:
                clean[f - a, i, 0] = 0.0
    return out, clean


def hampel_np(rec, n_values, half_window, k_sigma=3.0, min_scale=0.0, min_count=None, frame_range=None):
    """The same definition for every entry at once, for the sweeps the loops above are too slow for.  The windows are laid out
    in g order (NaN where a frame is invalid or outside [0, n)) and sorted by NumPy's STABLE sort, which compares with `<` and
    puts NaN last: equal values, -0.0 and +0.0 among them, stay in g order, which is the (x, g) order; the ranks are read from
    the first c places.  `tests/test_robust_host.py` holds it to `hampel` bit for bit on gaps, ties and both zeros, and `check`
    below evaluates both."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    n, s, cols = rec.shape
    nv, h = int(n_values), int(half_window)
    mc = h + 1 if min_count is None else int(min_count)
    a, b = (0, n) if frame_range is None else frame_range
    thr = float(k_sigma) * 1.4826
    valid = rec[..., 0] != 0
    x = np.where(valid[..., None], rec[..., 1:1 + nv], np.nan)
    pad = np.full((h, s, nv), np.nan)
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, x, pad]), 2 * h + 1, axis=0)[a:b]     # [b-a, s, nv, W]
    vp = np.concatenate([np.zeros((h, s), bool), valid, np.zeros((h, s), bool)])
    c = np.lib.stride_tricks.sliding_window_view(vp, 2 * h + 1, axis=0)[a:b].sum(axis=-1)                       # [b-a, s]
    judged = c >= mc
    lo, hi = np.maximum(c - 1, 0) // 2, c // 2
    lo, hi = lo[..., None, None], np.minimum(hi, 2 * h)[..., None, None]
    odd = (c & 1).astype(bool)[..., None]

    def middle(w):
        q = np.sort(w, axis=-1, kind="stable")
        ql = np.take_along_axis(q, np.broadcast_to(lo, q.shape[:-1] + (1,)), axis=-1)[..., 0]
        qh = np.take_along_axis(q, np.broadcast_to(hi, q.shape[:-1] + (1,)), axis=-1)[..., 0]
        return np.where(odd, ql, 0.5 * ql + 0.5 * qh)
    with np.errstate(all="ignore"):
        med = middle(win)
        mad = middle(np.abs(win - med[..., None]))
        dev = np.abs(x[a:b] - med)
        spike = ((dev > thr * mad) & (dev > float(min_scale))).any(axis=-1) & valid[a:b] & judged
    med = np.where(judged[..., None], med, 0.0)
    mad = np.where(judged[..., None], mad, 0.0)
    flag = valid[a:b] + 2.0 * judged + 4.0 * spike
    out = np.concatenate([flag[..., None], c.astype(np.float64)[..., None], med, mad], axis=2)
    clean = rec[a:b].copy()
    clean[..., 0] = np.where(spike, 0.0, clean[..., 0])
    return out, clean


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


LOOP_ENTRIES = 4000      # `check` runs the loops of `hampel` on all series up to this many (frame, series, value) entries


def check(got_out, got_clean, rec, n_values, half_window, k_sigma=3.0, min_scale=0.0, min_count=None, frame_range=None, what=""):
    """The device's (out, clean) against the restatement, EVERY entry, on uint64 views.  The restatement is `hampel_np`; the loops
    of `hampel` are evaluated beside it on all series where the shape is small and otherwise on the first, the middle (where the
    tests put the long gap) and the last series (the dead one), and must give the same bits.  Returns the restatement's pair."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    want_out, want_clean = hampel_np(rec, n_values, half_window, k_sigma, min_scale, min_count, frame_range)
    n, s, _ = rec.shape
    pick = list(range(s)) if want_out.shape[0] * s * int(n_values) <= LOOP_ENTRIES else sorted({0, s // 2, s - 1})
    loop_out, loop_clean = hampel(rec[:, pick], n_values, half_window, k_sigma, min_scale, min_count, frame_range)
    assert np.array_equal(bits(loop_out), bits(want_out[:, pick])) and np.array_equal(bits(loop_clean), bits(want_clean[:, pick])), \
        f"{what}: the two restatements disagree"
    got_out = np.asarray(got_out)
    assert got_out.shape == want_out.shape and got_out.dtype == np.float64, (what, got_out.shape, want_out.shape)
    diff = bits(got_out) != bits(want_out)
    assert not diff.any(), f"{what}: {int(diff.sum())} entries of out differ in bits from the restatement, first at " \
                           f"{tuple(np.argwhere(diff)[0])}: {got_out[tuple(np.argwhere(diff)[0])]!r} for " \
                           f"{want_out[tuple(np.argwhere(diff)[0])]!r}"
    if got_clean is not None:
        got_clean = np.asarray(got_clean)
        assert got_clean.shape == want_clean.shape and got_clean.dtype == np.float64, (what, got_clean.shape)
        assert np.array_equal(bits(got_clean), bits(want_clean)), f"{what}: clean differs in bits from the restatement"
    return want_out, want_clean


def table_record(table, source="xyz", slots=None):
    """The record `pipeline.despike_table` builds from a table [N, M, 10], restated in NumPy."""
    t = np.asarray(table)
    bit, cols = (2, (6, 7, 8)) if source == "xyz" else (1, (1, 2))
    valid = (t[..., 0].astype(np.int64) & bit) != 0
    if slots is not None:
        pick = np.zeros(t.shape[1], dtype=bool)
        pick[np.asarray(slots, dtype=np.int64)] = True
        valid &= pick[None, :]
    return np.concatenate([valid.astype(np.float64)[..., None], t[..., list(cols)].astype(np.float64)], axis=2)
