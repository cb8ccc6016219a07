"""NumPy restatement of the probe-indentation analysis (`include/vbs.h`: vbs_step_response_f64, vbs_find_steps_f64,
vbs_dwell_stats_f64), the synthetic Figure-6(b) signal, and the bounds the restatement itself is held to.

The restatement is the SAME IEEE operations in the SAME order as the device: every window sum starts at 0.0 and adds its valid
frames in ascending order (vectorised over frames and series only: an output's own order stays), the dwell sums are the 64 lane
sums folded a[i] + a[i + 32], then 16, 8, 4, 2, 1; select, never multiply by zero; NumPy's ufuncs do not contract a product into
a sum.  So the device is held to it BIT FOR BIT (`same`: NaN where NaN, the same bits elsewhere).  The peak search only
compares, so it has no order to state.  The independent sides use another order; their bounds are those of the summation error,
with 2^-52 = 2 u so that both sides' own rounding fits:
    response, gap-free interior:   |r - ref| <= 2 (w 2^-52 sum|x| / w) + 2 2^-52 |ref|    (two means of w values, one difference)
    dwell mean over c frames:      |mean - fsum / c| <= c 2^-52 sum|x| / c + 2^-52 |fsum / c|
None of them comes from what the device gives."""
import json
import math
import os

import numpy as np

U2 = 2.0 ** -52
MAX_WINDOW, MAX_STEPS = 64, 64


def same(a, b):
    """NaN exactly where NaN, the same bits everywhere else."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def response(rec, window, n_values=None, min_count=None):
    """-> out [n, s, 2 + nv] exactly as vbs_step_response_f64 states it."""
    rec = np.asarray(rec, dtype=np.float64)
    n, s, cols = rec.shape
    nv = cols - 1 if n_values is None else int(n_values)
    w = int(window)
    mc = (w + 1) // 2 if min_count is None else int(min_count)
    valid = rec[..., 0] != 0
    x = rec[..., 1:1 + nv]
    sl, sr = np.zeros((n, s, nv)), np.zeros((n, s, nv))
    cl, cr = np.zeros((n, s), dtype=np.int64), np.zeros((n, s), dtype=np.int64)
    with np.errstate(all="ignore"):
        for d in range(-w, w):                               # g = f + d: ascending g for every f at once
            lo, hi = max(0, -d), min(n, n - d)
            if hi <= lo:
                continue
            v = valid[lo + d:hi + d]
            acc, cnt = (sl, cl) if d < 0 else (sr, cr)
            acc[lo:hi] = np.where(v[..., None], acc[lo:hi] + x[lo + d:hi + d], acc[lo:hi])
            cnt[lo:hi] += v
        ok = (cl >= mc) & (cr >= mc)
        r = sr / cr[..., None].astype(np.float64) - sl / cl[..., None].astype(np.float64)
        r = np.where(ok[..., None], r, 0.0)
        score = np.zeros((n, s))
        for c in range(nv):
            score = score + r[..., c] * r[..., c]
    return np.concatenate([ok.astype(np.float64)[..., None], score[..., None], r], axis=2)


def find_steps(resp, window, thr2, max_steps=MAX_STEPS):
    """-> steps int32 [s, 1 + max_steps] exactly as vbs_find_steps_f64 states it (thr2: the squared threshold)."""
    resp = np.asarray(resp, dtype=np.float64)
    n, s, _ = resp.shape
    w = int(window)
    ok = resp[..., 0] != 0
    with np.errstate(invalid="ignore"):
        score = np.where(ok, resp[..., 1], np.nan)           # a row that is not ok compares false on both sides, as NaN does
        step = score >= thr2
        for d in range(-w, w + 1):
            lo, hi = max(0, -d), min(n, n - d)
            if d == 0 or hi <= lo:
                continue
            other, mine = score[lo + d:hi + d], score[lo:hi]
            step[lo:hi] &= ~((other >= mine) if d < 0 else (other > mine))
    steps = np.full((s, 1 + max_steps), -1, dtype=np.int32)
    for i in range(s):
        f = np.nonzero(step[:, i])[0]
        steps[i, 0] = f.size
        steps[i, 1:1 + min(f.size, max_steps)] = f[:max_steps]
    return steps


def _fold(lanes):
    off = 32
    while off >= 1:                                          # a[i] + a[i + 32], then + 16, 8, 4, 2, 1
        lanes = lanes[:, :off] + lanes[:, off:2 * off]
        off //= 2
    return lanes[:, 0]


def dwell_stats(rec, steps, guard, n_values=None):
    """-> out [s, max_steps + 1, 3 + 2 nv] exactly as vbs_dwell_stats_f64 states it (steps [s or 1, 1 + max_steps])."""
    rec = np.asarray(rec, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.int64)
    n, s, cols = rec.shape
    nv = cols - 1 if n_values is None else int(n_values)
    ms = steps.shape[1] - 1
    if steps.shape[0] == 1:
        steps = np.repeat(steps, s, axis=0)
    k = np.clip(steps[:, 0], 0, ms)
    out = np.full((s, ms + 1, 3 + 2 * nv), np.nan)
    out[..., 0:2], out[..., 2] = -1.0, 0.0
    lane, sidx = np.arange(64)[None, :], np.arange(s)[:, None]
    for j in range(ms + 1):
        live = j <= k
        if not live.any():
            break
        begin = np.zeros(s, dtype=np.int64) if j == 0 else steps[:, j] + guard
        end = np.where(j == k, n, steps[:, min(1 + j, ms)] - guard)
        begin, end = np.clip(begin, 0, n), np.clip(end, 0, n)
        end = np.maximum(end, begin)
        begin, end = np.where(live, begin, 0), np.where(live, end, 0)
        rounds = int(((end - begin).max() + 63) // 64)

        def lane_sums(term):
            acc = np.zeros((s, 64, nv))
            cnt = np.zeros((s, 64), dtype=np.int64)
            for r in range(rounds):                          # lane l: frames begin + l, begin + l + 64, ... in ascending order
                f = begin[:, None] + r * 64 + lane
                inside = f < end[:, None]
                row = rec[np.where(inside, f, 0), sidx]      # [s, 64, cols]
                use = inside & (row[..., 0] != 0)
                acc = np.where(use[..., None], acc + term(row[..., 1:1 + nv]), acc)
                cnt += use
            return _fold(acc), cnt.sum(axis=1)

        with np.errstate(all="ignore"):
            total, cnt = lane_sums(lambda x: x)
            mean = np.where((cnt > 0)[:, None], total / cnt[:, None].astype(np.float64), np.nan)
            m2, _ = lane_sums(lambda x: (x - mean[:, None, :]) * (x - mean[:, None, :]))
        row = np.concatenate([begin[:, None].astype(np.float64), end[:, None].astype(np.float64),
                              cnt[:, None].astype(np.float64), mean, m2], axis=1)
        out[live, j] = row[live]
    return out


def dwell_std(stats, n_values):
    """std (ddof = 1) per dwell and value from dwell_stats' rows; NaN below two frames."""
    cnt = stats[..., 2:3]
    with np.errstate(all="ignore"):
        return np.where(cnt >= 2, np.sqrt(stats[..., 3 + n_values:3 + 2 * n_values] / (cnt - 1)), np.nan)


# ---- the independent sides -----------------------------------------------------------------------------------------------
def check_response_gap_free(out, rec, window):
    """A gap-free record: the response against np.convolve with a +-1/w box, on the interior [w, n - w]."""
    rec = np.asarray(rec, dtype=np.float64)
    n, s, cols = rec.shape
    w = int(window)
    box = np.concatenate([np.full(w, 1.0 / w), np.full(w, -1.0 / w)])     # y[f] = (sum x[f .. f+w-1] - sum x[f-w .. f-1]) / w
    worst = 0.0
    for i in range(s):
        for c in range(cols - 1):
            x = rec[:, i, 1 + c]
            ref = np.convolve(x, box)[w - 1 + w:n]                          # f = w .. n - w
            mass = np.convolve(np.abs(x), np.abs(box))[w - 1 + w:n]
            bound = 2 * w * U2 * mass + 2 * U2 * np.abs(ref)
            err = np.abs(out[w:n - w + 1, i, 2 + c] - ref)
            assert (err <= bound).all(), (i, c, float((err / bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert (out[w:n - w + 1, :, 0] == 1).all()
    return worst


def check_dwell_means(stats, rec, n_values):
    """The dwell means against math.fsum over the frames the rows themselves name."""
    rec = np.asarray(rec, dtype=np.float64)
    for i in range(stats.shape[0]):
        for j in range(stats.shape[1]):
            b, e, c = (int(v) for v in stats[i, j, :3])
            if b < 0:
                continue
            v = rec[b:e, i, 0] != 0
            assert c == int(v.sum()), (i, j)
            for a in range(n_values):
                x = rec[b:e, i, 1 + a][v]
                if c == 0:
                    assert np.isnan(stats[i, j, 3 + a])
                    continue
                ref = math.fsum(x.tolist()) / c
                assert abs(stats[i, j, 3 + a] - ref) <= c * U2 * float(np.abs(x).sum()) / c + U2 * abs(ref), (i, j, a)


# ---- the synthetic Figure-6(b) signal ------------------------------------------------------------------------------------------
FIGURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "figure_6b.json")))
LEVELS = np.asarray(FIGURE["cumulative_mm"], dtype=np.float64)
ERRORS = np.asarray(FIGURE["single_step_error_mm"], dtype=np.float64)
STEP_MM = float(FIGURE["step_mm"])


def figure6_signal(dwell, ramp, noise, levels=LEVELS):
    """The figure's 13 levels held for `dwell` frames each, `ramp` frames on the straight line between two of them (its interior
    points), plus noise (-1)^f.  -> (z [n], dwell_begin [13]): n = 13 dwell + 12 ramp."""
    levels = np.asarray(levels, dtype=np.float64)
    parts, begins, at = [], [], 0
    for k, lv in enumerate(levels):
        begins.append(at)
        parts.append(np.full(dwell, lv))
        at += dwell
        if k + 1 < levels.size and ramp > 0:
            parts.append(lv + (levels[k + 1] - lv) * np.arange(1, ramp + 1) / (ramp + 1.0))
            at += ramp
    z = np.concatenate(parts)
    return z + noise * np.where(np.arange(z.size) % 2 == 0, 1.0, -1.0), np.asarray(begins)


def analyse(rec, window, threshold, guard, step_mm, max_steps=MAX_STEPS):
    """The chain `pipeline.indentation_analysis` runs on ONE series rec [n, 1, 1 + nv], on the restatement: a dict with its
    fields."""
    nv = rec.shape[2] - 1
    steps = find_steps(response(rec, window), window, float(threshold) * float(threshold), max_steps)
    k = min(int(steps[0, 0]), max_steps)
    st = dwell_stats(rec, steps, guard)[0, :k + 1]
    with np.errstate(all="ignore"):
        cum = st[:, 3] if nv == 1 else np.sqrt((st[:, 3:3 + nv] ** 2).sum(axis=1))
        std = np.where(st[:, 2] >= 2, np.sqrt(st[:, 3 + nv:].sum(axis=1) / (st[:, 2] - 1)), np.nan)
    delta = np.diff(cum)
    return {"steps": steps, "step_frames": steps[0, 1:1 + k].astype(np.int64), "begin": st[:, 0].astype(np.int64),
            "end": st[:, 1].astype(np.int64), "count": st[:, 2].astype(np.int64), "cumulative": cum, "std": std, "delta": delta,
            "abs_error": np.abs(delta - step_mm), "overflow": int(steps[0, 0]) > max_steps}
