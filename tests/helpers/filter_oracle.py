"""NumPy restatement of the dynamic-polishing analysis (`include/vbs.h`: vbs_axis_displacement, vbs_fir_series_f64), the checks
that do not share its order of summation, and the bounds both are held to.

The restatement is the SAME IEEE operations in the SAME order as the device (sequential in k, vectorised over frames and
series; lane-then-fold for the totals; select, never multiply by zero; NumPy's ufuncs do not contract a product into a sum), so
the device is held to it BIT FOR BIT.  The independent checks (`np.convolve`, `math.fsum`) use another order; the bounds are
those of the summation error, with 2^-52 = 2 u so that the device's and the check's own rounding both fit:
    FIR, all 2h+1 inputs valid:   |y - ref| <= K 2^-52 sum|w x| / |den| + 2 2^-52 |ref|
    FIR, gaps or edges:           the same with sum|w x| + |ref| sum|w| for sum|w x|: there the check's denominator is a
                                  rounded sum over the valid taps as well (on a gap-free interior it is the exact fsum of w)
    totals over m slots:          |t - fsum| <= m 2^-52 sum|d|
None of them comes from what the device gives."""
import math

import numpy as np

U2 = 2.0 ** -52


def full_taps(half):
    half = np.asarray(half, dtype=np.float64)
    return np.concatenate([half[:0:-1], half])


def fir(rec, half, n_values, min_coverage=0.5, frame_range=None):
    """-> out [b-a, s, 1 + 2 nv] exactly as vbs_fir_series_f64 states it."""
    rec = np.asarray(rec, dtype=np.float64)
    half = np.asarray(half, dtype=np.float64)
    n, s, _ = rec.shape
    nv, h = int(n_values), half.size - 1
    valid = rec[..., 0] != 0
    x = rec[..., 1:1 + nv]
    sw = 0.0
    for k in range(-h, h + 1):
        sw = sw + float(half[abs(k)])
    need = float(min_coverage) * sw
    num, den = np.zeros((n, s, nv)), np.zeros((n, s))
    with np.errstate(all="ignore"):
        for k in range(-h, h + 1):
            lo, hi = max(0, -k), min(n, n - k)
            if hi <= lo:
                continue
            w, v = half[abs(k)], valid[lo + k:hi + k]
            den[lo:hi] = np.where(v, den[lo:hi] + w, den[lo:hi])
            num[lo:hi] = np.where(v[..., None], num[lo:hi] + w * x[lo + k:hi + k], num[lo:hi])
        ok = valid & (den >= need)
        y = np.where(ok[..., None], num / den[..., None], 0.0)
        res = np.where(ok[..., None], x - y, 0.0)
    out = np.concatenate([(valid + 2.0 * ok)[..., None], y, res], axis=2)
    a, b = (0, n) if frame_range is None else frame_range
    return out[a:b]


def fir_check(rec, half, n_values):
    """The independent side: per entry (ref, bound, full) from np.convolve on the cleaned series (invalid entries REPLACED by
    0, not multiplied), `full` = all 2h+1 inputs valid and inside [0, n).  ref = num / den wherever den != 0."""
    rec = np.asarray(rec, dtype=np.float64)
    w = full_taps(half)
    K, h = w.size, (w.size - 1) // 2
    n, s, _ = rec.shape
    nv = int(n_values)
    valid = rec[..., 0] != 0
    ref, bound = np.zeros((n, s, nv)), np.zeros((n, s, nv))
    full = np.zeros((n, s), dtype=bool)
    sw_exact, aw = math.fsum(w.tolist()), np.abs(w)
    for j in range(s):
        vj = valid[:, j].astype(np.float64)
        den = np.convolve(vj, w)[h:h + n]
        sabs_w = np.convolve(vj, aw)[h:h + n]
        full[:, j] = np.convolve(vj, np.ones(K))[h:h + n] > K - 0.5
        den = np.where(full[:, j], sw_exact, den)
        for c in range(nv):
            xc = np.where(valid[:, j], rec[:, j, 1 + c], 0.0)
            num = np.convolve(xc, w)[h:h + n]
            sabs = np.convolve(np.abs(xc), aw)[h:h + n]
            with np.errstate(all="ignore"):
                r = np.where(den != 0, num / den, 0.0)
                extra = np.where(full[:, j], 0.0, np.abs(r) * sabs_w)
                bound[:, j, c] = np.where(den != 0, K * U2 * (sabs + extra) / np.abs(den) + 2 * U2 * np.abs(r), np.inf)
            ref[:, j, c] = r
    return ref, bound, full


def check_fir(got, rec, half, n_values, min_coverage=0.5, frame_range=None, what=""):
    """`got` (the device's, or the restatement's own) against both sides.  Returns the largest |y - ref| / bound seen."""
    got = np.asarray(got)
    rec = np.asarray(rec, dtype=np.float64)
    n = rec.shape[0]
    nv = int(n_values)
    a, b = (0, n) if frame_range is None else frame_range
    want = fir(rec, half, nv, min_coverage, (a, b))
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"{what}: {int((got.view(np.uint64) != want.view(np.uint64)).sum())} entries differ in bits from the restatement"
    ref, bound, _ = fir_check(rec, half, nv)
    ref, bound = ref[a:b], bound[a:b]
    ok = got[..., 0] == 3.0
    x = rec[a:b, :, 1:1 + nv]
    worst = 0.0
    if ok.any():
        err = np.abs(got[..., 1:1 + nv] - ref)[ok]
        assert (err <= bound[ok]).all(), f"{what}: filtered off the convolution by {float((err / bound[ok]).max())} of the bound"
        worst = float((err / np.maximum(bound[ok], 1e-300)).max())
        err_r = np.abs(got[..., 1 + nv:] - (x - ref))[ok]
        assert (err_r <= bound[ok] + U2 * np.abs(x[ok])).all(), f"{what}: residual"
    assert (got[..., 1:][~ok] == 0).all(), f"{what}: an entry without a trend is not zero"
    return worst


def axis_total(table, ref_frame=0, mask=None, frame_range=None):
    """-> (axis [b-a, m, 4], total [b-a, 5]) exactly as vbs_axis_displacement states them (lane sums, then the fold)."""
    t = np.asarray(table)
    n, m, _ = t.shape
    a, b = (0, n) if frame_range is None else frame_range
    sel = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    xyz = (t[..., 0].astype(np.int64) & 2) != 0
    in_ref = sel & xyz[ref_frame]
    ok = xyz[a:b] & in_ref[None, :]
    d = t[a:b, :, 6:9].astype(np.float64) - t[ref_frame, :, 6:9].astype(np.float64)[None]
    d = np.where(ok[..., None], d, 0.0)
    axis = np.concatenate([ok.astype(np.float64)[..., None], d], axis=2)
    rows = (m + 63) // 64
    dp = np.zeros((b - a, rows * 64, 3))
    okp = np.zeros((b - a, rows * 64), dtype=bool)
    dp[:, :m], okp[:, :m] = d, ok
    dp, okp = dp.reshape(b - a, rows, 64, 3), okp.reshape(b - a, rows, 64)
    lane = np.zeros((b - a, 64, 3))
    for r in range(rows):                                # lane l: slots l, l + 64, ... in ascending order
        lane = np.where(okp[:, r, :, None], lane + dp[:, r], lane)
    off = 32
    while off >= 1:                                      # a[i] + a[i + 32], then + 16, 8, 4, 2, 1
        lane = lane[:, :off] + lane[:, off:2 * off]
        off //= 2
    cnt = ok.sum(axis=1)
    want = int(in_ref.sum())
    total = np.concatenate([((cnt == want) & (want >= 1)).astype(np.float64)[:, None], lane[:, 0], cnt.astype(np.float64)[:, None]],
                           axis=1)
    return axis, total


def check_axis_total(axis, total, table, ref_frame=0, mask=None, frame_range=None, what=""):
    want_axis, want_total = axis_total(table, ref_frame, mask, frame_range)
    if axis is not None:
        axis = np.asarray(axis)
        assert axis.shape == want_axis.shape and np.array_equal(axis.view(np.uint64), want_axis.view(np.uint64)), f"{what}: axis"
    total = np.asarray(total)
    assert total.shape == want_total.shape and np.array_equal(total.view(np.uint64), want_total.view(np.uint64)), f"{what}: total"
    m = np.asarray(table).shape[1]
    for i in range(want_axis.shape[0]):                  # the side that shares no order: the exactly rounded sum
        for c in range(3):
            col = want_axis[i, :, 1 + c]
            assert abs(total[i, 1 + c] - math.fsum(col.tolist())) <= m * U2 * float(np.abs(col).sum()), (what, i, c)
        assert total[i, 4] == want_axis[i, :, 0].sum()


# ---- the synthetic Figure-11 signal: a ramp to -10 mm, then an oscillation of 0.8 mm and period 8 frames plus noise ---------------
RAMP_MM, OSC_MM, OSC_PERIOD, NOISE_MM = -10.0, 0.8, 8, 0.05


def figure11_signal(n, ramp_frames, seed=0):
    t = np.arange(n)
    ramp = RAMP_MM * np.minimum(t / float(ramp_frames), 1.0)
    osc = np.where(t >= ramp_frames, OSC_MM * np.sin(2 * np.pi * (t - ramp_frames) / OSC_PERIOD), 0.0)
    return ramp + osc + np.random.default_rng(seed).normal(0.0, NOISE_MM, n)


def figure11_table(n, m, ramp_frames, seed=0):
    """A float32 table [n, m, 10], every slot seen in every frame: slot j sits at its own (X, Y, Z) and moves in Z by the signal
    scaled by 1 - 0.3 j / m (the rim moves less than the centre), with its own noise."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    base = rng.uniform(-20.0, 20.0, (m, 3))
    t[..., 6] = (base[None, :, 0] + rng.normal(0.0, 0.01, (n, m))).astype(np.float32)
    t[..., 7] = (base[None, :, 1] + rng.normal(0.0, 0.01, (n, m))).astype(np.float32)
    for j in range(m):
        t[:, j, 8] = (base[j, 2] + (1.0 - 0.3 * j / m) * figure11_signal(n, ramp_frames, seed + 1 + j)).astype(np.float32)
    return t
