"""References for the gap-aware local polynomial fit along time (k_kinematics.hip): `engine.poly_moments_f64`,
`engine.poly_fit_f64`, `pipeline.kinematic_analysis`, `pipeline.fill_table`.  NumPy, scipy and `fractions` only.

  * `taps` / `moments`   the LOOP RESTATEMENT of include/vbs.h: the tap rows w u^k (u^k exact, one rounding a tap), then every sum
                         over the valid frames of its window in ascending frame order.  The device promises no order, so this is
                         held BIT FOR BIT only on inputs on which every order is exact (`dyadic_case`, with its bit budget), and
  * `exact_moments`      within the DERIVED bound gamma_(K+8) sum |tap term| of exact rational arithmetic otherwise;
  * `ldl` / `fit`        the restatement of the fit in the stated order: the device is held to it bit for bit;
  * `lstsq_window`       np.linalg.lstsq on sqrt(w) [1, u, .., u^q] over the valid frames of a window: the independent reference
                         from which KIN_TOL is MEASURED (never against the device).
"""
from fractions import Fraction

import numpy as np

from envelope_oracle import assert_bits, gaps, poison       # noqa: F401  (the same record conventions)

U = Fraction(1, 2 ** 53)
MAX_HALF, MAX_DEGREE = 127, 3
PIV_REL = 5e-3                                               # the documented default of `piv_rel` (DESIGN 4.20's table)


def scale(h):
    """H: the smallest power of two >= max(h, 1)."""
    H = 1
    while H < h:
        H *= 2
    return H


def n_sums(d, nv):
    return 2 * d + 1 + (d + 2) * nv


def window(h, kind="hann"):
    """The window's 2h + 1 weights: `spectra.window_taps`'s own for a name, the array itself otherwise."""
    from vbs_amd import spectra
    return spectra.window_taps(h, kind) if isinstance(kind, str) else np.asarray(kind, np.float64)


def taps(h, d, kind="hann"):
    """taps [2d + 1, 2h + 1]: taps[k][delta + h] = w[delta] * u^k, u = delta / H, the power by repeated multiplication, one entry
    at a time."""
    w, H = window(h, kind), scale(h)
    out = np.zeros((2 * d + 1, 2 * h + 1))
    for j in range(2 * h + 1):
        u = float(j - h) / float(H)
        p = 1.0
        for k in range(2 * d + 1):
            assert Fraction(p) == Fraction(j - h, H) ** k    # every power is exact
            out[k, j] = w[j] * p
            p = p * u
    return out


def ascending_sums(tp):
    S = np.zeros(tp.shape[0])
    for j in range(tp.shape[1]):
        S = S + tp[:, j]
    return S


def moments(rec, tp, d, nv, frame_range=None):
    """mom [b-a, s, M]: S_k (k <= 2d), then X_k (k <= d), XX per value over the VALID frames j of [f-h, f+h] n [0, n) in ascending
    j; every product rounded once, the square first; an invalid entry adds nothing (its value is never touched)."""
    rec = np.asarray(rec, np.float64)
    n, s = rec.shape[:2]
    h = tp.shape[1] // 2
    a, b = (0, n) if frame_range is None else frame_range
    valid = rec[..., 0] != 0.0
    x = np.where(valid[..., None], rec[..., 1:1 + nv], 0.0)
    xx = x * x
    R = 2 * d + 1
    out = np.zeros((b - a, s, n_sums(d, nv)))
    for f in range(a, b):
        o = out[f - a]
        for j in range(max(0, f - h), min(n, f + h + 1)):
            t = tp[:, j - f + h]
            v = valid[j]
            for k in range(R):
                o[:, k] += np.where(v, t[k], 0.0)
            for c in range(nv):
                base = R + c * (d + 2)
                for k in range(d + 1):
                    o[:, base + k] += np.where(v, t[k] * x[j, :, c], 0.0)
                o[:, base + d + 1] += np.where(v, t[0] * xx[j, :, c], 0.0)
    return out


def gamma(k):
    return k * U / (1 - k * U)


def exact_moments(rec, tp, d, nv, frame_range=None):
    """-> (sums, mags): the same sums of the ROUNDED taps and the rounded squares in exact rational arithmetic, and sum |tap term|;
    object arrays of Fractions [b-a, s, M]."""
    rec = np.asarray(rec, np.float64)
    n, s = rec.shape[:2]
    h = tp.shape[1] // 2
    a, b = (0, n) if frame_range is None else frame_range
    R, M = 2 * d + 1, n_sums(d, nv)
    T = [[Fraction(float(tp[k, j])) for j in range(2 * h + 1)] for k in range(R)]
    sums = np.empty((b - a, s, M), dtype=object)
    mags = np.empty((b - a, s, M), dtype=object)
    for i in range(s):
        val = rec[:, i, 0] != 0.0
        X = [[Fraction(float(rec[j, i, 1 + c])) if val[j] else None for j in range(n)] for c in range(nv)]
        XX = [[Fraction(float(rec[j, i, 1 + c] * rec[j, i, 1 + c])) if val[j] else None for j in range(n)] for c in range(nv)]
        for f in range(a, b):
            S, A = [Fraction(0)] * M, [Fraction(0)] * M
            for j in range(max(0, f - h), min(n, f + h + 1)):
                if not val[j]:
                    continue
                dj = j - f + h
                for k in range(R):
                    S[k] += T[k][dj]
                    A[k] += abs(T[k][dj])
                for c in range(nv):
                    base = R + c * (d + 2)
                    for k in range(d + 1):
                        p = T[k][dj] * X[c][j]
                        S[base + k] += p
                        A[base + k] += abs(p)
                    p = T[0][dj] * XX[c][j]
                    S[base + d + 1] += p
                    A[base + d + 1] += abs(p)
            sums[f - a, i], mags[f - a, i] = S, A
    return sums, mags


def check_within_bound(got, rec, tp, d, nv, frame_range=None, what=""):
    """Asserts |got - exact| <= gamma_(K+8) sum |tap term| entry by entry (K = 2h + 1) and returns the largest share of
    the bound seen."""
    h = tp.shape[1] // 2
    sums, mags = exact_moments(rec, tp, d, nv, frame_range)
    g = gamma(2 * h + 1 + 8)
    worst = 0.0
    assert got.shape == sums.shape, f"{what}: shape {got.shape}"
    for idx in np.ndindex(got.shape):
        assert np.isfinite(got[idx]), f"{what}: {got[idx]} at {idx}"
        err, bnd = abs(Fraction(float(got[idx])) - sums[idx]), g * mags[idx]
        assert err <= bnd, f"{what}: entry {idx}: error {float(err):.3g} above the bound {float(bnd):.3g}"
        if bnd:
            worst = max(worst, float(err / bnd))
    return worst


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
def ldl(S, d):
    """G[a][b] = S[..., a + b] = L diag(D) L^T in the order include/vbs.h states, vectorised over the leading axes: -> (D [..., d+1],
    L [..., d+1, d+1]); every expression as written, float64."""
    S = np.asarray(S, np.float64)
    lead = S.shape[:-1]
    D = np.zeros(lead + (d + 1,))
    L = np.zeros(lead + (d + 1, d + 1))
    V = np.zeros(lead + (d + 1, d + 1))
    with np.errstate(all="ignore"):
        for j in range(d + 1):
            t = S[..., 2 * j].copy()
            for m in range(j):
                t = t - V[..., j, m] * L[..., j, m]
            D[..., j] = t
            for a in range(j + 1, d + 1):
                w = S[..., a + j].copy()
                for m in range(j):
                    w = w - V[..., a, m] * L[..., j, m]
                V[..., a, j] = w
                L[..., a, j] = w / t
    return D, L


def thresholds(sw, piv_full, min_coverage=0.5, piv_rel=PIV_REL, h=None):
    """thr[0] = min_coverage * sw, thr[k] = piv_rel * piv_full[k]; with h, +inf for the orders k >= 2h + 1, which a window of 2h + 1
    frames cannot determine."""
    thr = np.array([np.float64(piv_rel) * np.float64(p) for p in piv_full])
    thr[0] = np.float64(min_coverage) * np.float64(sw)
    if h is not None:
        thr[2 * h + 1:] = np.inf
    return thr


def full_pivots(tp, d):
    """(sw, piv_full) of the gap-free full window from the ascending sums of the tap rows."""
    S = ascending_sums(tp)
    return float(S[0]), ldl(S, d)[0]


def fit(mom, centre_rows, thr, h, d, nv, fill_degree=1):
    """The restated `vbs_poly_fit_f64`: mom [F, s, M], centre_rows [F, s, cols] = the rows of rec at the frames of mom, thr [d + 1].
    -> (fit [F, s, 2 + (d + 2) nv], filled [F, s, cols])."""
    mom = np.asarray(mom, np.float64)
    rows = np.asarray(centre_rows, np.float64)
    F, s, M = mom.shape
    assert M == n_sums(d, nv) and rows.shape[:2] == (F, s)
    R = 2 * d + 1
    H = float(scale(h))
    out = np.zeros((F, s, 2 + (d + 2) * nv))
    with np.errstate(all="ignore"):
        D, L = ldl(mom[..., :R], d)
        q = np.full((F, s), -1, dtype=np.int64)
        ok = np.ones((F, s), dtype=bool)
        for k in range(d + 1):
            ok = ok & (D[..., k] > thr[k])
            q = np.where(ok, k, q)
        valid = rows[..., 0] != 0.0
        out[..., 0] = valid + 2.0 * (q >= 0) + 4.0 * (q == d)
        out[..., 1] = q
        y0 = np.zeros((F, s, nv))
        for c in range(nv):
            X = mom[..., R + c * (d + 2):R + (c + 1) * (d + 2)]
            z, g, cf = [None] * (d + 1), [None] * (d + 1), [None] * (d + 1)
            for k in range(d + 1):
                t = X[..., k].copy()
                for m in range(k):
                    t = t - L[..., k, m] * z[m]
                z[k] = t
                g[k] = t / D[..., k]
            for k in range(d, -1, -1):
                t = g[k].copy()
                for m in range(k + 1, d + 1):
                    t = np.where(m <= q, t - L[..., m, k] * cf[m], t)
                cf[k] = np.where(k <= q, t, 0.0)
            rss = X[..., d + 1].copy()
            for k in range(d + 1):
                rss = np.where(k <= q, rss - z[k] * g[k], rss)
            o = out[..., 2 + c * (d + 2):]
            o[..., 0] = cf[0]
            if d >= 1:
                o[..., 1] = cf[1] / H
            if d >= 2:
                o[..., 2] = (2.0 * cf[2]) / (H * H)
            if d >= 3:
                o[..., 3] = (6.0 * cf[3]) / (H * H * H)
            o[..., d + 1] = rss
            y0[..., c] = cf[0]
    filled = np.zeros_like(rows)
    fill = ~valid & (q >= fill_degree)
    filled[valid] = rows[valid]
    filled[fill, 0] = 2.0
    filled[..., 1:1 + nv][fill] = y0[fill]
    return out, filled


def degree_of(fit_out):
    return fit_out[..., 1].astype(np.int64)


def lstsq_window(x, valid, w, h, f, q):
    """np.linalg.lstsq of sqrt(w) x on sqrt(w) [1, u, .., u^q], u = (j - f) / H, over the valid frames j of the window round frame
    f -> (the derivatives y_0 .. y_q at the centre in units of frames, the weighted residual sum of squares)."""
    n, H = len(x), float(scale(h))
    j = np.array([k for k in range(max(0, f - h), min(n, f + h + 1)) if valid[k]], dtype=np.int64)
    sq = np.sqrt(np.asarray(w, np.float64)[j - f + h])
    u = (j - f) / H
    A = np.stack([u ** k for k in range(q + 1)], axis=1) * sq[:, None]
    rhs = np.asarray(x, np.float64)[j] * sq
    c = np.linalg.lstsq(A, rhs, rcond=None)[0]
    res = rhs - A @ c
    fact = (1.0, 1.0, 2.0, 6.0)
    return np.array([fact[k] * c[k] / H ** k for k in range(q + 1)]), float(res @ res)


# ---- generators ----------------------------------------------------------------------------------------------------------------
def bits(v):
    return int(v).bit_length()


def dyadic_case(n, s, cols, nv, h, d, seed, drop=0.2, kind=1e300):
    """-> (rec [n, s, cols], w [2h + 1], budget): inputs on which every order of summation is exact.  Weights k / 8 (1 <= k <= 8: 4
    bits) and values k / 16 (|k| <= 32: 6 bits) where the budget
        bits(h^2d) + bits(w) + bits(x) + bits(2h + 1) <= 53
    allows it (h <= 7 at every d: 17 + 4 + 6 + 4 = 31; h = 31, d = 3: 30 + 4 + 6 + 6 = 46; h = 127, d = 2: 28 + 4 + 6 + 8 = 46),
    otherwise rect weights (1 bit) and values in {-1, 0, 1} (1 bit): h = 127, d = 3: 42 + 1 + 1 + 8 = 52.  XX needs
    bits(w) + 2 bits(x) + bits(2h + 1), which is smaller."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    budget = bits(max(h, 1) ** (2 * d)) + 4 + 6 + bits(2 * h + 1)
    if budget <= 53:
        half = r.integers(1, 9, h + 1) / 8.0
        rec[..., 1:] = r.integers(-32, 33, (n, s, cols - 1)) / 16.0
    else:
        half = np.ones(h + 1)
        rec[..., 1:] = r.integers(-1, 2, (n, s, cols - 1)).astype(np.float64)
        budget = bits(max(h, 1) ** (2 * d)) + 1 + 1 + bits(2 * h + 1)
    assert budget <= 53
    w = np.concatenate([half[:0:-1], half])
    return (rec if kind is None else poison(rec, nv, kind)), w, budget


def random_case(n, s, cols, nv, seed, drop=0.2, kind=np.nan):
    """The same shapes with float content: values of mixed sign over six decades."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.standard_normal((n, s, cols - 1)) * 10.0 ** r.uniform(-3, 3, (n, s, cols - 1))
    return rec if kind is None else poison(rec, nv, kind)


# ---- the fit's cases: KIN_TOL ------------------------------------------------------------------------------------------------------
KIN_SIZES, KIN_HALVES, KIN_DEGREES = (64, 197, 600), (3, 7, 24, 40), (1, 2, 3)
KIN_TOL = 2.4e-13              # 10 x the largest difference `kin_measured()` sees (2.36e-14, at n = 197, h = 3, d = 3), rounded up to
#                                two digits; test_kinematics_host.py holds the measurement to it


def press_case(n, seed, drop=0.03, noise=0.002):
    """A series for the fit: rest, a smooth press (a raised cosine into a plateau with a slow drift) plus noise, `drop` of the frames
    missing and one gap of 2 * 40 + 5 frames, longer than any window here (shortened on short recordings).  -> rec [n, 1, 2]."""
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    z = np.clip((f - 0.3 * n) / (0.25 * n), 0.0, 1.0)
    x = 0.8 * 0.5 * (1.0 - np.cos(np.pi * z)) + 1e-4 * f + noise * r.standard_normal(n)
    rec = np.zeros((n, 1, 2))
    rec[:, 0, 0] = (r.random(n) >= drop).astype(np.float64)
    g = min(85, n // 3)
    rec[n // 2:n // 2 + g, 0, 0] = 0.0
    rec[:, 0, 1] = x
    return rec


def kin_difference(n, h, d, kind="hann"):
    """The largest |y_0 .. y_q difference| over the frames with q >= 0 between `fit` (fed `moments`) at the degree it reports and
    `lstsq_window` at that degree, on `press_case(n)`; and the count of frames compared."""
    rec = press_case(n, seed=2000 + n + h)
    tp = taps(h, d, kind)
    sw, piv = full_pivots(tp, d)
    out, _ = fit(moments(rec, tp, d, 1), rec, thresholds(sw, piv), h, d, 1)
    w = window(h, kind)
    worst, count = 0.0, 0
    for f in range(n):
        q = int(out[f, 0, 1])
        if q < 0:
            continue
        y, _ = lstsq_window(rec[:, 0, 1], rec[:, 0, 0] != 0.0, w, h, f, q)
        worst = max(worst, float(np.abs(out[f, 0, 2:3 + q] - y).max()))
        count += 1
    return worst, count


_KIN_MEASURED = []


def kin_measured():
    """The largest `kin_difference` over KIN_SIZES x KIN_HALVES x KIN_DEGREES: KIN_TOL is 10 x this, measured between the two
    references (never against the device).  Computed once."""
    if not _KIN_MEASURED:
        _KIN_MEASURED.append(max(kin_difference(n, h, d)[0] for n in KIN_SIZES for h in KIN_HALVES for d in KIN_DEGREES))
    return _KIN_MEASURED[0]


# ---- hand-built moments: the fit's rules ---------------------------------------------------------------------------------------------
HAND_H, HAND_D = 4, 1          # H = 4; M = 3 + 3 = 6 with one value: S_0, S_1, S_2, X_0, X_1, XX
HAND_THR = np.array([12.0, 3.0])


def hand_moments():
    """(mom [1, 11, 6], rows [1, 11, 2]) for d = 1, h = 4 (H = 4), thr = (12, 3).  Unless set: S = (16, 0, 8), so D_0 = 16, D_1 = 8,
    and X_0 = 4, X_1 = 2, XX = 3: c_0 = 0.25, c_1 = 0.25, y_1 = 0.0625, rss = 3 - 1 - 0.5 = 1.5, all exact.
      0  the plain case, the centre valid: flag 7, q = 1;
      1  the centre missing: flag 6, filled with y_0;
      2  S_0 = 12 = thr[0] exactly: strict, q = -1, flag 1, rss = XX;    3  S_0 one ulp above 12: q >= 0;
      4  S_2 = 3: D_1 == thr[1] exactly: falls back to the mean, q = 0, y_0 = X_0 / S_0, y_1 = 0;   5  S_2 one ulp above 3: q = 1;
      6  none valid: S = 0, X = 0: q = -1, nothing from 0 / 0 reaches the output;
      7  a NaN S_1: D_0 passes, D_1 is NaN, q = 0;
      8  a NaN S_0: q = -1;
      9  rss < 0 (XX = 1.25 under 1.5): reported as computed;
     10  the centre missing and q = 0 < fill_degree = 1: flag 2, not filled."""
    mom = np.zeros((1, 11, 6))
    mom[0, :] = (16.0, 0.0, 8.0, 4.0, 2.0, 3.0)
    rows = np.zeros((1, 11, 2))
    rows[0, :, 0], rows[0, :, 1] = 1.0, 0.375
    rows[0, 1] = (0.0, np.nan)
    mom[0, 2, 0] = 12.0
    mom[0, 3, 0] = np.nextafter(12.0, 20.0)
    mom[0, 4, 2] = 3.0
    mom[0, 5, 2] = np.nextafter(3.0, 4.0)
    mom[0, 6] = 0.0
    mom[0, 7, 1] = np.nan
    mom[0, 8, 0] = np.nan
    mom[0, 9, 5] = 1.25
    mom[0, 10, 2] = 3.0
    rows[0, 10] = (0.0, np.nan)
    return mom, rows


def check_hand(out, filled):
    """What `hand_moments` must give, on either side."""
    assert out.shape == (1, 11, 5) and filled.shape == (1, 11, 2)
    o, fl = out[0], filled[0]
    assert o[0].tolist() == [7.0, 1.0, 0.25, 0.0625, 1.5] and fl[0].tolist() == [1.0, 0.375]
    assert o[1].tolist() == [6.0, 1.0, 0.25, 0.0625, 1.5] and fl[1].tolist() == [2.0, 0.25]
    assert o[2].tolist() == [1.0, -1.0, 0.0, 0.0, 3.0]
    assert o[3, 0] == 7.0 and o[3, 1] == 1.0
    assert o[4].tolist() == [3.0, 0.0, 0.25, 0.0, 2.0]
    assert o[5, 0] == 7.0 and o[5, 1] == 1.0
    assert o[6].tolist() == [1.0, -1.0, 0.0, 0.0, 0.0]
    assert o[7].tolist() == [3.0, 0.0, 0.25, 0.0, 2.0]
    assert o[8].tolist() == [1.0, -1.0, 0.0, 0.0, 3.0]
    assert o[9, 0] == 7.0 and o[9, 4] == -0.25
    assert o[10].tolist() == [2.0, 0.0, 0.25, 0.0, 2.0] and fl[10].tolist() == [0.0, 0.0]


# ---- a synthetic recording: rest, a quadratic press, constant velocity, stop -----------------------------------------------------------
PRESS_HALF, PRESS_START, PRESS_RAMP, PRESS_STOP = 7, 60, 100, 150    # pieces [0, 60), [60, 100), [100, 150), [150, n)
PRESS_ACC = 2.0 ** -9          # mm / frame^2 of the press: dyadic, so the table's float32 holds every sample exactly
FAST_SLOT, FAST_FROM, FAST_LEN, FAST_V = 17, 105, 20, 0.25


def press_profile(n):
    """-> (z, v, a) float64 [n]: the analytic position, velocity and acceleration of the press, and `pieces`, the frame ranges on
    each of which z is one polynomial of degree <= 2."""
    f = np.arange(n, dtype=np.float64)
    t1, t2 = PRESS_RAMP - PRESS_START, PRESS_STOP - PRESS_RAMP
    v1 = PRESS_ACC * t1
    z = np.where(f < PRESS_START, 0.0,
                 np.where(f < PRESS_RAMP, 0.5 * PRESS_ACC * (f - PRESS_START) ** 2,
                          np.where(f < PRESS_STOP, 0.5 * PRESS_ACC * t1 ** 2 + v1 * (f - PRESS_RAMP),
                                   0.5 * PRESS_ACC * t1 ** 2 + v1 * t2)))
    v = np.where((f >= PRESS_START) & (f < PRESS_RAMP), PRESS_ACC * (f - PRESS_START), np.where((f >= PRESS_RAMP) & (f < PRESS_STOP), v1, 0.0))
    a = np.where((f >= PRESS_START) & (f < PRESS_RAMP), PRESS_ACC, 0.0)
    return z, v, a, ((0, PRESS_START), (PRESS_START, PRESS_RAMP), (PRESS_RAMP, PRESS_STOP), (PRESS_STOP, n))


def inside_one_piece(n, pieces, h):
    """bool [n]: the frame's window [f - h, f + h] n [0, n) lies inside one piece."""
    ok = np.zeros(n, dtype=bool)
    for a, b in pieces:
        lo = a + h if a > 0 else 0
        hi = b - h if b < n else n
        ok[lo:hi] = True
    return ok


def press_table(side=7, n=197, seed=0, drop=0.02):
    """-> (table float32 [n, side^2, 10], gain [side^2]): nodes on a side x side grid; marker i moves in Z by -gain_i z(f) (into the
    skin), in X by 0.25 gain_i z(f); gain_i in {0.5, 0.75, 1.0} (dyadic); marker FAST_SLOT has an extra X velocity FAST_V for the
    FAST_LEN frames from FAST_FROM, and keeps the offset after them.  `drop` of the entries are missing, flags cleared and values left
    as garbage (frame 0 never)."""
    r = np.random.default_rng(seed)
    m = side * side
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    gain = np.array([0.5, 0.75, 1.0])[np.arange(m) % 3]
    z = press_profile(n)[0]
    f = np.arange(n, dtype=np.float64)
    extra = FAST_V * np.clip(f - FAST_FROM, 0.0, float(FAST_LEN))
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    X = x0[None, :] + 0.25 * gain[None, :] * z[:, None]
    X[:, FAST_SLOT] += extra
    t[..., 6], t[..., 7], t[..., 8] = X, y0[None, :], 10.0 - gain[None, :] * z[:, None]
    assert np.array_equal(t[..., 6].astype(np.float64), X)                  # float32 holds every sample exactly
    gone = r.random((n, m)) < drop
    gone[0] = False
    t[gone, 0] = 0.0
    t[gone, 6:9] = 1e30
    return t, gain
