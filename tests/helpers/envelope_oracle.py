"""NumPy restatement of the time-resolved fit (`include/vbs.h`: vbs_window_moments_f64, vbs_window_fit_f64), the exact side, the
bound and the generators the tests of both share.

The moments.  The interface does NOT fix the order of summation, so there are two references:
  * `moments`: float64, plain loops, every window summed in ascending j over its valid frames, the staged products x c, x s, x x
    rounded once, then the product with w, then the addition (no fused multiply-add).  One admissible order among many; the
    device need not equal it bit for bit - EXCEPT where every order is exact (`dyadic_case`: carrier k / 8 with |k| <= 8, values
    k / 16 with |k| <= 32, weights k / 8 with 1 <= k <= 8, at most 255 frames a window: a staged product is a multiple of 2^-8
    of at most 4, times w a multiple of 2^-11 of at most 4, a sum of 255 of them below 2^10: 21 significant bits, no operation
    rounds, with or without fused multiply-add).
  * `exact_moments`: `fractions`, no rounding at all: every sum, and the sum of magnitudes  A = sum w |term|.
The bound (`bound`), derived in DESIGN 4.18 for ANY order of summation of the K = 2h + 1 terms of a window with or without fused
multiply-add, padding adding exact zeros:  |sum^ - sum| <= gamma_(K+8) A,  u = 2^-53, gamma_k = k u / (1 - k u).  Evaluated and
compared in rationals (`check_within_bound`), so the check itself rounds nothing.

The fit (`window_fit`) restates the expressions of the header verbatim, one IEEE operation after the other in the order written
(elementwise NumPy never contracts), and is compared bit for bit (a NaN for a NaN)."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)


def n_sums(n_values):
    return 5 + 4 * n_values


# ---- the moments -----------------------------------------------------------------------------------------------------------------
def terms(rec, carrier, n_values):
    """-> T [n, s, M]: the staged terms 1, c, s, c2, s2, then x, x c, x s, x x per value, products rounded once (whatever the
    cells of invalid entries hold: the caller selects)."""
    rec, carrier = np.asarray(rec, np.float64), np.asarray(carrier, np.float64)
    n, s, _ = rec.shape
    T = np.empty((n, s, n_sums(n_values)))
    T[..., 0] = 1.0
    for k in range(4):
        T[..., 1 + k] = carrier[k][:, None]
    with np.errstate(all="ignore"):
        for v in range(n_values):
            x = rec[..., 1 + v]
            T[..., 5 + 4 * v] = x
            T[..., 6 + 4 * v] = x * carrier[0][:, None]
            T[..., 7 + 4 * v] = x * carrier[1][:, None]
            T[..., 8 + 4 * v] = x * x
    return T


def moments(rec, carrier, half, n_values, frame_range=None):
    """-> mom [fe - fb, s, M] as vbs_window_moments_f64 states it, every window in ascending j over its valid frames."""
    rec, half = np.asarray(rec, np.float64), np.asarray(half, np.float64)
    n, s, _ = rec.shape
    h = half.size - 1
    fb, fe = (0, n) if frame_range is None else frame_range
    T = terms(rec, carrier, n_values)
    valid = rec[..., 0] != 0.0
    out = np.zeros((fe - fb, s, n_sums(n_values)))
    with np.errstate(all="ignore"):
        for f in range(fb, fe):
            acc = np.zeros((s, n_sums(n_values)))
            for j in range(max(0, f - h), min(n, f + h + 1)):
                acc = np.where(valid[j][:, None], acc + half[abs(j - f)] * T[j], acc)    # selected: an invalid entry is never read
            out[f - fb] = acc
    return out


def exact_moments(rec, carrier, half, n_values, frame_range=None):
    """-> (value, mag): object arrays of Fractions [fe - fb, s, M]: the sums and the sums of magnitudes sum w |term|."""
    rec, carrier, half = np.asarray(rec, np.float64), np.asarray(carrier, np.float64), np.asarray(half, np.float64)
    n, s, _ = rec.shape
    h, M = half.size - 1, n_sums(n_values)
    fb, fe = (0, n) if frame_range is None else frame_range
    wf = [Fraction(float(w)) for w in half]
    cf = [[Fraction(float(carrier[k, j])) for k in range(4)] for j in range(n)]
    value = np.empty((fe - fb, s, M), dtype=object)
    mag = np.empty((fe - fb, s, M), dtype=object)
    for i in range(s):
        T = {}
        for j in range(n):
            if rec[j, i, 0] != 0.0:
                t = [Fraction(1)] + cf[j]
                for v in range(n_values):
                    x = Fraction(float(rec[j, i, 1 + v]))
                    t += [x, x * cf[j][0], x * cf[j][1], x * x]
                T[j] = t
        for f in range(fb, fe):
            live = [j for j in range(max(0, f - h), min(n, f + h + 1)) if j in T]
            for m in range(M):
                value[f - fb, i, m] = sum((wf[abs(j - f)] * T[j][m] for j in live), Fraction(0))
                mag[f - fb, i, m] = sum((wf[abs(j - f)] * abs(T[j][m]) for j in live), Fraction(0))
    return value, mag


def gamma(k):
    return k * U / (1 - k * U)


def bound(h, mag):
    """gamma_(K+8) * (sum of magnitudes), K = 2h + 1, as a Fraction."""
    return gamma(2 * h + 1 + 8) * mag


def check_within_bound(got, rec, carrier, half, n_values, frame_range=None, what=""):
    """Every entry of `got` against `exact_moments` within the bound; where the bound is zero (no valid frame) the entry is an
    exact zero.  No entry is skipped.  Returns the largest error / bound ratio seen (a float, to print)."""
    value, mag = exact_moments(rec, carrier, half, n_values, frame_range)
    h = np.asarray(half).size - 1
    got = np.asarray(got)
    assert got.shape == value.shape, f"{what}: shape {got.shape} != {value.shape}"
    worst = 0.0
    for idx in np.ndindex(*value.shape):
        g = got[idx]
        assert np.isfinite(g), f"{what}: entry {idx} is {g}"
        err, lim = abs(Fraction(float(g)) - value[idx]), bound(h, mag[idx])
        assert err <= lim, f"{what}: entry {idx}: error {float(err):.3e} above the bound {float(lim):.3e}"
        if lim > 0:
            worst = max(worst, float(err / lim))
    return worst


def taps_sum(half):
    """sw: the ascending sum of all w[k] = half[|k|], k = -h .. h."""
    half = np.asarray(half, np.float64)
    sw = np.float64(0.0)
    for k in range(-(half.size - 1), half.size):
        sw = sw + half[abs(k)]
    return float(sw)


# ---- the fit -----------------------------------------------------------------------------------------------------------------
def window_fit(mom, sw, min_coverage=0.5, det_min=1e-3):
    """-> fit [F, s, 1 + 5 nv] exactly as vbs_window_fit_f64 states it."""
    mom = np.asarray(mom, np.float64)
    nv = (mom.shape[2] - 5) // 4
    assert mom.shape[2] == n_sums(nv)
    half, dm = np.float64(0.5), np.float64(det_min)
    need = np.float64(min_coverage) * np.float64(sw)
    fit = np.zeros(mom.shape[:2] + (1 + 5 * nv,))
    with np.errstate(all="ignore"):
        W, C1, S1, C2, S2 = (mom[..., k] for k in range(5))
        CC = half * (W + C2) - (C1 * C1) / W
        SS = half * (W - C2) - (S1 * S1) / W
        CS = half * S2 - (C1 * S1) / W
        det = CC * SS - CS * CS
        ok = (W > 0.0) & (W >= need) & (det > dm * (W * W))
        fit[..., 0] = ok
        for v in range(nv):
            X, XC, XS, XX = (mom[..., 5 + 4 * v + k] for k in range(4))
            m = X / W
            pc = XC - m * C1
            ps = XS - m * S1
            a = (pc * SS - ps * CS) / det
            b = (ps * CC - pc * CS) / det
            p = a * pc + b * ps
            c0 = m - (a * C1 + b * S1) / W
            M2 = XX - m * X
            for k, val in enumerate((a, b, p, c0, M2)):
                fit[..., 1 + 5 * v + k] = np.where(ok, val, 0.0)
    return fit


def lstsq_window(x, valid, carrier, half, f):
    """np.linalg.lstsq of sqrt(w) x on sqrt(w) [1, c, s] over the valid frames of the window round frame f -> (c0, a, b): the
    independent reference of the fit."""
    n, h = len(x), len(half) - 1
    j = np.array([k for k in range(max(0, f - h), min(n, f + h + 1)) if valid[k]], dtype=np.int64)
    sq = np.sqrt(np.asarray(half, np.float64)[np.abs(j - f)])
    A = np.stack([np.ones(j.size), carrier[0][j], carrier[1][j]], axis=1) * sq[:, None]
    return np.linalg.lstsq(A, np.asarray(x, np.float64)[j] * sq, rcond=None)[0]


# ---- generators ----------------------------------------------------------------------------------------------------------------
def poison(rec, n_values, kind=np.nan):
    """A copy of rec with `kind` in every cell that must not be read: the values of invalid entries and every column beyond
    n_values."""
    out = np.array(rec, dtype=np.float64, copy=True)
    dead = out[..., 0] == 0.0
    out[..., 1:][dead] = kind
    out[..., 1 + n_values:] = kind
    return out


def gaps(rec, kind, h):
    """A copy of rec with the flags of series 0 (and of the last series, when there are several) set by `kind`: "all" valid,
    "none", "long" = a gap longer than the window in the middle, "ends" = gaps at both ends."""
    rec = rec.copy()
    n = rec.shape[0]
    for i in {0, rec.shape[1] - 1}:
        if kind == "all":
            rec[:, i, 0] = 1.0
        elif kind == "none":
            rec[:, i, 0] = 0.0
        elif kind == "long":
            a = max(0, n // 2 - h - 2)
            rec[:, i, 0] = 1.0
            rec[a:a + 2 * h + 3, i, 0] = 0.0
        elif kind == "ends":
            k = min(n, h + 2)
            rec[:, i, 0] = 1.0
            rec[:k, i, 0] = 0.0
            rec[n - k:, i, 0] = 0.0
    return rec


def dyadic_half(h, seed):
    """h + 1 weights k / 8, 1 <= k <= 8 (the centre first)."""
    return np.random.default_rng(seed).integers(1, 9, h + 1) / 8.0


def dyadic_case(n, s, cols, n_values, seed, drop=0.2, kind=1e300):
    """rec [n, s, cols], carrier [4, n]: carrier k / 8 with |k| <= 8 (hand-made: the entry takes any finite carrier), values
    k / 16 with |k| <= 32: every order of summation is exact.  `kind`: what `poison` writes into every cell that must not be
    read (None: ordinary numbers stay there)."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.integers(-32, 33, (n, s, cols - 1)) / 16.0
    carrier = r.integers(-8, 9, (4, n)) / 8.0
    return (rec if kind is None else poison(rec, n_values, kind)), carrier


def random_case(n, s, cols, n_values, seed, nu=0.0837, drop=0.2, kind=np.nan):
    """The same shapes with float content: a true carrier, values of mixed sign over six decades."""
    from vbs_amd import spectra
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.standard_normal((n, s, cols - 1)) * 10.0 ** r.uniform(-3, 3, (n, s, cols - 1))
    return (rec if kind is None else poison(rec, n_values, kind)), spectra.carrier(n, nu)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    # a NaN for a NaN: IEEE 754 leaves the sign and payload of a NaN that an operation hands on to the implementation
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {got[i]!r} != {want[i]!r}")


# ---- hand-built moments: the fit's rules -------------------------------------------------------------------------------------------
HAND_SW, HAND_COVERAGE, HAND_DET_MIN = 32.0, 0.375, 0.1875        # need = 12 exactly


def hand_moments():
    """mom [1, 10, 9] for (sw, min_coverage, det_min) = (32, 3/8, 3/16).  Unless set, W = 16 and the carrier sums are zero, so
    CC = SS = 8, CS = S2 / 2, det = 64 - S2^2 / 4 against the edge 3/16 * 256 = 48, all exact; X = 4, XC = 2, XS = -1, XX = 3:
      0  the plain case: a = 0.25, b = -0.125, p = 0.625, c0 = 0.25, M2 = 2;
      1  W = 0: not ok (0 / 0 inside never reaches the output);
      2  W = 12 = need exactly: ok;    3  W one ulp below need: not ok;    4  W one ulp above: ok;
      5  S2 = 8: det == 48 exactly, NOT ok;    6  S2 = 7.75: ok;
      7  a NaN XC: ok, a, b, p, c0 NaN, M2 = 2;
      8  M2 < p (XX = 1.5: M2 = 0.5 under p = 0.625: rounding and weights can do this; nothing clamps it);
      9  nonzero C1, S1 (the mean is taken out of the numerators and c0 differs from the mean)."""
    mom = np.zeros((1, 10, 9))
    mom[0, :] = (16.0, 0.0, 0.0, 0.0, 0.0, 4.0, 2.0, -1.0, 3.0)
    mom[0, 1, 0] = 0.0
    mom[0, 2, 0] = 12.0
    mom[0, 3, 0] = np.nextafter(12.0, 0.0)
    mom[0, 4, 0] = np.nextafter(12.0, 20.0)
    mom[0, 5, 4] = 8.0
    mom[0, 6, 4] = 7.75
    mom[0, 7, 6] = np.nan
    mom[0, 8, 8] = 1.5
    mom[0, 9, 1], mom[0, 9, 2] = 1.5, -0.75
    return mom


def check_hand(fit):
    """What `hand_moments` must give, on either side."""
    assert fit.shape == (1, 10, 6)
    assert fit[0, 0].tolist() == [1.0, 0.25, -0.125, 0.625, 0.25, 2.0]
    assert fit[0, 1].tolist() == [0.0] * 6 and fit[0, 3].tolist() == [0.0] * 6 and fit[0, 5].tolist() == [0.0] * 6
    assert fit[0, 2, 0] == 1.0 and fit[0, 4, 0] == 1.0 and fit[0, 6, 0] == 1.0
    assert fit[0, 7, 0] == 1.0 and np.isnan(fit[0, 7, 1:5]).all() and fit[0, 7, 5] == 2.0
    assert fit[0, 8, 0] == 1.0 and fit[0, 8, 5] == 0.5 and fit[0, 8, 3] == 0.625
    assert fit[0, 9, 0] == 1.0 and fit[0, 9, 4] != 0.25


# ---- the fit's cases: ENV_TOL -------------------------------------------------------------------------------------------------------
ENV_SIZES, ENV_HALVES, ENV_NUS = (64, 197, 600), (3, 7, 24, 40), (0.05, 0.0837)


def burst_envelope(n):
    """Quiet 0.02, a Gaussian burst of 0.4 around 0.45 n (sigma 0.04 n), steady 0.15 after it."""
    f = np.arange(n, dtype=np.float64)
    z = (f - 0.45 * n) / (0.04 * n)
    return 0.02 + 0.13 * 0.5 * (1.0 + np.tanh(z)) + 0.4 * np.exp(-0.5 * z * z)


def burst_case(n, nu, seed, drop=0.03, noise=0.005):
    """A series for the fit: the burst envelope on a line at nu, noise and a small drift, `drop` of the frames missing.
    -> (rec [n, 1, 2], carrier [4, n])."""
    from vbs_amd import spectra
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    x = burst_envelope(n) * np.cos(2 * np.pi * nu * f - 0.9) + 0.01 + 2e-5 * f + noise * r.standard_normal(n)
    rec = np.zeros((n, 1, 2))
    rec[:, 0, 0] = (r.random(n) >= drop).astype(np.float64)
    rec[:, 0, 1] = x
    return rec, spectra.carrier(n, nu)


def env_difference(n, h, nu):
    """The largest |c0, a, b difference| over the ok frames between `window_fit` (fed `moments`) and `lstsq_window` on
    `burst_case(n, nu)` under a Hann window of half width h, and the smallest det / W^2 among those frames."""
    from vbs_amd import spectra
    from vbs_amd.filters import half_taps
    rec, car = burst_case(n, nu, seed=1000 + n + h)
    half = half_taps(spectra.window_taps(h))
    mom = moments(rec, car, half, 1)
    fit = window_fit(mom, taps_sum(half))
    worst, cond = 0.0, np.inf
    for f in np.nonzero(fit[:, 0, 0])[0]:
        c0, a, b = lstsq_window(rec[:, 0, 1], rec[:, 0, 0] != 0.0, car, half, int(f))
        worst = max(worst, abs(fit[f, 0, 4] - c0), abs(fit[f, 0, 1] - a), abs(fit[f, 0, 2] - b))
        W, C1, S1, C2, S2 = mom[f, 0, :5]
        cond = min(cond, ((0.5 * (W + C2) - C1 * C1 / W) * (0.5 * (W - C2) - S1 * S1 / W) - (0.5 * S2 - C1 * S1 / W) ** 2) / (W * W))
    return worst, cond


_ENV_TOL = []


def env_tol():
    """ENV_TOL: 10 x the largest `env_difference` over ENV_SIZES x ENV_HALVES x ENV_NUS, measured between the two references (never
    against the device); the 10 is the project's standing margin for a bound taken from a measurement.  Computed once."""
    if not _ENV_TOL:
        _ENV_TOL.append(10.0 * max(env_difference(n, h, nu)[0] for n in ENV_SIZES for h in ENV_HALVES for nu in ENV_NUS))
    return _ENV_TOL[0]


# ---- a synthetic recording: an oscillation switched on at frame 90 ---------------------------------------------------------------------
ON_NU0, ON_FRAME, ON_AMP, ON_HALF, ON_LOUD = 0.08, 90, 0.3, 16, 17


def switch_on_table(side=7, n=197, seed=0, drop=0.02):
    """-> (table float32 [n, side^2, 10], gain float64 [side^2]): nodes on a side x side grid; marker i moves in Z by
    env_i(f) cos(2 pi ON_NU0 f - phi_i), env_i = 0 before ON_FRAME and gain_i ON_AMP from it on, gain_i falling off with the
    distance from marker ON_LOUD (gain 1 there, the largest), phi_i its polar angle.  `drop` of the entries are missing, flags
    cleared and values left as garbage, in bad frames as on a real recording (12 % of the frames, frame 0 never)."""
    r = np.random.default_rng(seed)
    m = side * side
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    c = (side - 1) / 2.0
    phi = np.arctan2(y0 - c, x0 - c)
    gain = 1.0 / (1.0 + 0.25 * ((x0 - x0[ON_LOUD]) ** 2 + (y0 - y0[ON_LOUD]) ** 2))
    f = np.arange(n, dtype=np.float64)
    env = np.where(f >= ON_FRAME, ON_AMP, 0.0)[:, None] * gain[None, :]
    dz = env * np.cos(2 * np.pi * ON_NU0 * f[:, None] - phi[None, :])
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    t[..., 6], t[..., 7], t[..., 8] = x0[None, :], y0[None, :], 10.0 + dz
    bad = r.random(n) < 0.12
    bad[0] = False
    gone = bad[:, None] & (r.random((n, m)) < drop / 0.12)
    t[gone, 0] = 0.0
    t[gone, 6:9] = 1e30
    return t, gain
