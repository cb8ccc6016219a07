"""NumPy restatement of the displacement spectra (`include/vbs.h`: vbs_project_series_f64, vbs_harmonic_fit_f64), the exact side,
the bound and the generators the tests of both share.

The projection.  The interface does NOT fix the order of summation, so there are two references:
  * `project`: float64, sums in ascending f over the valid frames, products rounded (no fused multiply-add).  One admissible
    order among many; the device need not equal it bit for bit - EXCEPT where every order is exact (`dyadic_case`: basis in
    multiples of 1/8 with |k| <= 16, x in multiples of 1/16 with |k| <= 32, n <= 300: a product is a multiple of 2^-7 below 2^2,
    a sum of 300 of them below 2^11, 18 significant bits: no operation rounds, with or without fused multiply-add).
  * `exact_project`: `fractions`, no rounding at all: den, num, and D = sum |basis|, A = sum |basis x|.
The bound (`bound`), derived in DESIGN 4.15 for ANY order of summation of n terms with or without fused multiply-add, zero padding
adding nothing:  |num^ - num| <= gamma_(n+6) A,  |den^ - den| <= gamma_(n+6) D,  u = 2^-53, gamma_k = k u / (1 - k u).  It is
evaluated in rationals and compared in rationals (`check_within_bound`), so the check itself rounds nothing.

The fit (`harmonic_fit`) restates the expressions of the header verbatim in scalar float64, one IEEE operation after the other in
the order written (NumPy scalars never contract), and is compared bit for bit."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
PEAK_COLS = 7


# ---- the projection ------------------------------------------------------------------------------------------------------------
def project(rec, basis, n_values):
    """-> proj [s, R, 1 + n_values] as vbs_project_series_f64 states it, sums in ascending f over the valid frames."""
    rec, basis = np.asarray(rec, np.float64), np.asarray(basis, np.float64)
    n, s, _ = rec.shape
    R = basis.shape[0]
    out = np.zeros((s, R, 1 + n_values))
    for i in range(s):
        for f in range(n):
            if rec[f, i, 0] != 0.0:                              # selected: an invalid entry is never read
                out[i, :, 0] = out[i, :, 0] + basis[:, f]
                for v in range(n_values):
                    out[i, :, 1 + v] = out[i, :, 1 + v] + basis[:, f] * rec[f, i, 1 + v]
    return out


def exact_project(rec, basis, n_values):
    """-> (value, mag): object arrays of Fractions [s, R, 1 + n_values]: (den, num ..) and (D, A ..), the sums of the magnitudes."""
    rec, basis = np.asarray(rec, np.float64), np.asarray(basis, np.float64)
    n, s, _ = rec.shape
    R = basis.shape[0]
    Bf = [[Fraction(float(basis[r, f])) for f in range(n)] for r in range(R)]
    value = np.empty((s, R, 1 + n_values), dtype=object)
    mag = np.empty((s, R, 1 + n_values), dtype=object)
    for i in range(s):
        live = [f for f in range(n) if rec[f, i, 0] != 0.0]
        xs = {f: [Fraction(float(rec[f, i, 1 + v])) for v in range(n_values)] for f in live}
        for r in range(R):
            row = Bf[r]
            value[i, r, 0] = sum((row[f] for f in live), Fraction(0))
            mag[i, r, 0] = sum((abs(row[f]) for f in live), Fraction(0))
            for v in range(n_values):
                value[i, r, 1 + v] = sum((row[f] * xs[f][v] for f in live), Fraction(0))
                mag[i, r, 1 + v] = sum((abs(row[f] * xs[f][v]) for f in live), Fraction(0))
    return value, mag


def gamma(k):
    return k * U / (1 - k * U)


def bound(n, mag):
    """gamma_(n+6) * (sum of magnitudes) as a Fraction."""
    return gamma(n + 6) * mag


def check_within_bound(got, rec, basis, n_values, what=""):
    """Every entry of `got` against `exact_project` within the bound; where the bound is zero (no valid frame, an all-zero row) the
    entry is an exact zero.  No entry is skipped.  Returns the largest error / bound ratio seen (a float, to print)."""
    value, mag = exact_project(rec, basis, n_values)
    n = np.asarray(rec).shape[0]
    got = np.asarray(got)
    assert got.shape == value.shape, f"{what}: shape {got.shape} != {value.shape}"
    worst = 0.0
    for idx in np.ndindex(*value.shape):
        g = got[idx]
        assert np.isfinite(g), f"{what}: entry {idx} is {g}"
        err, lim = abs(Fraction(float(g)) - value[idx]), bound(n, mag[idx])
        assert err <= lim, f"{what}: entry {idx}: error {float(err):.3e} above the bound {float(lim):.3e}"
        if lim > 0:
            worst = max(worst, float(err / lim))
    return worst


# ---- the fit -----------------------------------------------------------------------------------------------------------------
def harmonic_fit(proj, Q, min_count, det_min):
    """-> (fit [s, Q, 1 + 3 nv], peak [s, nv, 7]) exactly as vbs_harmonic_fit_f64 states them."""
    proj = np.asarray(proj, np.float64)
    s, R, oc = proj.shape
    nv = oc - 1
    assert R == 1 + 4 * Q
    fit = np.zeros((s, Q, 1 + 3 * nv))
    peak = np.zeros((s, nv, PEAK_COLS))
    half, dm, mc = np.float64(0.5), np.float64(det_min), np.float64(min_count)
    with np.errstate(all="ignore"):
        for i in range(s):
            P = proj[i]
            N = P[0, 0]
            enough = bool(N >= mc)
            m = [P[0, 1 + v] / N if enough else np.float64(0.0) for v in range(nv)]
            best = [(-1, np.float64(0.0), np.float64(0.0), np.float64(0.0)) for _ in range(nv)]      # bin, p, a, b
            for q in range(Q):
                c1, s1 = P[1 + 2 * q, 0], P[2 + 2 * q, 0]
                c2, s2 = P[1 + 2 * Q + 2 * q, 0], P[2 + 2 * Q + 2 * q, 0]
                CC = half * (N + c2) - (c1 * c1) / N
                SS = half * (N - c2) - (s1 * s1) / N
                CS = half * s2 - (c1 * s1) / N
                det = CC * SS - CS * CS
                ok = enough and bool(det > dm * (N * N))
                if not ok:
                    continue
                fit[i, q, 0] = 1.0
                for v in range(nv):
                    pc = P[1 + 2 * q, 1 + v] - m[v] * c1
                    ps = P[2 + 2 * q, 1 + v] - m[v] * s1
                    a = (pc * SS - ps * CS) / det
                    b = (ps * CC - pc * CS) / det
                    p = a * pc + b * ps
                    fit[i, q, 1 + 3 * v:4 + 3 * v] = (a, b, p)
                    if not np.isnan(p) and (best[v][0] < 0 or p > best[v][1]):     # ascending q: the earliest of equal maxima stays
                        best[v] = (q, p, a, b)
            for v in range(nv):
                q, p, a, b = best[v]
                if not enough:
                    peak[i, v] = (0.0, N, 0.0, -1.0, 0.0, 0.0, 0.0)
                elif q < 0:
                    peak[i, v] = (1.0, N, m[v], -1.0, 0.0, 0.0, 0.0)
                else:
                    peak[i, v] = (2.0, N, m[v], q, a, b, p)
    return fit, peak


def lstsq_fit(x, valid, nu):
    """np.linalg.lstsq of x over the valid frames on [1, cos, sin] of 2 pi nu f -> (c0, a, b): the independent reference of the fit."""
    f = np.nonzero(valid)[0].astype(np.float64)
    th = 2.0 * np.pi * nu * f
    A = np.stack([np.ones_like(f), np.cos(th), np.sin(th)], axis=1)
    return np.linalg.lstsq(A, np.asarray(x, np.float64)[np.asarray(valid, bool)], rcond=None)[0]


# ---- generators ----------------------------------------------------------------------------------------------------------------
def poison(rec, n_values, kind=np.nan):
    """A copy of rec with `kind` in every cell that must not be read: the values of invalid entries and every column beyond
    n_values."""
    out = np.array(rec, dtype=np.float64, copy=True)
    dead = out[..., 0] == 0.0
    out[..., 1:][dead] = kind
    out[..., 1 + n_values:] = kind
    return out


def with_edges(rec, basis):
    """An all-invalid series (the last, when there are several), an all-invalid frame (the second, when there are several) and an
    all-zero basis row (the last, when there are several)."""
    rec, basis = rec.copy(), basis.copy()
    if rec.shape[1] > 1:
        rec[:, -1, 0] = 0.0
    if rec.shape[0] > 1:
        rec[1, :, 0] = 0.0
    if basis.shape[0] > 1:
        basis[-1] = 0.0
    return rec, basis


def dyadic_case(n, R, s, cols, n_values, seed, drop=0.2, kind=1e300):
    """rec [n, s, cols], basis [R, n]: basis k / 8 with |k| <= 16, values k / 16 with |k| <= 32, n <= 300: every order of
    summation is exact.  `kind`: what `poison` writes into every cell that must not be read (None: ordinary numbers stay there)."""
    assert n <= 300
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.integers(-32, 33, (n, s, cols - 1)) / 16.0
    basis = r.integers(-16, 17, (R, n)) / 8.0
    return (rec if kind is None else poison(rec, n_values, kind)), basis


def random_case(n, R, s, cols, n_values, seed, drop=0.2, kind=np.nan):
    """The same shapes with float content: a basis of mixed sign within [-1, 1] (what sines are), values of mixed sign over six
    decades."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.standard_normal((n, s, cols - 1)) * 10.0 ** r.uniform(-3, 3, (n, s, cols - 1))
    basis = np.cos(r.uniform(0.0, 2.0 * np.pi, (R, n)))
    return (rec if kind is None else poison(rec, n_values, kind)), basis


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    # a NaN for a NaN: IEEE 754 leaves the sign and payload of a NaN that an operation hands on to the implementation (x - NaN keeps
    # the operand's sign on the host and not on the device), so those bits are no property of the code under test
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {got[i]!r} != {want[i]!r}")


# ---- hand-built projections: the fit's rules ---------------------------------------------------------------------------------------
HAND_Q, HAND_MIN_COUNT, HAND_DET_MIN = 70, 8, 0.1875


def hand_proj():
    """proj [6, 1 + 4 * 70, 3] for (min_count, det_min) = (8, 3/16), N = 16 and the sums of the basis zero unless set, so that
    CC = SS = 8, CS = s2 / 2, det = 64 - s2^2 / 4 against the edge 3/16 * 256 = 48, and p = (pc^2 + ps^2) / 8, all exact:
      series 0  value 1 has the same largest power in bins 69, 5 and 40 (5 and 69 meet in one lane): bin 5 wins;
      series 1  value 1 has a NaN numerator in bin 2 and the largest finite power in bin 7: the NaN neither wins nor suppresses;
                value 2 is the same in every bin: bin 0 wins;
      series 2  bin 3 has s2 = 8: det == 48 exactly, NOT ok, though its numerator is the largest; bin 4 (s2 = 7.75) is ok and wins;
      series 3  N = min_count - 1: flag 0, mean 0, no fit;
      series 4  s2 = 8 in every bin: no ok bin, flag 1;
      series 5  nonzero c1, s1 (the mean is taken out of the numerators) and a peak in bin 33."""
    Q = HAND_Q
    proj = np.zeros((6, 1 + 4 * Q, 3))
    proj[:, 0] = (16.0, 4.0, -8.0)
    proj[:, 1:1 + 2 * Q, 1], proj[:, 1:1 + 2 * Q, 2] = 0.125, 0.0625
    for q in (69, 5, 40):
        proj[0, 1 + 2 * q, 1], proj[0, 2 + 2 * q, 1] = 2.0, -1.0
    proj[1, 1 + 2 * 2, 1], proj[1, 1 + 2 * 7, 1] = np.nan, 1.0
    proj[2, 2 + 2 * Q + 2 * 3, 0], proj[2, 1 + 2 * 3, 1] = 8.0, 4.0
    proj[2, 2 + 2 * Q + 2 * 4, 0], proj[2, 1 + 2 * 4, 1] = 7.75, 3.0
    proj[3, 0, 0] = HAND_MIN_COUNT - 1.0
    proj[4, 2 + 2 * Q::2, 0] = 8.0
    proj[5, 1:1 + 2 * Q:2, 0], proj[5, 2:2 + 2 * Q:2, 0], proj[5, 1 + 2 * 33, 1] = 1.5, -0.75, 2.5
    return proj


def check_hand(fit, peak):
    """What `hand_proj` must give, on either side."""
    assert peak[0, 0].tolist() == [2.0, 16.0, 0.25, 5.0, 0.25, -0.125, 0.625]
    assert peak[1, 0, 3] == 7.0 and peak[1, 0, 0] == 2.0 and np.isnan(fit[1, 2, 3]) and fit[1, 2, 0] == 1.0
    assert peak[1, 1, 3] == 0.0 and peak[1, 1, 2] == -0.5
    assert fit[2, 3].tolist() == [0.0] * 7 and fit[2, 4, 0] == 1.0 and peak[2, 0, 3] == 4.0
    assert peak[3].tolist() == [[0.0, 7.0, 0.0, -1.0, 0.0, 0.0, 0.0]] * 2 and not fit[3].any()
    assert peak[4].tolist() == [[1.0, 16.0, 0.25, -1.0, 0.0, 0.0, 0.0], [1.0, 16.0, -0.5, -1.0, 0.0, 0.0, 0.0]] and not fit[4].any()
    assert peak[5, 0, 3] == 33.0 and fit[5, :, 0].all()


def low_frequency_case(n=200):
    """A complete series and the two frequencies 0.2 / n and 0.5 / n: a fifth of a period cannot be told from the mean
    (det / N^2 ~ 4e-4, under det_min = 1e-3: not ok), half a period can (0.047).  -> (rec [n, 1, 2], freqs [2])."""
    f = np.arange(n, dtype=np.float64)
    rec = np.ones((n, 1, 2))
    rec[:, 0, 1] = 0.3 + 0.5 * np.cos(2 * np.pi * 0.5 / n * f - 0.4)
    return rec, np.array([0.2 / n, 0.5 / n])


# ---- a synthetic recording: a load running round the node grid -------------------------------------------------------------------
LINE_NU0, LINE_AMP, LINE_TAPS = 0.08, 0.7, 25


def line_table(side=13, n=197, seed=0, drop=0.02):
    """-> (table float32 [n, side^2, 10], phi float64 [side^2]): nodes on a side x side grid; marker i moves in Z by
    LINE_AMP cos(2 pi LINE_NU0 f - phi_i), phi_i its polar angle about the grid's centre (the centre marker: 0), plus a slow tilt
    drift proportional to its x (a trend whose sum over the grid is zero, to be removed by a moving average of LINE_TAPS = two
    periods).  `drop` of the entries are missing, flags cleared and values left as garbage; as on a real recording they come in
    bad frames - 12 % of the frames, frame 0 never, lose `drop` / 0.12 of their markers - so that the per-frame total keeps
    its complete frames."""
    r = np.random.default_rng(seed)
    m = side * side
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    c = (side - 1) / 2.0
    phi = np.arctan2(y0 - c, x0 - c)
    f = np.arange(n, dtype=np.float64)
    u = f / n
    dz = LINE_AMP * np.cos(2 * np.pi * LINE_NU0 * f[:, None] - phi[None, :]) + 0.05 * ((x0 - c) / c)[None, :] * (u + u * u)[:, None]
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    t[..., 6], t[..., 7], t[..., 8] = x0[None, :], y0[None, :], 10.0 + dz
    bad = r.random(n) < 0.12
    bad[0] = False
    gone = bad[:, None] & (r.random((n, m)) < drop / 0.12)
    t[gone, 0] = 0.0
    t[gone, 6:9] = 1e30
    return t, phi


# ---- the fit's cases -------------------------------------------------------------------------------------------------------------
FIT_NU0 = 0.0837
FIT_BINS = 33


def fit_case(n, seed, drop=0.03):
    """A series for the fit: a line at FIT_NU0, a small trend and noise, `drop` of the frames missing; the 33-bin zoom grid of
    +- 2 / n round it.  -> (rec [n, 1, 2], freqs [33])."""
    from vbs_amd import spectra
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    x = 0.7 * np.cos(2 * np.pi * FIT_NU0 * f - 0.9) + 0.05 + 2e-4 * f + 0.02 * r.standard_normal(n)
    rec = np.zeros((n, 1, 2))
    rec[:, 0, 0] = (r.random(n) >= drop).astype(np.float64)
    rec[:, 0, 1] = x
    return rec, spectra.zoom_grid(FIT_NU0, 2.0 / n, FIT_BINS)


def fit_difference(n, seed):
    """The largest |a, b difference| over all bins between `harmonic_fit` (fed `project` of `spectra.harmonic_basis`) and
    `lstsq_fit`, on `fit_case(n, seed)`; every bin must be ok."""
    from vbs_amd import spectra
    rec, nu = fit_case(n, seed)
    fit, _ = harmonic_fit(project(rec, spectra.harmonic_basis(n, nu), 1), nu.size, 8, 1e-3)
    assert (fit[0, :, 0] == 1.0).all()
    worst = 0.0
    for q in range(nu.size):
        _, a, b = lstsq_fit(rec[:, 0, 1], rec[:, 0, 0] != 0.0, nu[q])
        worst = max(worst, abs(fit[0, q, 1] - a), abs(fit[0, q, 2] - b))
    return worst


FIT_SIZES = (64, 197, 1000)
_FIT_TOL = []


def fit_tol():
    """FIT_TOL: 10 x the largest `fit_difference` over FIT_SIZES, measured between the two references (never against the device);
    the 10 is the project's standing margin for a bound taken from a measurement.  Computed once."""
    if not _FIT_TOL:
        _FIT_TOL.append(10.0 * max(fit_difference(n, 1000 + n) for n in FIT_SIZES))
    return _FIT_TOL[0]
