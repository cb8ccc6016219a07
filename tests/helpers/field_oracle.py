"""NumPy restatement of the contact maps (`include/vbs.h`: vbs_field_map_f64, vbs_patch_stats_f64), the exact side, the bound and
the generators the tests of both share.

The map.  The interface does NOT fix the order of summation, so there are two references:
  * `field_map`: float64, sums in ascending m over the selected slots, products rounded (no fused multiply-add).  One admissible
    order among many; the device need not equal it bit for bit - EXCEPT where every order is exact (`dyadic_case`: W in multiples
    of 2^-8 within [0, 1], x in multiples of 2^-10 with |x| <= 64, s <= 1024: a product has at most 8 + 16 = 24 significant bits
    below 2^6, a sum of 1024 of them at most 34, so no operation rounds, with or without fused multiply-add), where num and den
    are exact and the one rounded division makes the quotient bit for bit NumPy's.
  * `exact_map`: `fractions`, no rounding at all: num / den as a rational, and A = sum W |x|, d = sum W.
The bound (`bound`), derived in DESIGN 4.14 for ANY order of summation of s terms with or without fused multiply-add, zero padding
adding nothing:  |value - num / den| <= (2 gamma_(s+6) + 2 u) A / d,  u = 2^-53, gamma_k = k u / (1 - k u).  It is evaluated in
rationals and compared in rationals (`check_within_bound`), so the check itself rounds nothing.
The coverage decision `den >= min_coverage * wsum[p]` is one rounded product and one comparison on either side, but den itself
depends on the order: a test that compares flags first asserts ON THE REFERENCE that no decision lies within 1e-9 relative of its
edge (`coverage_margin`), far above the bound on den (gamma_1030 ~ 1.2e-13).

The patch statistics restate the device's IEEE operations in its order (lane l of 64 adds points l, l + 64, .. ascending, the 64
lane sums fold 32, 16, 8, 4, 2, 1) and are compared bit for bit."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
PATCH_COLS = 8


# ---- the map -------------------------------------------------------------------------------------------------------------------
def field_map(rec, W, wsum, min_coverage, n_values, frame_range=None):
    """-> map [b-a, P, 1 + n_values] as vbs_field_map_f64 states it, sums in ascending m over the valid slots."""
    rec, W, wsum = np.asarray(rec, np.float64), np.asarray(W, np.float64), np.asarray(wsum, np.float64)
    n, s, _ = rec.shape
    a, b = (0, n) if frame_range is None else frame_range
    P = W.shape[0]
    out = np.zeros((b - a, P, 1 + n_values))
    need = np.float64(min_coverage) * wsum
    for f in range(a, b):
        den = np.zeros(P)
        num = np.zeros((P, n_values))
        for m in range(s):
            if rec[f, m, 0] != 0.0:                              # selected: an invalid row is never read
                den = den + W[:, m]
                for v in range(n_values):
                    num[:, v] = num[:, v] + W[:, m] * rec[f, m, 1 + v]
        ok = (den > 0.0) & (den >= need)
        out[f - a, :, 0] = ok
        with np.errstate(divide="ignore", invalid="ignore"):
            out[f - a, :, 1:] = np.where(ok[:, None], num / den[:, None], 0.0)
    return out


def exact_map(rec, W, n_values, frame_range=None):
    """-> (value, A, d): object arrays of Fractions [b-a, P, n_values], [b-a, P, n_values], [b-a, P]; value is None where d == 0."""
    rec, W = np.asarray(rec, np.float64), np.asarray(W, np.float64)
    n, s, _ = rec.shape
    a, b = (0, n) if frame_range is None else frame_range
    P = W.shape[0]
    Wf = [[Fraction(float(W[p, m])) for m in range(s)] for p in range(P)]
    value = np.empty((b - a, P, n_values), dtype=object)
    A = np.empty((b - a, P, n_values), dtype=object)
    d = np.empty((b - a, P), dtype=object)
    for f in range(a, b):
        live = [m for m in range(s) if rec[f, m, 0] != 0.0]
        xs = {m: [Fraction(float(rec[f, m, 1 + v])) for v in range(n_values)] for m in live}
        for p in range(P):
            row = Wf[p]
            den = sum((row[m] for m in live), Fraction(0))
            d[f - a, p] = den
            for v in range(n_values):
                num = sum((row[m] * xs[m][v] for m in live), Fraction(0))
                A[f - a, p, v] = sum((row[m] * abs(xs[m][v]) for m in live), Fraction(0))
                value[f - a, p, v] = num / den if den > 0 else None
    return value, A, d


def gamma(k):
    return k * U / (1 - k * U)


def bound(s, A, d):
    """(2 gamma_(s+6) + 2 u) A / d as a Fraction."""
    return (2 * gamma(s + 6) + 2 * U) * A / d


def coverage_margin(d, wsum, min_coverage):
    """The smallest relative distance of an exact den from its coverage edge min_coverage * wsum[p] (over points with wsum > 0;
    a point with zero row weight has den = 0 exactly and is never ok, on any side)."""
    best = None
    for f in range(d.shape[0]):
        for p in range(d.shape[1]):
            edge = Fraction(float(min_coverage)) * Fraction(float(wsum[p]))
            if edge > 0:
                rel = abs(d[f, p] - edge) / edge
                best = rel if best is None or rel < best else best
    return best


def check_within_bound(got, rec, W, wsum, min_coverage, n_values, frame_range=None, what=""):
    """Every entry of `got` against `exact_map`: flags equal (the caller has asserted the margin), every value of an ok point
    within the bound, zeros elsewhere.  No entry is skipped.  Returns the largest error / bound ratio seen (a float, to print)."""
    value, A, d = exact_map(rec, W, n_values, frame_range)
    s = np.asarray(rec).shape[1]
    worst = 0.0
    for f in range(d.shape[0]):
        for p in range(d.shape[1]):
            ok = d[f, p] > 0 and d[f, p] >= Fraction(float(min_coverage)) * Fraction(float(wsum[p]))
            assert got[f, p, 0] == (1.0 if ok else 0.0), f"{what}: flag of frame {f} point {p}"
            for v in range(n_values):
                g = got[f, p, 1 + v]
                if not ok:
                    assert g == 0.0, f"{what}: frame {f} point {p} value {v} is {g} where not ok"
                    continue
                assert np.isfinite(g), f"{what}: frame {f} point {p} value {v} is {g}"
                err, lim = abs(Fraction(float(g)) - value[f, p, v]), bound(s, A[f, p, v], d[f, p])
                assert err <= lim, f"{what}: frame {f} point {p} value {v}: error {float(err):.3e} above the bound {float(lim):.3e}"
                if lim > 0:
                    worst = max(worst, float(err / lim))
    return worst


# ---- generators ----------------------------------------------------------------------------------------------------------------
def poison(rec, n_values, kind=np.nan):
    """A copy of rec with `kind` in every cell that must not be read: the values of invalid rows and every column beyond n_values."""
    out = np.array(rec, dtype=np.float64, copy=True)
    dead = out[..., 0] == 0.0
    out[..., 1:][dead] = kind
    out[..., 1 + n_values:] = kind
    return out


def dyadic_case(F, P, s, cols, n_values, seed, drop=0.2, kind=1e300):
    """rec [F, s, cols], W [P, s], wsum [P]: W in multiples of 2^-8 within [0, 1] (a third of them 0), x in multiples of 2^-10
    with |x| <= 64: every order of summation is exact.  wsum is the exact row sum.  `kind`: what `poison` writes into every cell
    that must not be read (None: ordinary numbers are left there)."""
    r = np.random.default_rng(seed)
    rec = np.zeros((F, s, cols))
    rec[..., 0] = (r.random((F, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.integers(-65536, 65537, (F, s, cols - 1)) / 1024.0
    W = r.integers(0, 257, (P, s)) / 256.0
    W[r.random((P, s)) < 1 / 3] = 0.0
    return (rec if kind is None else poison(rec, n_values, kind)), W, W.sum(axis=1)


def random_case(F, P, s, cols, n_values, seed, drop=0.2, kind=np.nan):
    """The same shapes with float content: Gaussian-like weights with exact zeros, values of mixed sign over six decades."""
    r = np.random.default_rng(seed)
    rec = np.zeros((F, s, cols))
    rec[..., 0] = (r.random((F, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.standard_normal((F, s, cols - 1)) * 10.0 ** r.uniform(-3, 3, (F, s, cols - 1))
    W = np.exp(-r.uniform(0.0, 6.0, (P, s)))
    W[r.random((P, s)) < 1 / 3] = 0.0
    wsum = np.zeros(P)
    for m in range(s):
        wsum = wsum + W[:, m]
    return (rec if kind is None else poison(rec, n_values, kind)), W, wsum


# ---- the patch statistics --------------------------------------------------------------------------------------------------------
def _fold(lanes):
    a = np.array(lanes, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        a[:off] = a[:off] + a[off:2 * off]
    return a[0]


def patch_stats(mp, grid_xy, component, sign, thr):
    """-> patch [F, 8] exactly as vbs_patch_stats_f64 states it; thr is what the entry takes (squared for component -1)."""
    mp, g = np.asarray(mp, np.float64), np.asarray(grid_xy, np.float64)
    F, P, oc = mp.shape
    nv = oc - 1
    out = np.zeros((F, PATCH_COLS))
    sign, thr = np.float64(sign), np.float64(thr)
    for f in range(F):
        S, Sx, Sy = np.zeros(64), np.zeros(64), np.zeros(64)
        covered = count = 0
        peak, pidx = None, -1
        with np.errstate(all="ignore"):
            for p in range(P):
                e = mp[f, p]
                if e[0] == 0.0:
                    continue
                covered += 1
                if component >= 0:
                    sc = sign * e[1 + component]
                else:
                    sc = e[1] * e[1]
                    for v in range(1, nv):
                        sc = sc + e[1 + v] * e[1 + v]
                if not (sc >= thr):
                    continue
                count += 1
                lane = p & 63
                S[lane] = S[lane] + sc
                Sx[lane] = Sx[lane] + sc * g[p, 0]
                Sy[lane] = Sy[lane] + sc * g[p, 1]
                if pidx < 0 or sc > peak:                       # ascending p: the earliest of equal maxima stays
                    peak, pidx = sc, p
            s, sx, sy = _fold(S), _fold(Sx), _fold(Sy)
            centre = covered > 0 and count > 0 and s > 0.0
            out[f] = (0.0 if covered == 0 else 2.0 if centre else 1.0, covered, count, s, sx / s if centre else 0.0,
                      sy / s if centre else 0.0, peak if centre else 0.0, pidx if centre else (0.0 if covered == 0 else -1.0))
    return out


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    same = got.view(np.uint64) == want.view(np.uint64)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {got[i]!r} != {want[i]!r}")


# ---- a synthetic recording: a Gaussian dimple moving over a node grid ---------------------------------------------------------------
def dimple_table(side=13, n=24, pitch=1.0, depth=0.8, width=1.6, seed=0, drop=0.02):
    """-> (table float32 [n, side^2, 10], centres float64 [n, 2]): nodes on a side x side grid of `pitch`; in frame f > 0 a dimple
    dZ = depth exp(-r^2 / 2 width^2) whose centre walks along a diagonal of the inner part; frame 0 is at rest and complete;
    `drop` of the other entries are missing (flags cleared, values left as garbage)."""
    r = np.random.default_rng(seed)
    m = side * side
    gx, gy = np.meshgrid(np.arange(side) * pitch, np.arange(side) * pitch)
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    t = np.zeros((n, m, 10), dtype=np.float32)
    lo, hi = 3.0 * pitch, (side - 4.0) * pitch
    cen = np.stack([np.linspace(lo, hi, n), np.linspace(hi, lo, n) * 0.5 + (lo + hi) * 0.25], axis=1)
    for f in range(n):
        r2 = (x0 - cen[f, 0]) ** 2 + (y0 - cen[f, 1]) ** 2
        dz = depth * np.exp(-r2 / (2 * width * width)) if f > 0 else np.zeros(m)
        t[f, :, 0] = 3.0
        t[f, :, 6], t[f, :, 7], t[f, :, 8] = x0, y0, 10.0 + dz
    gone = r.random((n, m)) < drop
    gone[0] = False
    t[gone, 0] = 0.0
    t[gone, 6:9] = 1e30
    return t, cen
