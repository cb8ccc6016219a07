"""CPU tests of the local polynomial fit's host side (no GPU): the two new C symbols and their constants, what both entries refuse
before a device is touched, `filters.poly_taps`, `kinematic_analysis`'s argument checks, host arithmetic and sheet, and the NumPy
restatements the GPU tests hold the device to (`tests/helpers/kinematics_oracle.py`): the moments' bit for bit where every order of
summation is exact (with the bit budget of each case) and within the derived bound of exact rational arithmetic otherwise; the
fit's against `np.linalg.lstsq` (KIN_TOL), against scipy's Savitzky-Golay coefficients, on polynomials with gaps and
on hand-built moments."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import _build, filters

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import kinematics_oracle as O                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_constants_and_source_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vbs_poly_moments_f64", "vbs_poly_fit_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    for name in ("KIN_TILE", "KIN_MAX_HALF", "KIN_MAX_DEGREE"):
        assert getattr(L, name) == defs["VBS_" + name], name
    assert (L.KIN_MAX_HALF, L.KIN_MAX_DEGREE) == (filters.KIN_MAX_HALF, filters.KIN_MAX_DEGREE) == (O.MAX_HALF, O.MAX_DEGREE) == (127, 3)
    assert 2 * L.KIN_MAX_HALF + 1 <= L.FIR_MAX_TAPS and L.KIN_TILE % 16 == 0
    assert L.KIN_MAX_HALF ** (2 * L.KIN_MAX_DEGREE) < 2 ** 42      # every power u^k is exact: a tap is rounded once
    assert "k_kinematics.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "k_kinematics.hip"))
    pm, pf = L.lib().vbs_poly_moments_f64, L.lib().vbs_poly_fit_f64
    assert len(pm.argtypes) == 13 and len(pf.argtypes) == 16
    from vbs_amd.engine import KIN_PIV_REL
    assert KIN_PIV_REL == O.PIV_REL == 5e-3


def test_refusals_without_a_gpu():
    """Both C entries decide every refusal before the device is touched: with device pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY.  The weights and thresholds live on the host and are read."""
    lib = L.lib()
    p, nul = C.c_void_p(8), None
    good_half = np.array([1.0, 0.5, 0.25])

    def pm(rec=p, n=10, s=5, cols=4, nv=3, half=good_half, n_half=None, d=2, fb=0, fe=10, out=p):
        hp = None if half is None else np.ascontiguousarray(half, np.float64).ctypes.data_as(C.c_void_p)
        nh = (0 if half is None else len(half)) if n_half is None else n_half
        return lib.vbs_poly_moments_f64(0, rec, n, s, cols, nv, hp, nh, d, fb, fe, out, None)
    for bad in (dict(rec=nul), dict(half=None, n_half=3), dict(out=nul), dict(n=0, fe=0), dict(s=0), dict(n=-1), dict(cols=1), dict(cols=9),
                dict(nv=0), dict(nv=4, cols=8), dict(nv=3, cols=3), dict(n_half=0), dict(half=np.ones(L.KIN_MAX_HALF + 2)),
                dict(half=[1.0, -0.5]), dict(half=[1.0, math.nan]), dict(half=[1.0, math.inf]), dict(half=[0.0, 1.0]), dict(half=[-1.0]),
                dict(d=-1), dict(d=4), dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert pm(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)):
        assert pm(**big) == L.VBS_ECAPACITY, big
        assert pm(**dict(big, rec=nul)) == L.VBS_EINVAL          # a bad argument comes before a capacity
        assert pm(**dict(big, d=4)) == L.VBS_EINVAL

    def pf(mom=p, rec=p, n=10, s=5, cols=4, nv=3, d=2, h=7, thr=(4.0, 0.1, 0.01), fd=1, fb=0, fe=10, fit=p, filled=nul):
        tp = None if thr is None else np.ascontiguousarray(thr, np.float64).ctypes.data_as(C.c_void_p)
        return lib.vbs_poly_fit_f64(0, mom, rec, n, s, cols, nv, d, h, tp, fd, fb, fe, fit, filled, None)
    for bad in (dict(mom=nul), dict(rec=nul), dict(thr=None), dict(fit=nul), dict(n=0, fe=0), dict(s=0), dict(cols=1), dict(cols=9), dict(nv=0),
                dict(nv=3, cols=3), dict(d=-1), dict(d=4), dict(h=-1), dict(h=128), dict(thr=(4.0, -0.1, 0.01)), dict(thr=(math.nan, 0.1, 0.01)),
                dict(thr=(4.0, 0.1, -math.inf)), dict(fd=-1), dict(fd=4), dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert pf(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)):
        assert pf(**big) == L.VBS_ECAPACITY, big
        assert pf(**dict(big, fd=4)) == L.VBS_EINVAL


def test_kin_args():
    from vbs_amd.engine import _kin_args, _kin_fit_args, kin_thresholds, n_kin_sums
    good = dict(n=10, s=5, cols=4, half_window=3, degree=2, window="hann", n_values=None, frame_range=None)
    assert _kin_args(**good) == (3, 2, 3, 0, 10)
    assert _kin_args(**dict(good, cols=8, frame_range=(2, 7), window="rect")) == (3, 2, 3, 2, 7)
    assert _kin_args(**dict(good, cols=2, s=1, frame_range=(4, 4), half_window=0, degree=0)) == (0, 0, 1, 4, 4)
    assert _kin_args(**dict(good, window=np.ones(7))) == (3, 2, 3, 0, 10)
    for bad in (dict(n=0), dict(s=0), dict(cols=1), dict(cols=9), dict(n_values=4, cols=8), dict(n_values=0), dict(n_values=3, cols=3),
                dict(half_window=-1), dict(half_window=128), dict(half_window=2.5), dict(degree=-1), dict(degree=4), dict(degree=1.5),
                dict(window="hamming"), dict(frame_range=(0, 11)), dict(frame_range=(-1, 3)), dict(frame_range=(5, 4))):
        with pytest.raises(ValueError):
            _kin_args(**dict(good, **bad))
    for big, name in ((dict(n=L.PROJ_MAX_FRAMES + 1), "VBS_PROJ_MAX_FRAMES"), (dict(s=L.PROJ_MAX_SLOTS + 1), "VBS_PROJ_MAX_SLOTS")):
        with pytest.raises(L.VbsError, match=name):
            _kin_args(**dict(good, **big))
    assert [n_kin_sums(d, v) for d, v in ((0, 1), (1, 1), (2, 3), (3, 3))] == [3, 6, 17, 22]
    gf = dict(F=10, s=5, M=17, n=10, cols=4, half_window=3, degree=2, window="hann", n_values=None, min_coverage=0.5, piv_rel=5e-3,
              fill_degree=1, frame_range=None)
    h, d, nv, thr, fd, a, b = _kin_fit_args(**gf)
    _, sw, piv = filters.poly_taps(3, 2)
    assert (h, d, nv, fd, a, b) == (3, 2, 3, 1, 0, 10) and thr.tolist() == [0.5 * sw, 5e-3 * piv[1], 5e-3 * piv[2]]
    O.assert_bits(thr, O.thresholds(sw, piv), "thresholds")
    O.assert_bits(kin_thresholds(sw, piv, 0.7, 0.0), O.thresholds(sw, piv, 0.7, 0.0), "thresholds")
    assert _kin_fit_args(**dict(gf, F=4, frame_range=(3, 7), fill_degree=3))[4:] == (3, 3, 7)
    thr = _kin_fit_args(**dict(gf, half_window=1, degree=3, M=22))[3]
    assert np.isfinite(thr[:3]).all() and thr[3] == math.inf      # 3 frames never determine a cubic
    O.assert_bits(thr, O.thresholds(*filters.poly_taps(1, 3)[1:], h=1), "thresholds")
    for bad in (dict(F=9), dict(M=16), dict(min_coverage=0.0), dict(min_coverage=1.5), dict(piv_rel=-1e-9), dict(piv_rel=1.0),
                dict(piv_rel=math.nan), dict(fill_degree=-1), dict(fill_degree=4), dict(fill_degree=0.5), dict(degree=4), dict(n_values=4)):
        with pytest.raises(ValueError):
            _kin_fit_args(**dict(gf, **bad))


@pytest.mark.parametrize("kind", ("hann", "rect"))
def test_poly_taps_equal_the_restatement_bit_for_bit(kind):
    for h in (0, 1, 2, 3, 7, 8, 9, 31, 64, 65, 127):
        for d in range(4):
            tp, sw, piv = filters.poly_taps(h, d, kind)
            want = O.taps(h, d, kind)
            assert tp.shape == (2 * d + 1, 2 * h + 1)
            O.assert_bits(tp, want, f"taps h {h} d {d}")
            sw2, piv2 = O.full_pivots(want, d)
            assert sw == sw2
            O.assert_bits(piv, piv2, f"piv_full h {h} d {d}")       # bit for bit, NaN for NaN
            assert O.scale(h) == filters.poly_scale(h) and O.scale(h) >= max(h, 1) and O.scale(h) < 2 * max(h, 1)
            O.assert_bits(tp[0], O.window(h, kind), "row 0 is the window")
            if 2 * h + 1 > d:
                assert (piv > 0).all()
    w = np.array([0.25, 0.5, 1.0, 0.5, 0.25])
    O.assert_bits(filters.poly_taps(2, 1, w)[0], O.taps(2, 1, w), "weights of the caller's")
    for bad in (lambda: filters.poly_taps(128, 1), lambda: filters.poly_taps(-1, 1), lambda: filters.poly_taps(3, 4), lambda: filters.poly_taps(3, -1),
                lambda: filters.poly_taps(3, 1, "hamming"), lambda: filters.poly_taps(2, 1, np.ones(7)), lambda: filters.poly_taps(1, 1, [1.0, 1.0, 2.0]),
                lambda: filters.poly_taps(1, 1, [1.0, 0.0, 1.0]), lambda: filters.poly_taps(1, 1, [-1.0, 1.0, -1.0])):
        with pytest.raises(ValueError):
            bad()


def test_piv_rel_keeps_every_gap_free_one_sided_window_at_full_degree():
    """DESIGN 4.20's table: D_k(one-sided) / D_k(full) over EVERY h in d + 1 .. 127, both windows, d = 1 .. 3: the smallest ratio lies
    above the default piv_rel."""
    smallest = np.inf
    for kind in ("rect", "hann"):
        for d in (1, 2, 3):
            for h in range(d + 1, 128):
                tp = O.taps(h, d, kind)
                _, piv = O.full_pivots(tp, d)
                D, _ = O.ldl(O.ascending_sums(tp[:, h:]), d)
                smallest = min(smallest, float((D / piv).min()))
    print(f"smallest one-sided / full pivot ratio: {smallest:.4g}")
    assert smallest > O.PIV_REL and 7.9e-3 < smallest < 8.1e-3      # rect, d = 3, h = 127


DYADIC = ((131, 3, 4, 3, 127, 3), (40, 2, 5, 2, 127, 2), (65, 5, 8, 3, 31, 3), (17, 4, 2, 1, 7, 3), (16, 3, 3, 2, 7, 2), (9, 2, 4, 3, 1, 1),
          (5, 1, 2, 1, 0, 0), (20, 3, 4, 3, 3, 3))


@pytest.mark.parametrize("n,s,cols,nv,h,d", DYADIC)
def test_restated_moments_are_exact_on_dyadic_inputs(n, s, cols, nv, h, d):
    rec, w, budget = O.dyadic_case(n, s, cols, nv, h, d, seed=n + h)
    assert budget <= 53                                           # bits(h^2d) + bits(w) + bits(x) + bits(2h + 1)
    tp = O.taps(h, d, w)
    got = O.moments(rec, tp, d, nv)
    sums, _ = O.exact_moments(rec, tp, d, nv)
    for idx in np.ndindex(got.shape):
        assert O.Fraction(float(got[idx])) == sums[idx], idx
    a, b = n // 3, n // 3 + min(5, n - n // 3)
    O.assert_bits(O.moments(rec, tp, d, nv, (a, b)), got[a:b], "a range of the restatement")


@pytest.mark.parametrize("n,s,nv,h,d,kind", ((40, 2, 3, 7, 3, "hann"), (30, 1, 1, 31, 2, "hann"), (25, 2, 2, 3, 1, "rect"), (12, 1, 3, 127, 3, "hann")))
def test_restated_moments_lie_within_the_derived_bound(n, s, nv, h, d, kind):
    rec = O.random_case(n, s, nv + 2, nv, seed=n)
    tp = O.taps(h, d, kind)
    worst = O.check_within_bound(O.moments(rec, tp, d, nv), rec, tp, d, nv, what=f"n {n} h {h} d {d}")
    print(f"largest error / bound = {worst:.3g}")
    assert worst < 1.0


def test_kin_tol_is_ten_times_what_the_two_references_differ_by():
    m = O.kin_measured()
    print(f"largest |fit - lstsq| = {m:.3g}; KIN_TOL = {O.KIN_TOL:.3g}")
    assert 10.0 * m <= O.KIN_TOL <= 40.0 * m


@pytest.mark.parametrize("d", (1, 2, 3))
def test_fit_reproduces_savgol_on_gap_free_interior_rect_windows(d):
    from scipy.signal import savgol_coeffs
    for h in (d, 3, 7, 24, 40):
        if 2 * h + 1 <= d:
            continue
        n = 2 * h + 1
        tp = O.taps(h, d, "rect")
        sw, piv = O.full_pivots(tp, d)
        # the effective coefficients: the response of the centre frame to a unit sample at every offset
        eff = np.zeros((d + 1, n))
        for j in range(n):
            rec = np.zeros((n, 1, 2))
            rec[:, 0, 0] = 1.0
            rec[j, 0, 1] = 1.0
            out, _ = O.fit(O.moments(rec, tp, d, 1, (h, h + 1)), rec[h:h + 1], O.thresholds(sw, piv), h, d, 1)
            assert out[0, 0, 0] == 7.0 and out[0, 0, 1] == d
            eff[:, j] = out[0, 0, 2:3 + d]
        for k in range(d + 1):
            want = savgol_coeffs(n, d, deriv=k, use="dot")
            assert np.abs(eff[k] - want).max() <= O.KIN_TOL, (h, d, k, np.abs(eff[k] - want).max())


@pytest.mark.parametrize("d", (0, 1, 2, 3))
def test_polynomials_with_gaps_are_reproduced(d):
    n, s = 120, 3
    r = np.random.default_rng(d)
    f = np.arange(n, dtype=np.float64)
    t = (f - 60.0) / 64.0
    coef = r.uniform(-1.0, 1.0, (s, d + 1))
    for h, kind in ((5, "rect"), (12, "hann")):
        rec = np.zeros((n, s, 2))
        rec[..., 0] = r.random((n, s)) >= 0.1
        rec[:h + 1, :, 0], rec[n - h - 1:, :, 0] = 1.0, 1.0       # gap-free one-sided windows at both ends keep the full degree
        rec[40:47, 0, 0] = 0.0                                    # a gap shorter than the window: filled at full degree
        rec[70:70 + 2 * h + 4, 1, 0] = 0.0                        # ... and one longer: nothing reaches full degree deep inside it
        rec[..., 1] = sum(coef[None, :, k] * t[:, None] ** k for k in range(d + 1))
        tp = O.taps(h, d, kind)
        sw, piv = O.full_pivots(tp, d)
        # (min_coverage 0.25: a one-sided window holds half of the weight before its dropouts)
        out, filled = O.fit(O.moments(rec, tp, d, 1), rec, O.thresholds(sw, piv, 0.25), h, d, 1, fill_degree=d)
        full = out[..., 1] == d
        assert full[0].all() and full[-1].all() and full[43, 0] and not full[70 + h + 1, 1]
        assert (full & (rec[..., 0] == 0.0)).sum() > 10             # frames inside gaps included
        worst = 0.0
        for k in range(d + 1):
            want = sum(coef[None, :, j] * math.perm(j, k) * t[:, None] ** (j - k) for j in range(k, d + 1)) / 64.0 ** k
            worst = max(worst, np.abs(out[..., 2 + k] - want)[full].max())
        print(f"d {d} h {h} {kind}: largest error {worst:.3g} over {int(full.sum())} full-degree frames")
        assert worst <= O.KIN_TOL
        assert np.abs(out[..., 2 + d + 1][full]).max() <= O.KIN_TOL     # nothing is left over
        gone = (rec[..., 0] == 0.0) & full
        assert (filled[..., 0][gone] == 2.0).all() and np.abs(filled[..., 1] - rec[..., 1])[gone].max() <= O.KIN_TOL


def test_rss_is_the_weighted_residual_sum_of_squares():
    rec = O.press_case(197, seed=5, noise=0.05)
    h, d = 7, 2
    tp = O.taps(h, d)
    sw, piv = O.full_pivots(tp, d)
    # (min_coverage 0.05: at the default 0.5 a window at the edge of the long gap is refused before its pivots fail)
    out, _ = O.fit(O.moments(rec, tp, d, 1), rec, O.thresholds(sw, piv, 0.05), h, d, 1)
    seen = 0
    for f in range(0, 197):
        q = int(out[f, 0, 1])
        if q < 0:
            continue
        _, rss = O.lstsq_window(rec[:, 0, 1], rec[:, 0, 0] != 0.0, O.window(h), h, f, q)
        assert abs(out[f, 0, 2 + d + 1] - rss) <= 1e-12, (f, q)
        seen += 1
    assert seen > 30 and set(np.unique(out[:, 0, 1])) >= {-1.0, 0.0, 1.0, 2.0}     # the long gap walks through every fallback


def test_fit_rules_on_hand_built_moments():
    mom, rows = O.hand_moments()
    out, filled = O.fit(mom, rows, O.HAND_THR, O.HAND_H, O.HAND_D, 1)
    O.check_hand(out, filled)


def test_fit_edges():
    """h = 0 and 2h + 1 <= d can never be full; all valid; none valid; a slot never valid."""
    n = 12
    rec = np.zeros((n, 3, 2))
    rec[..., 0] = 1.0
    rec[:, 1, 0] = 0.0                                           # a slot never valid
    rec[..., 1] = np.arange(n)[:, None] / 8.0
    for h, d in ((0, 0), (0, 1), (0, 3), (1, 3), (1, 2), (2, 3)):
        tp = O.taps(h, d, "rect")
        sw, piv = O.full_pivots(tp, d)
        thr = O.thresholds(sw, piv, 0.5, O.PIV_REL, h)
        assert np.isinf(thr[2 * h + 1:]).all() and np.isfinite(thr[:2 * h + 1]).all()
        out, filled = O.fit(O.moments(rec, tp, d, 1), rec, thr, h, d, 1, fill_degree=0)
        q = out[..., 1]
        assert (q[:, 1] == -1).all() and (out[:, 1, 0] == 0.0).all() and not filled[:, 1].any()
        if 2 * h + 1 <= d:
            assert (q < d).all()                                  # fewer frames than coefficients: never full
        else:
            assert (q[h:n - h, 0] == d).all()
        if h == 0:
            assert (q[:, 0] == 0).all() and np.array_equal(out[:, 0, 2], rec[:, 0, 1]) and (out[:, 0, 0] == (7.0 if d == 0 else 3.0)).all()
        O.assert_bits(filled[:, 0], rec[:, 0], "valid rows travel bit for bit")


def test_kinematic_rows_and_sheet():
    from vbs_amd import pipeline as PL
    d, F, k = 2, 4, 3
    fit = np.zeros((F, k, 2 + 3 * (d + 2)))
    mom = np.ones((F, k, 2 * d + 1 + 3 * (d + 2)))
    fit[..., 0], fit[..., 1] = 7.0, 2.0
    fit[..., 3] = 3.0                                            # vx of every marker
    fit[..., 7] = 4.0                                            # vy: speed 5
    fit[1, 2, 3] = 6.0                                           # marker 2 faster in frame 1: speed sqrt(52)
    fit[2, :, 1] = -1.0                                          # a frame without a degree
    fit[3, 1, 3], fit[3, 2, 3] = 30.0, 30.0                      # a tie in frame 3: the smaller slot
    fit[..., 5] = 0.5                                            # rss of x
    rows = PL._kinematic_rows(fit, mom, d, fps=10.0, onset_frac=0.5)
    assert rows["velocity"][0, 0].tolist() == [30.0, 40.0, 0.0] and rows["speed"][0, 0] == 50.0
    assert np.isnan(rows["speed"][2]).all() and rows["fastest"].tolist() == [0, 2, -1, 1]
    assert np.isnan(rows["mean_speed"][2]) and rows["max_speed"][1] == math.sqrt(60.0 ** 2 + 40.0 ** 2)
    assert rows["peak_frame"].tolist() == [0, 3, 3] and rows["onset"] == 3 and rows["degree"][2].tolist() == [-1] * 3
    assert rows["noise"][0, 0, 0] == math.sqrt(0.5) and np.isnan(rows["noise"][2]).all()
    assert PL._kinematic_rows(fit[..., :2 + 3 * 2], mom[..., :3 + 3 * 2], 0)["onset"] == -1     # degree 0: no velocity
    df = PL.to_kinematic_frame(rows, fps=10.0)
    assert tuple(df.columns) == PL.KINEMATIC_FRAME_COLUMNS + ("time_s",) and len(df) == 3 * F * k
    assert df["velocity"].iloc[0] == 30.0 and df["degree"].iloc[3 * k * 2] == -1 and df["frameno"].iloc[-1] == F
    for bad in (dict(half_window=128), dict(degree=4), dict(window="x"), dict(ref_frame=9), dict(min_coverage=0.0), dict(piv_rel=1.0),
                dict(onset_frac=0.0), dict(axis="w")):
        good = dict(n=9, m=4, half_window=3, degree=2, window="hann", ref_frame=0, min_coverage=0.5, piv_rel=5e-3, onset_frac=0.1)
        assert PL._kinematic_args(**good) == (3, 2, 2)
        with pytest.raises(ValueError):
            PL._kinematic_args(**dict(good, **bad))
