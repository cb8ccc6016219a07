"""CPU tests of the time-resolved fit's host side (no GPU): the two new C symbols and their constants, what both entries refuse
before a device is touched, `spectra.carrier` / `spectra.window_taps`, the sheet, `envelope_analysis`'s argument checks and host
arithmetic, and the NumPy restatements the GPU tests hold the device to (`tests/helpers/envelope_oracle.py`): the moments' against
exact rational arithmetic within the derived bound and bit for bit where every order of summation is exact, the fit's against
`np.linalg.lstsq` (ENV_TOL) and on hand-built moments."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import _build, spectra
from vbs_amd.filters import half_taps

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import envelope_oracle as O                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_constants_and_source_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vbs_window_moments_f64", "vbs_window_fit_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    for name in ("ENV_TILE", "ENV_MAX_HALF"):
        assert getattr(L, name) == defs["VBS_" + name], name
    assert L.ENV_MAX_HALF == 127 and 2 * L.ENV_MAX_HALF + 1 <= L.FIR_MAX_TAPS and L.ENV_TILE % 16 == 0
    assert (2 * L.ENV_MAX_HALF + 9) * 2.0 ** -53 < 1e-12          # gamma_(K+8) is far from its pole at every admitted h
    assert "k_envelope.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "k_envelope.hip"))
    wm, wf = L.lib().vbs_window_moments_f64, L.lib().vbs_window_fit_f64
    assert len(wm.argtypes) == 13 and len(wf.argtypes) == 10 and wf.argtypes[5] is C.c_double and wf.argtypes[7] is C.c_double


def test_refusals_without_a_gpu():
    """Both C entries decide every refusal before the device is touched: with device pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY.  The weights live on the host and are read."""
    lib = L.lib()
    p, nul = C.c_void_p(8), None
    good_half = np.array([1.0, 0.5, 0.25])

    def wm(rec=p, n=10, s=5, cols=4, nv=3, car=p, half=good_half, n_half=None, fb=0, fe=10, out=p):
        hp = None if half is None else np.ascontiguousarray(half, np.float64).ctypes.data_as(C.c_void_p)
        nh = (0 if half is None else len(half)) if n_half is None else n_half
        return lib.vbs_window_moments_f64(0, rec, n, s, cols, nv, car, hp, nh, fb, fe, out, None)
    for bad in (dict(rec=nul), dict(car=nul), dict(half=None, n_half=3), dict(out=nul), dict(n=0, fe=0), dict(s=0), dict(n=-1), dict(cols=1),
                dict(cols=9), dict(nv=0), dict(nv=4, cols=8), dict(nv=3, cols=3), dict(n_half=0), dict(half=np.ones(L.ENV_MAX_HALF + 2)),
                dict(half=[1.0, -0.5]), dict(half=[1.0, math.nan]), dict(half=[1.0, math.inf]), dict(half=[0.0, 1.0]), dict(half=[-1.0]),
                dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert wm(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)):
        assert wm(**big) == L.VBS_ECAPACITY, big
        assert wm(**dict(big, rec=nul)) == L.VBS_EINVAL          # a bad argument comes before a capacity
        assert wm(**dict(big, half=[1.0, -1.0])) == L.VBS_EINVAL

    def wf(mom=p, F=10, s=5, nv=3, sw=4.0, mc=0.5, dm=1e-3, fit=p):
        return lib.vbs_window_fit_f64(0, mom, F, s, nv, sw, mc, dm, fit, None)
    for bad in (dict(mom=nul), dict(fit=nul), dict(F=0), dict(s=0), dict(nv=0), dict(nv=4), dict(sw=0.0), dict(sw=-1.0), dict(sw=math.nan),
                dict(sw=math.inf), dict(mc=0.0), dict(mc=1.0000001), dict(mc=math.nan), dict(dm=-1e-9), dict(dm=0.25), dict(dm=math.nan)):
        assert wf(**bad) == L.VBS_EINVAL, bad
    for big in (dict(F=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)):
        assert wf(**big) == L.VBS_ECAPACITY, big
        assert wf(**dict(big, dm=0.25)) == L.VBS_EINVAL

    from vbs_amd.engine import _envelope_args, _envelope_fit_args
    good = dict(n=10, s=5, cols=4, carrier_shape=(4, 10), half=good_half, n_values=None, frame_range=None)
    assert _envelope_args(**good) == (3, 0, 10)
    assert _envelope_args(**dict(good, cols=8, frame_range=(2, 7))) == (3, 2, 7)
    assert _envelope_args(**dict(good, cols=2, s=1, frame_range=(4, 4))) == (1, 4, 4)
    for bad in (dict(carrier_shape=(4, 11)), dict(carrier_shape=(3, 10)), dict(carrier_shape=(40,)), dict(n_values=4, cols=8),
                dict(n_values=3, cols=3), dict(n_values=0), dict(cols=9), dict(cols=1), dict(s=0), dict(half=np.ones(L.ENV_MAX_HALF + 2)),
                dict(half=[1.0, -0.5]), dict(half=[0.0, 1.0]), dict(half=[1.0, math.nan]), dict(half=[]), dict(frame_range=(-1, 5)),
                dict(frame_range=(0, 11)), dict(frame_range=(6, 5))):
        with pytest.raises(ValueError):
            _envelope_args(**dict(good, **bad))
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}"):
        _envelope_args(**dict(good, s=L.PROJ_MAX_SLOTS + 1))
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_FRAMES = {L.PROJ_MAX_FRAMES}"):
        _envelope_args(**dict(good, n=L.PROJ_MAX_FRAMES + 1, carrier_shape=(4, L.PROJ_MAX_FRAMES + 1)))
    fgood = dict(F=10, s=5, M=17, taps_sum=4.0, min_coverage=0.5, det_min=1e-3)
    assert _envelope_fit_args(**fgood) == (3, 4.0, 0.5, 1e-3) and _envelope_fit_args(**dict(fgood, M=9, det_min=0))[0] == 1
    for bad in (dict(M=5), dict(M=10), dict(M=21), dict(F=0), dict(s=0), dict(taps_sum=0.0), dict(taps_sum=math.nan), dict(min_coverage=0.0),
                dict(min_coverage=1.5), dict(det_min=0.25), dict(det_min=-0.1), dict(det_min=math.nan)):
        with pytest.raises(ValueError):
            _envelope_fit_args(**dict(fgood, **bad))
    with pytest.raises(L.VbsError, match="VBS_PROJ_MAX_FRAMES"):
        _envelope_fit_args(**dict(fgood, F=L.PROJ_MAX_FRAMES + 1))


def test_window_taps_and_carrier_properties():
    for h in (0, 1, 7, 40, 127):
        for kind in ("hann", "rect"):
            w = spectra.window_taps(h, kind)
            assert w.shape == (2 * h + 1,) and w.dtype == np.float64 and np.array_equal(w, w[::-1]) and (w > 0.0).all() and w[h] == 1.0
            O.assert_bits(half_taps(w), w[h:], f"{kind} {h}: the half taps are the window's own")
        w = spectra.window_taps(h)
        assert h == 0 or (np.diff(w[h:]) < 0).all()              # strictly falling from the centre
        assert w[0] == pytest.approx(0.5 * (1 + math.cos(math.pi * h / (h + 1))))
    assert spectra.window_taps(3, "rect").tolist() == [1.0] * 7
    for bad in (lambda: spectra.window_taps(-1), lambda: spectra.window_taps(2.5), lambda: spectra.window_taps(3, "hamming")):
        with pytest.raises(ValueError):
            bad()
    n, nu = 37, 0.0837
    car = spectra.carrier(n, nu)
    assert car.shape == (4, n) and car.dtype == np.float64 and car.flags.c_contiguous and np.isfinite(car).all()
    f = np.arange(n, dtype=np.float64)
    O.assert_bits(car[0], np.cos(2 * np.pi * nu * f), "c")
    O.assert_bits(car[1], np.sin(2 * np.pi * nu * f), "s")
    O.assert_bits(car[2], np.cos(2 * np.pi * (2 * nu) * f), "c2")
    O.assert_bits(car[3], np.sin(2 * np.pi * (2 * nu) * f), "s2")
    O.assert_bits(car, spectra.harmonic_basis(n, [nu])[1:5], "the rows of the harmonic basis")
    for bad in (0.0, -0.1, 0.2500001, math.nan, math.inf):
        with pytest.raises(ValueError):
            spectra.carrier(n, bad)
    with pytest.raises(ValueError):
        spectra.carrier(0, 0.1)
    # a whole number of periods without gaps: det / W^2 is 1/4
    n, nu, h = 101, 0.05, 20                                     # a rect window of 40 frames would be 2 periods; 41 is close to it
    rec = np.ones((n, 1, 2))
    half = half_taps(spectra.window_taps(h, "rect"))[:h + 1]
    mom = O.moments(rec, spectra.carrier(n, nu), half, 1, (50, 51))[0, 0]
    W, C1, S1, C2, S2 = mom[:5]
    det = (0.5 * (W + C2) - C1 * C1 / W) * (0.5 * (W - C2) - S1 * S1 / W) - (0.5 * S2 - C1 * S1 / W) ** 2
    print(f"rect window of 41 frames at 20 frames a period: det / W^2 = {det / W ** 2:.4f}")
    assert W == 41.0 and det / W ** 2 == pytest.approx(0.25, abs=0.02)


@pytest.mark.parametrize("n,s,h", ((1, 2, 0), (17, 5, 3), (40, 3, 31), (70, 2, 127)))
def test_restated_moments_are_exact_on_dyadic_cases(n, s, h):
    """Where every order is exact the restatement's sums are the rationals."""
    rec, car = O.dyadic_case(n, s, 5, 3, seed=n)
    if s > 1:
        rec[:, -1, 0] = 0.0
    half = O.dyadic_half(h, n)
    got = O.moments(rec, car, half, 3)
    value, _ = O.exact_moments(rec, car, half, 3)
    for idx in np.ndindex(*value.shape):
        assert O.Fraction(float(got[idx])) == value[idx], idx
    if s > 1:
        assert not got[:, -1].any()                              # a series with no valid frame: exact zeros
    O.assert_bits(O.moments(rec, car, half, 3, (n // 3, n // 3 + 1)), got[n // 3:n // 3 + 1], "a range")


@pytest.mark.parametrize("n,s,h,seed", ((3, 2, 1, 1), (64, 3, 8, 2), (100, 2, 40, 3), (300, 1, 127, 4)))
def test_restated_moments_within_the_bound_of_exact_arithmetic(n, s, h, seed):
    rec, car = O.random_case(n, s, 6, 3, seed)
    half = half_taps(spectra.window_taps(h))
    rng = (0, n) if n <= 100 else (n // 2 - 20, n // 2 + 20)
    worst = O.check_within_bound(O.moments(rec, car, half, 3, rng), rec, car, half, 3, rng, what=f"n {n} h {h}")
    print(f"n {n} h {h}: restatement's largest error / bound = {worst:.3g}")
    assert worst <= 1.0


def test_poison_never_enters_the_restatement():
    rec, car = O.random_case(40, 7, 8, 2, seed=9, kind=None)
    half = half_taps(spectra.window_taps(5))
    clean = O.moments(rec, car, half, 2)
    for kind in (np.nan, 1e300):
        O.assert_bits(O.moments(O.poison(rec, 2, kind), car, half, 2), clean, f"poison {kind}")
    assert np.isfinite(clean).all()


@pytest.mark.parametrize("n", O.ENV_SIZES)
def test_restated_fit_agrees_with_weighted_lstsq(n):
    """The elimination with the half-angle sums against np.linalg.lstsq on sqrt(w) [1, c, s] over the valid frames of every ok
    window.  Both solve one 3-parameter problem; with det / W^2 > det_min = 1e-3 an error e in a sum of size <= W max|x| moves a
    and b by about e W / (1e-3 W^2), and the sums carry gamma_(K+8) W max|x|: 1000 gamma_(K+8) max|x|, a few of them together
    (max|x| <= 0.6 here): 4000 gamma_(K+8) bounds the difference.  The figures are printed; 10 x the largest over all shapes is
    ENV_TOL."""
    for h in O.ENV_HALVES:
        for nu in O.ENV_NUS:
            d, cond = O.env_difference(n, h, nu)
            print(f"n {n} h {h} nu {nu}: largest |c0, a, b difference| = {d:.3g}, smallest det / W^2 = {cond:.3g}")
            assert d <= 4000 * float(O.gamma(2 * h + 9))
            assert O.env_tol() >= 10 * d
    print(f"ENV_TOL = {O.env_tol():.3g}")
    assert O.env_tol() < 1e-12


def test_fit_rules_on_hand_built_moments():
    fit = O.window_fit(O.hand_moments(), O.HAND_SW, O.HAND_COVERAGE, O.HAND_DET_MIN)
    O.check_hand(fit)
    # h = 0: one frame cannot tell a cosine from a mean: det is 0 up to rounding, nothing is ok
    rec, car = O.burst_case(64, 0.05, 1)
    mom = O.moments(rec, car, np.array([1.0]), 1)
    assert not O.window_fit(mom, 1.0)[..., 0].any() and not O.window_fit(mom, 1.0).any()


def test_onset_and_peak_of_a_synthetic_burst():
    """Quiet 0.02, a Gaussian burst of 0.4 around 0.45 n, steady 0.15 (n = 600, nu = 0.05, h = 40): the onset lies within h frames
    of the frame where the true envelope reaches half its maximum, the peak frame within h / 2 of the true one."""
    from vbs_amd.pipeline import _envelope_rows
    n, nu, h = 600, 0.05, 40
    rec, car = O.burst_case(n, nu, seed=5)
    half = half_taps(spectra.window_taps(h))
    fit1 = O.window_fit(O.moments(rec, car, half, 1), O.taps_sum(half))
    fit = np.zeros((n, 1, 16))
    fit[..., :6] = fit1
    fit[..., 6:11], fit[..., 11:16] = fit1[..., 1:6], fit1[..., 1:6]
    rows = _envelope_rows(fit, 0.5)
    env = O.burst_envelope(n)
    true_peak = int(np.argmax(env))
    true_onset = int(np.nonzero(env >= 0.5 * env.max())[0][0])
    peak, frame, level, onset, count = rows["summary"][0, 0]
    print(f"onset {onset:.0f} against {true_onset}, peak frame {frame:.0f} against {true_peak}, peak {peak:.3f} against {env.max():.3f}, "
          f"level {level:.3f}, {count:.0f} ok frames")
    assert abs(onset - true_onset) <= h and abs(frame - true_peak) <= h / 2
    assert 0.3 < peak <= env.max() + 0.02 and 0.02 < level < 0.2 and count > 0.9 * n
    assert np.array_equal(rows["summary"][0, 1], rows["summary"][0, 0])
    amp = rows["amplitude"][:, 0, 0]
    assert np.nanmax(np.abs(amp[500:] - 0.15)) < 0.02 and np.nanmax(amp[:100]) < 0.05
    assert abs(rows["freq_dev"][0, 0]) < 1e-3                    # the line sits on the carrier


def test_envelope_rows_host_arithmetic():
    """`envelope_analysis`'s host arithmetic with the two device calls replaced by the restatement."""
    from vbs_amd.pipeline import _envelope_rows
    n, nu, h, dnu = 200, 0.08, 12, 0.002
    f = np.arange(n, dtype=np.float64)
    rec = np.zeros((n, 2, 4))
    rec[..., 0] = 1.0
    rec[:, 0, 1] = 0.5 * np.cos(2 * np.pi * (nu + dnu) * f - 0.3)          # a line above the carrier
    rec[:, 0, 2] = np.where(f >= 100, 0.2, 0.05) * np.cos(2 * np.pi * nu * f - 1.0)
    rec[:, 0, 3] = 0.0
    rec[:, 1, 1:] = rec[:, 0, 1:]
    rec[30:80, 1, 0] = 0.0                                                 # a long gap: windows inside it are not ok
    rec[:, 1, 1:][rec[:, 1, 0] == 0.0] = np.nan
    half = half_taps(spectra.window_taps(h))
    fit = O.window_fit(O.moments(rec, spectra.carrier(n, nu), half, 3), O.taps_sum(half))
    rows = _envelope_rows(fit, 0.5)
    ok = fit[..., 0] != 0
    assert ok[:, 0].all() and not ok[40:70, 1].any() and ok[100:, 1].all()
    for key in ("amplitude", "phase_deg", "explained"):
        assert rows[key].shape == (n, 2, 3) and np.isnan(rows[key][~ok]).all()
    a, b = fit[..., 1::5], fit[..., 2::5]
    assert np.array_equal(rows["amplitude"][ok], np.hypot(a, b)[ok])
    assert np.array_equal(rows["phase_deg"][ok], np.degrees(np.arctan2(b, a))[ok])
    assert np.nanmax(np.abs(rows["amplitude"][20:180, 0, 0] - 0.5)) < 0.01
    assert 0.99 < np.nanmin(rows["explained"][20:180, 0, 0]) and np.nanmax(rows["explained"][20:180, 0, 0]) < 1 + 1e-9
    assert rows["freq_dev"][0, 0] == pytest.approx(dnu, rel=0.02) and abs(rows["freq_dev"][0, 1]) < 2e-4
    assert rows["freq_dev"][1, 0] == pytest.approx(dnu, rel=0.02)          # over the longest ok run
    s = rows["summary"]
    assert s.shape == (2, 3, 5) and s[0, 1, 4] == n and s[1, 1, 4] == ok[:, 1].sum()
    assert abs(s[0, 1, 3] - 100) <= h and s[0, 1, 1] >= 100 and s[0, 1, 0] == pytest.approx(0.2, abs=0.01)
    assert s[0, 1, 2] == np.nanmedian(rows["amplitude"][:, 0, 1])
    assert s[0, 2, 0] == 0.0 and s[0, 2, 3] == 0.0                         # an all-zero series: amplitude 0 reaches 0.5 x 0 at once
    dead = np.zeros((5, 1, 16))
    rows = _envelope_rows(dead)
    assert np.isnan(rows["summary"][0, :, 0]).all() and (rows["summary"][0, :, 1] == -1).all() and (rows["summary"][0, :, 3] == -1).all()
    assert (rows["summary"][0, :, 4] == 0).all() and np.isnan(rows["freq_dev"]).all()


def test_envelope_analysis_argument_checks():
    from vbs_amd.pipeline import _envelope_analysis_args
    good = dict(n=197, m=49, nu=0.08, half_window=16, window="hann", ref_frame=0, slot_mask=None, min_coverage=0.5, det_min=1e-3,
                onset_frac=0.5)
    nu, w, slots, ax = _envelope_analysis_args(**good)
    assert nu == 0.08 and w.shape == (33,) and slots is None and ax == 2
    mask = np.zeros(49, dtype=bool)
    mask[[3, 7]] = True
    nu, w, slots, ax = _envelope_analysis_args(**dict(good, nu={"common_freq": 0.0837}, slot_mask=mask, window="rect", axis="x"))
    assert nu == 0.0837 and w.tolist() == [1.0] * 33 and slots.tolist() == [3, 7] and ax == 0
    for bad in (dict(nu=0.3), dict(nu=0.0), dict(nu={"common_freq": math.nan}), dict(half_window=128), dict(half_window=-1),
                dict(window="hamming"), dict(ref_frame=197), dict(ref_frame=-1), dict(min_coverage=0.0), dict(det_min=0.25),
                dict(onset_frac=0.0), dict(onset_frac=1.5), dict(slot_mask=np.ones(48)), dict(axis="w"), dict(m=L.PROJ_MAX_SLOTS + 1),
                dict(n=L.PROJ_MAX_FRAMES + 1)):
        with pytest.raises(ValueError):
            _envelope_analysis_args(**dict(good, **bad))


def test_envelope_sheet_columns_and_round_trip(tmp_path):
    from vbs_amd import pipeline as PL
    from vbs_amd.xlsx_io import read_xlsx
    r = np.random.default_rng(3)
    res = {k: r.integers(0, 4096, (4, 2, 3)) / 64.0 for k in ("amplitude", "phase_deg", "explained")}      # exact as decimal text
    for k in res:
        res[k][1, 0] = np.nan                                    # a window that is not ok
    df = PL.to_envelope_frame(res)
    assert tuple(df.columns) == PL.ENVELOPE_FRAME_COLUMNS == ("frameno", "marker_id", "axis", "amplitude", "phase_deg", "explained")
    assert len(df) == 24 and df["frameno"].tolist()[:7] == [1] * 6 + [2] and df["marker_id"].tolist()[:6] == [1, 1, 1, 2, 2, 2]
    assert df["axis"].tolist() == ["x", "y", "z"] * 8 and df["amplitude"][5] == res["amplitude"][0, 1, 2]
    assert df["amplitude"].isna().tolist()[6:9] == [True] * 3 and not df["amplitude"].isna()[9:].any()
    ids = np.array([[1, 0], [0, 0]])
    df2 = PL.to_envelope_frame(res, ids=ids, fps=120.0, path=str(tmp_path / "envelope.xlsx"))
    assert tuple(df2.columns) == PL.ENVELOPE_FRAME_COLUMNS + ("time_s",) and df2["marker_id"].tolist()[:6] == [2, 2, 2, 1, 1, 1]
    assert df2["time_s"][6] == 1 / 120.0
    back = read_xlsx(str(tmp_path / "envelope.xlsx"))
    assert list(back.columns) == list(df2.columns) and len(back) == 24 and back["axis"].tolist() == df2["axis"].tolist()
    for c in df2.columns:
        if c != "axis":
            assert np.array_equal(back[c].to_numpy(dtype=np.float64), df2[c].to_numpy(dtype=np.float64), equal_nan=True), c
    import pandas as pd
    PL.to_envelope_frame(res, path=str(tmp_path / "envelope.csv"))
    back = pd.read_csv(str(tmp_path / "envelope.csv"))
    assert tuple(back.columns) == tuple(df.columns) and back["axis"].tolist() == df["axis"].tolist()
    for c in df.columns:
        if c != "axis":
            assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64), equal_nan=True), c
    for bad in (lambda: PL.to_envelope_frame({k: v[..., :2] for k, v in res.items()}), lambda: PL.to_envelope_frame(res, ids=ids[:1]),
                lambda: PL.to_envelope_frame(dict(res, explained=res["explained"][:3])), lambda: PL.to_envelope_frame(res, fps=0.0)):
        with pytest.raises(ValueError):
            bad()
