"""CPU tests of the displacement spectra's host side (no GPU): the two new C symbols and their constants, what both entries refuse
before a device is touched, `vbs_amd.spectra`, the sheet, `spectral_analysis`'s argument checks, and the NumPy restatements the
GPU tests hold the device to (`tests/helpers/spectrum_oracle.py`): the projection's against exact rational arithmetic within the
derived bound and bit for bit where every order of summation is exact, the fit's against `np.linalg.lstsq` and on hand-built
projections."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import spectra

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import spectrum_oracle as O                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vbs_project_series_f64", "vbs_harmonic_fit_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    names = ("PROJ_SLOTS", "PROJ_CHUNK", "PROJ_ROWS", "PROJ_WG_SLOTS", "PROJ_MAX_ROWS", "PROJ_MAX_FRAMES", "PROJ_MAX_SLOTS", "FIT_GROUP",
             "PEAK_COLS")
    for name in names:
        assert getattr(L, name) == defs["VBS_" + name], name
    assert L.PROJ_SLOTS == 4 and L.PEAK_COLS == 7 == O.PEAK_COLS
    assert L.PROJ_CHUNK % 16 == 0 and L.PROJ_ROWS % 16 == 0 and L.PROJ_WG_SLOTS % 4 == 0 and 1 <= L.FIT_GROUP <= 16
    assert L.PROJ_MAX_ROWS >= 1 + 4 * 256 and L.PROJ_MAX_FRAMES >= 4096 and L.PROJ_MAX_SLOTS >= 441
    assert (L.PROJ_MAX_FRAMES + 6) * 2.0 ** -53 < 1e-9            # gamma_(n+6) is far from its pole at every admitted n
    pj, hf = L.lib().vbs_project_series_f64, L.lib().vbs_harmonic_fit_f64
    assert len(pj.argtypes) == 10 and len(hf.argtypes) == 11 and hf.argtypes[7] is C.c_double


def test_refusals_without_a_gpu():
    """Both C entries decide every refusal before the device is touched: with pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY."""
    lib = L.lib()
    p, nul = C.c_void_p(8), None

    def pj(rec=p, n=10, s=5, cols=4, nv=3, basis=p, R=9, out=p):
        return lib.vbs_project_series_f64(0, rec, n, s, cols, nv, basis, R, out, None)
    for bad in (dict(rec=nul), dict(basis=nul), dict(out=nul), dict(n=0), dict(s=0), dict(R=0), dict(n=-1), dict(cols=1), dict(cols=9),
                dict(nv=0), dict(nv=4, cols=8), dict(nv=3, cols=3)):
        assert pj(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1), dict(R=L.PROJ_MAX_ROWS + 1)):
        assert pj(**big) == L.VBS_ECAPACITY, big
        assert pj(**dict(big, rec=nul)) == L.VBS_EINVAL          # a bad argument comes before a capacity

    def hf(proj=p, s=5, R=1 + 4 * 33, nv=3, Q=33, mc=8, dm=1e-3, fit=p, peak=p):
        return lib.vbs_harmonic_fit_f64(0, proj, s, R, nv, Q, mc, dm, fit, peak, None)
    for bad in (dict(proj=nul), dict(fit=nul, peak=nul), dict(s=0), dict(mc=2), dict(mc=-1), dict(dm=-1e-9), dict(dm=0.25), dict(dm=math.nan),
                dict(Q=0), dict(Q=-3, R=-11), dict(R=4 * 33), dict(R=2 + 4 * 33), dict(Q=32), dict(nv=0), dict(nv=4),
                dict(Q=1 << 29, R=1)):
        assert hf(**bad) == L.VBS_EINVAL, bad

    from vbs_amd.engine import _fit_args, _project_args
    good = dict(n=10, s=5, cols=4, basis_shape=(9, 10), n_values=None)
    assert _project_args(**good) == (9, 3)
    assert _project_args(**dict(good, cols=8)) == (9, 3)         # the default never asks for more than 3 values
    assert _project_args(**dict(good, cols=2, s=1)) == (9, 1)
    for bad in (dict(basis_shape=(9, 11)), dict(basis_shape=(10,)), dict(basis_shape=(0, 10)), dict(n_values=4, cols=8),
                dict(n_values=3, cols=3), dict(n_values=0), dict(cols=9), dict(cols=1), dict(s=0)):
        with pytest.raises(ValueError):
            _project_args(**dict(good, **bad))
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}"):
        _project_args(**dict(good, s=L.PROJ_MAX_SLOTS + 1))
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_ROWS = {L.PROJ_MAX_ROWS}"):
        _project_args(**dict(good, basis_shape=(L.PROJ_MAX_ROWS + 1, 10)))
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_FRAMES = {L.PROJ_MAX_FRAMES}"):
        _project_args(**dict(good, n=L.PROJ_MAX_FRAMES + 1, basis_shape=(9, L.PROJ_MAX_FRAMES + 1)))
    fgood = dict(s=5, R=133, oc=4, Q=33, min_count=8, det_min=1e-3)
    assert _fit_args(**fgood) == (3, 8, 1e-3) and _fit_args(**dict(fgood, oc=2, det_min=0)) == (1, 8, 0.0)
    for bad in (dict(oc=1), dict(oc=5), dict(Q=32), dict(Q=0), dict(R=132), dict(min_count=2), dict(det_min=0.25), dict(det_min=-0.1),
                dict(det_min=math.nan), dict(s=0)):
        with pytest.raises(ValueError):
            _fit_args(**dict(fgood, **bad))


def test_harmonic_basis_rows_grid_and_helpers():
    nu = np.array([0.01, 0.0837, 0.25])
    n, Q = 37, 3
    B = spectra.harmonic_basis(n, nu)
    assert B.shape == (1 + 4 * Q, n) and B.dtype == np.float64 and B.flags.c_contiguous and np.isfinite(B).all()
    assert np.all(B[0] == 1.0)
    f = np.arange(n, dtype=np.float64)
    for q in range(Q):
        O.assert_bits(B[1 + 2 * q], np.cos(2.0 * np.pi * nu[q] * f), f"cos row of bin {q}")
        O.assert_bits(B[2 + 2 * q], np.sin(2.0 * np.pi * nu[q] * f), f"sin row of bin {q}")
        O.assert_bits(B[1 + 2 * Q + 2 * q], np.cos(2.0 * np.pi * (2.0 * nu[q]) * f), f"cos row of twice bin {q}")
        O.assert_bits(B[2 + 2 * Q + 2 * q], np.sin(2.0 * np.pi * (2.0 * nu[q]) * f), f"sin row of twice bin {q}")
    # the half-angle identities the fit rests on
    assert np.allclose(B[1] * B[1], 0.5 * (1 + B[1 + 2 * Q]), atol=1e-14) and np.allclose(B[1] * B[2], 0.5 * B[2 + 2 * Q], atol=1e-14)
    assert spectra.harmonic_basis(1, [0.1]).shape == (5, 1)
    for bad in ([0.0], [-0.1], [0.2500001], [0.1, math.nan], [math.inf], []):
        with pytest.raises(ValueError):
            spectra.harmonic_basis(n, bad)
    with pytest.raises(ValueError):
        spectra.harmonic_basis(0, [0.1])
    g = spectra.zoom_grid(0.0837, 2.0 / 197, 33)
    assert g.shape == (33,) and g[16] == 0.0837 and g[0] == pytest.approx(0.0837 - 2 / 197) and g[-1] == pytest.approx(0.0837 + 2 / 197)
    assert np.all(np.diff(g) > 0) and spectra.zoom_grid(0.1, 0.05, 1).tolist() == [0.1]
    for bad in (lambda: spectra.zoom_grid(0.01, 0.02, 5), lambda: spectra.zoom_grid(0.24, 0.02, 5), lambda: spectra.zoom_grid(0.1, 0.01, 0),
                lambda: spectra.zoom_grid(0.1, -0.01, 3)):
        with pytest.raises(ValueError):
            bad()
    amp, ph = spectra.amplitude_phase([3.0, 0.0, -1.0], [4.0, 2.0, 0.0])
    assert amp.tolist() == [5.0, 2.0, 1.0] and ph[1] == 90.0 and ph[2] == 180.0 and ph[0] == pytest.approx(math.degrees(math.atan2(4, 3)))
    assert spectra.to_hz([0.1, 0.25], 120.0).tolist() == [12.0, 30.0]
    with pytest.raises(ValueError):
        spectra.to_hz([0.1], 0.0)


@pytest.mark.parametrize("n,R,s", ((1, 3, 2), (17, 9, 5), (130, 33, 3), (300, 5, 4)))
def test_restated_projection_is_exact_on_dyadic_cases(n, R, s):
    """Where every order is exact the restatement's sums are the rationals."""
    rec, basis = O.with_edges(*O.dyadic_case(n, R, s, 5, 3, seed=n))
    got = O.project(rec, basis, 3)
    value, _ = O.exact_project(rec, basis, 3)
    for idx in np.ndindex(*value.shape):
        assert O.Fraction(float(got[idx])) == value[idx], idx
    if s > 1:
        assert not got[-1].any()                                 # a series with no valid frame: exact zeros
    if R > 1:
        assert not got[:, -1].any()


@pytest.mark.parametrize("n,R,s,seed", ((3, 4, 2, 1), (64, 9, 3, 2), (441, 5, 2, 3), (2000, 3, 1, 4)))
def test_restated_projection_within_the_bound_of_exact_arithmetic(n, R, s, seed):
    rec, basis = O.random_case(n, R, s, 6, 3, seed)
    worst = O.check_within_bound(O.project(rec, basis, 3), rec, basis, 3, what=f"n {n}")
    print(f"n {n}: restatement's largest error / bound = {worst:.3g}")
    assert worst <= 1.0


def test_poison_never_enters_the_restatement():
    rec, basis = O.random_case(40, 6, 7, 8, 2, seed=9, kind=None)
    clean = O.project(rec, basis, 2)
    for kind in (np.nan, 1e300):
        O.assert_bits(O.project(O.poison(rec, 2, kind), basis, 2), clean, f"poison {kind}")
    assert np.isfinite(clean).all()


@pytest.mark.parametrize("n", O.FIT_SIZES)
def test_restated_fit_agrees_with_lstsq(n):
    """The elimination with the half-angle sums against np.linalg.lstsq on [1, cos, sin] over the valid frames, in every bin of the
    33-bin zoom grid.  Both solve one 3-parameter problem whose normal matrix, with det / N^2 > 1e-3, has a condition number below
    (N / 2)^2 / (1e-3 N^2) = 250; sums of n terms of size <= 1 carry gamma_(n+6): 250 gamma_(n+6) bounds the difference of a and b
    (amplitude 0.7).  The figure is printed; 10 x the largest of the three is FIT_TOL."""
    d = O.fit_difference(n, 1000 + n)
    print(f"n {n}: largest |a, b difference| between the restated fit and lstsq = {d:.3g}")
    assert d <= 250 * float(O.gamma(n + 6))
    assert O.fit_tol() >= 10 * d and O.fit_tol() < 1e-12


def test_fit_rules_on_hand_built_projections():
    fit, peak = O.harmonic_fit(O.hand_proj(), O.HAND_Q, O.HAND_MIN_COUNT, O.HAND_DET_MIN)
    O.check_hand(fit, peak)
    # a frequency so low that the cosine cannot be told from the mean
    rec, nu = O.low_frequency_case()
    n = rec.shape[0]
    B = spectra.harmonic_basis(n, nu)
    proj = O.project(rec, B, 1)
    fit, peak = O.harmonic_fit(proj, 2, 8, 1e-3)
    assert fit[0, 0].tolist() == [0.0, 0.0, 0.0, 0.0] and fit[0, 1, 0] == 1.0 and peak[0, 0, 0] == 2.0 and peak[0, 0, 3] == 1.0
    dets = []
    for q in range(2):
        th = 2 * np.pi * nu[q] * np.arange(n)
        c, s = np.cos(th) - np.cos(th).mean(), np.sin(th) - np.sin(th).mean()
        dets.append(((c * c).sum() * (s * s).sum() - (c * s).sum() ** 2) / n ** 2)
    print(f"det / N^2 at 0.2 / n and 0.5 / n: {dets[0]:.3g}, {dets[1]:.3g}")
    assert dets[0] == pytest.approx(4e-4, rel=0.1) and dets[1] == pytest.approx(0.047, rel=0.05)
    _, a, b = O.lstsq_fit(rec[:, 0, 1], rec[:, 0, 0] != 0, nu[1])
    assert fit[0, 1, 1] == pytest.approx(a, abs=1e-12) and fit[0, 1, 2] == pytest.approx(b, abs=1e-12)
    assert fit[0, 1, 1] == pytest.approx(0.5 * math.cos(0.4), abs=1e-12) and fit[0, 1, 2] == pytest.approx(0.5 * math.sin(0.4), abs=1e-12)
    fit0, _ = O.harmonic_fit(proj, 2, 8, 0.0)
    assert fit0[0, 0, 0] == 1.0                                  # det_min = 0 lets it through


def test_spectrum_sheet_columns_and_round_trip(tmp_path):
    from vbs_amd import pipeline as PL
    from vbs_amd.xlsx_io import read_xlsx
    marker = np.zeros((2, 3, 6))
    marker[0] = [[0.08, 0.7, 30.0, 40.0, 0.9, 190], [0.081, 0.1, -170.0, 1.0, 0.2, 190], [0.08, 0.5, 0.0, 20.0, 0.8, 190]]
    marker[1] = [[np.nan] * 5 + [3], [0.08, 0.7, 90.0, 41.0, 0.95, 150], [np.nan] * 5 + [0]]
    df = PL.to_spectrum_frame(marker)
    assert tuple(df.columns) == PL.SPECTRUM_FRAME_COLUMNS == ("marker_id", "axis", "freq", "amplitude", "phase_deg", "power", "explained",
                                                               "count")
    assert len(df) == 6 and df["marker_id"].tolist() == [1, 1, 1, 2, 2, 2] and df["axis"].tolist() == ["x", "y", "z"] * 2
    assert df["count"].tolist() == [190, 190, 190, 3, 150, 0] and df["freq"].isna().tolist() == [False, False, False, True, False, True]
    assert df["phase_deg"][1] == -170.0 and df["explained"][4] == 0.95
    ids = np.array([[1, 0], [0, 0]])
    df2 = PL.to_spectrum_frame(marker, ids=ids, fps=120.0, path=str(tmp_path / "spectrum.xlsx"))
    assert tuple(df2.columns) == PL.SPECTRUM_FRAME_COLUMNS + ("freq_hz",) and df2["marker_id"].tolist() == [2, 2, 2, 1, 1, 1]
    assert df2["freq_hz"][0] == 0.08 * 120.0 and np.isnan(df2["freq_hz"][3])
    back = read_xlsx(str(tmp_path / "spectrum.xlsx"))
    assert list(back.columns) == list(df2.columns) and len(back) == 6 and back["axis"].tolist() == df2["axis"].tolist()
    for c in df2.columns:
        if c != "axis":
            assert np.array_equal(back[c].to_numpy(dtype=np.float64), df2[c].to_numpy(dtype=np.float64), equal_nan=True), c
    import pandas as pd
    PL.to_spectrum_frame(marker, path=str(tmp_path / "spectrum.csv"))
    back = pd.read_csv(str(tmp_path / "spectrum.csv"))
    assert tuple(back.columns) == tuple(df.columns) and back["axis"].tolist() == df["axis"].tolist()
    for c in df.columns:
        if c != "axis":
            assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64), equal_nan=True), c
    for bad in (lambda: PL.to_spectrum_frame(marker[:, :2]), lambda: PL.to_spectrum_frame(marker[..., :5]),
                lambda: PL.to_spectrum_frame(marker, ids=ids[:1])):
        with pytest.raises(ValueError):
            bad()


def test_spectral_analysis_argument_checks():
    from vbs_amd.pipeline import _spectrum_args
    good = dict(n=197, m=169, freqs=spectra.zoom_grid(0.0837, 2 / 197, 33), ref_frame=0, slot_mask=None, min_count=None, det_min=1e-3)
    nu, mc, slots, ax = _spectrum_args(**good)
    assert nu.shape == (33,) and mc == 49 and slots is None and ax == 2
    mask = np.zeros(169, dtype=bool)
    mask[[3, 7]] = True
    nu, mc, slots, ax = _spectrum_args(**dict(good, slot_mask=mask, min_count=12, axis="x", n=20))
    assert mc == 12 and slots.tolist() == [3, 7] and ax == 0
    assert _spectrum_args(**dict(good, n=20))[1] == 8
    for bad in (dict(freqs=[0.3]), dict(freqs=[]), dict(freqs=[0.0]), dict(ref_frame=197), dict(ref_frame=-1), dict(min_count=2),
                dict(det_min=0.25), dict(det_min=-1.0), dict(slot_mask=np.ones(168)), dict(axis="w"),
                dict(freqs=np.full(L.PROJ_MAX_ROWS // 4 + 1, 0.1)), dict(m=L.PROJ_MAX_SLOTS + 1), dict(n=L.PROJ_MAX_FRAMES + 1)):
        with pytest.raises(ValueError):
            _spectrum_args(**dict(good, **bad))
