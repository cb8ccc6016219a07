"""GPU tests of the displacement spectra (k_spectrum.hip; run on the MI355X box: `pytest -m gpu`): `engine.project_series_f64`,
`engine.harmonic_fit_f64`, `pipeline.spectral_analysis` and the sheet.

The projection's order of summation is not part of its interface (the order inside the float64 matrix instruction is not
documented), so it is held three ways (`tests/helpers/spectrum_oracle.py`): BIT FOR BIT to the NumPy restatement where every order
is exact (dyadic inputs) - which is what catches a wrong lane map or a wrong permutation -, within the DERIVED bound
gamma_(n+6) * sum |basis x| of exact rational arithmetic on float content, and bit for bit to ITSELF under every change of
batching.  The fit has a stated order and is held bit for bit to its restatement, fed the device's own projections.  No entry is
skipped or masked.  Shapes are the smallest at which the kernel can go wrong: around the 16-frame block of K and the chunk of
VBS_PROJ_CHUNK frames, the 16-row tile and the VBS_PROJ_ROWS rows of a workgroup, the 4-slot column tile and the VBS_PROJ_WG_SLOTS
slots of a workgroup, and the 64-lane walk over the bins; not the workload's.
"""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import spectra                                   # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import spectrum_oracle as O                                   # noqa: E402

CH, B, S, G = L.PROJ_CHUNK, L.PROJ_ROWS, L.PROJ_WG_SLOTS, L.FIT_GROUP
FRAMES = tuple(sorted({1, 3, 4, 5, 15, 16, 17, CH - 1, CH, CH + 1, 2 * CH + 3}))
ROWS = tuple(sorted({1, 2, 15, 16, 17, 33, B - 1, B, B + 1}))
SLOTS = tuple(sorted({1, 3, 4, 5, S - 1, S, S + 1, 130}))
BUDGET = 60000                                                # n R s of the exact side (rational arithmetic in Python)


def proj(rec, basis, nv=None):
    from vbs_amd.engine import project_series_f64
    return project_series_f64(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), torch.from_numpy(np.ascontiguousarray(basis)).cuda(),
                              nv).cpu().numpy()


def shape_of(n, k=0, budget=None):
    """The k-th shape for a frame count: R, s, cols, n_values rotate through their lists; with `budget`, R then s shrink until
    n R s stays below it."""
    i = FRAMES.index(n)
    R, s = ROWS[(2 * i + 3 * k + 1) % len(ROWS)], SLOTS[(3 * i + 5 * k + 2) % len(SLOTS)]
    if budget:
        while n * R * s > budget and R > 1:
            R = ROWS[ROWS.index(R) - 1]
        while n * R * s > budget and s > 1:
            s = SLOTS[SLOTS.index(s) - 1]
    nv = 1 + (i + k) % 3
    cols = nv + 1 + (i + 2 * k) % (8 - nv)
    return R, s, cols, nv


# every row count and every slot count is met by the rotation, and so is every n_values and every cols
_met = [shape_of(n, k) for n in FRAMES for k in range(3)]
assert {m[0] for m in _met} == set(ROWS) and {m[1] for m in _met} == set(SLOTS)
assert {m[3] for m in _met} == {1, 2, 3} and {m[2] for m in _met} == set(range(2, 9))


@pytest.mark.parametrize("n", FRAMES)
def test_dyadic_projections_equal_the_restatement_bit_for_bit(n):
    for k in range(3):
        R, s, cols, nv = shape_of(n, k)
        rec, basis = O.with_edges(*O.dyadic_case(n, R, s, cols, nv, seed=100 * n + k))
        want = O.project(rec, basis, nv)
        O.assert_bits(proj(rec, basis, nv), want, f"n {n} R {R} s {s} cols {cols} nv {nv}")
        if s > 1:
            assert not want[-1].any()                            # an all-invalid series
        if R > 1:
            assert not want[:, -1].any()                         # an all-zero basis row


@pytest.mark.parametrize("n", (5, CH + 1))
def test_dyadic_projections_on_every_row_and_slot_count(n):
    for R in ROWS:
        for s in SLOTS:
            rec, basis = O.dyadic_case(n, R, s, 4, 3, seed=R * 1000 + s)
            O.assert_bits(proj(rec, basis, 3), O.project(rec, basis, 3), f"n {n} R {R} s {s}")


@pytest.mark.parametrize("n", FRAMES)
def test_random_projections_lie_within_the_derived_bound(n):
    R, s, cols, nv = shape_of(n, 1, budget=BUDGET)
    rec, basis = O.with_edges(*O.random_case(n, R, s, cols, nv, seed=7000 + n, kind=None))
    got = proj(O.poison(rec, nv, np.nan), basis, nv)
    worst = O.check_within_bound(got, rec, basis, nv, what=f"n {n} R {R} s {s} nv {nv}")
    print(f"n {n} R {R} s {s} cols {cols} nv {nv}: largest error / bound = {worst:.3g}")
    for kind in (1e300, -np.inf):                                # NaN and 1e300 in every cell that must not be read change no bit
        O.assert_bits(proj(O.poison(rec, nv, kind), basis, nv), got, f"n {n}: poison {kind}")
    O.assert_bits(proj(rec, basis, nv), got, f"n {n}: ordinary numbers in the cells that are not read")


def test_projections_are_bit_identical_under_every_change_of_batching():
    from vbs_amd.engine import project_series_f64
    n, R, s = 2 * CH + 3, B + 1, 130
    rec, basis = O.random_case(n, R, s, 5, 3, seed=11)
    whole = proj(rec, basis)
    assert whole.shape == (s, R, 4) and np.isfinite(whole).all()
    O.assert_bits(proj(rec, basis), whole, "run to run")
    O.assert_bits(project_series_f64(rec, basis).cpu().numpy(), whole, "array against tensor input")
    for r in (0, 15, 16, B - 1, B):
        O.assert_bits(proj(rec, basis[r:r + 1]), whole[:, r:r + 1], f"row {r} alone")
    O.assert_bits(proj(rec, basis[5:40]), whole[:, 5:40], "rows 5:40 at other positions of their tiles")
    for i in (0, 3, S - 1, S, 129):
        O.assert_bits(proj(rec[:, i:i + 1], basis), whole[i:i + 1], f"series {i} alone")
    O.assert_bits(proj(rec[:, 2:S + 3], basis), whole[2:S + 3], "series 2 .. at other positions of their tiles")
    r = np.random.default_rng(12)
    for s2 in (131, 131 + S, 160):                               # the same workgroup, one more, several more
        rec2 = np.full((n, s2, 5), np.nan)
        rec2[:, :s] = rec
        rec2[:, s:, 0] = 0.0
        got = proj(rec2, basis)
        O.assert_bits(got[:s], whole, f"{s} slots with dead slots appended to {s2}")
        assert not got[s:].any()
    for n2 in (n + 1, 3 * CH, 3 * CH + 1):                       # one more frame, to the end of the chunk, into the next chunk
        rec2 = np.full((n2, s, 5), np.nan)
        rec2[:n] = rec
        rec2[n:, :, 0] = 0.0
        basis2 = np.ascontiguousarray(np.concatenate([basis, r.uniform(-1.0, 1.0, (R, n2 - n))], axis=1))
        O.assert_bits(proj(rec2, basis2), whole, f"{n} frames with dead frames appended to {n2}")


def hfit(p, Q, mc=8, dm=1e-3, **kw):
    from vbs_amd.engine import harmonic_fit_f64
    fit, peak = harmonic_fit_f64(torch.from_numpy(np.ascontiguousarray(p)).cuda(), Q, mc, dm, **kw)
    return (None if fit is None else fit.cpu().numpy()), (None if peak is None else peak.cpu().numpy())


@pytest.mark.parametrize("Q", (1, 63, 64, 65, 130))
def test_fit_equals_the_restatement_bit_for_bit(Q):
    n = 60
    r = np.random.default_rng(Q)
    nu = r.uniform(0.2 / n, 0.25, Q)                             # down to frequencies too low to be told from the mean
    nu[Q // 2] = 0.11                                            # (the line's own bin is not one of those)
    basis = spectra.harmonic_basis(n, nu)
    for j, s in enumerate(sorted({1, G - 1, G + 1})):
        nv = 1 + (j + Q) % 3
        rec = np.zeros((n, s, nv + 1))
        rec[..., 0] = r.random((n, s)) >= 0.1
        rec[..., 1:] = 0.3 * r.standard_normal((n, s, nv))
        rec[..., 1] += np.cos(2 * np.pi * nu[Q // 2] * np.arange(n) - 0.7)[:, None]        # a line on a bin in value 1
        if s > 1:
            rec[7:, -1, 0] = 0.0                                 # a series with 7 frames at the most: below min_count
        p = proj(rec, basis, nv)                                 # the device's own projections: this test inherits no tolerance
        want_fit, want_peak = O.harmonic_fit(p, Q, 8, 1e-3)
        fit, peak = hfit(p, Q)
        O.assert_bits(fit, want_fit, f"Q {Q} s {s} nv {nv}: fit")
        O.assert_bits(peak, want_peak, f"Q {Q} s {s} nv {nv}: peak")
        only_fit, none = hfit(p, Q, want_peak=False)
        assert none is None
        O.assert_bits(only_fit, want_fit, f"Q {Q} s {s}: fit with a null peak")
        none, only_peak = hfit(p, Q, want_fit=False)
        assert none is None
        O.assert_bits(only_peak, want_peak, f"Q {Q} s {s}: peak with a null fit")
        assert want_fit[0, :, 0].any() and want_peak[0, 0, 0] == 2.0 and (s == 1 or want_peak[-1, 0, 0] == 0.0)


def test_fit_rules_on_hand_built_projections():
    p = O.hand_proj()
    fit, peak = hfit(p, O.HAND_Q, O.HAND_MIN_COUNT, O.HAND_DET_MIN)
    want_fit, want_peak = O.harmonic_fit(p, O.HAND_Q, O.HAND_MIN_COUNT, O.HAND_DET_MIN)
    O.assert_bits(fit, want_fit, "hand-built: fit")
    O.assert_bits(peak, want_peak, "hand-built: peak")
    O.check_hand(fit, peak)
    rec, nu = O.low_frequency_case()
    p = proj(rec, spectra.harmonic_basis(rec.shape[0], nu), 1)
    fit, peak = hfit(p, 2)
    want_fit, want_peak = O.harmonic_fit(p, 2, 8, 1e-3)
    O.assert_bits(fit, want_fit, "low frequency: fit")
    O.assert_bits(peak, want_peak, "low frequency: peak")
    assert fit[0, 0].tolist() == [0.0, 0.0, 0.0, 0.0] and fit[0, 1, 0] == 1.0 and peak[0, 0, 3] == 1.0


def test_wrappers_refuse_what_the_entries_refuse():
    from vbs_amd.engine import harmonic_fit_f64, project_series_f64
    rec, basis = O.dyadic_case(12, 9, 3, 4, 3, seed=1)
    assert project_series_f64(rec, basis).shape == (3, 9, 4) and project_series_f64(rec, basis, n_values=1).shape == (3, 9, 2)
    for bad in (dict(n_values=4), dict(n_values=0)):
        with pytest.raises(ValueError):
            project_series_f64(rec, basis, **bad)
    with pytest.raises(ValueError):
        project_series_f64(rec, basis[:, :11])
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}"):
        project_series_f64(np.zeros((2, L.PROJ_MAX_SLOTS + 1, 2)), np.zeros((1, 2)))
    p = project_series_f64(rec, basis)
    fit, peak = harmonic_fit_f64(p, 2)
    assert fit.shape == (3, 2, 10) and peak.shape == (3, 3, L.PEAK_COLS)
    for bad in (dict(Q=3), dict(Q=2, min_count=2), dict(Q=2, det_min=0.25), dict(Q=2, want_fit=False, want_peak=False)):
        with pytest.raises(ValueError):
            harmonic_fit_f64(p, **bad)


def test_spectral_analysis_finds_the_line_and_its_phase_map():
    from vbs_amd import filters as F
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, phi = O.line_table()
    n, m = t.shape[0], t.shape[1]
    nu = spectra.zoom_grid(O.LINE_NU0, 2.0 / n, 33)
    FIT_TOL = O.fit_tol()
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        res = PL.spectral_analysis(eng, torch.from_numpy(t).cuda(), nu, taps=F.moving_average_taps(O.LINE_TAPS), fps=120.0)
        mc = max(8, n // 4)
        basis = spectra.harmonic_basis(n, nu)
        angle = math.degrees(math.atan(FIT_TOL / O.LINE_AMP))
        print(f"FIT_TOL = {FIT_TOL:.3g}, the angle it subtends at {O.LINE_AMP} = {angle:.3g} deg")
        for name, peak, fit, rows in (("", res["peak"], res["fit"], res["marker"]), ("total_", res["total_peak"], res["total_fit"],
                                                                                    res["total"][None])):
            series = res[name + "series"].cpu().numpy()
            peak, fit = peak.cpu().numpy(), fit.cpu().numpy()
            k = series.shape[1]
            # on the reference side alone first: enough frames everywhere, and a runner-up that no rounding can promote
            assert (series[..., 0] != 0).sum(axis=0).min() >= mc
            ref_fit, ref_peak = O.harmonic_fit(O.project(series, basis, 3), 33, mc, 1e-3)
            p = np.sort(ref_fit[:, :, 9], axis=1)
            assert (ref_peak[:, 2, 3] == 16.0).all() and (p[:, -2] / p[:, -1]).max() < 0.99
            print(f"{name or 'markers'}: runner-up / peak at most {(p[:, -2] / p[:, -1]).max():.3g}")
            assert (peak[:, 2, 0] == 2.0).all() and (peak[:, 2, 3] == 16.0).all()    # every series peaks on the centre bin
            worst = worst_angle = 0.0
            for i in range(k):
                _, a, b = O.lstsq_fit(series[:, i, 3], series[:, i, 0] != 0, nu[16])
                worst = max(worst, abs(peak[i, 2, 4] - a), abs(peak[i, 2, 5] - b))
                d = (rows[i, 2, 2] - math.degrees(math.atan2(b, a)) + 180.0) % 360.0 - 180.0
                worst_angle = max(worst_angle, abs(d))
                assert rows[i, 2, 1] == np.hypot(peak[i, 2, 4], peak[i, 2, 5]) and rows[i, 2, 0] == nu[16]
                assert rows[i, 2, 5] == (series[:, i, 0] != 0).sum() and 0.9 < rows[i, 2, 4] <= 1.0 + 1e-12     # explained
            print(f"{name or 'markers'}: largest |a, b - lstsq| = {worst:.3g}, largest phase difference = {worst_angle:.3g} deg")
            assert worst <= FIT_TOL and worst_angle <= angle
            O.assert_bits(fit[:, 16, 7:10], peak[:, 2, 4:7], "the peak is the fit's centre bin")
        assert res["common_bin"] == 16 and res["common_freq"] == nu[16] and res["common_freq_hz"] == nu[16] * 120.0
        assert res["common_power"].shape == (33,) and res["freqs_hz"].shape == (33,)
        pm = res["phase_map"]
        assert pm.shape == (m, 3) and (pm[:, 0] == 1.0).all() and np.array_equal(pm[:, 1:], res["marker"][:, 2, 1:3])
        d = (pm[:, 2] - np.degrees(phi) + 180.0) % 360.0 - 180.0
        print(f"phase map against the markers' polar angles: at most {np.abs(d).max():.3g} deg off")
        assert np.abs(d).max() < 0.5 and np.abs(pm[:, 1] - O.LINE_AMP).max() < 0.01
        df = PL.to_spectrum_frame(res["marker"], fps=120.0)
        assert tuple(df.columns) == PL.SPECTRUM_FRAME_COLUMNS + ("freq_hz",) and len(df) == 3 * m
        z = df[df["axis"] == "z"]
        assert (z["freq"] == nu[16]).all() and not z["amplitude"].isna().any() and (z["marker_id"].to_numpy() == np.arange(1, m + 1)).all()
        with pytest.raises(ValueError):
            PL.spectral_analysis(eng, torch.from_numpy(t).cuda(), [0.3])
    finally:
        eng.close()
