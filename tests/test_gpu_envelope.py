"""GPU tests of the time-resolved fit (k_envelope.hip; run on the MI355X box: `pytest -m gpu`): `engine.window_moments_f64`,
`engine.window_fit_f64`, `pipeline.envelope_analysis` and the sheet.

The moments' order of summation is not part of their interface (the order inside the float64 matrix instruction is not
documented), so they are held three ways (`tests/helpers/envelope_oracle.py`): BIT FOR BIT to the loop restatement where every
order is exact (dyadic inputs) - which is what catches a wrong lane map, band offset or column flattening -, within the DERIVED
bound gamma_(K+8) * sum w |term| of exact rational arithmetic on float content, and bit for bit to THEMSELVES under every change
of batching.  The fit has a stated order and is held bit for bit to its restatement, fed the device's own moments.  No entry is
skipped or masked.  Shapes are the smallest at which the kernel can go wrong: around the 16-frame tile and the VBS_ENV_TILE frames
of a workgroup, windows shorter and longer than a tile and than the staged chunk, column counts whose M = 9, 13, 17 sums make
tiles straddle slots and workgroups; not the workload's.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import spectra                                   # noqa: E402
from vbs_amd.filters import half_taps                         # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import envelope_oracle as O                                   # noqa: E402

T = L.ENV_TILE
FRAMES = tuple(sorted({1, 2, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3}))
HALVES = (0, 1, 7, 8, 31, 127)
SLOTS = (1, 3, 4, 15, 16, 17, 65, 130)
BUDGET = 300000                                               # frames x window x s x M of the exact side (rational arithmetic)


def full(half):
    """Half taps -> the full symmetric window the wrapper takes."""
    half = np.asarray(half, np.float64)
    return np.concatenate([half[:0:-1], half])


def mom(rec, car, half, nv=None, rng=None):
    from vbs_amd.engine import window_moments_f64
    return window_moments_f64(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), torch.from_numpy(np.ascontiguousarray(car)).cuda(),
                              full(half), nv, rng).cpu().numpy()


def shape_of(n, k=0, budget=None):
    """The k-th shape for a frame count: h, s, cols, n_values rotate through their lists; with `budget`, s shrinks until the
    exact side's work stays below it."""
    i = FRAMES.index(n)
    h, s = HALVES[(i + 2 * k) % len(HALVES)], SLOTS[(3 * i + 5 * k + 2) % len(SLOTS)]
    nv = 1 + (i + k) % 3
    cols = nv + 1 + (i + 2 * k) % (8 - nv)
    if budget:
        while n * min(n, 2 * h + 1) * s * O.n_sums(nv) > budget and s > 1:
            s = SLOTS[SLOTS.index(s) - 1]
    return h, s, cols, nv


# every half width and every slot count is met by the rotation, and so is every n_values and every cols
_met = [shape_of(n, k) for n in FRAMES for k in range(3)]
assert {m[0] for m in _met} == set(HALVES) and {m[1] for m in _met} == set(SLOTS)
assert {m[3] for m in _met} == {1, 2, 3} and {m[2] for m in _met} == set(range(2, 9))


@pytest.mark.parametrize("n", FRAMES)
def test_dyadic_moments_equal_the_restatement_bit_for_bit(n):
    for k in range(3):
        h, s, cols, nv = shape_of(n, k)
        rec, car = O.dyadic_case(n, s, cols, nv, seed=100 * n + k)
        if s > 1:
            rec[:, -1, 0] = 0.0                                  # an all-invalid series
        if n > 1:
            rec[1, :, 0] = 0.0                                   # an all-invalid frame
        half = O.dyadic_half(h, n + k)
        want = O.moments(rec, car, half, nv)
        O.assert_bits(mom(rec, car, half, nv), want, f"n {n} h {h} s {s} cols {cols} nv {nv}")
        if s > 1:
            assert not want[:, -1].any()


@pytest.mark.parametrize("n", (17, T + 1))
def test_dyadic_moments_on_every_half_width_and_slot_count(n):
    for h in HALVES:
        for j, s in enumerate(SLOTS):
            nv = 1 + (j + h) % 3
            rec, car = O.dyadic_case(n, s, 4, nv, seed=h * 1000 + s)
            half = O.dyadic_half(h, h + s)
            O.assert_bits(mom(rec, car, half, nv), O.moments(rec, car, half, nv), f"n {n} h {h} s {s} nv {nv}")


@pytest.mark.parametrize("n", FRAMES)
def test_random_moments_lie_within_the_derived_bound(n):
    h, s, cols, nv = shape_of(n, 1, budget=BUDGET)
    rec, car = O.random_case(n, s, cols, nv, seed=7000 + n, kind=None)
    if s > 1:
        rec[:, -1, 0] = 0.0
    half = half_taps(spectra.window_taps(h))
    got = mom(O.poison(rec, nv, np.nan), car, half, nv)
    worst = O.check_within_bound(got, rec, car, half, nv, what=f"n {n} h {h} s {s} nv {nv}")
    print(f"n {n} h {h} s {s} cols {cols} nv {nv}: largest error / bound = {worst:.3g}")
    for kind in (1e300, -np.inf):                                # NaN and 1e300 in every cell that must not be read change no bit
        O.assert_bits(mom(O.poison(rec, nv, kind), car, half, nv), got, f"n {n}: poison {kind}")
    O.assert_bits(mom(rec, car, half, nv), got, f"n {n}: ordinary numbers in the cells that are not read")


@pytest.mark.parametrize("kind", ("all", "none", "long", "ends"))
def test_gap_kinds(kind):
    for n, h, s, nv in ((T + 1, 7, 3, 3), (2 * T + 3, 31, 17, 2), (40, 127, 1, 1)):
        rec, car = O.dyadic_case(n, s, nv + 2, nv, seed=n + h, kind=None)
        rec = O.poison(O.gaps(rec, kind, h), nv, np.nan)
        half = O.dyadic_half(h, n)
        got = mom(rec, car, half, nv)
        O.assert_bits(got, O.moments(rec, car, half, nv), f"{kind}: n {n} h {h} s {s}")
        if kind == "none":
            assert not got[:, 0].any() and not got[:, -1].any()  # no valid frame in any window: exact zeros
        if kind == "long" and n > 4 * h + 6:
            assert not got[n // 2, 0].any()                      # a window inside the gap


def test_moments_are_bit_identical_under_every_change_of_batching():
    from vbs_amd.engine import window_moments_f64
    n, s, h = 2 * T + 3, 130, 8
    rec, car = O.random_case(n, s, 5, 3, seed=11)
    half = half_taps(spectra.window_taps(h))
    whole = mom(rec, car, half)
    assert whole.shape == (n, s, 17) and np.isfinite(whole).all()
    O.assert_bits(mom(rec, car, half), whole, "run to run")
    O.assert_bits(window_moments_f64(rec, car, full(half)).cpu().numpy(), whole, "array against tensor input")
    for a, b in ((0, 1), (5, 70), (T - 1, T + 1), (T, 2 * T), (100, n), (n - 1, n), (16, 32)):
        O.assert_bits(mom(rec, car, half, None, (a, b)), whole[a:b], f"range {a}:{b}")
    assert mom(rec, car, half, None, (17, 17)).shape == (0, s, 17)
    for i in (0, 3, 15, 16, 129):
        O.assert_bits(mom(rec[:, i:i + 1], car, half), whole[:, i:i + 1], f"series {i} alone")
    O.assert_bits(mom(rec[:, 2:19], car, half), whole[:, 2:19], "series 2 .. at other positions of their tiles")
    r = np.random.default_rng(12)
    for s2 in (131, 134, 160):                                   # the same workgroup, one more, several more
        rec2 = np.full((n, s2, 5), np.nan)
        rec2[:, :s] = rec
        rec2[:, s:, 0] = 0.0
        got = mom(rec2, car, half)
        O.assert_bits(got[:, :s], whole, f"{s} slots with dead slots appended to {s2}")
        assert not got[:, s:].any()
    for n2 in (n + 1, 3 * T, 3 * T + 1):                         # one more frame, to the end of the tile, into the next tile
        rec2 = np.full((n2, s, 5), np.nan)
        rec2[:n] = rec
        rec2[n:, :, 0] = 0.0
        car2 = np.ascontiguousarray(np.concatenate([car, r.uniform(-1.0, 1.0, (4, n2 - n))], axis=1))
        got = mom(rec2, car2, half)
        O.assert_bits(got[:n], whole, f"{n} frames with dead frames appended to {n2}")
        assert not got[n + h:].any()


def wfit(m, sw, mc=0.5, dm=1e-3):
    from vbs_amd.engine import window_fit_f64
    return window_fit_f64(torch.from_numpy(np.ascontiguousarray(m)).cuda(), sw, mc, dm).cpu().numpy()


@pytest.mark.parametrize("h", (0, 3, 24))
def test_fit_equals_the_restatement_bit_for_bit(h):
    n = 197
    r = np.random.default_rng(h)
    f = np.arange(n, dtype=np.float64)
    for j, s in enumerate((1, 5, 300)):
        nv = 1 + (j + h) % 3
        rec = np.zeros((n, s, nv + 1))
        rec[..., 0] = r.random((n, s)) >= 0.1
        rec[..., 1:] = 0.05 * r.standard_normal((n, s, nv))
        rec[..., 1] += (O.burst_envelope(n) * np.cos(2 * np.pi * 0.0837 * f - 0.7))[:, None]
        if s > 1:
            rec[60:140, -1, 0] = 0.0                             # a gap longer than the window: W = 0 inside it
        half = half_taps(spectra.window_taps(h))
        sw = O.taps_sum(half)
        m = mom(rec, spectra.carrier(n, 0.0837), half, nv)       # the device's own moments: this test inherits no tolerance
        want = O.window_fit(m, sw)
        O.assert_bits(wfit(m, sw), want, f"h {h} s {s} nv {nv}")
        if h == 0:
            assert not want.any()                                # one frame: det is 0 up to rounding, nothing is ok
        else:
            assert want[:, 0, 0].any() and (s == 1 or not want[70:130, -1].any())
        for mc, dm in ((1.0, 0.0), (0.9, 0.2)):
            O.assert_bits(wfit(m, sw, mc, dm), O.window_fit(m, sw, mc, dm), f"h {h} s {s}: min_coverage {mc} det_min {dm}")


def test_fit_rules_on_hand_built_moments():
    m = O.hand_moments()
    fit = wfit(m, O.HAND_SW, O.HAND_COVERAGE, O.HAND_DET_MIN)
    O.assert_bits(fit, O.window_fit(m, O.HAND_SW, O.HAND_COVERAGE, O.HAND_DET_MIN), "hand-built")
    O.check_hand(fit)


def test_wrappers_refuse_what_the_entries_refuse():
    from vbs_amd.engine import taps_sum, window_fit_f64, window_moments_f64
    rec, car = O.dyadic_case(12, 3, 4, 3, seed=1)
    w = spectra.window_taps(2)
    assert window_moments_f64(rec, car, w).shape == (12, 3, 17) and window_moments_f64(rec, car, w, n_values=1).shape == (12, 3, 9)
    assert window_moments_f64(rec, car, w, frame_range=(3, 7)).shape == (4, 3, 17)
    for bad in (dict(n_values=4), dict(n_values=0), dict(frame_range=(0, 13)), dict(frame_range=(5, 4))):
        with pytest.raises(ValueError):
            window_moments_f64(rec, car, w, **bad)
    for bad in (lambda: window_moments_f64(rec, car[:, :11], w), lambda: window_moments_f64(rec, car, np.ones(2 * L.ENV_MAX_HALF + 3)),
                lambda: window_moments_f64(rec, car, [1.0, 2.0]), lambda: window_moments_f64(rec, car, [-1.0, 1.0, -1.0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}"):
        window_moments_f64(np.zeros((2, L.PROJ_MAX_SLOTS + 1, 2)), np.zeros((4, 2)), w)
    m = window_moments_f64(rec, car, w)
    sw = taps_sum(half_taps(w))
    assert sw == O.taps_sum(half_taps(w)) and window_fit_f64(m, sw).shape == (12, 3, 16)
    for bad in (dict(taps_sum=0.0), dict(taps_sum=sw, min_coverage=0.0), dict(taps_sum=sw, det_min=0.25)):
        with pytest.raises(ValueError):
            window_fit_f64(m, **bad)
    with pytest.raises(ValueError):
        window_fit_f64(m[..., :10], sw)


def test_envelope_analysis_finds_the_switch_on_and_where_it_is_loudest():
    from vbs_amd import fields
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, gain = O.switch_on_table()
    n, m = t.shape[0], t.shape[1]
    h = O.ON_HALF
    ENV_TOL = O.env_tol()
    nodes = t[0, :, 6:8].astype(np.float64)
    grid_xy, _ = fields.grid_over(nodes, (13, 13), 0.0)          # a grid point every half marker spacing
    W = fields.gaussian_weights(nodes, grid_xy, 0.75)
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        res = PL.envelope_analysis(eng, torch.from_numpy(t).cuda(), {"common_freq": O.ON_NU0}, half_window=h, fps=120.0,
                                   grid=(W, fields.row_sums(W)))
        car = spectra.carrier(n, O.ON_NU0)
        half = half_taps(spectra.window_taps(h))
        print(f"ENV_TOL = {ENV_TOL:.3g}")
        for name in ("", "total_"):
            series, fit = res[name + "series"].cpu().numpy(), res[name + "fit"].cpu().numpy()
            assert series.shape == (n, m if not name else 1, 4) and fit.shape == series.shape[:2] + (16,)
            O.assert_bits(fit, O.window_fit(mom(series, car, half, 3), res["taps_sum"]), f"{name}fit is the fit of the moments")
            worst, count = 0.0, 0
            for i in range(series.shape[1]):
                valid = series[:, i, 0] != 0
                for f in np.nonzero(fit[:, i, 0])[0]:
                    c0, a, b = O.lstsq_window(series[:, i, 3], valid, car, half, int(f))
                    worst = max(worst, abs(fit[f, i, 14] - c0), abs(fit[f, i, 11] - a), abs(fit[f, i, 12] - b))
                    count += 1
            print(f"{name or 'markers'}: largest |c0, a, b - weighted lstsq| = {worst:.3g} over {count} ok windows")
            assert count > 0.5 * n * series.shape[1] * (1.0 if not name else 0.2) and worst <= ENV_TOL
        amp, summary = res["amplitude"], res["summary"]
        assert amp.shape == (n, m, 3) and summary.shape == (m, 3, 5) and res["freq_dev"].shape == (m, 3)
        onset = summary[:, 2, 3]
        print(f"onsets {onset.min():.0f} .. {onset.max():.0f} against {O.ON_FRAME}; peak amplitude of the loudest marker "
              f"{summary[O.ON_LOUD, 2, 0]:.4f} against {O.ON_AMP}")
        assert (np.abs(onset - O.ON_FRAME) <= h).all()           # every marker's onset within h of the switch-on
        assert np.abs(summary[:, 2, 0] - O.ON_AMP * gain).max() < 0.02 * O.ON_AMP and int(np.argmax(summary[:, 2, 0])) == O.ON_LOUD
        assert np.nanmax(np.abs(amp[O.ON_FRAME + h + 1:n - h, :, 2] - (O.ON_AMP * gain)[None, :])) < 1e-3
        assert np.nanmax(amp[:O.ON_FRAME - h - 1, :, 2]) < 1e-6
        amap = res["amplitude_map"].cpu().numpy()
        assert amap.shape == (n, 169, 2)
        f = n - h - 5
        assert amap[f, :, 0].all()
        peak = grid_xy[int(np.argmax(amap[f, :, 1]))]
        print(f"amplitude map of frame {f}: peak at {peak}, the loudest marker at {nodes[O.ON_LOUD]}")
        assert np.abs(peak - nodes[O.ON_LOUD]).max() <= 0.5 + 1e-9      # within one grid cell
        assert res["nu"] == O.ON_NU0 and res["nu_hz"] == O.ON_NU0 * 120.0 and res["total_summary"].shape == (3, 5)
        assert res["total_amplitude"].shape == (n, 3) and res["total_freq_dev_hz"].shape == (3,)
        df = PL.to_envelope_frame(res, fps=120.0)
        assert tuple(df.columns) == PL.ENVELOPE_FRAME_COLUMNS + ("time_s",) and len(df) == 3 * m * n
        z = df[df["axis"] == "z"]
        assert np.array_equal(z["amplitude"].to_numpy().reshape(n, m), amp[..., 2], equal_nan=True)
        assert (z["marker_id"].to_numpy()[:m] == np.arange(1, m + 1)).all() and z["frameno"].iloc[-1] == n
        with pytest.raises(ValueError):
            PL.envelope_analysis(eng, torch.from_numpy(t).cuda(), 0.3)
    finally:
        eng.close()
