"""GPU tests of the local polynomial fit along time (k_kinematics.hip; run on the MI355X box: `pytest -m gpu`):
`engine.poly_moments_f64`, `engine.poly_fit_f64`, `pipeline.kinematic_analysis`, `pipeline.fill_table` and the sheet.

The moments' order of summation is not part of their interface (the order inside the float64 matrix instruction is not
documented), so they are held three ways (`tests/helpers/kinematics_oracle.py`): BIT FOR BIT to the loop restatement where every
order is exact (dyadic inputs within the bit budget written next to `dyadic_case`) - which is what catches a wrong lane map, band
offset, tap row or scatter into `mom` -, within the DERIVED bound gamma_(K+8) * sum |tap term| of exact rational arithmetic on
float content, and bit for bit to THEMSELVES under every change of batching.  The fit has a stated order and is held bit for bit to
its restatement, fed the device's own moments.  No entry is skipped or masked.  Shapes are the smallest at which the kernel can go
wrong: around the 16-frame tile, the 16-frame staged chunk and the VBS_KIN_TILE frames of a workgroup, windows shorter and longer
than a tile, slot counts around the 4 slots of a value tile and the 16 of a workgroup; not the workload's.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import filters                                   # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import kinematics_oracle as O                                 # noqa: E402

FRAMES = (1, 15, 16, 17, 63, 64, 65, 131)
SLOTS = (1, 3, 4, 5, 17, 130)
HALVES = (0, 1, 7, 31, 127)
DEGREES = (0, 1, 2, 3)
BUDGET = 250000                                               # frames x window x s x M of the exact side (rational arithmetic)


def mom(rec, h, d, w="hann", nv=None, rng=None):
    from vbs_amd.engine import poly_moments_f64
    return poly_moments_f64(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), h, d, w, nv, rng).cpu().numpy()


def pfit(m, rec, h, d, w="hann", nv=None, mc=0.5, pr=O.PIV_REL, fd=1, rng=None):
    from vbs_amd.engine import poly_fit_f64
    fit, filled = poly_fit_f64(torch.from_numpy(np.ascontiguousarray(m)).cuda(), torch.from_numpy(np.ascontiguousarray(rec)).cuda(), h, d, w,
                               nv, mc, pr, fd, True, rng)
    return fit.cpu().numpy(), filled.cpu().numpy()


def shape_of(n, k=0):
    """The k-th shape for a frame count: h, d, s, cols, n_values rotate through their lists."""
    i = FRAMES.index(n)
    h, d = HALVES[(i + 2 * k) % len(HALVES)], DEGREES[(i + k) % len(DEGREES)]
    s = SLOTS[(3 * i + 5 * k + 2) % len(SLOTS)]
    nv = 1 + (i + k) % 3
    cols = nv + 1 + (i + 2 * k) % (8 - nv)
    return h, d, s, cols, nv


# every half width, degree and slot count is met by the rotation, and so is every n_values and every cols
_met = [shape_of(n, k) for n in FRAMES for k in range(4)]
assert {m[0] for m in _met} == set(HALVES) and {m[1] for m in _met} == set(DEGREES) and {m[2] for m in _met} == set(SLOTS)
assert {m[4] for m in _met} == {1, 2, 3} and {m[3] for m in _met} == set(range(2, 9))
assert (127, 3) in {(m[0], m[1]) for m in _met}


@pytest.mark.parametrize("n", FRAMES)
def test_dyadic_moments_equal_the_restatement_bit_for_bit(n):
    for k in range(4):
        h, d, s, cols, nv = shape_of(n, k)
        rec, w, budget = O.dyadic_case(n, s, cols, nv, h, d, seed=100 * n + k)
        assert budget <= 53
        if s > 1:
            rec[:, -1, 0] = 0.0                                  # an all-invalid series
        if n > 1:
            rec[1, :, 0] = 0.0                                   # an all-invalid frame
        want = O.moments(rec, O.taps(h, d, w), d, nv)
        O.assert_bits(mom(rec, h, d, w, nv), want, f"n {n} h {h} d {d} s {s} cols {cols} nv {nv}")
        if s > 1:
            assert not want[:, -1].any()


@pytest.mark.parametrize("d", DEGREES)
def test_dyadic_moments_on_every_half_width_and_slot_count(d):
    n = 33                                                       # (two tiles and a frame; the frame counts above go further)
    for h in HALVES:
        for j, s in enumerate(SLOTS):
            nv = 1 + (j + h) % 3
            rec, w, _ = O.dyadic_case(n, s, 4, nv, h, d, seed=h * 1000 + s)
            O.assert_bits(mom(rec, h, d, w, nv), O.moments(rec, O.taps(h, d, w), d, nv), f"n {n} h {h} d {d} s {s} nv {nv}")


@pytest.mark.parametrize("n", FRAMES)
def test_random_moments_lie_within_the_derived_bound(n):
    h, d, s, cols, nv = shape_of(n, 1)
    while n * min(n, 2 * h + 1) * s * O.n_sums(d, nv) > BUDGET and s > 1:
        s = SLOTS[SLOTS.index(s) - 1]
    rec = O.random_case(n, s, cols, nv, seed=7000 + n, kind=None)
    if s > 1:
        rec[:, -1, 0] = 0.0
    kind = ("hann", "rect")[n % 2]
    got = mom(O.poison(rec, nv, np.nan), h, d, kind, nv)
    worst = O.check_within_bound(got, rec, O.taps(h, d, kind), d, nv, what=f"n {n} h {h} d {d} s {s} nv {nv}")
    print(f"n {n} h {h} d {d} s {s} cols {cols} nv {nv} {kind}: largest error / bound = {worst:.3g}")
    for poison in (1e300, -np.inf):                              # NaN and 1e300 in every cell that must not be read change no bit
        O.assert_bits(mom(O.poison(rec, nv, poison), h, d, kind, nv), got, f"n {n}: poison {poison}")
    O.assert_bits(mom(rec, h, d, kind, nv), got, f"n {n}: ordinary numbers in the cells that are not read")


@pytest.mark.parametrize("kind", ("all", "none", "long", "ends"))
def test_gap_kinds(kind):
    for n, h, d, s, nv in ((65, 7, 2, 3, 3), (131, 31, 3, 17, 2), (40, 127, 1, 1, 1)):
        rec, w, _ = O.dyadic_case(n, s, nv + 2, nv, h, d, seed=n + h, kind=None)
        rec = O.poison(O.gaps(rec, kind, h), nv, np.nan)
        got = mom(rec, h, d, w, nv)
        O.assert_bits(got, O.moments(rec, O.taps(h, d, w), d, nv), f"{kind}: n {n} h {h} s {s}")
        if kind == "none":
            assert not got[:, 0].any() and not got[:, -1].any()  # no valid frame in any window: exact zeros
        if kind == "long" and n > 4 * h + 6:
            assert not got[n // 2, 0].any()                      # a window inside the gap


def test_moments_are_bit_identical_under_every_change_of_batching():
    from vbs_amd.engine import poly_moments_f64
    T = L.KIN_TILE
    n, s, h, d = 2 * T + 3, 130, 8, 3
    rec = O.random_case(n, s, 5, 3, seed=11)
    whole = mom(rec, h, d)
    M = O.n_sums(d, 3)
    assert whole.shape == (n, s, M) and np.isfinite(whole).all()
    O.assert_bits(mom(rec, h, d), whole, "run to run")
    O.assert_bits(poly_moments_f64(rec, h, d).cpu().numpy(), whole, "array against tensor input")
    for a, b in ((0, 1), (5, 70), (T - 1, T + 1), (T, 2 * T), (100, n), (n - 1, n), (16, 32)):
        O.assert_bits(mom(rec, h, d, "hann", None, (a, b)), whole[a:b], f"range {a}:{b}")
    assert mom(rec, h, d, "hann", None, (17, 17)).shape == (0, s, M)
    for i in (0, 3, 15, 16, 129):
        O.assert_bits(mom(rec[:, i:i + 1], h, d), whole[:, i:i + 1], f"series {i} alone")
    O.assert_bits(mom(rec[:, 2:19], h, d), whole[:, 2:19], "series 2 .. at other positions of their tiles")
    for s2 in (131, 134, 160):                                   # the same workgroup, one more, several more
        rec2 = np.full((n, s2, 5), np.nan)
        rec2[:, :s] = rec
        rec2[:, s:, 0] = 0.0
        got = mom(rec2, h, d)
        O.assert_bits(got[:, :s], whole, f"{s} slots with dead slots appended to {s2}")
        assert not got[:, s:].any()
    for n2 in (n + 1, 3 * T, 3 * T + 1):                         # one more frame, to the end of the tile, into the next tile
        rec2 = np.full((n2, s, 5), np.nan)
        rec2[:n] = rec
        rec2[n:, :, 0] = 0.0
        got = mom(rec2, h, d)
        O.assert_bits(got[:n], whole, f"{n} frames with dead frames appended to {n2}")
        assert not got[n + h:].any()


def restated_fit(m, rec, h, d, w, nv, mc=0.5, pr=O.PIV_REL, fd=1, rng=None):
    tp = O.taps(h, d, w)
    sw, piv = O.full_pivots(tp, d)
    a, b = (0, rec.shape[0]) if rng is None else rng
    return O.fit(m, rec[a:b], O.thresholds(sw, piv, mc, pr, h), h, d, nv, fd)


@pytest.mark.parametrize("h,d", ((0, 1), (3, 1), (7, 2), (24, 3), (1, 3)))
def test_fit_equals_the_restatement_bit_for_bit(h, d):
    n = 197
    r = np.random.default_rng(h)
    for j, s in enumerate((1, 5, 300)):
        nv = 1 + (j + h) % 3
        cols = nv + 1 + j
        rec = np.zeros((n, s, cols))
        rec[..., 0] = r.random((n, s)) >= 0.1
        rec[..., 1:] = 0.05 * r.standard_normal((n, s, cols - 1))
        rec[..., 1] += O.press_case(n, seed=j)[:, :, 1]
        if s > 1:
            rec[60:140, -1, 0] = 0.0                             # a gap longer than the window
        kind = ("hann", "rect")[j % 2]
        m = mom(rec, h, d, kind, nv)                             # the device's own moments: this test inherits no tolerance
        for mc, pr, fd in ((0.5, O.PIV_REL, 1), (0.05, O.PIV_REL, 0), (1.0, 0.0, 1), (0.2, 0.3, d)):
            dead = O.poison(rec, nv)                             # NaN in every cell that must not be read; valid rows travel whole
            fit, filled = pfit(m, dead, h, d, kind, nv, mc, pr, fd)
            want, wfilled = restated_fit(m, dead, h, d, kind, nv, mc, pr, fd)
            O.assert_bits(fit, want, f"h {h} d {d} s {s} nv {nv}: min_coverage {mc} piv_rel {pr}")
            O.assert_bits(filled, wfilled, f"h {h} d {d} s {s} nv {nv}: filled, fill_degree {fd}")
        fit, filled = pfit(m[40:150], rec, h, d, kind, nv, rng=(40, 150))
        want, wfilled = restated_fit(m[40:150], rec, h, d, kind, nv, rng=(40, 150))
        O.assert_bits(fit, want, "a range of frames")
        O.assert_bits(filled, wfilled, "a range of frames: filled")
        q = want[..., 1]
        if 2 * h + 1 <= d:
            assert (q < d).all()                                 # fewer frames than coefficients: never full
        elif h >= 3:
            assert (q == d).sum() > 0.5 * q.size


def test_fit_rules_on_hand_built_moments():
    import ctypes as C
    m, rows = O.hand_moments()
    # (the wrapper forms its thresholds from the window; the hand-built ones go to the entry itself)
    dev = torch.device("cuda", torch.cuda.current_device())
    mt, rt = torch.from_numpy(m).to(dev), torch.from_numpy(rows).to(dev)
    F, s, cols = rows.shape
    fit = torch.full((F, s, 2 + (O.HAND_D + 2)), np.nan, dtype=torch.float64, device=dev)
    filled = torch.full((F, s, cols), np.nan, dtype=torch.float64, device=dev)
    thr = np.ascontiguousarray(O.HAND_THR)
    rc = L.lib().vbs_poly_fit_f64(dev.index, C.c_void_p(mt.data_ptr()), C.c_void_p(rt.data_ptr()), F, s, cols, 1, O.HAND_D, O.HAND_H,
                                  thr.ctypes.data_as(C.c_void_p), 1, 0, F, C.c_void_p(fit.data_ptr()), C.c_void_p(filled.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == L.VBS_OK
    torch.cuda.synchronize()
    fit, filled = fit.cpu().numpy(), filled.cpu().numpy()
    want, wfilled = O.fit(m, rows, O.HAND_THR, O.HAND_H, O.HAND_D, 1)
    O.assert_bits(fit, want, "hand-built")
    O.assert_bits(filled, wfilled, "hand-built: filled")
    O.check_hand(fit, filled)


def test_filled_goes_straight_into_the_filter():
    from vbs_amd.engine import fir_series_f64
    import filter_oracle as FO
    n, s, h, d = 131, 5, 7, 2
    r = np.random.default_rng(3)
    rec = np.zeros((n, s, 4))
    rec[..., 0] = r.random((n, s)) >= 0.15
    rec[..., 1:] = r.standard_normal((n, s, 3))
    rec[50:80, 2, 0] = 0.0
    m = mom(rec, h, d)
    _, filled = pfit(m, rec, h, d)
    want = restated_fit(m, rec, h, d, "hann", 3)[1]
    O.assert_bits(filled, want, "filled")
    assert (filled[..., 0] == 2.0).sum() > 20 and (filled[60:70, 2, 0] == 0.0).all()
    taps = filters.lowpass_taps(9, 0.3)
    got = fir_series_f64(torch.from_numpy(filled).cuda(), taps, 3).cpu().numpy()
    O.assert_bits(got, FO.fir(want, filters.half_taps(taps), 3), "fir_series_f64 of the filled record")


def test_wrappers_refuse_what_the_entries_refuse():
    from vbs_amd.engine import poly_fit_f64, poly_moments_f64
    rec, _, _ = O.dyadic_case(12, 3, 4, 3, 2, 2, seed=1)
    assert poly_moments_f64(rec, 2, 2).shape == (12, 3, 17) and poly_moments_f64(rec, 2, 1, n_values=1).shape == (12, 3, 6)
    assert poly_moments_f64(rec, 2, 3, "rect", frame_range=(3, 7)).shape == (4, 3, 22)
    for bad in (dict(n_values=4), dict(n_values=0), dict(frame_range=(0, 13)), dict(frame_range=(5, 4)), dict(window="hamming"),
                dict(window=np.ones(7))):
        with pytest.raises(ValueError):
            poly_moments_f64(rec, 2, 2, **bad)
    for bad in (lambda: poly_moments_f64(rec, 128, 2), lambda: poly_moments_f64(rec, 2, 4), lambda: poly_moments_f64(rec[0], 2, 2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(L.VbsError, match=f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}"):
        poly_moments_f64(np.zeros((2, L.PROJ_MAX_SLOTS + 1, 2)), 1, 1)
    m = poly_moments_f64(rec, 2, 2)
    assert poly_fit_f64(m, rec, 2, 2).shape == (12, 3, 14)
    fit, filled = poly_fit_f64(m, rec, 2, 2, want_filled=True)
    assert filled.shape == (12, 3, 4)
    for bad in (dict(min_coverage=0.0), dict(piv_rel=1.0), dict(fill_degree=4), dict(frame_range=(0, 5))):
        with pytest.raises(ValueError):
            poly_fit_f64(m, rec, 2, 2, **bad)
    with pytest.raises(ValueError):
        poly_fit_f64(m[..., :16], rec, 2, 2)
    with pytest.raises(ValueError):
        poly_fit_f64(m, rec, 2, 3)


def test_kinematic_analysis_finds_the_press_and_the_fastest_marker():
    from vbs_amd import fields
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, gain = O.press_table()
    n, m = t.shape[0], t.shape[1]
    h, d = O.PRESS_HALF, 2
    z, v, a, pieces = O.press_profile(n)
    inside = O.inside_one_piece(n, pieces, h)
    nodes = t[0, :, 6:8].astype(np.float64)
    grid_xy, _ = fields.grid_over(nodes, (13, 13), 0.0)
    W = fields.gaussian_weights(nodes, grid_xy, 0.75)
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        res = PL.kinematic_analysis(eng, torch.from_numpy(t).cuda(), h, d, grid=(W, fields.row_sums(W), grid_xy))
        print(f"KIN_TOL = {O.KIN_TOL:.3g}")
        for name, k in (("", m), ("total_", 1)):
            series, fit = res[name + "series"].cpu().numpy(), res[name + "fit"].cpu().numpy()
            assert series.shape[:2] == (n, k) and fit.shape == (n, k, 2 + 3 * (d + 2))
            mo = mom(series, h, d, "hann", 3)
            O.assert_bits(res[name + "moments"].cpu().numpy(), mo, f"{name}moments")
            O.assert_bits(fit, restated_fit(mo, series, h, d, "hann", 3)[0], f"{name}fit is the fit of the moments")
        vel, acc, dis, deg = res["velocity"], res["acceleration"], res["displacement"], res["degree"]
        assert vel.shape == (n, m, 3) and deg.shape == (n, m) and res["speed"].shape == (n, m)
        slow = np.arange(m) != O.FAST_SLOT
        full = (deg == d) & inside[:, None]
        assert full[:, slow].sum() > 0.8 * inside.sum() * (m - 1)
        ev = np.abs(vel[..., 2] - (-gain[None, :] * v[:, None]))[full]
        ea = np.abs(acc[..., 2] - (-gain[None, :] * a[:, None]))[full]
        ez = np.abs(dis[..., 2] - (-gain[None, :] * z[:, None]))[full]
        evx = np.abs(vel[..., 0] - 0.25 * gain[None, :] * v[:, None])[full & slow[None, :]]
        print(f"largest |dZ, vZ, aZ, vX - analytic| = {ez.max():.3g}, {ev.max():.3g}, {ea.max():.3g}, {evx.max():.3g} over {int(full.sum())} windows")
        assert max(ez.max(), ev.max(), ea.max(), evx.max()) <= O.KIN_TOL
        assert np.abs(vel[..., 1][deg >= 1]).max() <= O.KIN_TOL      # nothing moves in Y
        print(f"onset {res['onset']} against {O.PRESS_START}")
        assert abs(res["onset"] - O.PRESS_START) <= h
        fast = np.arange(O.FAST_FROM + h, O.FAST_FROM + O.FAST_LEN - h)
        assert fast.size >= 5 and (res["fastest"][fast] == O.FAST_SLOT).all()
        assert abs(res["peak_speed"][O.FAST_SLOT] - np.nanmax(res["speed"][:, O.FAST_SLOT])) == 0.0
        assert O.FAST_FROM <= res["peak_frame"][O.FAST_SLOT] < O.FAST_FROM + O.FAST_LEN
        assert res["total_velocity"].shape == (n, 3) and res["speed_map"].shape == (n, 169, 2) and res["speed_patch"].shape == (n, 8)
        f = O.FAST_FROM + O.FAST_LEN // 2
        smap = res["speed_map"].cpu().numpy()
        peak = grid_xy[int(np.argmax(smap[f, :, 1]))]
        assert smap[f, :, 0].all() and np.abs(peak - nodes[O.FAST_SLOT]).max() <= 0.5 + 1e-9         # within one grid cell
        res2 = PL.kinematic_analysis(eng, torch.from_numpy(t).cuda(), h, d, fps=100.0)
        assert np.array_equal(res2["velocity"], vel * 100.0, equal_nan=True) and np.array_equal(res2["acceleration"], acc * 1e4, equal_nan=True)
        df = PL.to_kinematic_frame(res, fps=100.0)
        assert tuple(df.columns) == PL.KINEMATIC_FRAME_COLUMNS + ("time_s",) and len(df) == 3 * m * n
        zz = df[df["axis"] == "z"]
        assert np.array_equal(zz["velocity"].to_numpy().reshape(n, m), vel[..., 2], equal_nan=True)
        with pytest.raises(ValueError):
            PL.kinematic_analysis(eng, torch.from_numpy(t).cuda(), 128, 2)
    finally:
        eng.close()


@pytest.mark.parametrize("source,dtype", (("xyz", np.float32), ("pixel", np.float32)))
def test_fill_table_fills_with_the_restated_constant_term(source, dtype):
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, _ = O.press_table(seed=3, drop=0.05)
    n, m = t.shape[:2]
    r = np.random.default_rng(4)
    t[..., 1] = 100.0 + 3.0 * r.standard_normal((n, m)).astype(np.float32).cumsum(axis=0)
    t[..., 2] = 50.0 + r.standard_normal((n, m)).astype(np.float32)
    t[60:90, 5, 0] = 0.0                                         # a gap longer than the window: its inside stays missing
    h, d = 7, 2
    bit, cols = (L.FLAG_XYZ, (6, 7, 8)) if source == "xyz" else (L.FLAG_TRACKED, (1, 2))
    nv = len(cols)
    valid = (t[..., 0].astype(np.int64) & bit) != 0
    rec = np.concatenate([valid[..., None].astype(np.float64), t[..., list(cols)].astype(np.float64)], axis=2)
    mo = O.moments(rec, O.taps(h, d), d, nv)
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        out, rep = PL.fill_table(eng, torch.from_numpy(t).cuda(), h, d, source=source)
        mo_dev = mom(rec, h, d, "hann", nv)
        fit, filled = restated_fit(mo_dev, rec, h, d, "hann", nv)
        out, did = out.cpu().numpy(), rep["filled"].cpu().numpy()
        want_did = filled[..., 0] == 2.0
        assert np.array_equal(did, want_did) and did.sum() > 100 and not did[70:80, 5].any() and not (did & valid).any()
        for k, c in enumerate(cols):
            assert np.array_equal(out[..., c][did], filled[..., 1 + k][did].astype(dtype))       # rounded to the table's dtype once
        # nothing else changes: flags, the other columns, every row that was not filled
        keep = out.copy()
        for c in cols:
            keep[..., c][did] = t[..., c][did]
        assert np.array_equal(keep.view(np.uint32), t.view(np.uint32))
        assert np.array_equal(rep["degree"].cpu().numpy(), fit[..., 1].astype(np.int64))
        assert np.array_equal(rep["per_marker"].cpu().numpy(), did.sum(axis=0)) and np.array_equal(rep["per_frame"].cpu().numpy(), did.sum(axis=1))
        # close to the loop restatement's moments too (the device's differ from it by roundings only)
        assert np.abs(mo_dev - mo).max() <= 1e-9 * np.abs(mo).max()
        only = PL.fill_table(eng, torch.from_numpy(t).cuda(), h, d, source=source, slots=[5, 6])[1]["filled"].cpu().numpy()
        assert np.array_equal(only[:, 5:7], did[:, 5:7]) and not only[:, :5].any() and not only[:, 7:].any()
    finally:
        eng.close()


def test_despike_fill_and_the_sheet_have_no_missing_row_where_a_degree_was_reached():
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, _ = O.press_table(seed=5, drop=0.03)
    n, m = t.shape[:2]
    t[40, 3, 0], t[40, 3, 6:9] = 3.0, (3.0, 0.0, 15.0)           # a spike of 5 mm at rest that despiking turns into a gap
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        clean, srep = PL.despike_table(eng, torch.from_numpy(t).cuda(), 7, 3.0, min_scale=0.5)
        assert bool(srep["spike"][40, 3])
        out, rep = PL.fill_table(eng, clean, 7, 2, fill_degree=1)
        did, deg = rep["filled"], rep["degree"]
        assert bool(did[40, 3])
        flags = out[..., 0].to(torch.int64)
        flags = torch.where(did, flags | L.FLAG_XYZ, flags)      # the caller's decision: OR the report in
        out[..., 0] = flags.to(out.dtype)
        have = (flags & L.FLAG_XYZ) != 0
        assert bool((have | (deg < 1)).all()) and int((~have).sum()) == int(((deg < 1) & ~have).sum())
        val = out[40, 3, 8].item()
        assert abs(val - 10.0) < 0.1                             # the filled value follows the series, not the spike
        ids = np.stack([np.zeros(m, dtype=np.int64), np.arange(m, dtype=np.int64)], axis=1)
        df = PL.to_marker_frame(out, ids)
        reached = (deg >= 1).cpu().numpy()
        on_sheet = np.zeros((n, m), dtype=bool)
        on_sheet[df["frameno"].to_numpy(), df["marker_id"].to_numpy() - 1] = True
        assert on_sheet[reached].all() and len(df) == int(have.sum())      # the complete sheet: no missing row where q >= fill_degree
    finally:
        eng.close()
