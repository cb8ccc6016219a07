"""GPU tests of the contact maps (k_field.hip; run on the MI355X box: `pytest -m gpu`): `engine.field_map_f64`,
`engine.patch_stats_f64`, `pipeline.contact_analysis` and the sheet.

The map's order of summation is not part of its interface (the order inside the float64 matrix instruction is not documented), so
the map is held three ways (`tests/helpers/field_oracle.py`): BIT FOR BIT to the NumPy restatement where every order is exact
(dyadic inputs), within the DERIVED bound (2 gamma_(s+6) + 2 u) A / d of exact rational arithmetic on float content, and bit for
bit to ITSELF under every change of batching.  The patch statistics have a stated order and are held bit for bit to their
restatement, fed the device's own map.  No entry is skipped or masked.  Shapes are the smallest at which the kernel can go wrong:
around the 16-point grid tile, the 4-frame column tile, the 16-slot block of K, and the slot counts at which a workgroup takes
4, 2 or 1 frame tiles (256 | 257, 512 | 513), not the workload's.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import fields                                    # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import field_oracle as O                                      # noqa: E402

FRAMES = (1, 3, 4, 5, 9)
POINTS = (1, 15, 16, 17, 33, 100)
SLOTS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 256, 257, 441, 512, 513, 1024)
G = L.PATCH_GROUP


def fmap(rec, W, wsum, mc=0.5, nv=None, frame_range=None):
    from vbs_amd.engine import field_map_f64
    return field_map_f64(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(wsum).cuda(), mc, nv,
                         frame_range).cpu().numpy()


def shape_of(s, k=0, budget=None):
    """The k-th shape for a slot count: F, P, cols, n_values rotate through their lists; with `budget`, P then F shrink until
    F P s stays below it (the exact side is rational arithmetic in Python)."""
    i = SLOTS.index(s)
    F, P = FRAMES[(i + k) % 5], POINTS[(i * 5 + 3 + 2 * k) % 6]
    if budget:
        while F * P * s > budget and P > 1:
            P = POINTS[POINTS.index(P) - 1]
        while F * P * s > budget and F > 1:
            F = FRAMES[FRAMES.index(F) - 1]
    nv = 1 + (i + k) % 3
    cols = nv + 1 + (i + 2 * k) % (8 - nv)
    return F, P, cols, nv


def with_edges(rec, W, wsum):
    """An all-invalid frame (the last, when there are several) and a grid point with zero row weight (the last, when there are
    several): zeros and flag 0."""
    rec, W, wsum = rec.copy(), W.copy(), wsum.copy()
    if rec.shape[0] > 1:
        rec[-1, :, 0] = 0.0
    if W.shape[0] > 1:
        W[-1], wsum[-1] = 0.0, 0.0
    return rec, W, wsum


@pytest.mark.parametrize("s", SLOTS)
def test_dyadic_maps_equal_the_restatement_bit_for_bit(s):
    for k in range(3):
        F, P, cols, nv = shape_of(s, k)
        rec, W, wsum = with_edges(*O.dyadic_case(F, P, s, cols, nv, seed=100 * s + k))
        want = O.field_map(rec, W, wsum, 0.5, nv)
        O.assert_bits(fmap(rec, W, wsum, 0.5, nv), want, f"s {s} F {F} P {P} cols {cols} nv {nv}")
        if F > 1:
            assert not want[-1].any()
        if P > 1:
            assert not want[:, -1].any()
        assert want[..., 0].any() or s < 4


@pytest.mark.parametrize("s", (5, 65))
def test_dyadic_maps_on_every_frame_and_point_count(s):
    for F in FRAMES:
        for P in POINTS:
            rec, W, wsum = O.dyadic_case(F, P, s, 4, 3, seed=F * 1000 + P)
            O.assert_bits(fmap(rec, W, wsum, 0.5, 3), O.field_map(rec, W, wsum, 0.5, 3), f"s {s} F {F} P {P}")


def test_coverage_edge_all_invalid_frame_and_zero_row():
    """den == min_coverage * wsum exactly is ok; one slot fewer is not; an all-invalid frame and a point without weight are zeros."""
    s, P = 8, 3
    W = np.zeros((P, s))
    W[0] = 0.5
    W[1] = np.arange(s) / 8.0
    wsum = W.sum(axis=1)
    rec = np.zeros((3, s, 3))
    rec[..., 1:] = np.arange(3 * s * 2).reshape(3, s, 2) / 16.0 - 1.0
    rec[0, :4, 0] = 1.0                                          # den = 2.0 = 0.5 * 4.0 at point 0
    rec[1, :3, 0] = 1.0
    rec = O.poison(rec, 2, np.nan)
    got = fmap(rec, W, wsum, 0.5, 2)
    O.assert_bits(got, O.field_map(rec, W, wsum, 0.5, 2), "edge")
    assert got[0, 0, 0] == 1.0 and got[0, 0, 1] == rec[0, :4, 1].mean() and got[1, 0].tolist() == [0.0, 0.0, 0.0]
    assert not got[2].any() and not got[:, 2].any()
    assert got[0, 1, 0] == 0.0                                   # 0.75 of 3.5: below half


def random_shape(s):
    F, P, cols, nv = shape_of(s, 1, budget=60000)
    return F, P, cols, nv, 7000 + s


@pytest.mark.parametrize("s", SLOTS)
def test_random_maps_lie_within_the_derived_bound(s):
    F, P, cols, nv, seed = random_shape(s)
    rec, W, wsum = with_edges(*O.random_case(F, P, s, cols, nv, seed))
    _, _, d = O.exact_map(rec, W, nv)
    margin = O.coverage_margin(d, wsum, 0.5)                     # on the reference alone: no decision near its edge
    assert margin is None or margin > O.Fraction(1, 10 ** 9), f"seed {seed}: a coverage decision within 1e-9 of its edge"
    got = fmap(rec, W, wsum, 0.5, nv)
    worst = O.check_within_bound(got, rec, W, wsum, 0.5, nv, what=f"s {s} F {F} P {P} nv {nv}")
    print(f"s {s} F {F} P {P} cols {cols} nv {nv}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("s,P", ((130, 33), (441, 17), (1024, 16)))
def test_maps_are_bit_identical_under_every_change_of_batching(s, P):
    from vbs_amd.engine import field_map_f64
    F = 9
    rec, W, wsum = O.random_case(F, P, s, 5, 3, seed=s)
    whole = fmap(rec, W, wsum)
    O.assert_bits(fmap(rec, W, wsum), whole, "run to run")
    O.assert_bits(field_map_f64(rec, W, wsum).cpu().numpy(), whole, "array against tensor input")
    O.assert_bits(field_map_f64(rec, W).cpu().numpy(), fmap(rec, W, fields.row_sums(W)), "default row sums")
    for a, b in ((0, 1), (1, 4), (3, 8), (4, 9), (8, 9), (2, 7)):
        O.assert_bits(fmap(rec, W, wsum, frame_range=(a, b)), whole[a:b], f"range {a}:{b}")
    assert fmap(rec, W, wsum, frame_range=(5, 5)).shape == (0, P, 4)
    other = O.random_case(F, P, s, 5, 3, seed=s + 1)[0]
    for f in (0, 6):
        O.assert_bits(fmap(rec[f:f + 1], W, wsum), whole[f:f + 1], f"frame {f} alone")
        for pos in range(8):                                     # every position of a tile, in the first and in the second tile
            batch = other.copy()
            batch[pos] = rec[f]
            O.assert_bits(fmap(batch, W, wsum)[pos], whole[f], f"frame {f} at position {pos}")


def test_dead_slots_appended_change_no_bit():
    s, P, F = 130, 33, 5
    rec, W, wsum = O.random_case(F, P, s, 4, 3, seed=31)
    base = fmap(rec, W, wsum)
    r = np.random.default_rng(32)
    for s2 in (131, 144, 300, 1024):                             # the same block, the next, 2 frame tiles a workgroup, 1
        rec2 = np.full((F, s2, 4), np.nan)
        rec2[:, :s] = rec
        rec2[:, s:, 0] = 0.0
        W2 = np.ascontiguousarray(np.concatenate([W, r.random((P, s2 - s))], axis=1))
        O.assert_bits(fmap(rec2, W2, wsum), base, f"{s} slots padded to {s2}")       # (wsum is the caller's: kept)


@pytest.mark.parametrize("s", (5, 130, 513))
def test_poison_changes_no_bit(s):
    F, P, cols, nv = 5, 17, 8, 2
    rec, W, wsum = O.random_case(F, P, s, cols, nv, seed=50 + s, kind=None)
    clean = fmap(rec, W, wsum, 0.5, nv)
    assert np.isfinite(clean).all()
    for kind in (np.nan, 1e300, -np.inf):
        O.assert_bits(fmap(O.poison(rec, nv, kind), W, wsum, 0.5, nv), clean, f"poison {kind}")


def pstats(mp, grid, component, sign, threshold):
    from vbs_amd.engine import patch_stats_f64
    return patch_stats_f64(torch.from_numpy(np.ascontiguousarray(mp)).cuda(), grid, component, sign, threshold).cpu().numpy()


@pytest.mark.parametrize("P", (1, 63, 64, 65, 130))
def test_patch_statistics_equal_the_restatement_bit_for_bit(P):
    s = 37
    side = int(np.ceil(np.sqrt(P)))
    grid = np.stack([np.arange(P) % side * 0.37, np.arange(P) // side * 0.41], axis=1)
    for i, F in enumerate(sorted({1, G - 1, G, G + 1, 2 * G + 1})):
        nv = 1 + i % 3
        rec, W, wsum = with_edges(*O.random_case(F, P, s, nv + 1, nv, seed=P * 10 + i))
        mp = fmap(rec, W, wsum, 0.5, nv)                         # the device's own map: this test inherits no tolerance
        for comp, sign, thr in ((nv - 1, 1.0, 0.0), (0, -1.0, 0.5), (-1, 1.0, 2.0), (-1, 1.0, 0.0)):
            got = pstats(mp, grid, comp, sign, thr)
            O.assert_bits(got, O.patch_stats(mp, grid, comp, sign, thr * thr if comp < 0 else thr), f"P {P} F {F} comp {comp} sign {sign}")
        if F > 1:
            assert got[-1].tolist() == [0.0] * 8                 # nothing covered


def test_patch_rules_on_hand_built_maps():
    P = 130
    grid = np.stack([np.arange(P) % 10 * 1.0, np.arange(P) // 10 * 1.0], axis=1)
    mp = np.zeros((G + 2, P, 4))
    mp[1, 3:9, 0], mp[1, 3:9, 3] = 1.0, -1.0                     # covered, empty patch
    mp[2, 3:9, 0] = 1.0                                          # covered, S = 0 at thr 0
    mp[3, :, 0], mp[3, :, 3] = 1.0, 0.25                         # tied peaks: p = 5 and 69 share a lane, 40 and 104 another
    mp[3, [104, 69, 5, 40], 3] = 2.0
    mp[4] = mp[3]
    mp[4, 5, 3] = np.nan                                         # a NaN score: not in the patch, not a peak
    mp[4, 40, 0], mp[4, 40, 1:] = 0.0, np.nan                    # not covered: not read
    mp[5, :, 0], mp[5, :, 1:] = 1.0, np.nan                      # every score NaN
    mp[6, 7, :] = (2.0, 9.0, 9.0, 1e-300)                        # any nonzero flag covers; a lone point is its own centre
    mp[G + 1, P - 1, :] = (1.0, 0.0, 0.0, 3.0)
    for comp, sign, thr in ((2, 1.0, 0.0), (2, 1.0, 0.25), (2, -1.0, 0.5), (-1, 1.0, 0.0)):
        got = pstats(mp, grid, comp, sign, thr)
        O.assert_bits(got, O.patch_stats(mp, grid, comp, sign, thr * thr if comp < 0 else thr), f"comp {comp} sign {sign} thr {thr}")
    got = pstats(mp, grid, 2, 1.0, 0.25)
    assert got[0].tolist() == [0.0] * 8
    assert got[1].tolist() == [1.0, 6.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]
    assert pstats(mp, grid, 2, 1.0, 0.0)[2].tolist() == [1.0, 6.0, 6.0, 0.0, 0.0, 0.0, 0.0, -1.0]
    assert got[3, 0] == 2.0 and got[3, 2] == 130.0 and got[3, 6] == 2.0 and got[3, 7] == 5.0
    assert got[4, :3].tolist() == [2.0, 129.0, 128.0] and got[4, 7] == 69.0
    assert got[5].tolist() == [1.0, 130.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]
    assert got[G + 1].tolist() == [2.0, 1.0, 1.0, 3.0, 9.0, 12.0, 3.0, 129.0]


def test_wrappers_refuse_what_the_entries_refuse():
    from vbs_amd.engine import field_map_f64, patch_stats_f64
    rec, W, wsum = O.dyadic_case(3, 5, 6, 4, 3, seed=1)
    assert field_map_f64(rec, W, wsum).shape == (3, 5, 4) and field_map_f64(rec, W, wsum, n_values=1).shape == (3, 5, 2)
    for bad in (dict(min_coverage=0.0), dict(min_coverage=1.5), dict(n_values=4), dict(frame_range=(2, 1)), dict(frame_range=(0, 4))):
        with pytest.raises(ValueError):
            field_map_f64(rec, W, wsum, **bad)
    with pytest.raises(ValueError):
        field_map_f64(rec, W[:, :5], wsum)
    with pytest.raises(L.VbsError, match="VBS_FIELD_MAX_SLOTS = 1024"):
        field_map_f64(np.zeros((1, 1025, 2)), np.zeros((2, 1025)), np.zeros(2))
    mp, grid = field_map_f64(rec, W, wsum), np.zeros((5, 2))
    assert patch_stats_f64(mp, grid).shape == (3, 8) and patch_stats_f64(mp[:0], grid).shape == (0, 8)
    for bad in (dict(component=3), dict(component=-2), dict(sign=0.0), dict(threshold=-1.0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            patch_stats_f64(mp, grid, **bad)
    with pytest.raises(ValueError):
        patch_stats_f64(mp, grid[:4])


def test_contact_analysis_follows_a_moving_dimple():
    from vbs_amd import filters as F
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine
    t, cen = O.dimple_table()
    n = t.shape[0]
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        dev = torch.from_numpy(t).cuda()
        per_frame = 24 * 24 * 32
        kw = dict(grid_shape=(24, 24), component="z", threshold=0.2, taps=F.moving_average_taps(5), keep_maps=(0, 7, n - 1))
        res = PL.contact_analysis(eng, dev, max_map_bytes=5 * per_frame, **kw)
        one = PL.contact_analysis(eng, dev, max_map_bytes=256 << 20, **kw)
        patch = res["patch"].cpu().numpy()
        O.assert_bits(patch, one["patch"].cpu().numpy(), "ranges stitched")
        O.assert_bits(res["patch_filtered"].cpu().numpy(), one["patch_filtered"].cpu().numpy(), "trend")
        assert sorted(res["maps"]) == [0, 7, n - 1]
        for f in res["maps"]:
            O.assert_bits(res["maps"][f].cpu().numpy(), one["maps"][f].cpu().numpy(), f"map {f}")
        grid = res["grid_xy"].cpu().numpy()
        cell = grid[1, 0] - grid[0, 0]
        assert res["bandwidth"] == 1.0 and res["cell_area"] == pytest.approx(cell * cell) and cell == pytest.approx(12.0 / 23)
        assert patch[0, 0] == 1.0 and patch[0, 2] == 0.0         # at rest: covered, no patch
        has = patch[:, 0] == 2.0
        assert has[1:].all() and (patch[:, 1] == 576.0).all()
        err = np.abs(patch[has, 4:6] - cen[has]).max()
        print(f"largest |centre - truth| = {err:.4f} of a cell of {cell:.4f}")
        assert err <= cell
        pk = grid[patch[has, 7].astype(int)]
        assert np.abs(pk - cen[has]).max() <= cell               # the peak sits on the grid: half a cell, and the dropouts
        # the map the patch came from, against the restatement fed the same axis displacement and weights
        axis = eng.axis_displacement(dev, 0)[0].cpu().numpy()
        nodes = t[0, :, 6:8].astype(np.float64)
        W = fields.gaussian_weights(nodes, grid, 1.0)
        O.check_within_bound(res["maps"][7].cpu().numpy()[None], axis, W, fields.row_sums(W), 0.5, 3, (7, 8), "map 7")
        df = PL.to_contact_frame(res["patch"], res["cell_area"], res["grid_xy"], res["patch_filtered"])
        assert tuple(df.columns) == PL.CONTACT_FRAME_COLUMNS + PL.CONTACT_TREND_COLUMNS == (
            "frameno", "flag", "covered", "count", "area_mm2", "sum", "cx", "cy", "peak", "peak_x", "peak_y", "sum_f", "cx_f", "cy_f")
        assert len(df) == n and np.isnan(df["cx"][0]) and np.isnan(df["cx_f"][0]) and not df["cx"][1:].isna().any()
        trend = df["cx_f"].to_numpy()[3:n - 2]
        assert np.abs(trend - cen[3:n - 2, 0]).max() <= cell
        with pytest.raises(ValueError):
            PL.contact_analysis(eng, dev, component="w")
        with pytest.raises(ValueError):
            PL.contact_analysis(eng, dev, grid_shape=(24, 24), max_map_bytes=per_frame - 1)
    finally:
        eng.close()
