"""CPU tests of the contact maps' host side (no GPU): the two new C symbols and their constants, what both entries refuse before a
device is touched, `vbs_amd.fields`, the sheet, `contact_analysis`'s argument checks, and the NumPy restatements the GPU tests
hold the device to (`tests/helpers/field_oracle.py`): the map's against exact rational arithmetic within the derived bound and
bit for bit where every order of summation is exact, the patch rules on hand-built maps."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import fields

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import field_oracle as O                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vbs_field_map_f64", "vbs_patch_stats_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.FIELD_FRAMES, L.FIELD_MAX_SLOTS, L.FIELD_MAX_POINTS, L.PATCH_COLS, L.PATCH_GROUP) == (
        defs["VBS_FIELD_FRAMES"], defs["VBS_FIELD_MAX_SLOTS"], defs["VBS_FIELD_MAX_POINTS"], defs["VBS_PATCH_COLS"],
        defs["VBS_PATCH_GROUP"])
    assert (L.FIELD_FRAMES, L.FIELD_MAX_SLOTS, L.FIELD_MAX_POINTS, L.PATCH_COLS) == (4, 1024, 65536, 8) and 1 <= L.PATCH_GROUP <= 16
    assert L.FIELD_MAX_SLOTS == L.IDS_MAX_MARKERS             # the cap of max_markers
    assert O.PATCH_COLS == L.PATCH_COLS
    fm, ps = L.lib().vbs_field_map_f64, L.lib().vbs_patch_stats_f64
    assert len(fm.argtypes) == 14 and fm.argtypes[9] is C.c_double
    assert len(ps.argtypes) == 11 and ps.argtypes[7] is C.c_double and ps.argtypes[8] is C.c_double


def test_refusals_without_a_gpu():
    """Both C entries decide every refusal before the device is touched: with pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY."""
    lib = L.lib()
    p, nul = C.c_void_p(8), None

    def fm(rec=p, n=10, s=5, cols=4, nv=3, W=p, wsum=p, P=16, mc=0.5, fb=0, fe=10, out=p):
        return lib.vbs_field_map_f64(0, rec, n, s, cols, nv, W, wsum, P, mc, fb, fe, out, None)
    for bad in (dict(rec=nul), dict(W=nul), dict(wsum=nul), dict(out=nul), dict(n=0), dict(s=0), dict(P=0), dict(cols=1),
                dict(cols=9), dict(nv=0), dict(nv=4, cols=8), dict(nv=3, cols=3), dict(mc=0.0), dict(mc=-0.5), dict(mc=1.5),
                dict(mc=math.nan), dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert fm(**bad) == L.VBS_EINVAL, bad
    assert fm(s=L.FIELD_MAX_SLOTS + 1) == L.VBS_ECAPACITY and fm(P=L.FIELD_MAX_POINTS + 1) == L.VBS_ECAPACITY
    assert fm(s=L.FIELD_MAX_SLOTS + 1, rec=nul) == L.VBS_EINVAL              # a bad argument comes before a capacity

    def ps(mp=p, F=3, P=16, nv=3, g=p, comp=2, sign=1.0, thr=0.0, out=p):
        return lib.vbs_patch_stats_f64(0, mp, F, P, nv, g, comp, sign, thr, out, None)
    for bad in (dict(mp=nul), dict(g=nul), dict(out=nul), dict(F=0), dict(P=0), dict(nv=0), dict(nv=4), dict(comp=-2), dict(comp=3),
                dict(comp=1, nv=1), dict(sign=0.0), dict(sign=2.0), dict(sign=math.nan), dict(thr=-1e-300), dict(thr=math.nan)):
        assert ps(**bad) == L.VBS_EINVAL, bad
    assert ps(P=L.FIELD_MAX_POINTS + 1) == L.VBS_ECAPACITY

    from vbs_amd.engine import _field_args, _patch_args
    good = dict(n=10, s=5, cols=4, P=16, w_shape=(16, 5), wsum_shape=(16,), min_coverage=0.5, n_values=None, frame_range=None)
    assert _field_args(**good) == (0, 10, 3)
    assert _field_args(**dict(good, cols=8, n_values=None)) == (0, 10, 3)     # the default never asks for more than 3 values
    assert _field_args(**dict(good, cols=2, frame_range=(4, 4))) == (4, 4, 1)
    for bad in (dict(w_shape=(16, 4)), dict(w_shape=(5, 16)), dict(wsum_shape=(15,)), dict(min_coverage=0.0), dict(min_coverage=1.01),
                dict(n_values=4, cols=8), dict(n_values=3, cols=3), dict(n_values=0), dict(frame_range=(3, 2)),
                dict(frame_range=(0, 11)), dict(cols=9), dict(cols=1)):
        with pytest.raises(ValueError):
            _field_args(**dict(good, **bad))
    with pytest.raises(L.VbsError, match="VBS_FIELD_MAX_SLOTS = 1024"):
        _field_args(**dict(good, s=1025, w_shape=(16, 1025)))
    with pytest.raises(L.VbsError, match="VBS_FIELD_MAX_POINTS = 65536"):
        _field_args(**dict(good, P=65537, w_shape=(65537, 5), wsum_shape=(65537,)))
    assert _patch_args(3, 16, 4, (16, 2), 2, 1.0, 0.5) == (3, 2, 1.0, 0.5)
    assert _patch_args(3, 16, 4, (16, 2), -1, -1.0, 0.5) == (3, -1, -1.0, 0.25)   # the norm: the entry takes the square
    for bad in (dict(oc=1), dict(oc=5), dict(grid_shape=(15, 2)), dict(component=3), dict(component=-2), dict(sign=0.5),
                dict(threshold=-1.0), dict(threshold=math.nan)):
        args = dict(F=3, P=16, oc=4, grid_shape=(16, 2), component=2, sign=1.0, threshold=0.0)
        with pytest.raises(ValueError):
            _patch_args(**dict(args, **bad))


@pytest.mark.parametrize("s", (1, 5, 65, 257))
def test_restatement_is_exact_on_dyadic_cases(s):
    """Where every order is exact the restatement's num and den are the rationals, and its quotient the correctly rounded one."""
    rec, W, wsum = O.dyadic_case(3, 7, s, 5, 3, seed=s)
    got = O.field_map(rec, W, wsum, 0.5, 3)
    value, _, d = O.exact_map(rec, W, 3)
    for f in range(3):
        for p in range(7):
            ok = d[f, p] > 0 and d[f, p] >= O.Fraction(0.5) * O.Fraction(float(wsum[p]))
            assert got[f, p, 0] == float(ok)
            for v in range(3):
                want = float(value[f, p, v]) if ok else 0.0           # float(Fraction) rounds correctly
                assert got[f, p, 1 + v] == want and not (ok and math.copysign(1, got[f, p, 1 + v]) != math.copysign(1, want))


@pytest.mark.parametrize("s,seed", ((3, 1), (64, 2), (441, 3), (1024, 4)))
def test_restatement_within_the_bound_of_exact_arithmetic(s, seed):
    rec, W, wsum = O.random_case(2, 5, s, 6, 3, seed)
    _, _, d = O.exact_map(rec, W, 3)
    assert O.coverage_margin(d, wsum, 0.5) > O.Fraction(1, 10 ** 9)
    worst = O.check_within_bound(O.field_map(rec, W, wsum, 0.5, 3), rec, W, wsum, 0.5, 3, what=f"s {s}")
    print(f"s {s}: restatement's largest error / bound = {worst:.3g}")
    assert worst <= 1.0


def test_poison_never_enters_the_restatement():
    rec, W, wsum = O.random_case(3, 6, 37, 8, 2, seed=9, kind=None)
    clean = O.field_map(rec, W, wsum, 0.5, 2)
    for kind in (np.nan, 1e300):
        O.assert_bits(O.field_map(O.poison(rec, 2, kind), W, wsum, 0.5, 2), clean, f"poison {kind}")
    assert np.isfinite(clean).all()


def test_fields_grid_weights_and_row_sums():
    r = np.random.default_rng(0)
    gx, gy = np.meshgrid(np.arange(13) * 1.5, np.arange(9) * 1.5)
    nodes = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1) + r.uniform(-0.1, 0.1, (117, 2))
    nodes[5] = np.nan                                            # a slot without a position
    grid, area = fields.grid_over(nodes, (4, 6), margin=0.5)
    assert grid.shape == (24, 2) and grid.flags.c_contiguous
    fin = nodes[np.isfinite(nodes).all(axis=1)]
    lo, hi = fin.min(axis=0) - 0.5, fin.max(axis=0) + 0.5
    assert np.allclose(grid[0], lo) and np.allclose(grid[-1], hi)
    assert np.all(np.diff(grid[:6, 0]) > 0) and np.all(grid[:6, 1] == grid[0, 1])       # row-major: x fastest
    assert np.all(grid[::6, 0] == grid[0, 0]) and np.all(np.diff(grid[::6, 1]) > 0)
    assert area == pytest.approx((hi[0] - lo[0]) / 5 * (hi[1] - lo[1]) / 3)
    assert fields.grid_over(nodes[:1], (1, 1))[1] == 1.0
    h = fields.default_bandwidth(nodes)
    assert 1.2 < h < 1.8
    W = fields.gaussian_weights(nodes, grid, h, cutoff=3.0)
    assert W.shape == (24, 117) and W.dtype == np.float64 and (W >= 0).all() and np.isfinite(W).all()
    assert np.all(W[:, 5] == 0.0)                                # the non-finite node
    r2 = ((grid[:, None, :] - np.nan_to_num(nodes)[None, :, :]) ** 2).sum(axis=2)
    far = r2 > (3.0 * h) ** 2 * (1 + 1e-12)
    near = r2 < (3.0 * h) ** 2 * (1 - 1e-12)
    near[:, 5] = False
    assert far.any() and np.all(W[far] == 0.0) and np.all(W[near] > 0.0)                # exact zeros beyond the cutoff
    assert np.allclose(W[near], np.exp(-r2[near] / (2 * h * h)), rtol=1e-15)
    ws = fields.row_sums(W)
    want = np.zeros(24)
    for m in range(117):
        want = want + W[:, m]
    O.assert_bits(ws, want, "row_sums")
    assert (ws > 0).all() and np.allclose((W / ws[:, None]).sum(axis=1), 1.0, rtol=1e-14)   # a partition of unity
    # all slots valid with one constant value: the smoother returns that constant
    rec = np.ones((1, 117, 2))
    rec[..., 1] = 0.375
    mp = O.field_map(rec, W, ws, 0.5, 1)
    assert np.all(mp[0, :, 0] == 1.0) and np.allclose(mp[0, :, 1], 0.375, rtol=1e-14)
    for bad in (lambda: fields.grid_over(nodes, (0, 4)), lambda: fields.grid_over(nodes, (4, 4), -1.0),
                lambda: fields.grid_over(np.full((3, 2), np.nan), (4, 4)), lambda: fields.gaussian_weights(nodes, grid, 0.0),
                lambda: fields.gaussian_weights(nodes, grid, h, cutoff=0.0), lambda: fields.gaussian_weights(nodes[:, :1], grid, h),
                lambda: fields.row_sums(np.zeros(4))):
        with pytest.raises(ValueError):
            bad()


def _hand_map(P=70, nv=3):
    mp = np.zeros((1, P, 1 + nv))
    g = np.stack([np.arange(P) % 10, np.arange(P) // 10], axis=1).astype(np.float64)
    return mp, g


def test_patch_rules_on_hand_built_maps():
    mp, g = _hand_map()
    O.assert_bits(O.patch_stats(mp, g, 2, 1.0, 0.0), np.zeros((1, 8)), "nothing covered")          # flag 0: all zeros
    mp[0, 3:9, 0] = 1.0
    mp[0, 3:9, 3] = -1.0
    assert O.patch_stats(mp, g, 2, 1.0, 0.5)[0].tolist() == [1.0, 6.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0]    # covered, empty patch
    assert O.patch_stats(mp, g, 2, -1.0, 0.5)[0, :4].tolist() == [2.0, 6.0, 6.0, 6.0]                # the other sign finds it
    mp[0, 3:9, 3] = 0.0
    assert O.patch_stats(mp, g, 2, 1.0, 0.0)[0].tolist() == [1.0, 6.0, 6.0, 0.0, 0.0, 0.0, 0.0, -1.0]    # S = 0: no centre
    # tied peaks: the earliest wins, across lanes (p = 5 and p = 69 share lane 5) and within the fold
    mp[0, :, 0] = 1.0
    mp[0, :, 3] = 0.25
    mp[0, [69, 5, 40], 3] = 2.0
    out = O.patch_stats(mp, g, 2, 1.0, 0.25)[0]
    assert out[0] == 2.0 and out[2] == 70.0 and out[6] == 2.0 and out[7] == 5.0
    assert out[3] == 67 * 0.25 + 6.0 and out[4] == pytest.approx((mp[0, :, 3] * g[:, 0]).sum() / out[3], rel=1e-14)
    # a NaN score is never in the patch and never a peak; an uncovered point is not read
    mp[0, 5, 3] = np.nan
    mp[0, 40, 0] = 0.0
    mp[0, 40, 1:] = np.nan
    out = O.patch_stats(mp, g, 2, 1.0, 0.25)[0]
    assert out.tolist()[:3] == [2.0, 69.0, 68.0] and out[7] == 69.0 and np.isfinite(out).all()
    # the squared norm, added left to right; thr is the square
    mp2, g2 = _hand_map(P=3)
    mp2[0, :, 0] = 1.0
    mp2[0, 1, 1:] = (3.0, 4.0, 12.0)
    out = O.patch_stats(mp2, g2, -1, 1.0, 169.0)[0]
    assert out.tolist() == [2.0, 3.0, 1.0, 169.0, 1.0, 0.0, 169.0, 1.0]
    assert O.patch_stats(mp2, g2, -1, 1.0, 169.0 + 1e-9)[0, 0] == 1.0


def test_contact_sheet_columns_and_round_trip(tmp_path):
    from vbs_amd import pipeline as PL
    from vbs_amd.xlsx_io import read_xlsx
    g = np.stack([np.arange(6) % 3 * 0.5, np.arange(6) // 3 * 0.5], axis=1)
    patch = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [1, 6, 0, 0, 0, 0, 0, -1], [2, 6, 3, 1.5, 0.25, 0.5, 0.75, 4], [2, 5, 1, 0.5, 1.0, 0.0, 0.5, 2]],
                     dtype=np.float64)
    pf = np.zeros((4, 7))
    pf[2] = (3, 1.25, 0.3, 0.4, 0.25, -0.05, 0.1)
    pf[3] = (1, 0, 0, 0, 0, 0, 0)
    df = PL.to_contact_frame(patch, 0.25, g, frame_offset=100)
    assert tuple(df.columns) == PL.CONTACT_FRAME_COLUMNS == ("frameno", "flag", "covered", "count", "area_mm2", "sum", "cx", "cy",
                                                              "peak", "peak_x", "peak_y")
    assert df["frameno"].tolist() == [100, 101, 102, 103] and df["flag"].tolist() == [0, 1, 2, 2]
    assert df["area_mm2"].tolist() == [0.0, 0.0, 0.75, 0.25] and df["sum"].tolist() == [0.0, 0.0, 1.5, 0.5]
    for name in ("cx", "cy", "peak", "peak_x", "peak_y"):
        assert df[name].isna().tolist() == [True, True, False, False], name
    assert (df["peak_x"][2], df["peak_y"][2], df["peak_x"][3], df["peak_y"][3]) == (0.5, 0.5, 1.0, 0.0)
    path = str(tmp_path / "contact.xlsx")
    df2 = PL.to_contact_frame(patch, 0.25, g, pf, path=path)
    assert tuple(df2.columns) == PL.CONTACT_FRAME_COLUMNS + PL.CONTACT_TREND_COLUMNS
    assert df2["sum_f"].isna().tolist() == [True, True, False, True] and df2["cx_f"][2] == 0.3 and df2["cy_f"][2] == 0.4
    back = read_xlsx(path)
    assert list(back.columns) == list(df2.columns) and len(back) == 4
    for c in df2.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), df2[c].to_numpy(dtype=np.float64), equal_nan=True), c
    csv = str(tmp_path / "contact.csv")
    PL.to_contact_frame(patch, 0.25, g, pf, path=csv)
    import pandas as pd
    back = pd.read_csv(csv)
    assert tuple(back.columns) == tuple(df2.columns) and back.equals(df2)
    with pytest.raises(ValueError):
        PL.to_contact_frame(patch[:, :7], 0.25, g)
    with pytest.raises(ValueError):
        PL.to_contact_frame(patch, 0.25, g, pf[:3])
    with pytest.raises(ValueError):
        PL.to_contact_frame(patch, 0.25, g[:4])                  # the peak of frame 2 is point 4


def test_contact_analysis_argument_checks():
    from vbs_amd.pipeline import _contact_args
    good = dict(n=20, m=169, grid_shape=(16, 16), bandwidth=None, component="z", sign=1.0, threshold=0.1, ref_frame=0,
                min_coverage=0.5, keep_maps=(), max_map_bytes=256 << 20)
    assert _contact_args(**good) == (256, (256 << 20) // (256 * 32), [])
    assert _contact_args(**dict(good, keep_maps=(7, 3, 7), max_map_bytes=256 * 32 * 5 + 1, component="xyz", sign=-1)) == (256, 5, [3, 7])
    for bad in (dict(grid_shape=(0, 4)), dict(grid_shape=(16,)), dict(grid_shape=(257, 256)), dict(m=1025), dict(component="w"),
                dict(sign=0.0), dict(threshold=-0.1), dict(threshold=math.nan), dict(bandwidth=0.0), dict(bandwidth=math.inf),
                dict(ref_frame=20), dict(ref_frame=-1), dict(min_coverage=0.0), dict(min_coverage=1.5), dict(keep_maps=(20,)),
                dict(keep_maps=(-1,)), dict(max_map_bytes=256 * 32 - 1)):
        with pytest.raises(ValueError):
            _contact_args(**dict(good, **bad))
