"""CPU tests of the strain entries' host side (no GPU): the new C symbols and their constants, what is refused before a device
is touched, the neighbour lists, the sheet, and the NumPy restatement the GPU tests hold the device to bit for bit
(`tests/helpers/motion_oracle.py`) against `np.linalg.lstsq` and against closed forms.  Bounds: see the helper; every test that
holds one prints the figure it met."""
import ctypes as C
import functools
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import strain as ST

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import motion_oracle as O                                     # noqa: E402
from pose_oracle import grid_ref                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.SYMBOLS)
    for name in ("vbs_motion_series_f64", "vbs_local_strain_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.STRAIN_COLS, L.LSTRAIN_COLS, L.MOTION_GROUP, L.LSTRAIN_GROUP, L.STRAIN_MAX_NBR) == (
        defs["VBS_STRAIN_COLS"], defs["VBS_LSTRAIN_COLS"], defs["VBS_MOTION_GROUP"], defs["VBS_LSTRAIN_GROUP"], defs["VBS_STRAIN_MAX_NBR"])
    assert (L.STRAIN_COLS, L.LSTRAIN_COLS, L.STRAIN_MAX_NBR) == (16, 8, 12) and 1 <= L.MOTION_GROUP <= 16 and L.LSTRAIN_GROUP >= 1
    assert (O.STRAIN_COLS, O.LSTRAIN_COLS) == (L.STRAIN_COLS, L.LSTRAIN_COLS) and O.DEG == ST.DEG
    assert L.LSTRAIN_COLS <= 8                                # `out` is a record of the contact-map entry: cols <= 8
    ms, ls = L.lib().vbs_motion_series_f64, L.lib().vbs_local_strain_f64
    assert len(ms.argtypes) == 14 and ms.argtypes[7] is C.c_double
    assert len(ls.argtypes) == 14 and ls.argtypes[9] is C.c_double


def test_refusals_without_a_gpu():
    """Both C entries decide every refusal before the device is touched: with pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY; `_motion_args` and `_lstrain_args` raise the same way."""
    lib = L.lib()
    p, nul = C.c_void_p(16), None

    def ms(rec=p, n=10, s=5, cols=4, pos=p, mask=nul, k=0.0, fb=0, fe=10, grad=p, strain=p, res=p):
        return lib.vbs_motion_series_f64(0, rec, n, s, cols, pos, mask, k, fb, fe, grad, strain, res, None)
    for bad in (dict(rec=nul), dict(pos=nul), dict(grad=nul, strain=nul, res=nul), dict(n=0), dict(s=0), dict(cols=3), dict(cols=9),
                dict(k=-1.0), dict(k=math.nan), dict(k=math.inf), dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert ms(**bad) == L.VBS_EINVAL, bad
    assert ms(s=L.FIELD_MAX_SLOTS + 1) == L.VBS_ECAPACITY
    assert ms(s=L.FIELD_MAX_SLOTS + 1, rec=nul) == L.VBS_EINVAL             # a bad argument comes before a capacity

    def ls(rec=p, n=10, s=5, cols=4, pos=p, nbr=p, K=6, mc=4, dr=0.01, fb=0, fe=10, out=p):
        return lib.vbs_local_strain_f64(0, rec, n, s, cols, pos, nbr, K, mc, dr, fb, fe, out, None)
    for bad in (dict(rec=nul), dict(pos=nul), dict(nbr=nul), dict(out=nul), dict(n=0), dict(s=0), dict(cols=3), dict(cols=9),
                dict(K=0), dict(K=13), dict(mc=2), dict(mc=8), dict(K=1, mc=3), dict(dr=-0.1), dict(dr=1.0), dict(dr=math.nan),
                dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert ls(**bad) == L.VBS_EINVAL, bad
    assert ls(s=L.FIELD_MAX_SLOTS + 1) == L.VBS_ECAPACITY
    assert ls(s=L.FIELD_MAX_SLOTS + 1, nbr=nul) == L.VBS_EINVAL

    from vbs_amd.engine import _lstrain_args, _motion_args
    good = dict(n=10, s=5, cols=4, pos_shape=(5, 2), slots=None, reject_k=0.0, frame_range=None, want=("grad", "strain", "residual"))
    assert _motion_args(**good) == (0, 10, ("grad", "strain", "residual"))
    assert _motion_args(**dict(good, cols=8, frame_range=(4, 4), want="strain", slots=[0, 4], reject_k=3.0)) == (4, 4, ("strain",))
    for bad in (dict(n=0), dict(s=0, pos_shape=(0, 2)), dict(cols=3), dict(cols=9), dict(pos_shape=(4, 2)), dict(pos_shape=(5, 3)),
                dict(reject_k=-1.0), dict(reject_k=math.nan), dict(reject_k=math.inf), dict(frame_range=(3, 2)),
                dict(frame_range=(0, 11)), dict(frame_range=(-1, 4)), dict(slots=[5]), dict(slots=[-1]), dict(want=()),
                dict(want=("grad", "pose"))):
        with pytest.raises(ValueError):
            _motion_args(**dict(good, **bad))
    with pytest.raises(L.VbsError, match="VBS_FIELD_MAX_SLOTS = 1024"):
        _motion_args(**dict(good, s=1025, pos_shape=(1025, 2)))
    good = dict(n=10, s=5, cols=4, pos_shape=(5, 2), nbr_shape=(5, 6), min_count=4, det_rel=0.01, frame_range=None)
    assert _lstrain_args(**good) == (0, 10, 6)
    assert _lstrain_args(**dict(good, nbr_shape=(5, 12), min_count=13, det_rel=0.0, frame_range=(2, 7))) == (2, 7, 12)
    for bad in (dict(cols=3), dict(pos_shape=(6, 2)), dict(nbr_shape=(4, 6)), dict(nbr_shape=(5, 0)), dict(nbr_shape=(5, 13)),
                dict(nbr_shape=(5,)), dict(min_count=2), dict(min_count=8), dict(det_rel=-0.5), dict(det_rel=1.0),
                dict(det_rel=math.nan), dict(frame_range=(0, 11))):
        with pytest.raises(ValueError):
            _lstrain_args(**dict(good, **bad))
    with pytest.raises(L.VbsError, match="VBS_FIELD_MAX_SLOTS = 1024"):
        _lstrain_args(**dict(good, s=1025, pos_shape=(1025, 2), nbr_shape=(1025, 6)))


def _conditioning(pos, nbr):
    """1 - rho^2 = det / (xx yy) of every slot's neighbourhood (itself and its neighbours)."""
    out = []
    for i in range(pos.shape[0]):
        p = pos[[i] + [j for j in nbr[i] if j >= 0]]
        c = p - p.mean(axis=0)
        xx, xy, yy = (c[:, 0] ** 2).sum(), (c[:, 0] * c[:, 1]).sum(), (c[:, 1] ** 2).sum()
        out.append((xx * yy - xy * xy) / (xx * yy))
    return np.array(out)


def test_neighbour_lists():
    pos = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [3.0, 0.0]])
    nb = ST.neighbour_lists(pos, 3)
    assert nb.dtype == np.int32 and nb.shape == (6, 3)
    assert nb[0].tolist() == [1, 2, 3]                        # four at distance 1: the lower indices, in order
    assert nb[5].tolist() == [1, 0, 3]                        # 2, 3, then sqrt(10) twice: the lower index
    assert ST.neighbour_lists(pos, 8)[0].tolist() == [1, 2, 3, 4, 5, -1, -1, -1]             # K >= s: padded
    r = ST.neighbour_lists(pos, 4, radius=1.0)
    assert r[0].tolist() == [1, 2, 3, 4] and r[1].tolist() == [0, -1, -1, -1] and r[5].tolist() == [-1] * 4   # the radius is inclusive
    v = ST.neighbour_lists(pos, 3, valid=[True, False, True, True, True, True])
    assert v[1].tolist() == [-1, -1, -1] and v[0].tolist() == [2, 3, 4] and not (v == 1).any()
    assert ST.neighbour_lists(pos[:1], 2).tolist() == [[-1, -1]]
    for bad in (dict(pos=pos[:, :1], K=3), dict(pos=pos, K=0), dict(pos=pos, K=3, valid=[True]), dict(pos=pos, K=3, radius=-1.0)):
        with pytest.raises(ValueError):
            ST.neighbour_lists(**bad)
    grid = grid_ref(169)[:, :2]
    for K in (4, 6, 8):
        nb = ST.neighbour_lists(grid, K)
        assert (nb >= 0).all() and all(len(set(row.tolist()) | {i}) == K + 1 for i, row in enumerate(nb))
        c = _conditioning(grid, nb)
        print(f"grid K {K}: 1 - rho^2 >= {c.min():.3f}")
        assert c.min() >= 0.84                                # so the default det_rel = 0.01 refuses none of them
    ring = O.ring_layout()                                    # (synthetic: full lists, nothing said about the sensor's own layout)
    assert ring.shape == (65, 2) and len({tuple(p) for p in ring.tolist()}) == 65 and (ST.neighbour_lists(ring, 8) >= 0).all()


def _global_cases(m):
    """(rec, pos, mask, reject_k, what) for the host comparisons: an affine field with noise and 10 % dropouts per frame."""
    for i, seed in enumerate((11, 12, 13)):
        rec, pos = O.random_case(6, m, 4 + i, 100 * m + seed, drop=0.1 if m > 4 else 0.0, thin=False)
        if m == 65:
            pos = O.ring_layout()
        mask = None if i != 2 or m < 8 else np.random.default_rng(seed).random(m) < 0.8
        yield rec, pos, mask, (0.0, 3.0, 1.5)[i], f"m {m} case {i}"


LSTSQ_M = (3, 4, 65, 441)


@functools.lru_cache(maxsize=None)
def _lstsq_worst(m):
    """The global and the local restatement against `np.linalg.lstsq` on [x, y, 1] over the cases of m (each held to FIT_TOL on
    the way) -> the worst scaled differences (global, local)."""
    wg = wl = 0.0
    for rec, pos, mask, k, what in _global_cases(m):
        grad, strain, residual, rms2 = O.motion_series(rec, pos, mask, k)
        assert (grad[:, 0, 0] != 0).all(), what
        wg = max(wg, O.check_global_against_independent(rec, pos, grad, residual, what))
        assert np.array_equal(strain[:, 13:15], np.sqrt(rms2)) and (strain[:, 2] <= strain[:, 1]).all()
        assert ((residual[..., 0] == 1).sum(axis=1) == strain[:, 2]).all()   # the slots of the final fit are flagged 1
        if k == 0.0:
            assert (strain[:, 0] == 1).all() and not (residual[..., 0] == 2).any()
        if m >= 4:
            K = min(6, m - 1)
            nbr = ST.neighbour_lists(pos, K)
            out = O.local_strain(rec, pos, nbr, min(4, K + 1), 0.01)
            assert (out[..., 0] != 0).any(), what
            wl = max(wl, O.check_local_against_independent(rec, pos, nbr, out, what))
    return wg, wl


@pytest.mark.parametrize("m", LSTSQ_M)
def test_restatement_against_lstsq(m):
    """Printed: the worst scaled difference, which FIT_TOL is 10 x of (see the helper)."""
    wg, wl = _lstsq_worst(m)
    print(f"m = {m}: worst scaled difference from lstsq: global {wg:.2e}, local {wl:.2e}")


def _recorded(bound, measured, what):
    """A bound IS 10 x a figure measured here and recorded in the helper.  What is met now is held to the bound itself by the
    tests above; here it is held to the RECORD: within 0.5 .. 1.25 of the recorded figure, so that a change which shrinks the
    error (the bound has gone stale) or grows it (the bound is no longer 10 x) makes this test say so.  A band and not an
    equality: lstsq's rounding may differ between BLAS builds."""
    print(f"{what}: measured {measured:.3e}, bound {bound:.3e} = {bound / measured:.1f} x")
    assert 0.5 * bound <= 10.0 * measured <= 1.25 * bound, what


def test_bounds_are_ten_times_the_measured_figures():
    _recorded(O.FIT_TOL, max(max(_lstsq_worst(m)) for m in LSTSQ_M), "FIT_TOL")
    _recorded(O.CLOSED_TOL, max(_closed_worst(th) for th in THETAS), "CLOSED_TOL")


def test_poison_never_enters_the_restatement():
    rec, pos = O.random_case(10, 130, 8, 5)
    mask = np.random.default_rng(1).random(130) < 0.7
    pos = pos.copy()
    pos[~mask] = np.nan
    for out in O.motion_series(rec, pos, mask, 2.0)[:3]:
        assert np.isfinite(out).all()
    clean = np.where(np.isnan(pos), 0.0, pos)
    assert np.isfinite(O.local_strain(rec, clean, ST.neighbour_lists(clean, 6))).all()


THETAS = (0.0, 0.5, 30.0, -170.0)


@functools.lru_cache(maxsize=None)
def _closed_worst(theta):
    """d = (R(theta) S - I) p + t on the synthetic ring: the rotation of the polar decomposition, the principal stretches, the
    linearised invariants by their definitions on R S - I, t, and a residual of rounding size -> the worst difference."""
    pos = O.ring_layout()
    S = np.array([[1.05, 0.02], [0.02, 0.97]])
    d, G = O.affine_field(pos, theta, S, (0.3, -0.2, 0.1), (0.01, -0.02))
    grad, strain, residual, _ = O.motion_series(O.record(d[None]), pos)
    lam = np.linalg.eigvalsh(S)[::-1]
    want = {3: G[0, 0] + G[1, 1], 4: 0.5 * (G[1, 0] - G[0, 1]), 5: 0.5 * (G[0, 0] - G[1, 1]), 6: 0.5 * (G[0, 1] + G[1, 0]), 9: theta,
            10: lam[0], 11: lam[1], 12: math.degrees(math.atan(math.hypot(0.01, 0.02))), 13: 0.0, 14: 0.0}
    worst = max(abs(strain[0, c] - w) for c, w in want.items())
    worst = max(worst, float(np.abs(residual[0, :, 1:]).max()), float(np.abs(grad[0, :, 1] - (0.3, -0.2, 0.1)).max()))
    assert strain[0, 0] == 1 and strain[0, 1] == 65
    assert abs(strain[0, 7] - math.hypot(want[5], want[6])) <= O.CLOSED_TOL
    assert np.array_equal(ST.invariants(grad), strain[:, 3:13])
    return worst


@pytest.mark.parametrize("theta", THETAS)
def test_closed_forms(theta):
    """Printed: the worst difference (CLOSED_TOL is 10 x the largest over the four angles)."""
    worst = _closed_worst(theta)
    print(f"theta {theta}: worst closed-form difference {worst:.2e}")
    assert worst <= O.CLOSED_TOL


def test_exactly_affine_dyadic_field_leaves_nothing():
    """Integer positions whose means and centred sums are exact, dyadic gradients: every residual and both rms are exactly 0."""
    pos = O.grid_pos(49, 2.0)
    G = np.array([[0.25, -0.5], [0.125, 0.0625], [-0.03125, 0.5]])
    d = pos @ G.T + np.array([1.5, -0.75, 0.25])
    grad, strain, residual, _ = O.motion_series(O.record(d[None]), pos)
    assert np.array_equal(grad[0, :, 2:], G) and np.array_equal(grad[0, :, 1], [1.5, -0.75, 0.25])
    assert (residual[0, :, 1:] == 0).all() and (residual[0, :, 0] == 1).all() and (strain[0, 13:15] == 0).all()
    assert strain[0, 15] == 0                                 # all q equal: the smallest index
    out = O.local_strain(O.record(d[None]), pos, ST.neighbour_lists(pos, 8), 4, 0.01)
    i = np.arange(49)
    inner = (i % 7 >= 1) & (i % 7 <= 5) & (i // 7 >= 1) & (i // 7 <= 5)      # a whole 3 x 3 block: its mean is the slot itself
    assert (out[0, :, 0] == 9).all() and (out[0, inner, 1] == 0.3125).all() and (out[0, inner, 2] == 0.3125).all()
    assert np.array_equal(out[0, inner, 6:], np.broadcast_to(G[2], (25, 2)))
    assert np.abs(out[0, :, 1:3] - 0.3125).max() <= 1e-13 and np.abs(out[0, :, 6:] - G[2]).max() <= 1e-13


def test_rejection_recovers_the_undisturbed_markers():
    pos = O.ring_layout()
    rng = np.random.default_rng(3)
    d, _ = O.affine_field(pos, 2.0, np.array([[1.01, 0.0], [0.0, 0.99]]), (0.2, 0.1, -0.3), (0.005, 0.0))
    d = d + rng.normal(0.0, 0.002, d.shape)
    hit = [7, 30, 64]
    d[hit] += np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    rec = O.record(d[None])
    grad, strain, residual, _ = O.motion_series(rec, pos, None, 3.0)
    assert strain[0, 0] == 2 and strain[0, 1] == 65 and strain[0, 2] == 62
    assert sorted(np.flatnonzero(residual[0, :, 0] == 2).tolist()) == hit
    others = np.ones(65, dtype=bool)
    others[hit] = False
    alone = O.motion_series(rec, pos, others, 0.0)
    assert np.array_equal(grad[0, :, 1:], alone[0][0, :, 1:])                # the refit IS the fit of the 62
    assert O.check_global_against_independent(rec, pos, grad, residual, "rejection") <= O.FIT_TOL
    plain = O.motion_series(rec, pos)
    assert plain[1][0, 0] == 1 and int(plain[1][0, 15]) in hit and int(strain[0, 15]) not in hit
    assert (np.abs(residual[0, hit, 1:]).max(axis=1) > 0.9).all()            # the rejected keep a residual against the final fit


def test_invariants_equal_the_strain_columns_bit_for_bit():
    rec, pos = O.random_case(12, 65, 4, 9)
    grad, strain, _, _ = O.motion_series(rec, O.ring_layout(), None, 3.0)
    assert set(strain[:, 0].tolist()) >= {0.0, 1.0}
    inv = ST.invariants(grad)
    assert inv.shape == (12, 10) and np.array_equal(inv.view(np.uint64), np.ascontiguousarray(strain[:, 3:13]).view(np.uint64))
    assert (inv[strain[:, 0] == 0] == 0).all() and len(ST.INVARIANT_COLUMNS) == 10
    with pytest.raises(ValueError):
        ST.invariants(grad[:, :2])


def test_trend_follows_the_ramps_on_the_cpu():
    """The drag-and-twist recording through the restatements of the axis displacement, the fit and the FIR.  Printed: what the
    trend meets over all frames, which TREND_TOL_* is 10 x of (see the helper)."""
    from vbs_amd import filters as F
    t, pos, tx, th = O.drag_twist_table()
    grad, strain, gf, trend = O.motion_analysis_cpu(t, F.lowpass_taps(15, 0.2))
    ok = trend[:, 0] != 0
    rot, t_f = np.abs(trend[ok, 7] - th[ok]).max(), np.abs(gf[ok, 0, 1] - tx[ok]).max()
    print(f"trend on the CPU: rot_deg off the ramp by {rot:.4f} deg, t_X by {t_f:.4f} mm")
    assert ok.all() and (strain[:, 0] == 1).all() and (strain[1:, 1] < 65).any()
    _recorded(O.TREND_TOL_DEG, rot, "TREND_TOL_DEG")
    _recorded(O.TREND_TOL_MM, t_f, "TREND_TOL_MM")


def test_motion_sheet_columns_and_nan_cells(tmp_path):
    pytest.importorskip("pandas")
    from vbs_amd import pipeline as P
    rec, _ = O.random_case(9, 65, 4, 21)
    grad, strain, _, _ = O.motion_series(rec, O.ring_layout(), None, 3.0)
    trend = np.concatenate([(np.arange(9) % 3 != 0)[:, None].astype(np.float64), ST.invariants(grad)], axis=1)
    df = P.to_motion_frame(strain, grad, trend, frame_offset=100, path=str(tmp_path / "motion.xlsx"))
    assert tuple(df.columns) == P.MOTION_FRAME_COLUMNS + P.MOTION_TREND_COLUMNS and len(df) == 9
    assert df["frameno"].tolist() == list(range(100, 109)) and os.path.getsize(tmp_path / "motion.xlsx") > 0
    fit = strain[:, 0] != 0
    assert not fit.all() and fit.any()
    for name in P.MOTION_FRAME_COLUMNS[4:25]:
        assert df[name][~fit].isna().all() and df[name][fit].notna().all(), name
    assert np.array_equal(df["gYx"][fit].to_numpy(), grad[fit, 1, 2]) and np.array_equal(df["tZ"][fit].to_numpy(), grad[fit, 2, 1])
    assert np.array_equal(df["rot_deg"][fit].to_numpy(), strain[fit, 9]) and np.array_equal(df["rms_z"][fit].to_numpy(), strain[fit, 14])
    assert (df["worst"][~fit] == -1).all() and df["n_used"].tolist() == strain[:, 2].astype(int).tolist()
    has = trend[:, 0] != 0
    assert df["rot_deg_f"][~has].isna().all() and np.array_equal(df["rot_deg_f"][has].to_numpy(), trend[has, 7])
    assert tuple(P.to_motion_frame(strain, grad).columns) == P.MOTION_FRAME_COLUMNS
    with pytest.raises(ValueError):
        P.to_motion_frame(strain[:, :15], grad)
    with pytest.raises(ValueError):
        P.to_motion_frame(strain, grad, trend[:, :10])
