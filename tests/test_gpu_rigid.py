"""GPU tests of the rigid motion (`vbs_rigid_series`) against the NumPy restatement `tests/helpers/rigid_oracle.py`:
`rigid`, `coef` and `residual` bit for bit, +0 and -0 told apart, but the six columns that pass through a root or an arc tangent
(4 ulp), nothing masked.  Shapes are the smallest at which the kernel can go wrong - around three common slots, around one and two
lane strides (64 slots), the workload's 441, around the frames a workgroup takes (VBS_RIGID_GROUP) - the tables hold rows without a
3-D point, a frame with every slot missing next to full ones, source slots with flag 0, planted outliers for the rejection, and
NaN / 1e30 / 1e300 in every cell that must not be read."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import vbs_amd._lib as L                                       # noqa: E402
from vbs_amd import engine as E                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import field_oracle as FO                                      # noqa: E402
import filter_oracle as FI                                     # noqa: E402
import posecov_cases as PC                                     # noqa: E402
import rigid_cases as RC                                       # noqa: E402
import rigid_oracle as O                                       # noqa: E402
import uncert_cases as UC                                      # noqa: E402
import uncert_oracle as U                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.RIGID_GROUP
WANT = ("rigid", "coef", "residual")
#        m,   F,  with_scale, reject_k, mask, outliers, empty frame
CASES = [(1,   1,  False, 0.0, False, 0, None),
         (2,   4,  True,  0.0, False, 0, None),
         (3,   5,  False, 3.0, False, 0, None),
         (4,   4,  True,  3.0, False, 0, 2),
         (63,  11, False, 3.0, False, 2, 6),
         (64,  4,  True,  0.0, True,  0, 1),
         (65,  11, True,  3.0, True,  2, 4),
         (129, 5,  False, 3.0, False, 3, 1),
         (441, 5,  True,  3.0, True,  4, 2)]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(480, 640, max_markers=256, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """Every recording with its restatement, computed once."""
    out = {}
    for i, (m, n, ws, rk, mask, outliers, empty) in enumerate(CASES):
        k = RC.recording(n, m, seed=i, drop=0.0 if m < 10 else 0.1, outliers=outliers, empty_frame=empty,
                         bad_src=0.0 if m < 10 else 0.05, scale=1.01 if ws else 1.0)
        slots = np.flatnonzero(np.random.default_rng(i).random(m) < 0.8) if mask else None
        sel = None if slots is None else np.isin(np.arange(m), slots)
        k.update(ws=ws, rk=rk, slots=slots, n=n, m=m)
        k["want"] = O.rigid_series(k["table"], k["source"], sel, ws, rk)
        out[m] = k
    return out


def _run(k, **over):
    a = dict(table=k["table"], source=k["source"], slots=k["slots"], with_scale=k["ws"], reject_k=k["rk"])
    a.update(over)
    out = E.rigid_series(**a)
    return tuple(out[w].cpu().numpy() if w in out else None for w in WANT)


@pytest.mark.parametrize("m", [c[0] for c in CASES])
def test_every_output_equals_the_restatement(cases, m):
    k = cases[m]
    got = _run(k)
    want = k["want"]
    O.check(got, want, f"m = {m}")
    assert np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
    flag = want[0][:, 0]
    if m >= 63:
        assert (want[0][:, 1] == 0.0).any() and (flag[want[0][:, 1] == 0.0] == 0.0).all(), "no frame without a common slot"
        assert (flag >= 1.0).any()
    if k["rk"] > 0.0 and m >= 63:
        assert (flag == 2.0).any() and (want[0][flag == 2.0, 2] < want[0][flag == 2.0, 1]).all(), "the planted outliers were not rejected"
        assert (flag == 1.0).any(), "no frame keeps its first fit"
    if k["ws"] and m >= 63:
        assert (want[0][flag >= 1.0, 25] != 1.0).any()
    if m < 3:
        assert (flag == 0.0).all() and (want[0][:, 1] == float(m)).all()
    if m == 3:
        assert (flag == 1.0).all()
    # any one output alone equals the same output requested with the others
    for w, i in zip(WANT, range(3)):
        alone = _run(k, want=(w,))
        assert [x is None for x in alone] == [j != i for j in range(3)]
        assert np.array_equal(alone[i].view(np.uint64), got[i].view(np.uint64)), w
    # a table and a source that live on the device already give the same bits as host arrays
    dev = _run(k, table=torch.from_numpy(k["table"]).cuda(), source=torch.from_numpy(k["source"]).cuda())
    for a, b in zip(dev, got):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_special_frames():
    """The identity frame (R = I exactly), an exact half turn about z, the same about an oblique axis as float32 makes it, a frame
    whose points lie on a line (flag 0 and zeros) and a coincident one."""
    lay = RC.layout65().astype(np.float32).astype(np.float64)
    half_z = lay * np.array([-1.0, -1.0, 1.0])
    half = RC.moved(lay, RC.rotation((0.6, 0.0, 0.8), 180.0), (1.0, -2.0, 0.5))
    t = np.linspace(-8.0, 8.0, 65)
    line = np.column_stack([1.0 + 0.6 * t, -2.0 + 0.8 * t, 0.25 * t])
    tab = RC.table_of_points(np.stack([lay, half_z, half, line, np.ones((65, 3))]))
    src = RC.source_of(lay)
    for ws in (False, True):
        want = O.rigid_series(tab, src, None, ws, 3.0)
        out = E.rigid_series(tab, src, with_scale=ws, reject_k=3.0)
        O.check(tuple(out[w].cpu().numpy() for w in WANT), want, f"special frames, with_scale {ws}")
        r = want[0]
        assert r[0, 9:22].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        if ws:                                                    # s = D / Sqq: two sums of the same squares in two orders
            assert abs(r[0, 25] - 1.0) <= 4 * 2.0 ** -52 and np.abs(r[0, 22:25]).max() <= 1e-15 and r[0, 26] <= 1e-14
        else:
            assert r[0, 22:26].tolist() == [0.0, 0.0, 0.0, 1.0] and r[0, 26] == 0.0
        assert r[:3, 0].tolist() == [1.0, 1.0, 1.0] and (r[0, 27:32] == 0.0).all()
        assert abs(r[1, 28] - 180.0) < 1e-9 and abs(abs(r[1, 31]) - 180.0) < 1e-9 and r[1, 29] < 1e-9 and r[1, 26] < 1e-12
        assert abs(r[2, 28] - 180.0) < 1e-4 and r[2, 26] < 1e-5
        assert (r[3:, 0] == 0.0).all() and (r[3:, 9:32] == 0.0).all() and (r[3:, 1] == 65.0).all()
        assert (want[1][3:] == 0.0).all() and (want[2][3:] == 0.0).all()


@pytest.mark.parametrize("m", [65, 129])
def test_frame_ranges_equal_the_rows_of_the_full_call(cases, m):
    k = cases[m]
    full = _run(k)
    n = k["n"]
    for cut in (G - 1, G, G + 1):
        for a, b in ((0, cut), (cut, n)):
            part = _run(k, frame_range=(a, b))
            for g, f in zip(part, full):
                assert g.shape[0] == b - a and np.array_equal(g.view(np.uint64), f[a:b].view(np.uint64)), (cut, a, b)
    empty = _run(k, frame_range=(2, 2))
    assert empty[0].shape == (0, 33) and empty[1].shape == (0, 4, 4) and empty[2].shape == (0, m, 4)


def test_refusals_leave_the_outputs_untouched(cases):
    k = cases[4]
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m = k["n"], 4
    t = torch.from_numpy(k["table"]).to(dev)
    src = torch.from_numpy(k["source"]).to(dev)
    rigid = torch.full((n, 33), -7.5, dtype=torch.float64, device=dev)
    coef = torch.full((n, 4, 4), -7.5, dtype=torch.float64, device=dev)
    res = torch.full((n, m, 4), -7.5, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)       # noqa: E731
    good = dict(table=t, n=n, m=m, src=src, ws=1, rk=3.0, gap=1e-6, fb=0, fe=n, rigid=rigid, coef=coef, res=res)

    def call(**over):
        a = dict(good, **over)
        return L.lib().vbs_rigid_series(dev.index, p(a["table"]), a["n"], a["m"], p(a["src"]), C.c_void_p(0), a["ws"], a["rk"], a["gap"],
                                        a["fb"], a["fe"], p(a["rigid"]), p(a["coef"]), p(a["res"]), C.c_void_p(0))

    inf, nan = float("inf"), float("nan")
    for over in (dict(table=None), dict(src=None), dict(rigid=None, coef=None, res=None), dict(n=0), dict(m=0), dict(ws=2), dict(ws=-1),
                 dict(rk=-1.0), dict(rk=nan), dict(rk=inf), dict(gap=-1e-9), dict(gap=nan), dict(gap=inf), dict(fb=-1), dict(fe=n + 1),
                 dict(fb=2, fe=1)):
        assert call(**over) == L.VBS_EINVAL, over
    torch.cuda.synchronize()
    assert (rigid == -7.5).all() and (coef == -7.5).all() and (res == -7.5).all()
    assert call(fb=1, fe=1) == L.VBS_OK                           # an empty range emits nothing
    torch.cuda.synchronize()
    assert (rigid == -7.5).all() and (coef == -7.5).all() and (res == -7.5).all()
    assert call() == L.VBS_OK
    torch.cuda.synchronize()
    O.check((rigid.cpu().numpy(), coef.cpu().numpy(), res.cpu().numpy()), k["want"], "the direct call")
    with pytest.raises(ValueError):
        _run(k, reject_k=-1.0)
    with pytest.raises(ValueError):
        _run(k, source=k["source"][:, :3])
    with pytest.raises(ValueError):
        _run(k, frame_range=(0, n + 1))


def test_coef_feeds_the_filter_and_residual_the_field_map(cases):
    from vbs_amd import fields
    from vbs_amd.filters import half_taps
    k = cases[65]
    out = E.rigid_series(k["table"], k["source"], k["slots"], k["ws"], k["rk"])
    coef, res = out["coef"].cpu().numpy(), out["residual"].cpu().numpy()
    taps = np.array([0.25, 0.5, 0.25])
    got = E.fir_series_f64(out["coef"], taps, 3).cpu().numpy()
    FI.check_fir(got, coef, half_taps(taps), 3, what="coef through the filter")
    assert (got[..., 0] == 3.0).any()
    good = k["source"][:, 0] != 0
    nodes = np.where(good[:, None], k["layout"][:, :2], np.nan)       # (a slot without a source point gets no weight)
    grid_xy = np.stack([g.ravel() for g in np.meshgrid(np.linspace(-6, 6, 4), np.linspace(-6, 6, 4))], axis=1)
    W = fields.gaussian_weights(nodes, grid_xy, 3.0)
    wsum = fields.row_sums(W)
    mp = E.field_map_f64(out["residual"], W, wsum, 0.5, 3).cpu().numpy()
    _, _, d = FO.exact_map(res, W, 3)                            # (the map's order of summation is not part of its interface)
    assert FO.coverage_margin(d, wsum, 0.5) > FO.Fraction(1, 10 ** 9)
    FO.check_within_bound(mp, res, W, wsum, 0.5, 3, what="residual through the field map")
    assert (mp[..., 0] == 1.0).any()


def test_rigid_analysis_and_its_sheet_on_a_solved_recording(eng, tmp_path):
    """12 frames of the 65-marker shell, tilted 0 -> 2 degrees and twisted 0 -> 3 degrees, seen through an undistorted camera without
    pixel noise and solved by `Engine.solve3d`: the table is the engine's own.  What is left of the motion's angles is the float32 of
    the pixel columns (an ulp of 6e-5 px at 600 px, 4e-6 mm on the shell at 15 px per mm) over the shell's lever of 63 mm
    (`tests/test_rigid_host.py`): below 1e-5 degrees; the bound below is 1e-3."""
    import pandas as pd
    from vbs_amd import fields, pipeline as P, rigid as RG
    cam = UC.camera((640, 480), distorted=False, T=(0.0, 0.0, 45.0))
    c = U.Cam(*cam)
    F = 12
    lay = RC.layout65()
    centre = lay.mean(axis=0)
    tilt, twist = np.linspace(0.0, 2.0, F), np.linspace(0.0, 3.0, F)
    tab = np.zeros((F, 65, 10), dtype=np.float32)
    for f in range(F):
        X = RC.moved(lay - centre, RC.swing_twist(tilt[f], 35.0, twist[f]), centre + np.array([0.01 * f, 0.0, 0.0]))
        tab[f, :, 1:4] = PC.observe(c, X)
    tab[..., 0] = RC.FLAG_TRACKED
    tab[5, 7, 0] = 0.0                                            # one marker lost in one frame
    table = eng.solve3d(torch.from_numpy(tab).cuda(), L.make_camera(*cam), 5.0)
    solved = table.cpu().numpy()
    assert ((solved[..., 0].astype(np.int64) & 2) != 0).sum() == F * 65 - 1
    grid_xy = np.stack([g.ravel() for g in np.meshgrid(np.linspace(-12, 12, 5), np.linspace(-12, 12, 5))], axis=1)
    W = fields.gaussian_weights(lay[:, :2], grid_xy, 4.0)
    res = P.rigid_analysis(eng, table, "start", 0, taps=np.array([0.25, 0.5, 0.25]), grid=(W, fields.row_sums(W), grid_xy))
    src = RG.source_from_table(solved, 0)
    assert np.array_equal(res["source"], src)
    want = O.rigid_series(solved, src, None, False, 3.0)
    O.check((res["rigid"].cpu().numpy(), res["coef"].cpu().numpy(), res["residual"].cpu().numpy()), want, "the solved recording")
    rg = res["rigid"].cpu().numpy()                              # (the device's own, just held to the restatement)
    assert (rg[:, 0] >= 1.0).all() and rg[5, 1] == 64.0
    assert np.abs(rg[:, 29] - tilt).max() < 1e-3 and np.abs(rg[:, 31] - twist).max() < 1e-3
    assert np.abs(rg[3:, 30] - 35.0).max() < 0.1                  # (the direction of a lean of 0.5 degrees and more)
    assert np.array_equal(res["tilt_deg"], rg[:, 29]) and np.array_equal(res["twist_deg"], rg[:, 31])
    assert res["max_tilt_frame"] == F - 1 and res["max_twist_frame"] == F - 1
    assert res["rotvec"].shape == (F, 3) and np.allclose(np.sqrt((res["rotvec"] ** 2).sum(axis=1)), rg[:, 28], rtol=0, atol=1e-9)
    # the centroid of the USED set shifts by 0.01 mm a frame plus (R - I) times its offset from the layout's centroid, about which the
    # shell turns: two slots of 65 rejected at the rim move it by 2 x 16.3 / 63 = 0.52 mm, times the angle of 3.6 degrees = 0.033 mm
    assert np.allclose(res["shift"][:, 0], 0.01 * np.arange(F), rtol=0, atol=0.04) and (res["scale"] == 1.0).all()
    assert res["kind"][0] == RG.KIND_STILL and res["kind"][-1] == RG.KIND_MIXED
    assert res["slot_rms"].shape == (65,) and res["worst_slots"].shape == (5,) and np.isfinite(res["slot_rms"]).all()
    assert res["coef_filtered"].shape == (F, 4, 7) and res["trend"].shape == (F, 8) and (res["trend"][:, 0] == 1.0).all()
    assert np.abs(res["trend"][1:-1, 2] - tilt[1:-1]).max() < 0.01 and np.abs(res["trend"][1:-1, 4] - twist[1:-1]).max() < 0.01
    assert res["residual_map"].shape == (F, 25, 2) and res["residual_patch"].shape == (F, 8)
    df = P.to_rigid_frame(res, frame_offset=100, path=tmp_path / "rigid.csv")
    assert tuple(df.columns) == P.RIGID_FRAME_COLUMNS + P.RIGID_TREND_COLUMNS and len(df) == F
    assert df["frameno"].tolist() == list(range(100, 100 + F)) and df["frameno"].dtype == np.int64
    for name in ("flag", "count", "n_used"):
        assert df[name].dtype == np.int64, name
    for name in P.RIGID_FRAME_COLUMNS[5:] + P.RIGID_TREND_COLUMNS:
        assert df[name].dtype == np.float64, name
    assert np.array_equal(df["tilt_deg"].to_numpy(), rg[:, 29]) and df["kind"].tolist()[0] == "still"
    back = pd.read_csv(tmp_path / "rigid.csv", float_precision="round_trip")
    assert tuple(back.columns) == tuple(df.columns) and back["kind"].tolist() == df["kind"].tolist()
    for name in df.columns:
        if name != "kind":
            assert np.array_equal(back[name].to_numpy(), df[name].to_numpy(), equal_nan=True), name
