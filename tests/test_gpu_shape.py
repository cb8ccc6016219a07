"""GPU tests of the indentation shape (`vbs_shape_series`) against the NumPy restatement
`tests/helpers/shape_oracle.py`: `shape`, `coef` and `residual` bit for bit but the five columns that pass through sqrt or atan2
(4 ulp), nothing masked.  Shapes are the smallest at which the kernel can go wrong - around `min_count`, around one and two lane
strides (64 slots), around the frames a workgroup takes (VBS_SHAPE_GROUP) - not the workload's; the tables hold rows without a 3-D
point, a frame with every slot missing next to full ones, reference slots without a displacement, planted outliers for the
rejection, and NaN / 1e30 / 1e300 in every cell that must not be read."""
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
import shape_cases as SC                                       # noqa: E402
import shape_oracle as O                                       # noqa: E402
import uncert_cases as UC                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.SHAPE_GROUP
#        m,   F,  start, mode,    scale, reject_k, mask,  min_count, outliers, empty frame
CASES = [(1,   1,  0,  "plane", 1.0,  0.0, False, 9, 0, None),
         (5,   3,  1,  "shell", 25.0, 0.0, False, 9, 0, 2),
         (6,   4,  3,  "plane", 1.0,  3.0, False, 6, 0, None),
         (9,   5,  0,  "shell", 1.0,  0.0, False, 9, 0, 3),
         (63,  11, 5,  "plane", 25.0, 3.0, False, 9, 2, 6),
         (64,  4,  3,  "shell", 1.0,  0.0, True,  9, 0, 1),
         (65,  11, 10, "plane", 1.0,  3.0, True,  9, 2, 4),
         (129, 5,  2,  "shell", 25.0, 3.0, False, 9, 3, 0)]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(480, 640, max_markers=256, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """Every recording with its restatement, computed once."""
    out = {}
    for i, (m, n, start, mode, scale, rk, mask, mc, outliers, empty) in enumerate(CASES):
        k = SC.recording(n, m, start, seed=i, drop=0.0 if m < 10 else 0.1, outliers=outliers, empty_frame=empty,
                         bad_ref=0.0 if m < 10 else 0.05)
        slots = np.flatnonzero(np.random.default_rng(i).random(m) < 0.8) if mask else None
        sel = None if slots is None else np.isin(np.arange(m), slots)
        k.update(mode=mode, scale=scale, rk=rk, slots=slots, mc=mc, n=n, m=m)
        k["want"] = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], start, sel, mode == "shell", scale, k["length"], rk, mc)
        out[m] = k
    return out


def _run(k, **over):
    a = dict(table=k["table"], ref_disp=k["ref_disp"], ref_xyz=k["ref_xyz"], start_frame=k["start"], mode=k["mode"], scale=k["scale"],
             length=k["length"], slots=k["slots"], reject_k=k["rk"], min_count=k["mc"])
    a.update(over)
    out = E.shape_series(**a)
    return tuple(out[w].cpu().numpy() if w in out else None for w in ("shape", "coef", "residual"))


@pytest.mark.parametrize("m", [c[0] for c in CASES])
def test_every_output_equals_the_restatement(cases, m):
    k = cases[m]
    got = _run(k)
    want = k["want"]
    O.check(got, want, f"m = {m}")
    assert np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
    deg = want[0][:, 0]
    if m >= 63:
        assert (deg == 2.0).any() and (want[0][:, 19] == 1.0).any(), "no frame of the case has a quadric with an apex"
        assert (want[0][:, 1] == 0.0).any() and (deg[want[0][:, 1] == 0.0] == 0.0).all(), "no frame without a common slot"
    if k["rk"] > 0.0 and m >= 63:
        assert (want[0][:, 2] < want[0][:, 1]).any(), "the planted outliers were not rejected in any frame"
    if m == 1:
        assert deg.tolist() == [0.0] and want[0][0, 1] == 1.0
    if m == 5:
        assert set(deg.tolist()) == {0.0, 1.0}
    if m == 6:
        assert (deg == 2.0).any()
    # any one output alone equals the same output requested with the others
    for w, i in (("shape", 0), ("coef", 1), ("residual", 2)):
        alone = _run(k, want=(w,))
        assert [x is None for x in alone] == [j != i for j in range(3)]
        assert np.array_equal(alone[i].view(np.uint64), got[i].view(np.uint64)), w


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
    assert empty[0].shape == (0, 24) and empty[1].shape == (0, 2, 4) and empty[2].shape == (0, m, 2)


def test_degeneracies_and_both_outcomes_of_the_rejection():
    for name, (xy, dz, missing, mc, want_deg) in SC.degeneracies().items():
        k = SC.table_of_heights(xy, dz[None], missing[None])
        length = SC.rms_length(xy)
        want = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=length, min_count=mc)
        out = E.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=length, min_count=mc)
        O.check(tuple(out[w].cpu().numpy() for w in ("shape", "coef", "residual")), want, name)
        deg = want[0][1, 0]
        assert deg <= want_deg[1] if isinstance(want_deg, tuple) else deg == want_deg, (name, deg)
    for name, (xy, dz, mc, rk) in SC.rejection_sets().items():
        k = SC.table_of_heights(xy, dz[None])
        length = SC.rms_length(xy)
        want = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=length, reject_k=rk, min_count=mc)
        out = E.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=length, reject_k=rk, min_count=mc)
        O.check(tuple(out[w].cpu().numpy() for w in ("shape", "coef", "residual")), want, name)
        assert want[0][1, 2] == (29.0 if name == "outlier" else 9.0) and want[0][1, 0] == 2.0


def test_refusals_leave_the_outputs_untouched(cases):
    k = cases[9]
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m = k["n"], 9
    t = torch.from_numpy(k["table"]).to(dev)
    rd, rx = torch.from_numpy(k["ref_disp"]).to(dev), torch.from_numpy(k["ref_xyz"]).to(dev)
    shape = torch.full((n, 24), -7.5, dtype=torch.float64, device=dev)
    coef = torch.full((n, 2, 4), -7.5, dtype=torch.float64, device=dev)
    res = torch.full((n, m, 2), -7.5, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)       # noqa: E731
    good = dict(table=t, n=n, m=m, start=k["start"], rd=rd, rx=rx, shell=1, scale=1.0, length=k["length"], rk=0.0, mc=9, piv=1e-10,
                apex=1e-6, reach=2.0, fb=0, fe=n, shape=shape, coef=coef, res=res)

    def call(**over):
        a = dict(good, **over)
        return L.lib().vbs_shape_series(dev.index, p(a["table"]), a["n"], a["m"], a["start"], p(a["rd"]), p(a["rx"]), C.c_void_p(0),
                                        a["shell"], a["scale"], a["length"], a["rk"], a["mc"], a["piv"], a["apex"], a["reach"], a["fb"],
                                        a["fe"], p(a["shape"]), p(a["coef"]), p(a["res"]), C.c_void_p(0))

    inf, nan = float("inf"), float("nan")
    for over in (dict(table=None), dict(rd=None), dict(rx=None), dict(shape=None, coef=None, res=None), dict(n=0), dict(m=0),
                 dict(start=-1), dict(start=n), dict(shell=2), dict(scale=inf), dict(scale=nan), dict(rk=-1.0), dict(rk=nan), dict(rk=inf),
                 dict(length=0.0), dict(length=-2.0), dict(length=inf), dict(length=nan), dict(mc=5), dict(piv=-1.0), dict(piv=inf),
                 dict(piv=nan), dict(apex=-1.0), dict(apex=inf), dict(apex=nan), dict(reach=-1.0), dict(reach=inf), dict(reach=nan),
                 dict(fb=-1), dict(fe=n + 1), dict(fb=2, fe=1)):
        assert call(**over) == L.VBS_EINVAL, over
    torch.cuda.synchronize()
    assert (shape == -7.5).all() and (coef == -7.5).all() and (res == -7.5).all()
    assert call(fb=1, fe=1) == L.VBS_OK                           # an empty range emits nothing
    torch.cuda.synchronize()
    assert (shape == -7.5).all() and (coef == -7.5).all() and (res == -7.5).all()
    assert call() == L.VBS_OK
    torch.cuda.synchronize()
    O.check((shape.cpu().numpy(), coef.cpu().numpy(), res.cpu().numpy()), k["want"], "the direct call")
    with pytest.raises(ValueError):
        _run(k, start_frame=n)
    with pytest.raises(ValueError):
        _run(k, length=0.0)
    with pytest.raises(ValueError):
        _run(k, min_count=5)


def test_coef_feeds_the_filter_and_residual_the_field_map(cases):
    from vbs_amd import fields
    from vbs_amd.filters import half_taps
    k = cases[65]
    out = E.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], k["start"], k["mode"], k["scale"], k["length"], k["slots"], k["rk"],
                         k["mc"])
    coef, res = out["coef"].cpu().numpy(), out["residual"].cpu().numpy()
    taps = np.array([0.25, 0.5, 0.25])
    got = E.fir_series_f64(out["coef"], taps, 3).cpu().numpy()
    FI.check_fir(got, coef, half_taps(taps), 3, what="coef through the filter")
    assert (got[..., 0] == 3.0).any()
    good = k["ref_disp"][:, 0] != 0
    nodes = np.where(good[:, None], k["ref_xyz"][:, :2], np.nan)      # (a slot without a reference position gets no weight)
    grid_xy = np.stack([g.ravel() for g in np.meshgrid(np.linspace(-6, 6, 4), np.linspace(-6, 6, 4))], axis=1)
    W = fields.gaussian_weights(nodes, grid_xy, 3.0)
    wsum = fields.row_sums(W)
    mp = E.field_map_f64(out["residual"], W, wsum, 0.5, 1).cpu().numpy()
    _, _, d = FO.exact_map(res, W, 1)                            # (the map's order of summation is not part of its interface)
    assert FO.coverage_margin(d, wsum, 0.5) > FO.Fraction(1, 10 ** 9)
    FO.check_within_bound(mp, res, W, wsum, 0.5, 1, what="residual through the field map")
    assert (mp[..., 0] == 1.0).any()


def test_shape_analysis_and_its_sheet_on_a_cap_recording(eng, tmp_path):
    """12 frames: a cap pressed deeper and deeper - its radius shrinks from 90 to 57 mm - while its centre walks along x.  The apex
    follows the centre, the deepest frame is among the last, every pressed frame is a bowl, and the sheet has its columns and
    dtypes.  Bounds: those `tests/test_shape_host.py` derives for R = 60 mm, applied to the frames with R <= 60 mm."""
    from vbs_amd import fields, pipeline as P, shapes
    cam = UC.camera((640, 480), distorted=True)
    ref = SC.ring61()
    F = 12
    centres = [(-3.0 + 0.5 * f, 1.0) for f in range(F)]
    depths = [0.2 + 0.1 * f for f in range(F)]
    Rs = np.array([90.0 - 3.0 * f for f in range(F)])
    tab = SC.cap_recording(cam, ref, Rs, centres, depths, seed=9)   # frame 0 is the start, at rest
    flat = np.stack([tab[0], tab[0]])                            # the reference session does not move: ref_disp = 0
    grid_xy = np.stack([g.ravel() for g in np.meshgrid(np.linspace(-12, 12, 5), np.linspace(-12, 12, 5))], axis=1)
    W = fields.gaussian_weights(ref[:, :2], grid_xy, 4.0)
    res = P.shape_analysis(eng, torch.from_numpy(tab).cuda(), torch.from_numpy(flat).cuda(), ref, taps=np.array([0.25, 0.5, 0.25]),
                           grid=(W, fields.row_sums(W)))
    rd = np.zeros((61, 4))
    rd[:, 0] = 1.0
    want = O.shape_series(tab, rd, ref, 0, length=shapes.default_length(ref))
    O.check((res["shape"].cpu().numpy(), res["coef"].cpu().numpy(), res["residual"].cpu().numpy()), want, "the cap recording")
    sh = want[0]
    assert (sh[1:, 0] == 2.0).all() and (sh[1:, 19] == 1.0).all() and sh[0, 19] == 0.0
    assert (res["kind"][1:] == shapes.KIND_BOWL).all() and abs(res["kind_share"]["bowl"] - F / (F + 1.0)) < 1e-12
    assert res["deepest_frame"] == int(np.argmax(np.abs(sh[:, 23]))) and res["deepest_frame"] >= F - 3
    track = res["apex_track"]
    assert track.shape == (F + 1, 4) and (track[1:, 0] == 1.0).all() and np.isnan(track[0, 1:]).all()
    assert np.array_equal(track[1:, 1:], sh[1:, 20:23])
    tight = np.flatnonzero(Rs <= 60.0)                           # frames 1 + tight of the table
    err = np.hypot(track[1 + tight, 1] - np.array(centres)[tight, 0], track[1 + tight, 2] - 1.0)
    assert tight.size >= 2 and (err <= 0.55).all(), err
    assert (np.diff(track[1:, 1]) > -0.55).all() and track[-1, 1] - track[1, 1] > 3.0       # it walks with the centre
    assert res["coef_filtered"].shape == (F + 1, 2, 7) and res["trend"].shape == (F + 1, 6) and res["residual_map"].shape == (F + 1, 25, 2)
    tr = res["trend"].cpu().numpy()
    assert (tr[1:, 0] == 1.0).all()
    assert (np.abs(tr[1 + tight][:, 3:5] * Rs[tight, None] - 1.0) <= 0.20).all(), tr[1 + tight][:, 3:5]
    df = P.to_shape_frame(res, frame_offset=100, path=tmp_path / "shape.csv")
    assert tuple(df.columns) == P.SHAPE_FRAME_COLUMNS + P.SHAPE_TREND_COLUMNS and len(df) == F + 1
    assert df["frameno"].tolist() == list(range(100, 101 + F)) and df["frameno"].dtype == np.int64
    for name in ("degree", "count", "n_used", "apex"):
        assert df[name].dtype == np.int64, name
    for name in P.SHAPE_FRAME_COLUMNS[5:21] + P.SHAPE_FRAME_COLUMNS[22:] + P.SHAPE_TREND_COLUMNS:
        assert df[name].dtype == np.float64, name
    assert df["kind"].tolist() == ["ridge"] + ["bowl"] * F
    assert np.array_equal(df["depth"].to_numpy()[1:], sh[1:, 23]) and np.isnan(df["depth"].to_numpy()[0])
    assert (tmp_path / "shape.csv").exists()
