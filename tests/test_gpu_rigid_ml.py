"""GPU tests of the noise-weighted rigid motion (`vbs_rigid_ml_series`) against the NumPy restatement
`tests/helpers/rigid_ml_oracle.py`: `ml`, `pcov`, `coef` and `mahal` bit for bit, +0 and -0 told apart, but the four angle columns
that pass through an arc tangent last (4 ulp), nothing masked.  Shapes are the smallest at which the kernel can go wrong - three and
four slots, around one and two lane strides (64 slots), the workload's 441, around the frames a workgroup takes
(VBS_RIGID_ML_GROUP), 1, 8 and 16 steps, with and without a covariance of the source - the inputs hold rows without a point, cov
flags of 0, covariances with a zero pivot, a frame without a start, a frame that ends in flag 1, starts with and without
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
import rigid_ml_cases as MC                                    # noqa: E402
import rigid_ml_oracle as O                                    # noqa: E402
import rigid_oracle as RO                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.RIGID_ML_GROUP
WANT = ("ml", "pcov", "coef", "mahal")
#        m,   F,         iters, source_cov, reject_k, outliers
CASES = [(3,   1,         8,  False, 0.0, 0),
         (4,   G - 1,     16, True,  0.0, 0),
         (63,  G,         8,  False, 3.0, 2),
         (64,  2 * G + 1, 1,  True,  0.0, 0),
         (65,  2 * G + 1, 8,  True,  3.0, 2),
         (129, G,         16, False, 3.0, 3),
         (441, 2 * G + 1, 8,  True,  3.0, 4)]


@pytest.fixture(scope="module")
def cases():
    """Every recording with its restatement, computed once."""
    out = {}
    for i, (m, n, iters, sc, rk, outliers) in enumerate(CASES):
        k = MC.recording(n, m, seed=i, reject_k=rk, with_source_cov=sc, outliers=outliers)
        k.update(n=n, m=m, iters=iters)
        k["want"] = O.rigid_ml_series(k["table"], k["source"], k["cov"], k["rigid"], k["residual"], k["source_cov"], iters)
        out[m] = k
    return out


def _run(k, **over):
    a = dict(table=k["table"], source=k["source"], cov=k["cov"], rigid=k["rigid"], residual=k["residual"], source_cov=k["source_cov"],
             iters=k["iters"])
    a.update(over)
    out = E.rigid_ml_series(**a)
    return tuple(out[w].cpu().numpy() if w in out else None for w in WANT)


@pytest.mark.parametrize("m", [c[0] for c in CASES])
def test_every_output_equals_the_restatement(cases, m):
    k = cases[m]
    got = _run(k)
    want = k["want"]
    O.check(got, want, f"m = {m}")
    assert all(np.isfinite(w).all() for w in want)
    flag = want[0][:, 0]
    assert (flag == 2.0).any() or k["n"] < 2
    if k["n"] > 1:
        assert flag[1] == 0.0 and not want[0][1].any() and not want[3][1].any(), "the frame without a start"
    if k["n"] > 2:
        assert flag[2] == 1.0 and want[0][2, 2] <= 2.0 and want[1][2, 0] == 0.0, "the frame with two usable covariances"
        assert np.array_equal(want[0][2, 4:8], k["rigid"][2, 9:13]) and np.array_equal(want[0][2, 8:17], k["rigid_clean"][2, 13:22])
        assert np.array_equal(want[3][2, :, 1], want[3][2, :, 2])
    if m >= 63:
        fit = flag == 2.0
        assert (want[0][fit, 2] < want[0][fit, 1]).all(), "no slot lost to a cov flag of 0 or a singular covariance"
        if k["source_cov"] is None and k["iters"] >= 8:            # (with source_cov the weights move with R: chi^2 is not the objective)
            assert (want[0][fit, 26] < want[0][fit, 28]).all(), "the weighted pose does not lower chi^2 below the start's"
    if k["reject_k"] > 0.0 and k["n"] > 3:
        assert (k["rigid"][:, 0] == 2.0).any() and (k["rigid"][:, 0] == 1.0).any(), "starts with and without a rejected slot"
    # any one output alone equals the same output requested with the others
    for w, i in zip(WANT, range(4)):
        alone = _run(k, want=(w,))
        assert [x is None for x in alone] == [j != i for j in range(4)]
        assert np.array_equal(alone[i].view(np.uint64), got[i].view(np.uint64)), w
    # two runs are bit-identical; inputs that live on the device already give the same bits as host arrays
    dev = _run(k, **{name: torch.from_numpy(k[name]).cuda() for name in ("table", "source", "cov", "rigid", "residual")})
    for a, b in zip(dev, got):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("m", [65, 441])
def test_without_source_cov_and_other_step_counts(cases, m):
    k = cases[m]
    for iters in (1, 16):
        want = O.rigid_ml_series(k["table"], k["source"], k["cov"], k["rigid"], k["residual"], None, iters)
        O.check(_run(k, source_cov=None, iters=iters), want, f"m = {m}, no source_cov, iters {iters}")
        assert (want[0][want[0][:, 0] == 2.0, 3] == iters).all()


@pytest.mark.parametrize("m", [65, 129])
def test_frame_ranges_equal_the_rows_of_the_full_call(cases, m):
    k = cases[m]
    full = _run(k)
    n = k["n"]
    for cut in sorted({1, G - 1, min(G + 1, n - 1)}):
        for a, b in ((0, cut), (cut, n)):
            part = _run(k, frame_range=(a, b), cov=k["cov"][a:b], rigid=k["rigid"][a:b], residual=k["residual"][a:b])
            for g, f in zip(part, full):
                assert g.shape[0] == b - a and np.array_equal(g.view(np.uint64), f[a:b].view(np.uint64)), (cut, a, b)
    empty = _run(k, frame_range=(2, 2), cov=k["cov"][2:2], rigid=k["rigid"][2:2], residual=k["residual"][2:2])
    assert empty[0].shape == (0, 40) and empty[1].shape == (0, 22) and empty[2].shape == (0, 4, 4) and empty[3].shape == (0, m, 3)


def test_the_raw_entry_refusals_null_outputs_and_guard_bands(cases):
    k = cases[65]
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m = k["n"], 65
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                   # noqa: E731
    t, src, cov, rg, rs, sc = (up(k[x]) for x in ("table", "source", "cov", "rigid", "residual", "source_cov"))
    shapes = dict(ml=(n, 40), pcov=(n, 22), coef=(n, 16), mahal=(n, m * 3))
    PAD = 64                                                       # a guard band of 64 doubles before and after every output

    def fresh():
        return {w: torch.full((PAD + int(np.prod(s)) + PAD,), -7.5, dtype=torch.float64, device=dev) for w, s in shapes.items()}

    def ptr(x, off=0):
        return C.c_void_p(x.data_ptr() + 8 * off) if x is not None else C.c_void_p(0)

    def call(bufs, null=(), **over):
        a = dict(table=t, n=n, m=m, src=src, cov=cov, rg=rg, rs=rs, sc=sc, iters=k["iters"], piv=1e-12, fb=0, fe=n)
        a.update(over)
        outs = [ptr(None) if (w in null or bufs is None) else ptr(bufs[w], PAD) for w in WANT]
        return L.lib().vbs_rigid_ml_series(dev.index, ptr(a["table"]), a["n"], a["m"], ptr(a["src"]), ptr(a["cov"]), ptr(a["rg"]),
                                           ptr(a["rs"]), ptr(a["sc"]), a["iters"], a["piv"], a["fb"], a["fe"], *outs, C.c_void_p(0))

    inf, nan = float("inf"), float("nan")
    bufs = fresh()
    for over in (dict(table=None), dict(src=None), dict(cov=None), dict(rg=None), dict(rs=None), dict(n=0), dict(m=0), dict(iters=0),
                 dict(iters=-1), dict(iters=L.RIGID_ML_MAX_ITERS + 1), dict(piv=-1e-12), dict(piv=nan), dict(piv=inf), dict(fb=-1),
                 dict(fe=n + 1), dict(fb=2, fe=1)):
        assert call(bufs, **over) == L.VBS_EINVAL, over
    assert call(bufs, null=WANT) == L.VBS_EINVAL
    assert call(bufs, fb=1, fe=1) == L.VBS_OK                     # an empty range emits nothing
    torch.cuda.synchronize()
    assert all((b == -7.5).all() for b in bufs.values())
    # every output, then each NULL in turn: what is written equals the restatement and the guard bands stay as they were
    for null in ((),) + tuple((w,) for w in WANT):
        bufs = fresh()
        assert call(bufs, null=null) == L.VBS_OK
        torch.cuda.synchronize()
        got = []
        for w, want in zip(WANT, k["want"]):
            b = bufs[w].cpu().numpy()
            assert (b[:PAD] == -7.5).all() and (b[-PAD:] == -7.5).all(), (null, w, "guard band")
            if w in null:
                assert (b == -7.5).all(), (null, w)
                got.append(None)
            else:
                got.append(b[PAD:-PAD].reshape(want.shape))
        O.check(tuple(got), k["want"], f"the direct call without {null}")
    with pytest.raises(ValueError):
        _run(k, iters=0)
    with pytest.raises(ValueError):
        _run(k, piv_rel=-1.0)
    with pytest.raises(ValueError):
        _run(k, cov=k["cov"][1:])
    with pytest.raises(ValueError):
        _run(k, source_cov=k["source_cov"][:, :6])


def test_three_collinear_slots_end_in_flag_1_through_the_pivot_of_the_normal_matrix():
    """Three usable slots on one line leave the rotation about it free: not n_used < 3 but a pivot of the 6 x 6 stops the frame;
    next to it the same frame with a fourth usable slot off the line, which is fitted."""
    import rigid_cases as RC
    t = np.array([-8.0, 1.0, 6.0])
    lay = np.column_stack([1.0 + 0.6 * t, -2.0 + 0.8 * t, 0.0 * t])
    lay = np.concatenate([lay, RC.layout65()[:5]])               # five more slots so that Horn has a start
    P = lay[None] + np.random.default_rng(3).normal(size=(2, 8, 3)) * 1e-3
    k = dict(table=RC.table_of_points(P), source=RC.source_of(lay))
    usable = np.arange(8)[None] < np.array([[3], [4]])
    k["cov"] = MC.cov7(MC.needle(P, np.array([0.0, 0.0, 45.0])), usable)
    rigid, res = MC.poison_start(*MC.start_of(k), seed=1)
    want = O.rigid_ml_series(k["table"], k["source"], k["cov"], rigid, res, None, 8, piv_rel=1e-9)
    assert want[0][:, 0].tolist() == [1.0, 2.0] and want[0][:, 2].tolist() == [3.0, 4.0] and want[1][:, 0].tolist() == [0.0, 1.0]
    out = E.rigid_ml_series(k["table"], k["source"], k["cov"], rigid, res, None, 8, piv_rel=1e-9)
    O.check(tuple(out[w].cpu().numpy() for w in WANT), want, "three collinear slots")


def test_the_device_start_feeds_the_entry(cases):
    """The records of `rigid_series` on the device, handed over without a copy, give what the restated start gives."""
    k = cases[129]
    start = E.rigid_series(k["table"], k["source"], None, False, k["reject_k"], want=("rigid", "residual"))
    RO.check((start["rigid"].cpu().numpy(), None, start["residual"].cpu().numpy()), (k["rigid_clean"], None, k["residual_clean"]), "the start")
    # (the start's exact columns are the only ones the entry reads: qm, the quaternion, t and the residual's flags)
    out = E.rigid_ml_series(k["table"], k["source"], k["cov"], start["rigid"], start["residual"], None, k["iters"])
    O.check(tuple(out[w].cpu().numpy() for w in WANT), k["want"], "from the device's start")


def test_rigid_uncertainty_is_the_composition_of_its_entries(tmp_path):
    """12 frames of the 65-marker shell, tilted 0 -> 2 degrees and twisted 0 -> 3 degrees, seen through an undistorted camera with
    pixel noise of 0.05 px on the centres and 0.1 px on the diameter and solved by `Engine.solve3d`: `pipeline.rigid_uncertainty`
    against the restatements of `vbs_rigid_series`, `vbs_uncert_cov` and `vbs_rigid_ml_series` composed on the host, with the source
    taken from the table (so `source_cov` is the source frame's row of `cov`) and from the layout (none)."""
    import pandas as pd
    import posecov_cases as PC
    import rigid_cases as RC
    import uncert_cases as UC
    import uncert_oracle as U
    from vbs_amd import pipeline as P, rigid as RG
    cam = UC.camera((640, 480), distorted=False, T=(0.0, 0.0, 45.0))
    c = U.Cam(*cam)
    F = 12
    rng = np.random.default_rng(77)
    lay = RC.layout65()
    centre = lay.mean(axis=0)
    tilt, twist = np.linspace(0.0, 2.0, F), np.linspace(0.0, 3.0, F)
    tab = np.zeros((F, 65, 10), dtype=np.float32)
    for f in range(F):
        X = RC.moved(lay - centre, RC.swing_twist(tilt[f], 35.0, twist[f]), centre + np.array([0.01 * f, 0.0, 0.0]))
        tab[f, :, 1:4] = PC.observe(c, X) + rng.normal(size=(65, 3)) * np.array([0.05, 0.05, 0.1])
    tab[..., 0] = RC.FLAG_TRACKED
    tab[5, 7, 0] = 0.0                                            # one marker lost in one frame
    e = E.Engine(480, 640, max_markers=256, max_batch=2)
    try:
        table = e.solve3d(torch.from_numpy(tab).cuda(), L.make_camera(*cam), 5.0)
        solved = table.cpu().numpy()
        obs = np.array([0.05 ** 2, 0.0, 0.0, 0.05 ** 2, 0.0, 0.1 ** 2])
        taps = np.array([0.25, 0.5, 0.25])
        for source in ("start", "layout", 3):
            res = P.rigid_uncertainty(e, table, L.make_camera(*cam), obs, source=source, reject_k=3.0, taps=taps, layout=lay)
            src = RG.source_from_layout(lay) if source == "layout" else RG.source_from_table(solved, 0 if source == "start" else source)
            assert np.array_equal(res["source"], src)
            rigid, _, residual = RO.rigid_series(solved, src, None, False, 3.0)
            cov, _ = U.solve3d_cov(solved, c, obs)
            sc = None if source == "layout" else cov[0 if source == "start" else source]
            want = O.rigid_ml_series(solved, src, cov, rigid, residual, sc, 8)
            O.check(tuple(res[w].cpu().numpy() for w in WANT), want, f"the pipeline, source {source!r}")
            ml = want[0]
            assert (ml[:, 0] == 2.0).all() and ml[5, 1] == 64.0
            sr, sc3 = RG.pose_sigma(ml, want[1])
            assert np.array_equal(res["sigma_rot_deg"], sr) and np.array_equal(res["sigma_centre"], sc3)
            other = np.arange(F) != (-1 if source == "layout" else 0 if source == "start" else source)
            assert np.array_equal(res["consistent"], RG.consistent(ml, 3.0)) and RG.consistent(ml, 5.0)[other].all()
            if source != "layout":
                # the source frame against itself: what is left is the rounding of (Q - qm) + qm, an ulp of 20 mm = 3.6e-15 mm
                # against a sigma of 1e-3 mm and more - chi^2 below 195 x (3.6e-12)^2 = 2.5e-21 - and that is NOT consistent
                assert ml[~other, 26] < 1e-20 and not res["consistent"][~other].any()
            assert np.array_equal(res["significant"], ml[:, 38] > 9.0)
            # the tilt is found within 5 of its own sigmas, and the last frames are told from an untilted body
            if source != 3:
                assert (np.abs(res["tilt_deg"] - tilt) < 5.0 * np.maximum(sr[:, 0], sr[:, 1]) + 1e-3).all()
            assert res["significant"][-3:].all()
            assert res["worst_frames"].shape == (5,) and res["worst_slots"].shape == (5,) and res["trend"].shape == (F, 8)
            df = P.to_rigid_uncertainty_frame(res, frame_offset=100, path=tmp_path / "ml.csv")
            assert tuple(df.columns) == P.RIGID_UNCERTAINTY_COLUMNS + P.RIGID_TREND_COLUMNS and len(df) == F
            assert df["frameno"].tolist() == list(range(100, 100 + F)) and df["flag"].dtype == np.int64
            dml = res["ml"].cpu().numpy()                         # (the device's own, just held to the restatement: col 32 to 4 ulp)
            assert np.array_equal(df["tilt_deg"].to_numpy(), dml[:, 32]) and df["significant"].dtype == bool
            back = pd.read_csv(tmp_path / "ml.csv", float_precision="round_trip")
            for name in df.columns:
                assert np.array_equal(back[name].to_numpy(), df[name].to_numpy(), equal_nan=True), name
    finally:
        e.close()
