"""GPU tests of the uncertainty of the pose misalignment (`vbs_pose_cov`) against the NumPy restatement
`tests/helpers/posecov_oracle.py`: all 17 columns of `pcov` bit for bit, nothing masked.  Shapes are the smallest at which the
kernel can go wrong - around a wave (64 slots), around the frames a workgroup takes (VBS_POSECOV_GROUP), every count of camera
columns that takes another path (none, one, some, all 16) - not the workload's; the tables hold rows without a 3-D point, rows
below the size gate that carry the flag, frames with too few common slots, planted outliers for the rejection, and NaN / 1e30 in
every cell that must not be read."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import vbs_amd._lib as L                                       # noqa: E402
from vbs_amd import engine as E                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pose_oracle as PO                                       # noqa: E402
import posecov_cases as PC                                     # noqa: E402
import posecov_oracle as O                                     # noqa: E402
import uncert_cases as UC                                      # noqa: E402
import uncert_oracle as U                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.POSECOV_GROUP
#        m,   n,         q,  obs,    rows,  mode,    scale, reject_k, outliers, mask
CASES = [(3,   1,         0,  "one",  False, "plane", 1.0,  0.0, 0, False),
         (4,   G,         1,  "slot", True,  "shell", 25.0, 3.0, 0, False),
         (63,  G + 1,     5,  "one",  True,  "plane", 1.0,  3.0, 2, False),
         (64,  2 * G + 3, 16, "slot", False, "shell", 1.0,  0.0, 0, True),
         (65,  2 * G + 3, 16, "one",  True,  "plane", 25.0, 3.0, 2, False),
         (130, G + 1,     5,  "slot", True,  "shell", 25.0, 0.0, 0, True),
         (441, G,         1,  "one",  False, "plane", 1.0,  3.0, 3, True)]


def _cam(cam):
    return L.make_camera(*cam[:4], cam[4])


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(480, 640, max_markers=256, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """Every recording with its restatement, computed once."""
    out = {}
    for i, (m, n, q, form, rows, mode, scale, rk, outliers, mask) in enumerate(CASES):
        size = (640, 480) if i % 2 == 0 else (1920, 1200)
        cam = UC.camera(size, distorted=i % 3 != 1)
        extra = {}
        if m == 65:                                              # frames 4, 5, 6: 0, 1, 2 common slots; frame 7: a flagged row of 4 px
            extra = dict(sparse=((4, 0), (5, 1), (6, 2)), small=((7, 40),))
        k = PC.recording(cam, n, m, size, seed=i, drop=0.0 if m < 10 else 0.08, outliers=outliers, **extra)
        slots = np.flatnonzero(np.random.default_rng(i).random(m) < 0.8) if mask else None
        sel = None if slots is None else np.isin(np.arange(m), slots)
        k.update(cam=cam, obs=PC.obs_cov(form, m, i), L=UC.factor(q, i), rows=k["ref_rows"] if rows else None, mode=mode, scale=scale,
                 rk=rk, slots=slots, n=n, m=m)
        k["want"] = O.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], U.Cam(*cam), k["obs"], k["L"], k["rows"], k["start"], sel,
                               mode == "shell", scale, rk)
        out[m] = k
    return out


def _run(k, **over):
    a = dict(table=k["table"], ref_disp=k["ref_disp"], ref_xyz=k["ref_xyz"], cam=_cam(k["cam"]), obs_cov=k["obs"], cam_factor=k["L"],
             ref_rows=k["rows"], start_frame=k["start"], mode=k["mode"], scale=k["scale"], slots=k["slots"], reject_k=k["rk"])
    a.update(over)
    pose, pcov = E.pose_cov(**a)
    return (None if pose is None else pose.cpu().numpy()), (None if pcov is None else pcov.cpu().numpy())


@pytest.mark.parametrize("m", [c[0] for c in CASES])
def test_pcov_equals_the_restatement_bit_for_bit(cases, m):
    k = cases[m]
    pose, pcov = _run(k)
    wpose, wpcov = k["want"]
    O.check_pcov(pcov, wpcov, f"m = {m}")
    assert np.array_equal(pose[:, [0, 1, 2, 3, 7]], wpose[:, [0, 1, 2, 3, 7]])
    flag = wpcov[:, 0].astype(np.int64)
    assert ((flag & 1) != 0).any(), "no frame of the case has a covariance"
    bad = (flag & 1) == 0
    assert (wpcov[bad][:, 2:] == 0.0).all() and (wpcov[bad][:, 0] == 0.0).all()
    if k["rk"] > 0.0 and m >= 63:
        assert (wpose[:, 0] == 2.0).any(), "the planted outliers were not rejected in any frame"
    if m == 65:
        assert wpose[4:7, 7].tolist() == [0.0, 1.0, 2.0] and (wpose[4:7, 0] == 0.0).all() and (wpcov[4:7, 0] == 0.0).all()
        assert wpcov[7, 1] >= 1.0 and wpcov[7, 0] == 0.0 and wpose[7, 0] != 0.0
    # only pcov, only pose
    _, only = _run(k, want=("pcov",))
    O.check_pcov(only, wpcov, f"m = {m}, pcov alone")
    alone, none = _run(k, want=("pose",))
    assert none is None and np.array_equal(alone, pose)


@pytest.mark.parametrize("masked", [False, True])
def test_every_exit_of_the_rejection_round(masked):
    """Five frames (one workgroup and a partial one) of 7 slots, 8 under a slot mask, whose frame f leaves the rejection round by
    `posecov_cases.EXIT_FRAMES[f]`: no round (SSR = 0), rejected and refitted (flag 2), nothing rejected, fewer than 3 kept, kept
    set degenerate (its det fails); the case maker asserts that from the restatement (`tests/test_posecov_host.py` runs it on the
    CPU).  Of these the cases m = 63, 65 and 441 above already reach "refitted" (asserted there) and, without naming them, "no
    round" in their start frames; the other three were pinned nowhere.  `pose` and `pcov` are held to the restatement as above:
    flag, a, b, c, n_used and all of pcov bit for bit, the three columns that end in atan / atan2 / sqrt to 4 ulp."""
    cam = UC.camera((640, 480), distorted=True)
    k = PC.exit_recording(cam, masked)
    obs, fac = PC.obs_cov("one", 7), UC.factor(5, 2)
    sel = None if k["slots"] is None else np.isin(np.arange(k["table"].shape[1]), k["slots"])
    wpose, wpcov = O.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], U.Cam(*cam), obs, fac, k["ref_rows"], k["start"], sel, False, 1.0,
                              PC.EXIT_RK)
    assert wpose[:, 0].tolist() == [1.0, 2.0, 1.0, 1.0, 1.0] and ((wpcov[:, 0].astype(np.int64) & 1) != 0).all()
    pose, pcov = E.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], _cam(cam), obs, fac, k["ref_rows"], k["start"], "plane", 1.0,
                            k["slots"], PC.EXIT_RK)
    pose, pcov = pose.cpu().numpy(), pcov.cpu().numpy()
    O.check_pcov(pcov, wpcov, f"exits, masked = {masked}")
    exact = [0, 1, 2, 3, 7]
    assert np.array_equal(pose[:, exact].view(np.uint64), np.ascontiguousarray(wpose[:, exact]).view(np.uint64))
    for col in (4, 5, 6):
        assert (PO.ulps(pose[:, col], wpose[:, col]) <= 4).all(), col


@pytest.mark.parametrize("m", [65, 441])
def test_pose_output_equals_pose_series(cases, eng, m):
    k = cases[m]
    pose, _ = _run(k)
    _, _, want = eng.pose_series(torch.from_numpy(k["table"]).cuda(), k["ref_disp"], k["ref_xyz"], k["start"], k["mode"], k["scale"],
                                 k["slots"], k["rk"])
    want = want.cpu().numpy()
    exact = [0, 1, 2, 3, 7]
    assert np.array_equal(pose[:, exact].view(np.uint64), np.ascontiguousarray(want[:, exact]).view(np.uint64))
    for col in (4, 5, 6):
        assert (PO.ulps(pose[:, col], want[:, col]) <= 4).all(), col


@pytest.mark.parametrize("m", [65, 130])
def test_frame_ranges_equal_the_rows_of_the_full_call(cases, m):
    k = cases[m]
    pose, pcov = _run(k)
    n = k["n"]
    for a, b in ((0, 1), (1, G + 1), (G - 1, n), (n - 1, n), (2, 2)):
        rp, rc = _run(k, frame_range=(a, b))
        assert rp.shape == (b - a, 8) and rc.shape == (b - a, 17)
        assert np.array_equal(rc.view(np.uint64), pcov[a:b].view(np.uint64))
        assert np.array_equal(rp.view(np.uint64), pose[a:b].view(np.uint64))


def test_flat_frames_collinear_positions_and_an_exact_zero_tilt():
    """Frames whose deviation is exactly zero: on a grid of reference positions the plane is a = b = 0 exactly (bit 4 clear, the
    angle variances 0, t2 = 0 and valid); on exactly collinear positions there is no plane (flag 0, zeros)."""
    cam = UC.camera((640, 480), distorted=True)
    k = PC.recording(cam, 4, 65, seed=21, drop=0.05, flat=(0, 3))
    obs, fac, c = PC.obs_cov("one", 65), UC.factor(5, 1), U.Cam(*cam)
    pose, pcov = E.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], _cam(cam), obs, fac, k["ref_rows"], k["start"])
    wpose, wpcov = O.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], c, obs, fac, k["ref_rows"], k["start"])
    O.check_pcov(pcov.cpu().numpy(), wpcov, "flat")
    for f in (0, 3):
        assert wpose[f, 0] == 1.0 and wpose[f, 1] == 0.0 and wpose[f, 2] == 0.0
        assert wpcov[f, 0] == 3.0 and wpcov[f, 2] > 0.0 and (wpcov[f, 14:] == 0.0).all()
    assert wpcov[2, 0] == 7.0
    line = np.stack([np.arange(65) * 0.5, np.full(65, 1.25), np.zeros(65)], axis=1)
    pose, pcov = E.pose_cov(k["table"], k["ref_disp"], line, _cam(cam), obs, fac, k["ref_rows"], k["start"])
    wpose, wpcov = O.pose_cov(k["table"], k["ref_disp"], line, c, obs, fac, k["ref_rows"], k["start"])
    O.check_pcov(pcov.cpu().numpy(), wpcov, "collinear")
    assert np.array_equal(pose.cpu().numpy()[:, [0, 1, 2, 3, 7]], wpose[:, [0, 1, 2, 3, 7]])
    for f in (0, 3):
        assert wpose[f, 0] == 0.0 and wpose[f, 7] >= 3.0 and (wpcov[f, [0] + list(range(2, 17))] == 0.0).all()


def test_refusals_leave_the_outputs_untouched(cases):
    k = cases[4]
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m = k["n"], 4
    t = torch.from_numpy(k["table"]).to(dev)
    rd, rx = torch.from_numpy(k["ref_disp"]).to(dev), torch.from_numpy(k["ref_xyz"]).to(dev)
    rr = torch.from_numpy(k["ref_rows"]).to(dev)
    obs = np.ascontiguousarray(k["obs"], dtype=np.float64)
    fac = np.ascontiguousarray(k["L"], dtype=np.float64)
    pose = torch.full((n, 8), -7.5, dtype=torch.float64, device=dev)
    pcov = torch.full((n, 17), -7.5, dtype=torch.float64, device=dev)
    work = torch.full((m * L.UNCERT_WORK_COLS,), -7.5, dtype=torch.float64, device=dev)
    cam = _cam(k["cam"])
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)       # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)   # noqa: E731
    good = dict(table=t, n=n, m=m, start=k["start"], rd=rd, rx=rx, shell=0, scale=1.0, rk=0.0, obs=obs, obs_rows=m, fac=fac, q=1,
                min_size=5.0, piv=1e-12, fb=0, fe=n, work=work, pose=pose, pcov=pcov)

    def call(**over):
        a = dict(good, **over)
        return L.lib().vbs_pose_cov(dev.index, p(a["table"]), a["n"], a["m"], a["start"], p(a["rd"]), p(a["rx"]), C.c_void_p(0), a["shell"],
                                    a["scale"], a["rk"], C.byref(cam), hp(a["obs"]), a["obs_rows"], hp(a["fac"]), a["q"], a["min_size"],
                                    a["piv"], p(rr), a["fb"], a["fe"], p(a["work"]), p(a["pose"]), p(a["pcov"]), C.c_void_p(0))

    bad_obs = obs.copy()
    bad_obs[1, 2] = np.nan
    for over in (dict(table=None), dict(rd=None), dict(rx=None), dict(obs=None), dict(work=None), dict(pose=None, pcov=None),
                 dict(n=0), dict(m=0), dict(start=-1), dict(start=n), dict(shell=2), dict(scale=float("inf")), dict(rk=-1.0),
                 dict(rk=float("nan")), dict(obs_rows=2), dict(obs=bad_obs), dict(q=17), dict(q=-1), dict(fac=None),
                 dict(min_size=float("nan")), dict(piv=-1.0), dict(piv=float("inf")), dict(fb=-1), dict(fe=n + 1), dict(fb=2, fe=1)):
        assert call(**over) == L.VBS_EINVAL, over
    torch.cuda.synchronize()
    assert (pose == -7.5).all() and (pcov == -7.5).all() and (work == -7.5).all()
    assert call() == L.VBS_OK
    torch.cuda.synchronize()
    O.check_pcov(pcov.cpu().numpy(), O.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], U.Cam(*k["cam"]), obs, fac, k["ref_rows"],
                                                k["start"])[1], "the direct call")
    with pytest.raises(ValueError):
        _run(k, start_frame=n)
    with pytest.raises(ValueError):
        _run(k, ref_rows=k["ref_rows"][:1])


def test_misalignment_uncertainty_on_a_tilt_ramp(eng, tmp_path):
    """65 markers; four untilted frames, then a ramp to 2 degrees.  The untilted frames are not significant at k = 3, the end of
    the ramp is, sigma_tilt is of the size the geometry gives (a tenth of a degree), and the sheet round-trips."""
    from vbs_amd import pipeline as P
    from vbs_amd.xlsx_io import read_xlsx
    cam = UC.camera((640, 480), distorted=True)
    ref = PO.grid_ref(65)
    tilt = np.concatenate([np.zeros(4), np.linspace(0.25, 2.0, 8)])
    tab, obs = PC.tilted_recording(cam, ref, tilt, seed=5)
    tab_ref, _ = PC.tilted_recording(cam, ref, np.zeros(2), seed=6)
    fac = UC.factor(1)
    res = P.misalignment_uncertainty(eng, torch.from_numpy(tab).cuda(), torch.from_numpy(tab_ref).cuda(), ref, _cam(cam), obs, fac)
    n = tilt.size
    wpose, wpcov = O.pose_cov(tab, np.concatenate([np.ones((65, 1)), tab_ref[1, :, 6:9].astype(np.float64) -
                                                   tab_ref[0, :, 6:9].astype(np.float64)], axis=1), ref, U.Cam(*cam), obs, fac, tab_ref)
    O.check_pcov(res["pcov"], wpcov, "the ramp")
    assert (res["flag"][1:] == 7).all() and (res["n_unusable"] == 0).all()
    assert not res["significant"][:4].any() and res["significant"][-3:].all()
    assert (res["sigma_tilt_deg"][1:] > 0.02).all() and (res["sigma_tilt_deg"][1:] < 0.5).all()
    assert np.array_equal(res["significant"], wpcov[:, 16] > 9.0)
    assert np.allclose(res["sigma_abc"][1:], np.sqrt(wpcov[1:, [2, 5, 7]]), rtol=0, atol=0)
    assert ((res["camera_share"][1:] >= 0.0) & (res["camera_share"][1:] <= 1.0)).all()
    assert (res["tilt_limit_deg"][1:] > 0.0).all() and (res["tilt_limit_deg"][1:] < 2.0).all()
    exact = P.misalignment_uncertainty(eng, torch.from_numpy(tab).cuda(), torch.from_numpy(tab_ref).cuda(), ref, _cam(cam), obs, fac,
                                       exact_reference=True)
    assert (exact["pcov"][1:, 2] < res["pcov"][1:, 2]).all()      # the reference session's noise is part of the budget
    path = tmp_path / "pose_uncertainty.xlsx"
    df = P.to_pose_uncertainty_frame(res, path=path)
    back = read_xlsx(path)
    assert tuple(back.columns) == P.POSE_UNCERTAINTY_COLUMNS and len(back) == n
    for col in df.columns:
        assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64), equal_nan=True), col
    assert np.array_equal(df["t2"].to_numpy(), res["t2"], equal_nan=True)
