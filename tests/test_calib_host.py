"""Intrinsic calibration (row f9), the parts that need no GPU: the helper `tests/helpers/calib_oracle.py` is held to the
independent scipy optimum and to the generated truth BEFORE the device is held to the helper; the export and every argument check
of `vbs_calibrate_camera`; `rodrigues`; the Python entries on a monkey-patched engine function."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import calib_oracle as O                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return O.cases()


def test_yardstick_is_sound(cases):
    """Every regular case: scipy converges, its column-scaled Jacobian is conditioned below 1e4, and the helper's LM reaches its
    cost to a relative 1e-9 and its reprojection to 1e-6 px.  k2 and k3 are NOT compared with the truth anywhere: a 6 x 6 board
    leaves them weakly determined (k3 between -0.43 and 2.8 for a true 0.01 at 0.1 px of noise, at a cost at the noise level)."""
    assert [c["name"] for c in cases] == [n for n, *_ in O.CASES] and len(cases) == 7
    assert [(len(c["imgs"]), len(c["obj"])) for c in cases] == [(3, 36), (3, 36), (5, 36), (8, 28), (4, 65), (3, 256), (64, 12)]
    for c in cases:
        s, o = c["sol"], c["opt"]
        assert s["status"] == 0 and o["success"], c["name"]
        rel = abs(s["cost"] - o["cost"]) / o["cost"]
        gap = O.reprojection_gap(s["cam"], s["R"], s["t"], o["cam"], o["R"], o["t"], c["obj"])
        print(f"{c['name']:16s} iterations {s['iterations']:2d} cond {o['cond']:6.0f} cost rel {rel:.2e} reprojection {gap:.2e} px "
              f"K {np.abs(s['cam'][:4] - o['cam'][:4]).max():.2e} px k1 {abs(s['cam'][4] - o['cam'][4]):.2e} rms {s['rms']:.4f}")
        assert o["cond"] < 1e4
        assert rel <= 1e-9 and gap <= 1e-6
        assert 1 <= s["iterations"] <= 30
        # the noise shows in the rms: sigma sqrt(dof / (2 points)) within a factor 2 either way
        if c["noise"]:
            assert 0.5 * c["noise"] <= s["rms"] <= 2.0 * c["noise"]
        assert np.abs(s["std_intrinsics"] / o["std_intrinsics"] - 1.0).max() <= 1e-5
        # the closed form starts within 5 % of the true focal lengths (cv2's own standing: recalled, not verified)
        assert np.abs(s["init"]["cam"][:2] / c["cam"][:2] - 1.0).max() <= 0.05


def test_noise_free_case_recovers_truth(cases):
    c = cases[0]
    gap = np.abs(c["sol"]["cam"][:4] - c["cam"][:4]).max()
    print(f"fx fy cx cy vs truth: {gap:.2e} px (the float32 rounding of the corners)")
    assert gap <= 1e-3
    for R, t, Rt, tt in zip(c["sol"]["R"], c["sol"]["t"], c["R"], c["t"]):
        assert O.rotation_angle_deg(R, Rt) <= 1e-4 and np.abs(t - tt).max() <= 1e-4


def test_degenerate_inputs(cases):
    c = cases[2]
    assert O.solve(c["obj"], c["imgs"], c["size"], active=[0, 1])["status"] == O.FEW_VIEWS
    line = O.collinear_view(c)
    assert O.homography(c["obj"], line)[1] is False
    imgs = np.concatenate([c["imgs"], line[None]])
    assert O.solve(c["obj"], imgs, c["size"], active=[1, 2, 3, 5])["status"] == O.DEGENERATE
    assert O.solve(c["obj"], imgs, c["size"], active=[0, 2, 3, 4])["status"] == 0
    assert O.solve(c["obj"], O.fronto_parallel_views(c), c["size"])["status"] == O.DEGENERATE


def test_masked_helper_equals_the_views_alone(cases):
    c = cases[3]
    a = O.solve(c["obj"], c["imgs"], c["size"], active=[0, 2, 3, 5, 7])
    b = O.solve(c["obj"], c["imgs"][[0, 2, 3, 5, 7]], c["size"])
    assert a["cam"].tobytes() == b["cam"].tobytes() and a["iterations"] == b["iterations"]


def test_entry_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    assert re.search(r"\bint\s+vbs_calibrate_camera\s*\(", hdr)
    assert "intrinsic_calibration.py:97-98" in hdr
    assert "vbs_calibrate_camera" in L.SYMBOLS
    assert hasattr(C.CDLL(L.LIB_PATH), "vbs_calibrate_camera")
    assert (L.CALIB_MAX_VIEWS, L.CALIB_FEW_VIEWS, L.CALIB_DEGENERATE) == tuple(
        int(re.search(rf"#define\s+VBS_CALIB_{k}\s+(\d+)", hdr).group(1)) for k in ("MAX_VIEWS", "FEW_VIEWS", "DEGENERATE"))
    assert (O.FEW_VIEWS, O.DEGENERATE) == (L.CALIB_FEW_VIEWS, L.CALIB_DEGENERATE)
    src = open(os.path.join(ROOT, "vision-basedsensor_amd", "_build.py")).read()
    assert '"k_calib.hip"' in src


def test_entry_rejects_bad_arguments():
    one = C.c_void_p(8)                                       # never dereferenced: the argument checks come first
    #       device obj n   img views mask problems w h iter, 11 outputs, stream
    args = [0, one, 36, one, 5, None, 1, 640, 480, 30] + [one] * 11 + [None]
    fn = L.lib().vbs_calibrate_camera
    bad = [(1, None), (3, None), (2, 3), (4, 0), (6, 0), (7, 0), (8, 0), (9, 0)] + [(k, None) for k in range(10, 21)]
    for at, value in bad:
        a = list(args)
        a[at] = value
        assert fn(*a) == L.VBS_EINVAL, (at, value)
    for at, value in ((4, L.CALIB_MAX_VIEWS + 1), (2, L.CHESS_MAX_PATTERN + 1)):
        a = list(args)
        a[at] = value
        assert fn(*a) == L.VBS_ECAPACITY, (at, value)


def test_rodrigues_round_trip():
    from vbs_amd.intrinsic_calibration import rodrigues
    rng = np.random.default_rng(11)
    for w in list(rng.normal(0, 1.0, (20, 3))) + [np.zeros(3), np.array([1e-10, 0, 0]), np.array([np.pi - 1e-9, 0, 0]),
                                                  np.array([0, np.pi, 0]), np.array([2.0, -2.0, 1.0]) * (np.pi / 3.0)]:
        th = np.linalg.norm(w)
        if th > np.pi:
            w = w * ((th - 2 * np.pi) / th)
        r = rodrigues(O.rodrigues(w))
        assert r.shape == (3, 1) and r.dtype == np.float64
        assert np.abs(O.rodrigues(r.ravel()) - O.rodrigues(w)).max() < 1e-9, w


def fake_result(v=4, status=0):
    import torch
    R = np.stack([O.rodrigues([0.1 * k, -0.2, 0.05 * k]) for k in range(v)])
    return {"status": torch.tensor([status], dtype=torch.int32), "K4": torch.tensor([[800.0, 790.0, 320.5, 240.25]], dtype=torch.float64),
            "dist": torch.tensor([[-0.1, 0.02, 0.001, -0.002, 0.003]], dtype=torch.float64), "R": torch.from_numpy(R)[None],
            "T": torch.arange(3.0 * v, dtype=torch.float64).reshape(1, v, 3), "rms": torch.tensor([0.125], dtype=torch.float64),
            "view_rms": torch.full((1, v), 0.125, dtype=torch.float64), "std_intrinsics": torch.ones((1, 9), dtype=torch.float64),
            "iterations": torch.tensor([12], dtype=torch.int32), "homography": torch.zeros((v, 3, 3), dtype=torch.float64),
            "view_void": torch.zeros((v,), dtype=torch.int32)}


def test_calibrate_points_layout(monkeypatch):
    import vbs_amd.engine as E
    import vbs_amd.intrinsic_calibration as IC
    seen = {}

    def fake(obj_points, img_points, img_size, view_mask=None, max_iter=30, device=None):
        seen.update(obj=obj_points, img=img_points, size=img_size, mask=view_mask)
        return fake_result(len(img_points))
    monkeypatch.setattr(E, "calibrate_camera_points", fake)
    ret, mtx, dist, rvecs, tvecs = IC.calibrate_points(["o"] * 4, ["i"] * 4, (640, 480))
    assert seen["size"] == (640, 480) and seen["mask"] is None
    assert ret == 0.125 and isinstance(ret, float)
    assert mtx.dtype == np.float64 and np.array_equal(mtx, [[800.0, 0, 320.5], [0, 790.0, 240.25], [0, 0, 1]])
    assert dist.shape == (1, 5) and dist[0, 4] == 0.003
    assert isinstance(rvecs, tuple) and isinstance(tvecs, tuple) and len(rvecs) == len(tvecs) == 4
    assert all(r.shape == (3, 1) for r in rvecs) and np.array_equal(tvecs[1].ravel(), [3.0, 4.0, 5.0])
    assert np.allclose(rvecs[2].ravel(), [0.2, -0.2, 0.1], atol=1e-12)
    monkeypatch.setattr(E, "calibrate_camera_points", lambda *a, **k: fake_result(4, status=L.CALIB_DEGENERATE))
    with pytest.raises(L.VbsError, match="VBS_CALIB_DEGENERATE"):
        IC.calibrate_points(["o"] * 4, ["i"] * 4, (640, 480))


def test_calibrate_camera_default_refuses_and_device_finishes(monkeypatch, capsys):
    import vbs_amd.engine as E
    import vbs_amd.intrinsic_calibration as IC
    collected = (["obj"] * 4, ["img0", "img1", "img2", "img3"], ["a.png", "b.png", "c.png", "d.png"], (203, 157))
    monkeypatch.setattr(IC, "collect_corners", lambda d, p, s: collected)
    with pytest.raises(NotImplementedError, match="calibrateCamera"):
        IC.calibrate_camera("somewhere", (6, 6), 3.0)
    seen = {}

    def fake(obj_points, img_points, img_size, view_mask=None, max_iter=30, device=None):
        seen.update(obj=obj_points, img=img_points, size=img_size)
        return fake_result(4)
    monkeypatch.setattr(E, "calibrate_camera_points", fake)
    res = IC.calibrate_camera("somewhere", (6, 6), 3.0, calibrate="device")
    assert (seen["obj"], seen["img"], seen["size"]) == (collected[0], collected[1], collected[3])
    assert list(res) == ["mtx", "dist", "error", "obj_points", "img_points", "rvecs", "tvecs", "valid_imgs"]
    assert res["dist"].shape == (5,) and res["error"] == 0.125 and res["valid_imgs"] == collected[2]
    assert res["obj_points"] is collected[0] and res["img_points"] is collected[1]
    assert "Processing images in: somewhere" in capsys.readouterr().out
    monkeypatch.setattr(IC, "collect_corners", lambda d, p, s: (["obj"] * 2, ["i"] * 2, ["a", "b"], (203, 157)))
    assert IC.calibrate_camera("somewhere", (6, 6), 3.0, calibrate="device") is None
    with pytest.raises(ValueError):
        IC.calibrate_camera("somewhere", (6, 6), 3.0, calibrate="cv2")


def test_jackknife_standard_error(monkeypatch):
    import torch
    import vbs_amd.engine as E
    import vbs_amd.intrinsic_calibration as IC

    def fake(obj_points, img_points, img_size, view_mask=None, max_iter=30, device=None):
        m = np.asarray(view_mask)
        assert m.shape == (5, 4) and m[0].all() and all(m[k + 1].sum() == 3 and m[k + 1, k] == 0 for k in range(4))
        r = fake_result(4)
        b = m.shape[0]
        out = {k: (v if k in ("homography", "view_void") else v.repeat(b, *([1] * (v.dim() - 1)))) for k, v in r.items()}
        out["K4"] = out["K4"] + torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0], dtype=torch.float64)[:, None]
        out["status"][3] = L.CALIB_DEGENERATE
        return out
    monkeypatch.setattr(E, "calibrate_camera_points", fake)
    res = IC.jackknife(["o"] * 4, ["i"] * 4, (640, 480))
    assert res["K4"].tolist() == [800.0, 790.0, 320.5, 240.25] and list(res["loo_status"]) == [0, 0, L.CALIB_DEGENERATE, 0]
    want = np.sqrt(2.0 / 3.0 * ((np.array([1.0, 2.0, 4.0]) - 7.0 / 3.0) ** 2).sum())     # the failed fit is left out
    assert np.allclose(res["jackknife_se"][:4], want) and np.allclose(res["jackknife_se"][4:], 0.0)


def test_without_a_gpu_the_entries_raise(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from vbs_amd.engine import calibrate_camera_points
    from vbs_amd.intrinsic_calibration import calibrate_points, calibrate_subsets, jackknife
    c = O.make_case("tiny", 3, (4, 3), (0, 0, 0, 0, 0), 0.0, 1)
    args = ([c["objp"]] * 3, list(c["imgs"]), c["size"])
    for fn in (calibrate_camera_points, calibrate_points, jackknife):
        with pytest.raises(L.VbsError):
            fn(*args)
    with pytest.raises(L.VbsError):
        calibrate_subsets(*args, np.ones((1, 3)))


def test_package_does_not_import_the_helper():
    pkg = os.path.join(ROOT, "vision-basedsensor_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "calib_oracle" not in open(os.path.join(dirpath, f)).read(), f


def test_shim_exports_the_new_names():
    sys.path.insert(0, os.path.join(ROOT, "vision-basedsensor_amd", "Marker_Calibration"))
    import importlib
    m = importlib.import_module("intrinsic_calibration")
    for name in ("calibrate_points", "calibrate_subsets", "jackknife", "rodrigues", "calibrate_camera"):
        assert callable(getattr(m, name))


def test_rendered_boards_record():
    """The end-to-end inputs of tests/test_gpu_calib.py through the HELPER chain on the CPU (finder, (11,11) refinement, this
    helper): prints the gap of fx, fy, cx, cy to the rendered K, which calib_oracle.E2E_HELPER_K_GAP_PX records."""
    import chess_oracle as CO
    imgs = []
    for gray, truth in O.rendered_boards():
        r = CO.find_chessboard_corners(gray, (6, 6), want=True)
        assert r["found"]
        sub, _ = CO.corner_subpix(gray, r["corners"])
        imgs.append(sub.astype(np.float32).astype(np.float64))
        assert np.abs(np.linalg.norm(sub - r["corners"], axis=1)).max() < 1.0
    sol = O.solve(O.board((6, 6))[:, :2].astype(np.float64), np.array(imgs), (203, 157))
    assert sol["status"] == 0
    gap = float(np.abs(sol["cam"][:4] - np.array(O.E2E_K)).max())
    print(f"helper chain: K {sol['cam'][:4]} vs rendered {O.E2E_K}: {gap:.4f} px, rms {sol['rms']:.4f}")
    assert gap <= O.E2E_HELPER_K_GAP_PX + 1e-4 and gap >= 0.5 * O.E2E_HELPER_K_GAP_PX      # the record is this run's figure
