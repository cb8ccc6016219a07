"""GPU tests of the intrinsic calibration (k_calib.hip; `pytest -m gpu` on an MI355X): the device against the helper
`tests/helpers/calib_oracle.py` - the same steps in NumPy - and against the independent scipy optimum, over the seven regular
cases (3 to 64 views, 12 to 256 corners), then bit-identity over runs, input forms, masks and batches, the failure statuses, the
caps, and `calibrate_camera(dir, ..., calibrate="device")` end to end on rendered boards.

k2 and k3 are not compared anywhere: a small board leaves them weakly determined (see the helper's host test)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import calib_oracle as O                                      # noqa: E402

# Bounds = 10 x the largest gap measured on an MI355X over the seven regular cases, against scipy's optimum (the device result is
# deterministic: the margin is for other seeds); DESIGN.md 4.10 repeats them.  Measured:
#   relative cost gap 2.847e-10, fx fy cx cy 1.981e-06 px, k1 7.407e-09, reprojection 4.357e-08 px, rotation 1.578e-07 degrees,
#   translation 1.966e-07 mm, view_rms 4.409e-09 px, std_intrinsics relative 3.346e-07.
# Against the helper every gap measured 0 (the cost, re-summed on the host by NumPy, 3.3e-16): it repeats the device operation for
# operation, and `test_iterations_equal_the_helpers` asks for equality.
COST_REL_BOUND = 2.847e-9     # (a bound above 1e-6 would mean the LM has not converged: a defect, not a tolerance)
K_PX_BOUND = 1.981e-5
K1_BOUND = 7.407e-8
REPROJ_PX_BOUND = 4.357e-7
ROT_DEG_BOUND = 1.578e-6
T_MM_BOUND = 1.966e-6
VIEW_RMS_BOUND = 4.409e-8
STD_REL_BOUND = 3.346e-6

KEYS = ("status", "K4", "dist", "R", "T", "rms", "view_rms", "std_intrinsics", "iterations")


def run(c, views=None, mask=None, device_input=False, imgs=None):
    from vbs_amd.engine import calibrate_camera_points
    img = c["imgs"] if imgs is None else imgs
    if views is not None:
        img = img[list(views)]
    if device_input:
        return calibrate_camera_points(torch.from_numpy(c["obj"]).cuda(), torch.from_numpy(img).cuda(), c["size"], view_mask=mask)
    return calibrate_camera_points([c["objp"]] * len(img), [v.astype(np.float32).reshape(-1, 1, 2) for v in img], c["size"],
                                   view_mask=mask)


def host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def same_bits(a, b, row_a=0, row_b=0, views_a=None, views_b=None):
    """Problem row_a of a against row_b of b; views_x = the view indices of x to compare, in matching order (default all)."""
    for k in KEYS:
        x, y = a[k][row_a], b[k][row_b]
        if k in ("R", "T", "view_rms"):
            x = x[list(views_a)] if views_a is not None else x
            y = y[list(views_b)] if views_b is not None else y
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def cases():
    return O.cases()


@pytest.fixture(scope="module")
def results(cases):
    out = [host(run(c)) for c in cases]
    return out


def gaps(c, r, ref):
    """The device's result r (row 0) against ref = the helper's `sol` or scipy's `opt`."""
    cam = np.concatenate([r["K4"][0], r["dist"][0]])
    Rs, ts = list(r["R"][0]), list(r["T"][0])
    cost = float(O.view_costs(cam, Rs, ts, c["obj"], c["imgs"]).sum())
    return dict(cost=abs(cost - ref["cost"]) / ref["cost"], K=float(np.abs(cam[:4] - ref["cam"][:4]).max()),
                k1=float(abs(cam[4] - ref["cam"][4])), reproj=O.reprojection_gap(cam, Rs, ts, ref["cam"], ref["R"], ref["t"], c["obj"]),
                rot=max(O.rotation_angle_deg(a, b) for a, b in zip(Rs, ref["R"])),
                t=max(float(np.abs(a - b).max()) for a, b in zip(ts, ref["t"])),
                vrms=float(np.abs(r["view_rms"][0] - np.sqrt(np.asarray(ref["view_cost"]) / len(c["obj"]))).max()),
                std=float(np.abs(r["std_intrinsics"][0] / ref["std_intrinsics"] - 1.0).max()))


def test_regular_cases_against_helper_and_scipy(cases, results):
    worst = {"helper": {}, "scipy": {}}
    for c, r in zip(cases, results):
        assert r["status"][0] == L.VBS_OK, c["name"]
        assert not r["view_void"].any() and np.isfinite(r["homography"]).all()
        for who, ref in (("helper", c["sol"]), ("scipy", c["opt"])):
            g = gaps(c, r, ref)
            print(f"{c['name']:16s} vs {who:6s}: " + " ".join(f"{k}={v:.3e}" for k, v in g.items()))
            for k, v in g.items():
                worst[who][k] = max(worst[who].get(k, 0.0), v)
        # rms is that of the RETURNED parameters, recomputed on the host
        cam = np.concatenate([r["K4"][0], r["dist"][0]])
        vc = O.view_costs(cam, list(r["R"][0]), list(r["T"][0]), c["obj"], c["imgs"])
        assert abs(r["rms"][0] - np.sqrt(vc.sum() / c["imgs"][..., 0].size)) <= 1e-12, c["name"]
        for R in r["R"][0]:
            assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    for who in worst:
        print(f"worst vs {who}: " + " ".join(f"{k}={v:.3e}" for k, v in worst[who].items()))
    for who in worst:
        w = worst[who]
        assert w["cost"] <= COST_REL_BOUND
        assert w["K"] <= K_PX_BOUND and w["k1"] <= K1_BOUND and w["reproj"] <= REPROJ_PX_BOUND
        assert w["rot"] <= ROT_DEG_BOUND and w["t"] <= T_MM_BOUND
        assert w["vrms"] <= VIEW_RMS_BOUND and w["std"] <= STD_REL_BOUND


def test_iterations_equal_the_helpers(cases, results):
    """`iterations` equal to the helper's.  Once both sit at the optimum to rounding, the decisions cost_t <= cost_c and
    max |step| < 1e-11 hang on the last bits, so equal counts need equal bits all the way: the helper sums per lane and through
    the butterfly as the kernel does, and neither calls sin / cos (calib_apply_step).  Measured on an MI355X (device = helper):
    12, 24, 22, 30, 30, 20, 21 - and the intrinsics, poses and std_intrinsics come out bit for bit."""
    iters = [(c["name"], int(r["iterations"][0]), c["sol"]["iterations"]) for c, r in zip(cases, results)]
    print("iterations (device, helper): " + ", ".join(f"{n} {a} {b}" for n, a, b in iters))
    assert all(a == b for _, a, b in iters), iters
    for c, r in zip(cases, results):
        s = c["sol"]
        assert np.concatenate([r["K4"][0], r["dist"][0]]).tobytes() == s["cam"].tobytes(), c["name"]
        assert r["R"][0].tobytes() == np.array(s["R"]).tobytes() and r["T"][0].tobytes() == np.array(s["t"]).tobytes(), c["name"]
        assert r["std_intrinsics"][0].tobytes() == s["std_intrinsics"].tobytes() and r["rms"][0] == s["rms"], c["name"]


def test_homographies_against_helper(cases, results):
    worst = 0.0
    for c, r in zip(cases, results):
        for v in range(len(c["imgs"])):
            H, ok = O.homography(c["obj"], c["imgs"][v])
            assert ok
            worst = max(worst, float(np.abs(r["homography"][v].reshape(9) / H - 1.0).max()))
    print(f"homography entries, relative to the helper's: {worst:.3e}")
    assert worst <= 1e-9      # (measured 0: the helper repeats the kernel's sums in their order)


def test_runs_and_input_forms_are_bit_identical(cases, results):
    for c, r in zip(cases[:4], results[:4]):
        same_bits(host(run(c)), r)
        same_bits(host(run(c, device_input=True)), r)


def test_jackknife_rows(cases, results):
    """Row 0 of the jackknife batch is the all-views problem alone; row k + 1 is the call without view k (V = 5): the sums over
    the active views run in the order of the active list, whatever the mask around it."""
    c, r = cases[2], results[2]
    v = len(c["imgs"])
    assert v == 5
    mask = np.ones((v + 1, v), dtype=np.uint8)
    mask[np.arange(1, v + 1), np.arange(v)] = 0
    jk = host(run(c, mask=mask))
    assert (jk["status"] == L.VBS_OK).all()
    same_bits(jk, r)
    for k in range(v):
        rest = [i for i in range(v) if i != k]
        same_bits(jk, host(run(c, views=rest)), k + 1, 0, views_a=rest)
        assert np.isnan(jk["R"][k + 1, k]).all() and np.isnan(jk["T"][k + 1, k]).all() and np.isnan(jk["view_rms"][k + 1, k])
    from vbs_amd.intrinsic_calibration import jackknife
    res = jackknife([c["objp"]] * v, [i.astype(np.float32).reshape(-1, 1, 2) for i in c["imgs"]], c["size"])
    assert res["K4"].tobytes() == r["K4"][0].tobytes() and res["jackknife_se"].shape == (9,) and (res["jackknife_se"] > 0).all()
    print("std_intrinsics", res["std_intrinsics"], "jackknife", res["jackknife_se"])


def test_masked_problem_equals_the_views_alone(cases):
    c = cases[3]                                                # 8 views
    subsets = ([0, 2, 3, 5, 7], [1, 2, 3], [0, 1, 2, 3, 4, 5, 6], [4, 5, 6, 7])
    mask = np.zeros((len(subsets), 8), dtype=np.uint8)
    for b, s in enumerate(subsets):
        mask[b, s] = 1
    batch = host(run(c, mask=mask))
    for b, s in enumerate(subsets):
        assert batch["status"][b] == L.VBS_OK
        same_bits(batch, host(run(c, views=s)), b, 0, views_a=s)


def test_statuses_and_failed_neighbours(cases, results):
    c = cases[2]
    imgs = np.concatenate([c["imgs"], O.collinear_view(c)[None]])          # view 5 is the line
    mask = np.array([[1, 1, 1, 1, 1, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 0, 1], [1, 0, 1, 1, 1, 0]], dtype=np.uint8)
    r = host(run(c, mask=mask, imgs=imgs))
    assert list(r["view_void"]) == [0, 0, 0, 0, 0, 1] and np.isnan(r["homography"][5]).all()
    assert list(r["status"]) == [L.VBS_OK, L.CALIB_FEW_VIEWS, L.CALIB_DEGENERATE, L.CALIB_DEGENERATE, L.VBS_OK]
    for b in (1, 2, 3):
        for k in ("K4", "dist", "R", "T", "rms", "view_rms", "std_intrinsics"):
            assert np.isnan(r[k][b]).all(), (b, k)
    same_bits(r, results[2], 0, 0, views_a=range(5))
    same_bits(r, host(run(c, views=[0, 2, 3, 4])), 4, 0, views_a=[0, 2, 3, 4])
    fp = host(run(c, imgs=O.fronto_parallel_views(c)))
    assert fp["status"][0] == L.CALIB_DEGENERATE and np.isnan(fp["K4"]).all()
    from vbs_amd.intrinsic_calibration import calibrate_points
    with pytest.raises(L.VbsError, match="fewer than 3 views"):
        calibrate_points([c["objp"]] * 2, list(c["imgs"][:2]), c["size"])


def test_capacity(cases):
    from vbs_amd.engine import calibrate_camera_points
    c = cases[6]
    with pytest.raises(L.VbsError, match="VBS_CALIB_MAX_VIEWS"):
        calibrate_camera_points(c["obj"], np.concatenate([c["imgs"], c["imgs"][:1]]), c["size"])
    with pytest.raises(L.VbsError, match="VBS_CHESS_MAX_PATTERN"):
        calibrate_camera_points(np.zeros((257, 2)), np.zeros((3, 257, 2)), c["size"])


def test_calibrate_points_layout(cases, results):
    from vbs_amd.intrinsic_calibration import calibrate_points, rodrigues
    c, r = cases[1], results[1]
    ret, mtx, dist, rvecs, tvecs = calibrate_points([c["objp"]] * 3, [i.astype(np.float32).reshape(-1, 1, 2) for i in c["imgs"]], c["size"])
    assert ret == r["rms"][0] and mtx.shape == (3, 3) and mtx.dtype == np.float64 and dist.shape == (1, 5)
    assert (mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2]) == tuple(r["K4"][0]) and mtx[0, 1] == 0 and mtx[2, 2] == 1
    assert len(rvecs) == len(tvecs) == 3 and rvecs[0].shape == tvecs[0].shape == (3, 1)
    for k in range(3):
        assert np.abs(O.rodrigues(rvecs[k].ravel()) - r["R"][0][k]).max() < 1e-12


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_calibrate_camera_end_to_end(tmp_path):
    from PIL import Image
    from vbs_amd.intrinsic_calibration import calibrate_camera, crop_image, save_calib_results
    from vbs_amd.extrinsic_calibration import load_intrinsics_from_excel
    for k, (gray, _) in enumerate(O.rendered_boards()):
        big = O.padded(gray)
        assert np.array_equal(crop_image(big), gray)
        Image.fromarray(np.stack([big] * 3, axis=2)).save(tmp_path / f"board_{k}.png")
    res = calibrate_camera(str(tmp_path), (6, 6), 3.0, calibrate="device")
    assert sorted(res) == sorted(["mtx", "dist", "error", "obj_points", "img_points", "rvecs", "tvecs", "valid_imgs"])
    assert len(res["valid_imgs"]) == 4 and res["dist"].shape == (5,) and len(res["rvecs"]) == 4
    obj = res["obj_points"][0][:, :2].astype(np.float64)
    imgs = np.array([p.reshape(-1, 2).astype(np.float64) for p in res["img_points"]])
    sol = O.solve(obj, imgs, (203, 157))
    assert sol["status"] == 0
    got = np.array([res["mtx"][0, 0], res["mtx"][1, 1], res["mtx"][0, 2], res["mtx"][1, 2]])
    print(f"device K {got}, helper on the same corners {sol['cam'][:4]}, rendered {O.E2E_K}; error {res['error']!r} vs {sol['rms']!r}")
    assert np.abs(got - sol["cam"][:4]).max() <= K_PX_BOUND and abs(res["error"] - sol["rms"]) <= VIEW_RMS_BOUND
    gap = float(np.abs(got - np.array(O.E2E_K)).max())
    print(f"fx fy cx cy vs rendered: {gap:.4f} px (helper chain on the CPU: {O.E2E_HELPER_K_GAP_PX})")
    assert gap <= 2 * O.E2E_HELPER_K_GAP_PX
    save_calib_results(res["mtx"], res["dist"], res["error"], str(tmp_path / "out" / "IntrinsicParameters.xlsx"))
    K, dist = load_intrinsics_from_excel(str(tmp_path / "out" / "IntrinsicParameters.xlsx"))
    assert np.array_equal(K, res["mtx"].astype(np.float32)) and np.array_equal(np.ravel(dist), res["dist"].astype(np.float32))
