"""Extrinsic calibration (row f7), the parts that need no GPU: the sequential helper against the generated truth, the export of
`vbs_pnp_ransac`, the sheet round trips, and the sample table."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

import vbs_amd._lib as L

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pnp_oracle as P                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batches():
    return P.all_batches()


def test_helper_recovers_truth(batches):
    """Every non-degenerate case: the winner holds exactly the true inliers and the scipy refit lands on the generated pose.
    Exact image points: to their float32 rounding, 3e-5 px, which at 30 px / mm and 40 mm is far inside 1e-4 degrees and
    1e-5 mm.  With sigma = 0.3 px of noise on n >= 47 inliers spread over r = 250 px / 8 mm (rms) at Z = 40 mm, the weakest
    directions are the tilt, seen only through perspective, sigma Z / (r_px r_mm sqrt n) = 0.05 degrees, and the depth,
    Z sigma / (r_px sqrt n) = 0.007 mm: the bounds are three of those standard deviations, 0.15 degrees and 0.02 mm.
    The degenerate problems report their failure."""
    seen = 0
    for b in batches:
        for p in b["problems"]:
            sol = p["sol"]
            if p["kind"] == "three":
                assert sol["status"] == P.FEW_POINTS and sol["winner"] == -1
                continue
            if p["kind"] == "collinear":
                assert sol["status"] == P.NO_HYPOTHESIS and (sol["count"] == -1).all()
                continue
            assert sol["status"] == 0 and np.array_equal(sol["mask"], p["true_inliers"])
            ref = P.refine(sol, b["world"], p["image"])
            ang, dt = P.rotation_angle_deg(ref["R"], p["R"]), float(np.abs(ref["t"] - p["t"]).max())
            print(f"{b['layout']} noise={p['noise']} inliers={int(sol['mask'].sum())}: {ang:.3e} deg, {dt:.3e} mm")
            if p["exact"]:
                assert ang < 1e-4 and dt < 1e-5
            else:
                assert ang < 0.15 and dt < 0.02
            seen += 1
    assert seen == 6 * 8


def test_pnp_entry_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    assert re.search(r"\bint\s+vbs_pnp_ransac\s*\(", hdr)
    assert "extrinsic_calibration.py:81-123" in hdr
    assert "vbs_pnp_ransac" in L.SYMBOLS
    assert hasattr(C.CDLL(L.LIB_PATH), "vbs_pnp_ransac")
    assert (L.PNP_SAMPLE, L.PNP_MAX_POINTS, L.PNP_MAX_HYPOTHESES, L.PNP_FEW_POINTS, L.PNP_NO_HYPOTHESIS) == tuple(
        int(re.search(rf"#define\s+VBS_PNP_{k}\s+(\d+)", hdr).group(1))
        for k in ("SAMPLE", "MAX_POINTS", "MAX_HYPOTHESES", "FEW_POINTS", "NO_HYPOTHESIS"))


def test_pnp_entry_rejects_bad_arguments():
    cam = L.make_camera(P.K_CASES, P.DIST_OFF, np.eye(3), np.zeros(3))
    one = C.c_void_p(8)                                       # never dereferenced: the argument check comes first
    args = [0, one, 65, one, None, None, 1, C.byref(cam), one, 1000, 8.0] + [one] * 8 + [None]
    fn = L.lib().vbs_pnp_ransac
    for at, bad in ((2, 0), (2, L.PNP_MAX_POINTS + 1), (9, 0), (9, L.PNP_MAX_HYPOTHESES + 1), (4, one), (3, None), (10, -1.0)):
        a = list(args)
        a[at] = bad
        assert fn(*a) == L.VBS_EINVAL, (at, bad)


def test_extrinsics_sheet_round_trip(tmp_path):
    from vbs_amd.extrinsic_calibration import save_extrinsics_to_excel
    from vbs_amd.reconstruction3d import Config, MarkerAnalysis
    from vbs_amd.xlsx_io import write_xlsx, read_xlsx
    rng = np.random.default_rng(3)
    R, T = P.random_pose(rng)
    ext = tmp_path / "pre" / "ExtrinsicParameters.xlsx"
    assert save_extrinsics_to_excel(R, T.reshape(3, 1), 0.4321, str(ext))
    df = read_xlsx(ext)
    assert list(df.columns) == ["Parameter", "Value", "Description"]
    assert list(df["Parameter"][:3]) == ["--- Camera Extrinsic Parameters ---", "Calibration Date", "Reprojection Error (px)"]
    assert "--- World to Camera Transformation ---" in list(df["Parameter"]) and len(df) == 17
    assert float(df["Value"][2]) == 0.4321
    assert [p for p in df["Parameter"] if str(p).startswith(("R_wc_", "T_wc_"))] == [
        f"R_wc_{i}{j}" for i in (1, 2, 3) for j in (1, 2, 3)] + ["T_wc_X", "T_wc_Y", "T_wc_Z"]
    intr = tmp_path / "IntrinsicParameters.xlsx"
    write_xlsx(intr, ["Param", "Value"], [["fx", 1200.0], ["fy", 1195.0], ["cx", 640.0], ["cy", 512.0], ["k1", -0.12],
                                          ["k2", 0.06], ["p1", 0.0011], ["p2", -0.0008], ["k3", 0.01]])
    ma = MarkerAnalysis(Config(data_dir=tmp_path, output_dir=tmp_path / "o", plots_dir=tmp_path / "p"))
    ma.load_parameters(intr, ext)                             # raises when the rotation fails its orthogonality check
    assert np.array_equal(ma.camera.R_world_to_cam, R.astype(np.float32))
    assert np.array_equal(ma.camera.T_world_to_cam, T.astype(np.float32).reshape(3, 1))
    # the intrinsic reader: both spellings of the key column, coefficients in load_parameters' order
    from vbs_amd.extrinsic_calibration import load_intrinsics_from_excel
    K, dist = load_intrinsics_from_excel(str(intr))
    assert np.array_equal(K, ma.camera.matrix) and np.array_equal(dist, ma.camera.dist_coeffs)
    assert np.array_equal(dist, P.DIST_ON)


def test_pixel_markers_merge_round_trip(tmp_path):
    from vbs_amd.extrinsic_calibration import merge_correspondences
    from vbs_amd.pipeline import to_pixel_markers
    world = P.shell_layout()
    ids = np.array([(k, j) for k, cnt in enumerate(P.RING_COUNTS) for j in range(cnt)])
    rng = np.random.default_rng(5)
    order = rng.permutation(len(ids))                          # slots in another order than the marker ids
    table = np.zeros((2, len(ids), L.TABLE_COLS), dtype=np.float32)
    table[..., 0] = L.FLAG_TRACKED
    table[..., 1:3] = rng.uniform(10, 600, size=(2, len(ids), 2)).astype(np.float32)
    table[1, 7, 0] = 0                                         # one untracked slot in frame 1
    df = to_pixel_markers(table, ids[order], frame=1, path=tmp_path / "pixel_marker.csv")
    assert list(df.columns) == ["marker_id", "u", "v"] and len(df) == len(ids) - 1
    mid = np.arange(1, len(ids) + 1)
    pd.DataFrame({"marker_id": mid, "Xw": world[:, 0], "Yw": world[:, 1], "Zw": world[:, 2]}).to_csv(
        tmp_path / "world_marker_CMM.csv", index=False)
    obj, img, got_ids = merge_correspondences(pd.read_csv(tmp_path / "world_marker_CMM.csv"),
                                              pd.read_csv(tmp_path / "pixel_marker.csv"))
    missing = mid[order][7]
    want = [m for m in mid if m != missing]
    assert list(got_ids) == want                               # ID order, the untracked one dropped
    slot_of = {int(m): s for s, m in enumerate(mid[order])}
    assert np.array_equal(obj, world[[m - 1 for m in want]].astype(np.float32))
    assert np.array_equal(img, table[1, [slot_of[m] for m in want], 1:3])


def test_pnp_samples():
    from vbs_amd.engine import pnp_samples
    a, b = pnp_samples(65, 1000, 7), pnp_samples(65, 1000, 7)
    assert a.dtype == np.int32 and a.shape == (1000, 6) and np.array_equal(a, b)
    assert not np.array_equal(a, pnp_samples(65, 1000, 8))
    assert a.min() >= 0 and a.max() < 65
    assert all(len(set(r)) == 6 for r in a.tolist())
    assert np.array_equal(a, P.samples(65, 1000, 7))           # the helper draws the same table
    assert (pnp_samples(5, 10, 0) == -1).all()
    with pytest.raises(ValueError):
        pnp_samples(65, L.PNP_MAX_HYPOTHESES + 1, 0)


def test_plot_names_matplotlib():
    from vbs_amd.extrinsic_calibration import plot_3d_calibration_result
    with pytest.raises(NotImplementedError, match="matplotlib"):
        plot_3d_calibration_result(np.zeros((4, 3)), np.eye(3), np.zeros(3))
