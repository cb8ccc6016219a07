"""Chessboard corners, the parts that need no GPU: the NumPy helper (tests/helpers/chess_oracle.py) on the generated boards and
on the published shot, the layout `collect_corners` promises, the exports and the refusals."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import chess_cases as CC                                      # noqa: E402
import chess_oracle as CO                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vbs_chess_workspace", "vbs_chess_corners", "vbs_corner_subpix")
NAMES = [c["name"] for c in CC.cases()]


def _err(a, b):
    d = np.linalg.norm(np.asarray(a, dtype=np.float64) - b, axis=1)
    return float(d.max()), float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize("name", NAMES)
def test_helper_on_generated_cases(name):
    """The helper finds the board or refuses it as the case says; its peaks lie within 2 px of truth.  Over EVERY seed tried, no
    walk decision was a tie: no accepted nearest candidate had an equal-distance rival, no acceptance sat on its threshold.  (The
    first two steps of a seed do tie on a regular board of integer peaks - `step_ties`, lowest index on both sides - and are
    reported, not asserted.)"""
    c, r = CC.by_name(name), CC.helper_results()[name]
    assert r["found"] == c["found"]
    print(f"{name}: ties {r['ties']}, seeds with equidistant first steps {r['step_ties']}")
    assert r["ties"] == 0
    if c["found"]:
        assert _err(r["peaks"], c["truth"])[0] <= 2.0
    else:
        assert (r["peaks"] == -1).all() and np.isnan(r["corners"]).all()
    if name == "uniform":
        assert r["n_candidates"] == 0


def test_accuracy_record():
    """The helper's own distance to truth (largest, rms; px) per case, for the finder's (2,2) refinement and for the (11,11) one:
    printed, and equal to what chess_cases.HELPER_ERR_PX records.  Asserted: the (11,11) refinement is no worse than the peaks."""
    for c in CC.cases():
        if not c["found"]:
            continue
        r = CC.helper_results()[c["name"]]
        peak, finder, refined = _err(r["peaks"], c["truth"]), _err(r["corners"], c["truth"]), _err(r["refined"], c["truth"])
        print(f'    "{c["name"]}": dict(finder=({finder[0]:.4f}, {finder[1]:.4f}), refined=({refined[0]:.4f}, {refined[1]:.4f})),'
              f"   # peaks ({peak[0]:.4f}, {peak[1]:.4f})")
        assert refined[0] <= peak[0] and refined[1] <= peak[1]
        rec = CC.HELPER_ERR_PX[c["name"]]
        assert np.allclose(rec["finder"], finder, atol=1e-4) and np.allclose(rec["refined"], refined, atol=1e-4)


def test_reversed_sums_stay_within_one_iteration():
    """What the GPU test allows the device: with its sums in the opposite order the helper's iteration count moves by at most one,
    for at most 5 % of a case's corners."""
    for c in CC.cases():
        if not c["found"]:
            continue
        r = CC.helper_results()[c["name"]]
        for start, kw, its in ((r["peaks"].astype(np.float64), CO.FINDER_SUBPIX, r["iters"]), (r["corners"], {}, r["refined_iters"])):
            _, it2 = CO.corner_subpix(c["gray"], start, reverse=True, **kw)
            diff = np.abs(it2.astype(int) - its.astype(int))
            assert diff.max() <= 1 and (diff > 0).sum() <= 0.05 * len(diff)


def test_published_shot(golden_dir):
    """The helper finds 6 x 6 on the published shot; the peaks equal chess_shot.json; the scale from the corners is within one
    pixel per square (1 / 24.4) of the fixture's box rule, whose own uncertainty that is."""
    sys.path.insert(0, golden_dir)
    import make_chess_golden as G
    want = json.load(open(os.path.join(golden_dir, "chess_shot.json")))
    gray, box = G.shot_gray()
    r = CO.find_chessboard_corners(gray, G.PATTERN, want=True)
    assert r["found"] == 1 and r["n_candidates"] == want["n_candidates"]
    assert r["peaks"].tolist() == want["peaks"]
    assert np.allclose(r["corners"], want["corners"], atol=1e-9)
    from vbs_amd.diameter_validation import scale_from_corners
    for key, pts in (("scale_peaks", r["peaks"]), ("scale_corners", r["corners"])):
        s = float(scale_from_corners(pts, G.PATTERN, G.SQUARE_MM))
        print(f"{key}: {s:.4f} px/mm (box rule {box:.4f})")
        assert abs(s - want[key]) < 1e-9
        assert abs(s - box) * G.SQUARE_MM <= 1.0                 # one pixel per square
    assert abs(want["scale_refined"] - box) * G.SQUARE_MM <= 1.0


def test_crop_and_object_points():
    from vbs_amd import intrinsic_calibration as IC
    for h, w in ((749, 571), (481, 643), (97, 33)):
        img = np.arange(h * w, dtype=np.int64).reshape(h, w)
        left, right, top, bottom = int(w * (1 / 8)), int(w * (1 / 8)), int(h * (1 / 16)), int(h * 0)
        assert np.array_equal(IC.crop_image(img), img[top:h - bottom, left:w - right])
        assert IC.crop_image(img).base is not None            # a view
    for pat, sq in (((6, 6), 3.0), ((7, 4), 2.5)):
        objp = np.zeros((np.prod(pat), 3), np.float32)
        objp[:, :2] = np.mgrid[:pat[0], :pat[1]].T.reshape(-1, 2) * sq
        got = IC.object_points(pat, sq)
        assert got.dtype == np.float32 and np.array_equal(got, objp)
        assert tuple(got[1]) == (sq, 0.0, 0.0)                # corner (r, c) at index r * pw + c, x along a row


def test_sheet_round_trip(tmp_path):
    from vbs_amd import intrinsic_calibration as IC
    from vbs_amd.extrinsic_calibration import load_intrinsics_from_excel
    K = np.array([[900.5, 0.25, 320.0], [0, 905.0, 240.5], [0, 0, 1]])
    dist = np.array([-0.3, 0.1, 0.001, -0.002, 0.05])
    path = str(tmp_path / "out" / "calibration_results.xlsx")
    IC.save_calib_results(K, dist, 0.42, path)
    K2, d2 = load_intrinsics_from_excel(path)
    assert np.allclose(K2, K.astype(np.float32)) and np.allclose(d2, dist.astype(np.float32))


def test_exports_and_constants():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SYMBOLS and hasattr(lib, name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_CHESS_\w+)\s+(\d+)", hdr)}
    assert (defs["VBS_CHESS_MAX_CANDIDATES"], defs["VBS_CHESS_MAX_PATTERN"], defs["VBS_CHESS_MAX_WIN"]) == \
        (L.CHESS_MAX_CANDIDATES, L.CHESS_MAX_PATTERN, L.CHESS_MAX_WIN) == (CO.MAX_CANDIDATES, CO.MAX_PATTERN, CO.MAX_WIN)
    # argument checks happen before the device is touched: a pattern beyond the cap is VBS_ECAPACITY, never cut short
    one = C.c_void_p(8)
    f = L.lib().vbs_chess_corners
    assert f(0, one, 1, 64, 64, 4096, 64, 32, 9, one, one, one, one, None, one, None) == L.VBS_ECAPACITY
    assert f(0, one, 1, 64, 64, 4096, 64, 1, 9, one, one, one, one, None, one, None) == L.VBS_EINVAL
    assert L.lib().vbs_corner_subpix(0, one, 1, 64, 64, 4096, 64, one, 4, 16, 3, -1, -1, 30, 1e-3, None, None) == L.VBS_EINVAL
    assert L.lib().vbs_chess_workspace(2, 16, 32) == 2 * 28 * 8


def test_refusals(capsys):
    import torch
    from vbs_amd import diameter_validation as DV, intrinsic_calibration as IC
    with pytest.raises(NotImplementedError, match="matplotlib"):
        IC.plot_comparison("x.png", np.eye(3), np.zeros(5), 0.0)
    with pytest.raises(NotImplementedError, match="matplotlib"):
        IC.plot_3d_poses([], [], (6, 6), 3.0)
    # calibrate_camera after the corner collection: None with the reference's message below 3 valid images, otherwise the
    # refusal that names the missing last step
    three = ([np.zeros((36, 3), np.float32)] * 3, [np.zeros((36, 1, 2), np.float32)] * 3, ["a.png", "b.png", "c.png"], (640, 480))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(IC, "collect_corners", lambda *a, **k: three)
        with pytest.raises(NotImplementedError, match="calibrateCamera"):
            IC.calibrate_camera("some_dir", (6, 6), 3.0)
        mp.setattr(IC, "collect_corners", lambda *a, **k: tuple(v[:2] if isinstance(v, list) else v for v in three))
        capsys.readouterr()
        assert IC.calibrate_camera("some_dir", (6, 6), 3.0) is None
        out = capsys.readouterr().out
        assert "Processing images in: some_dir" in out and "Insufficient valid images" in out
    if not torch.cuda.is_available():
        img = np.zeros((64, 64), dtype=np.uint8)
        with pytest.raises(L.VbsError):
            IC.collect_corners([img], (6, 6), 3.0)
        with pytest.raises(L.VbsError):
            IC.calibrate_camera(os.path.join(ROOT, "tests", "golden"), (6, 6), 3.0)
        with pytest.raises(L.VbsError):
            DV.scale_from_image(img, (6, 6), 3.0)


def test_shim_names():
    sys.path.insert(0, os.path.join(ROOT, "vision-basedsensor_amd", "Marker_Calibration"))
    import importlib
    m = importlib.import_module("intrinsic_calibration")
    for name in ("crop_image", "save_calib_results", "calibrate_camera", "plot_comparison", "plot_3d_poses", "collect_corners"):
        assert callable(getattr(m, name))
