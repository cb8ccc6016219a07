"""Chessboard corners on the device (csrc/k_chess.hip) against the NumPy helper tests/helpers/chess_oracle.py and against the true
corners of the rendered boards (tests/helpers/chess_cases.py).  Response, candidates and ordering are integer: exact.  The
sub-pixel step differs from the helper only in the order of its five float64 sums."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import chess_cases as CC                                      # noqa: E402
import chess_oracle as CO                                     # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
NAMES = [c["name"] for c in CC.cases()]
# Largest gap between the device's and the helper's sub-pixel corners where both took the same number of iterations, over every
# case, both parameter sets and the published shot, measured on an MI355X: 5.7e-14 px (the tests print it).  The bound is 10 x that;
# only the summation order differs, so anything above 1e-6 px would mean a defect.
SAME_ITERS_PX = 5.7e-13
PARAMS = (("finder", CO.FINDER_SUBPIX), ("refined", dict(win=(11, 11), zero_zone=(-1, -1), max_iter=30, eps=1e-3)))

_engines = {}


def engine_for(h, w):
    from vbs_amd.engine import Engine
    if (h, w) not in _engines:
        _engines[(h, w)] = Engine(h, w, max_markers=64, max_batch=8)
    return _engines[(h, w)]


def device_case(name):
    """Device tensors of a case: the view itself for the strided crop."""
    c = CC.by_name(name)
    g = c["gray"]
    if name == "strided_crop":
        big = torch.from_numpy(np.ascontiguousarray(g.base)).cuda()
        g = big[40:40 + 157, 70:70 + 203]
        assert not g.is_contiguous()
    return c, g


@pytest.mark.parametrize("name", NAMES)
def test_response_and_ordering(name):
    c, g = device_case(name)
    want = CC.helper_results()[name]
    found, corners, peaks, ncand, resp = engine_for(*c["gray"].shape).find_chessboard_corners(g, c["pattern"], want_response=True)
    assert np.array_equal(resp[0].cpu().numpy(), want["response"])
    assert int(ncand[0]) == want["n_candidates"] and int(found[0]) == want["found"] == c["found"]
    assert np.array_equal(peaks[0].cpu().numpy(), want["peaks"])
    assert np.isnan(corners[0].cpu().numpy()).all() == (not c["found"])


def two_class_check(got, its, ref, ref_its, eps, label):
    """The sub-pixel rule against the helper: the same iteration count -> within SAME_ITERS_PX; one iteration apart -> within eps,
    for at most 5 % of the corners; further apart fails.  Returns the number of corners in the second class."""
    gap = np.linalg.norm(got - ref, axis=1)
    diff = np.abs(its.astype(int) - ref_its.astype(int))
    same = diff == 0
    print(f"{label}: same-iteration gap max {gap[same].max() if same.any() else 0.0:.3e} px, "
          f"{int((diff == 1).sum())} corners one iteration apart, {int((diff > 1).sum())} further")
    assert diff.max() <= 1
    assert (gap[same] <= SAME_ITERS_PX).all()
    assert (gap[~same] <= eps).all()
    assert (~same).sum() <= 0.05 * len(gap)
    return int((~same).sum())


def test_published_shot(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_chess_golden as G
    from vbs_amd import diameter_validation as DV
    want = json.load(open(os.path.join(golden_dir, "chess_shot.json")))
    gray, _ = G.shot_gray()
    eng = engine_for(*gray.shape)
    found, corners, peaks, ncand = eng.find_chessboard_corners(gray, G.PATTERN)
    assert int(found[0]) == 1 and int(ncand[0]) == want["n_candidates"] and peaks[0].cpu().tolist() == want["peaks"]
    # the finder's corners are its peaks through k_corner_subpix: held to the helper corner by corner, iteration counts included
    start = np.asarray(want["peaks"], dtype=np.float64)
    ref, ref_its = CO.corner_subpix(gray, start, **CO.FINDER_SUBPIX)
    assert np.array_equal(ref, np.asarray(want["corners"]))
    eps = CO.FINDER_SUBPIX["eps"]
    got, its = eng.corner_subpix(gray, start, **CO.FINDER_SUBPIX, want_iters=True)
    assert torch.equal(got, corners)
    apart = two_class_check(got[0].cpu().numpy(), its[0].cpu().numpy(), ref, ref_its, eps, "published shot, finder")
    # scale_from_image (BGR in) against scale_from_corners of the helper's corners: the per-corner bound carried through the mean
    # of the 60 neighbour distances - each moves by at most the sum of its two corners' bounds, and a corner of the second class
    # (bound eps instead of SAME_ITERS_PX) takes part in at most 4 of them
    scale, c32 = DV.scale_from_image(np.load(os.path.join(golden_dir, "diameter_shot.npz"))["bgr"], G.PATTERN, G.SQUARE_MM, engine=eng)
    bound = (2 * SAME_ITERS_PX + 4 * apart * eps / 60) / G.SQUARE_MM
    print(f"scale_from_image {scale:.9f} px/mm, helper {want['scale_corners']:.9f}, bound {bound:.3e}")
    assert abs(scale - want["scale_corners"]) <= bound
    assert c32.dtype == np.float32 and c32.shape == (36, 1, 2)
    assert DV.scale_from_image(np.full(gray.shape, 90, dtype=np.uint8), G.PATTERN, G.SQUARE_MM, engine=eng) == (None, None)
    DV.close_engines()


@pytest.mark.parametrize("name", [n for n in NAMES if CC.by_name(n)["found"]])
def test_subpix_against_helper_and_truth(name):
    c, g = device_case(name)
    want = CC.helper_results()[name]
    eng = engine_for(*c["gray"].shape)
    starts = {"finder": want["peaks"].astype(np.float64), "refined": want["corners"]}
    helper = {"finder": (want["corners"], want["iters"]), "refined": (want["refined"], want["refined_iters"])}
    for key, kw in PARAMS:
        got, its = eng.corner_subpix(g, starts[key], kw["win"], kw["zero_zone"], kw["max_iter"], kw["eps"], want_iters=True)
        got, its = got[0].cpu().numpy(), its[0].cpu().numpy()
        ref, ref_its = helper[key]
        two_class_check(got, its, ref, ref_its, kw["eps"], f"{name} {key}")
        to_truth = np.linalg.norm(got - c["truth"], axis=1)
        assert (to_truth <= CC.HELPER_ERR_PX[name][key][0] + 5e-5 + kw["eps"]).all()      # (the record is rounded to 1e-4)
    if name == "rotated_30":                                # the finder's corners are its peaks through the same kernel
        _, corners, _, _ = eng.find_chessboard_corners(g, c["pattern"])
        got, _ = eng.corner_subpix(g, starts["finder"], **{k: v for k, v in CO.FINDER_SUBPIX.items()}, want_iters=True)
        assert torch.equal(corners, got)


def test_determinism_and_batching():
    frames, cs = CC.batch()
    eng = engine_for(*frames.shape[1:])
    dev = torch.from_numpy(frames).cuda()
    a = eng.find_chessboard_corners(dev, (6, 6), want_response=True)
    b = eng.find_chessboard_corners(dev, (6, 6), want_response=True)
    assert a[0].cpu().tolist() == [c["found"] for c in cs] == [1, 0, 1, 0, 1]
    ra = eng.corner_subpix(dev, a[1], want_iters=True)
    rb = eng.corner_subpix(dev, b[1], want_iters=True)
    for x, y in zip(a + ra, b + rb):                         # two runs: the same bits (NaN rows included)
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for i in range(len(cs)):                                 # a frame alone = the frame in the batch
        one = eng.find_chessboard_corners(dev[i], (6, 6), want_response=True)
        for x, y in zip(one, a):
            assert torch.equal(bits(x[0]), bits(y[i]))
        r1 = eng.corner_subpix(dev[i], a[1][i], want_iters=True)
        assert torch.equal(bits(r1[0][0]), bits(ra[0][i])) and torch.equal(r1[1][0], ra[1][i])
    n = eng.find_chessboard_corners(frames, (6, 6))           # numpy in = device tensor in
    bgr = eng.find_chessboard_corners(dev[..., None].expand(-1, -1, -1, 3).contiguous(), (6, 6))   # gray = its BGR replication
    for x, y, z in zip(n, bgr, a):
        assert torch.equal(bits(x), bits(z)) and torch.equal(bits(y), bits(z))


def test_collect_corners_batch():
    """collect_corners on the batch: the found frames only, in order, in cv2's layout.  The images are padded so that the
    reference's crop gives the frames back."""
    from vbs_amd import diameter_validation as DV, intrinsic_calibration as IC
    frames, cs = CC.batch()
    h, w = frames.shape[1:]
    H, W = 168, 272                                          # crop: left = right = int(272 / 8) = 34, top = int(168 / 16) = 10
    padded = [np.full((H, W), CC.GROUND, dtype=np.uint8) for _ in cs]
    for p, f in zip(padded, frames):
        p[10:10 + h, 34:34 + w] = f[:H - 10, :W - 68]
    assert IC.crop_image(padded[0]).shape == (158, 204)
    obj, img, valid, size = IC.collect_corners(padded, (6, 6), 3.0)
    assert valid == [0, 2, 4] and size == (204, 158) and len(obj) == len(img) == 3
    for o, p, i in zip(obj, img, valid):
        assert o.dtype == np.float32 and np.array_equal(o, IC.object_points((6, 6), 3.0))
        assert p.dtype == np.float32 and p.shape == (36, 1, 2)
        assert np.linalg.norm(p.reshape(-1, 2) - cs[i]["truth"], axis=1).max() <= CC.HELPER_ERR_PX[cs[i]["name"]]["refined"][0] + 0.01
    with pytest.raises(NotImplementedError, match="calibrateCamera"):
        import tempfile
        from PIL import Image
        with tempfile.TemporaryDirectory() as td:
            for k in (0, 2, 4):
                Image.fromarray(padded[k]).save(os.path.join(td, f"b{k}.png"))
            IC.calibrate_camera(td, (6, 6), 3.0)
    DV.close_engines()


def test_capacity_is_reported():
    from vbs_amd import _lib as L
    eng = engine_for(157, 203)
    with pytest.raises(L.VbsError, match="VBS_CHESS_MAX_PATTERN"):
        eng.find_chessboard_corners(np.zeros((157, 203), dtype=np.uint8), (32, 9))
