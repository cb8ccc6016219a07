"""GPU tests of the marker diameter validation (k_diameter.hip; `pytest -m gpu` on an MI355X): the device against the
sequential helper `tests/helpers/diameter_oracle.py`.

Exact: the thresholded mask bits, the survivor set and its order, area2, n_axis, n_diag, first pixel.  Enclosing circle: the
circle through the REPORTED support points, rebuilt in exact arithmetic, contains every pixel centre of the component and its
squared radius equals the exact minimum's as fractions (the support set itself is not compared: digital discs have co-circular
points); float64 radius, centre and diameter_mm within 1e-12 relative of the correctly rounded values.  Circularity, area,
perimeter and the statistics: 1e-12 relative against float64 Python / NumPy.

Every case first asserts, with the helper alone, that no component's circularity lies within 1e-9 of the threshold and no area
equals min_area: both floating-point routes then take the same decisions.
"""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import diameter_cases as K                                    # noqa: E402
import diameter_oracle as D                                   # noqa: E402
from diameter_check import MIN_AREA, MIN_CIRC, check_frame, close, helper_frame, run     # noqa: E402


def engine(h, w, **kw):
    from vbs_amd.engine import Engine
    kw.setdefault("max_markers", 512)
    kw.setdefault("max_batch", 4)
    return Engine(h, w, **kw)


def board_expect(allc, surv):
    """The shot holds what the issue lists: a chessboard blob rejected by circularity (a square's is pi / 4, the board's far
    less), ellipses on both sides of 0.85, specks under 100 px, survivors."""
    big = max(allc, key=lambda c: c["area"])
    assert big["area"] > 5000 and big["circularity"] < math.pi / 4 and all(c is not big for c in surv)
    assert any(c["area"] < MIN_AREA for c in allc)
    assert any(c["area"] >= MIN_AREA and 0.3 < c["circularity"] < MIN_CIRC for c in allc)
    assert len(surv) >= 20
    # ... and ABOVE it: a survivor that is an ellipse, not a disc (axis ratio of its border well below 1), next to discs
    ratios = [D.axis_ratio(c["chain"]) for c in surv]
    assert min(ratios) < 0.9 and max(ratios) > 0.97 and sum(r < 0.9 for r in ratios) >= 2


def test_c1_gray_validation_shot_with_chessboard():
    g = K.shot(480, 640, 1, board=True)
    rec, counts, stats, bits = run(engine(480, 640), g[None], 20.0)
    surv = check_frame(g, rec[0], int(counts[0]), stats[0], bits[0], 20.0, expect=board_expect)
    # holes were ignored, blobs at the image edge measured: some survivor touches the edge, and the mask had holes
    mask = D.threshold_inv(D.blur5_u8(g), K.THRESHOLD)
    assert D.fill_holes(mask).sum() > mask.sum()
    assert any(min(x for x, _ in c["chain"]) == 0 or min(y for _, y in c["chain"]) == 0 for c in D.contours_of(mask))
    assert len(surv) > 0


def test_c3_gray_validation_shot_with_offset():
    g = K.shot(1024, 1280, 3, board=True)
    rec, counts, stats, bits = run(engine(1024, 1280, max_batch=2), g[None], 19.7, offset=-0.03)
    check_frame(g, rec[0], int(counts[0]), stats[0], bits[0], 19.7, offset=-0.03, expect=board_expect)


def test_bgr_frames_and_a_width_that_is_no_multiple_of_64():
    from oracle import stages as O
    g = [K.shot(300, 330, s, board=(s == 5)) for s in (5, 6)]
    f = np.stack([K.to_bgr(x, 40 + i) for i, x in enumerate(g)])
    rec, counts, stats, bits = run(engine(300, 330), f, 12.5)
    for i in range(2):
        check_frame(O.bgr2gray(f[i]), rec[i], int(counts[i]), stats[i], bits[i], 12.5)
    # gray input of the same size, as a crop VIEW of a wider tensor (strides)
    wide = np.full((2, 300, 400), 200, np.uint8)
    wide[:, :, 35:365] = np.stack(g)
    eng = engine(300, 330)
    ft = torch.from_numpy(wide).to(eng.device)[:, :, 35:365]
    rec, counts, stats = eng.measure_markers(ft, K.THRESHOLD, 12.5)
    b = eng.threshold_bits(ft, K.THRESHOLD)
    torch.cuda.synchronize()
    for i in range(2):
        check_frame(g[i], rec[i].cpu().numpy(), int(counts[i]), stats[i].cpu().numpy(), b[i].cpu().numpy(), 12.5)


def test_batch_of_72_frames_with_per_frame_differences_over_several_passes():
    frames = np.stack([K.shot(128, 256, 100 + s, board=False, pitch=50 + s % 7) for s in range(72)])
    eng = engine(128, 256, max_batch=32)                      # 72 frames = three internal passes, the last one short
    rec, counts, stats, bits = run(eng, frames, 20.0)
    seen = set()
    for i in range(72):
        surv = check_frame(frames[i], rec[i], int(counts[i]), stats[i], bits[i], 20.0)
        seen.add(tuple(c["first"] for c in surv))
    assert len(seen) > 36                                     # the frames really differ
    rec2, counts2, stats2, _ = run(eng, frames, 20.0)         # fixed summation order: the same bits run to run
    assert np.array_equal(counts, counts2) and np.array_equal(stats.view(np.int64), stats2.view(np.int64))
    for i in range(72):
        assert np.array_equal(rec[i, :counts[i]].view(np.int64), rec2[i, :counts[i]].view(np.int64))


def test_other_filter_settings_and_an_empty_frame():
    g = K.shot(480, 640, 7, board=True)
    blank = np.full((480, 640), 200, np.uint8)
    rec, counts, stats, bits = run(engine(480, 640), np.stack([g, blank]), 20.0, min_area=300.5, min_circ=0.5)
    check_frame(g, rec[0], int(counts[0]), stats[0], bits[0], 20.0, min_area=300.5, min_circ=0.5)
    check_frame(blank, rec[1], int(counts[1]), stats[1], bits[1], 20.0, min_area=300.5, min_circ=0.5)
    assert counts[1] == 0


def test_a_marker_beyond_the_stated_extent_is_reported_not_truncated():
    """A disc of 620 px passes both filters and exceeds VBS_DIAM_MAX_EXTENT: its frame gets VBS_ECAPACITY and the shim raises;
    the frame next to it in the batch is measured as usual.  A rejected blob of that size (a square) does not count."""
    import vbs_amd.diameter_validation as V
    H, W = 1024, 1280
    big = np.full((H, W), 200.0)
    K._ellipse(big, 640.0, 512.0, 310.0, 310.0, 0.0, 40.0)
    K._ellipse(big, 60.0, 60.0, 15.0, 15.0, 0.0, 40.0)
    big = big.astype(np.uint8)
    square = np.full((H, W), 200, np.uint8)
    square[100:800, 200:900] = 40                             # 700 px wide, circularity ~ pi / 4: rejected before the circle
    K_ = square.astype(np.float64)
    K._ellipse(K_, 1000.0, 500.0, 18.0, 18.0, 0.0, 40.0)
    square = K_.astype(np.uint8)
    assert L.DIAM_MAX_EXTENT < 620
    eng = engine(H, W, max_batch=2)
    rec, counts, stats, bits = run(eng, np.stack([big, square]), 20.0)
    assert counts[0] == L.VBS_ECAPACITY and math.isnan(stats[0][1])
    surv = check_frame(square, rec[1], int(counts[1]), stats[1], bits[1], 20.0)
    assert len(surv) == 1
    with pytest.raises(L.VbsError):
        V.measure_markers(big, 20.0, K.THRESHOLD, engine=eng)
    with pytest.raises(L.VbsError):
        V.measure_markers(big, 20.0, K.THRESHOLD)             # the module's own (cached) engine
    V.close_engines()
    r, d = V.measure_markers(square, 20.0, K.THRESHOLD, engine=eng)
    assert len(d) == 1 and close(d[0], surv[0]["diameter_mm"]) and r.shape == (1, L.DIAM_COLS)
    assert V.summarize(d) == (d[0], 0.0)


def test_drop_in_takes_one_bgr_image_and_keeps_one_engine_per_geometry():
    """`measure_markers(img, scale, threshold)` with no engine: a [H,W,3] array is ONE BGR image (not H frames), and a
    recording measured image by image reuses one handle."""
    from oracle import stages as O
    import vbs_amd.diameter_validation as V
    V.close_engines()
    g = [K.shot(300, 330, s) for s in (6, 8)]
    f = [K.to_bgr(x, 50 + i) for i, x in enumerate(g)]
    try:
        for img in (f[0], f[1], g[0]):
            gray = img if img.ndim == 2 else O.bgr2gray(img)
            _, _, surv = helper_frame(gray, 12.5)
            r, d = V.measure_markers(img, 12.5, K.THRESHOLD)
            assert len(d) == len(surv) and all(close(a, c["diameter_mm"]) for a, c in zip(d, surv))
            assert [int(v) for v in r[:, 22]] == [c["area2"] for c in surv]
            assert len(V._engines) == 1
        first = next(iter(V._engines.values()))
        rec, counts, stats = V.measure_frames(np.stack(f), 12.5, K.THRESHOLD)      # a batch: the engine is rebuilt ONCE for batches
        assert rec.shape[0] == 2 and len(V._engines) == 1 and next(iter(V._engines.values())) is not first
        V.measure_frames(np.stack(f), 12.5, K.THRESHOLD)
        assert next(iter(V._engines.values())).max_batch == 64
        with pytest.raises(ValueError):
            V.measure_markers(np.stack(g), 12.5, K.THRESHOLD)
    finally:
        V.close_engines()
    assert not V._engines


def test_published_validation_shot(golden_dir):
    """README Figure 5 (a), `img/diameter_shot.png`, decoded into tests/golden/diameter_shot.npz with the threshold and the
    px/mm scale its generator derives from the 3 mm chessboard in the image (tests/golden/make_diameter_golden.py states
    the rule).  Device and helper agree exactly on every integer quantity, on the mask and on the circles (check_frame).

    Informative, NOT asserted because it does not hold: the figure reports 2.01 +/- 0.04 mm over about 120 markers; this
    reproduction gives 119 markers, mean 2.129 mm, np.std 0.109 mm (threshold 115, 8.143 px/mm).  The image is a downscaled,
    annotated copy: at 8.1 px/mm one pixel is 0.12 mm - the whole offset is ONE pixel of diameter - a 2-px green outline of
    intermediate grey is drawn on every marker's edge, and the 5x5 blur spans 0.6 mm here."""
    from oracle import stages as O
    z = np.load(os.path.join(golden_dir, "diameter_shot.npz"))
    bgr, thr, scale = z["bgr"], int(z["threshold"]), float(z["scale"])
    H, W = bgr.shape[:2]
    gray = O.bgr2gray(bgr)
    eng = engine(H, W, max_batch=1)
    ft = torch.from_numpy(bgr[None]).to(eng.device)
    rec, counts, stats = eng.measure_markers(ft, thr, scale)
    bits = eng.threshold_bits(ft, thr)
    torch.cuda.synchronize()
    old = K.THRESHOLD
    K.THRESHOLD = thr                                         # (helper_frame reads the case module's level)
    try:
        surv = check_frame(gray, rec[0].cpu().numpy(), int(counts[0]), stats[0].cpu().numpy(), bits[0].cpu().numpy(), scale)
    finally:
        K.THRESHOLD = old
    d = np.array([c["diameter_mm"] for c in surv])
    print(f"published shot: {len(surv)} markers, mean {d.mean():.4f} mm, std {d.std():.4f} mm, device mean "
          f"{float(stats[0, 1]):.4f} std {float(stats[0, 2]):.4f}; figure: 2.01 +/- 0.04 mm")
    assert 100 <= len(surv) <= 140                            # "about 120 rigid markers"
    board = max(D.contours_of(D.threshold_inv(D.blur5_u8(gray), thr)), key=lambda c: c["area"])
    assert board["circularity"] < 0.3 and all(c["first"] != board["first"] for c in surv)
