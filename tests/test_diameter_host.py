"""Marker diameter validation, the parts that need no GPU: the step table against traced borders, the scale arithmetic against
the reference's own statements (tests/golden/diameter_scale.json), the exports, and the shim's refusal to run without a GPU."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage

import vbs_amd._lib as L
from oracle import stages as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import diameter_oracle as D                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vbs_step_lut", "vbs_threshold_bits", "vbs_measure_markers")


def _step_lut():
    lut = np.zeros(256, dtype=np.uint32)
    assert L.lib().vbs_step_lut(lut.ctypes.data_as(C.c_void_p)) == 0
    return lut


def lut_measures(fg, lut):
    """Sum the library's step table over the border pixels of every 8-connected component of `fg` (hole-free):
    {first pixel (x, y): (area2, n_axis, n_diag)}."""
    H, W = fg.shape
    p = np.zeros((H + 2, W + 2), dtype=np.uint8)
    p[1:-1, 1:-1] = fg
    pat = np.zeros((H, W), dtype=np.int64)
    for d in range(8):
        pat |= p[1 + O._DY[d]:1 + O._DY[d] + H, 1 + O._DX[d]:1 + O._DX[d] + W].astype(np.int64) << d
    lab, n = ndimage.label(fg, structure=np.ones((3, 3)))
    acc = {}
    first = {}
    for y, x in zip(*np.nonzero(fg)):
        c = int(lab[y, x])
        if c not in first:
            first[c] = (int(x), int(y))                      # np.nonzero is in raster order
            acc[c] = [0, 0, 0]
        v = int(lut[pat[y, x]])
        for d in range(8):
            k = (v >> (4 * d)) & 15
            acc[c][0] += k * (int(x) * O._DY[d] - int(y) * O._DX[d])
            acc[c][1 + (d & 1)] += k
    return {first[c]: tuple(acc[c]) for c in acc}


def traced_measures(fg):
    out = {}
    for cnt in O.find_contours_external(fg, approx_simple=False):
        out[(int(cnt[0][0]), int(cnt[0][1]))] = D.chain_measures(cnt)
    return out


def test_step_lut_layout():
    lut = _step_lut()
    assert lut[0] == 0 and lut[255] == 0
    assert lut[1 << 4] == 1 << 16                            # only W set: one step, to W
    assert lut[(1 << 0) | (1 << 4)] == (1 << 16) | 1         # E and W (inside a 1-px line): one step each way
    # at most one step per direction, and never more steps than the vertex table's visits could make
    assert all(((int(v) >> (4 * d)) & 15) <= 1 for v in lut for d in range(8))


@pytest.mark.parametrize("seed,opened", [(0, True), (1, True), (2, False), (3, False), (4, False), (5, False)])
def test_step_lut_equals_traced_borders(seed, opened):
    """For hole-free foreground the per-pixel step table, summed over a component's pixels, is exactly the traced outer
    border's chain: unit steps, diagonal steps and the shoelace sum - for every component, including 1-px lines whose pixels
    are visited twice, diagonal necks and single pixels."""
    rng = np.random.default_rng(seed)
    a = ndimage.gaussian_filter(rng.random((150, 170)), 3.0 if opened else 1.2)
    fg = a > np.quantile(a, 0.6)
    if opened:
        fg = O.morph_open5(fg)
    else:
        fg[40, 10:120] = True                                # 1-px lines: pixels visited twice
        fg[10:100, 60] = True
        for k in range(12):                                  # a diagonal line (necks all the way) and isolated pixels
            fg[120 + k, 20 + k] = True
        fg[3:9:3, 3:160:7] = True
    fg = ndimage.binary_fill_holes(fg, structure=np.ones((3, 3)))
    fg = ndimage.binary_fill_holes(fg)
    want = traced_measures(fg)
    got = lut_measures(fg, _step_lut())
    assert len(want) > 5 and any(v == (0, 0, 0) for v in want.values()) == (not opened)
    assert got == want


def test_step_lut_simple_shapes():
    lut = _step_lut()
    sq = np.zeros((12, 12), bool)
    sq[3:8, 2:9] = True                                      # 7 x 5 pixels: centres span 6 x 4
    assert list(lut_measures(sq, lut).values()) == [(-2 * 24, 20, 0)] or list(lut_measures(sq, lut).values()) == [(2 * 24, 20, 0)]
    one = np.zeros((5, 5), bool)
    one[2, 2] = True
    assert lut_measures(one, lut) == {(2, 2): (0, 0, 0)}
    line = np.zeros((5, 9), bool)
    line[2, 1:8] = True
    assert lut_measures(line, lut) == {(1, 2): (0, 12, 0)}
    dia = np.eye(6, dtype=bool)
    assert lut_measures(dia, lut) == {(0, 0): (0, 0, 10)}


def test_exact_circle_helper():
    from fractions import Fraction as F
    assert D.exact_mec([(0, 0), (4, 0), (2, 1)]) == (F(2), F(0), F(4))
    assert D.exact_mec([(0, 0), (4, 0), (0, 2), (4, 2), (2, 1)]) == (F(2), F(1), F(5))
    cx, cy, r2 = D.exact_mec([(0, 0), (6, 0), (3, 9), (3, 1)])
    assert (cx, cy, r2) == D.circle_through([(0, 0), (6, 0), (3, 9)]) and r2 == F(25)
    rng = np.random.default_rng(0)
    pts = [tuple(p) for p in rng.integers(0, 40, (200, 2))]
    c = D.exact_mec(pts)
    assert all(D._inside(c, p) for p in pts)


def test_scale_from_corners_equals_the_reference_statements(golden_dir):
    from vbs_amd.diameter_validation import scale_from_corners
    for case in json.load(open(os.path.join(golden_dir, "diameter_scale.json"))):
        corners = np.array(case["corners"], dtype=case["dtype"]).reshape(case["shape"])
        got = scale_from_corners(corners, tuple(case["pattern_size"]), case["square_mm"])
        # the same distances, summed by np.mean in another order: float32 corners give float32 norms (as in the reference)
        tol = 1e-6 if case["dtype"] == "float32" else 1e-14
        assert abs(float(got) - case["scale"]) <= tol * case["scale"], case["name"]


def test_module_keeps_the_reference_names_and_refuses_the_corner_finder():
    import vbs_amd.diameter_validation as V
    assert set(V.CONFIG) == {"INPUT_IMAGE", "OUTPUT_IMG", "OUTPUT_PLOT", "CHESSBOARD_SIZE", "SQUARE_SIZE_MM", "MIN_AREA",
                             "MIN_CIRCULARITY", "DIAMETER_OFFSET_MM"}
    assert (V.CONFIG["MIN_AREA"], V.CONFIG["MIN_CIRCULARITY"], V.CONFIG["SQUARE_SIZE_MM"]) == (100, 0.85, 3.0)
    with pytest.raises(NotImplementedError, match="findChessboardCorners"):
        V.calculate_scale(np.zeros((8, 8), np.uint8), (6, 6), 3.0)
    assert V.summarize([2.0, 2.0, 2.06]) == (float(np.mean([2.0, 2.0, 2.06])), float(np.std([2.0, 2.0, 2.06])))
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "dv_shim", os.path.join(ROOT, "vision-basedsensor_amd", "Precision_Validation", "DiameterValidation.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert shim.measure_markers is V.measure_markers and shim.CONFIG is V.CONFIG


def test_published_shot_fixture_and_its_rule(golden_dir):
    """tests/golden/diameter_shot.npz: pixels of the published shot plus the threshold and scale its generator derived from the
    chessboard.  The board is 7 squares of 3 mm: the stored scale is its box's mean extent over 21 mm, and the box is square to
    3 %.  With the helper alone: about 120 markers survive, the board does not, and no decision sits on a filter boundary."""
    z = np.load(os.path.join(golden_dir, "diameter_shot.npz"))
    assert set(z.files) == {"bgr", "threshold", "scale", "board_box"} and z["bgr"].dtype == np.uint8 and z["bgr"].shape[2] == 3
    x0, y0, x1, y1 = (int(v) for v in z["board_box"])
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    assert abs(bw - bh) <= 0.03 * bw and float(z["scale"]) == 0.5 * (bw + bh) / 21.0
    _, allc, surv = D.measure_gray(O.bgr2gray(z["bgr"]), int(z["threshold"]), float(z["scale"]))
    assert all(abs(c["circularity"] - 0.85) > 1e-9 and c["area"] != 100 for c in allc)
    assert 100 <= len(surv) <= 140 and max(allc, key=lambda c: c["area"])["circularity"] < 0.3
    d = np.array([c["diameter_mm"] for c in surv])
    assert 1.5 < d.mean() < 2.5                                # millimetres of the right order: the scale rule found the board


def test_config_and_batch_shapes():
    import torch
    import vbs_amd.diameter_validation as V
    assert V._as_batch(np.zeros((70, 130), np.uint8)).shape == (1, 70, 130)
    assert V._as_batch(np.zeros((70, 130, 3), np.uint8)).shape == (1, 70, 130, 3)      # ONE BGR image, not 70 frames
    assert V._as_batch(torch.zeros((5, 70, 130), dtype=torch.uint8)).shape == (5, 70, 130)
    assert V._as_batch(np.zeros((5, 70, 130, 3), np.uint8)).shape == (5, 70, 130, 3)
    for bad in (np.zeros((70, 130), np.float32), np.zeros((2, 70, 130, 4), np.uint8), np.zeros((7,), np.uint8)):
        with pytest.raises(ValueError):
            V._as_batch(bad)


def test_measure_markers_raises_without_a_gpu(monkeypatch):
    import torch
    import vbs_amd.diameter_validation as V
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(L.VbsError):
        V.measure_markers(np.zeros((64, 128), np.uint8), 20.0, 127)
    with pytest.raises(L.VbsError):
        V.measure_frames(np.zeros((3, 64, 128), np.uint8), 20.0, 127)


def test_new_header_symbols_are_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    assert declared == set(L.SYMBOLS)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.DIAM_COLS, L.DIAM_STATS_COLS, L.DIAM_MAX_EXTENT) == (
        defs["VBS_DIAM_COLS"], defs["VBS_DIAM_STATS_COLS"], defs["VBS_DIAM_MAX_EXTENT"])
