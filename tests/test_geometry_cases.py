"""The inputs of tests/test_gpu_geometry_edges.py (tests/helpers/geometry_cases.py) have the properties those tests rely
on - checked with the oracle alone, no GPU.  Per frame of every geometry:
  * `O.marker_center` returns at least 6 markers for frames and 7 for mask frames (1 for 64 x 128 and 481 x 128, which
    have no room for six whole dots);
  * in pipeline frames `area` and `mask` are both non-zero on each of the four border lines - at 64 x 128 too: its six dots
    cut all four borders;
  * a returned marker has its centre in the last 64 columns, and one in the last 16 rows - for pipeline frames of the large
    branch in the last 29 rows: no 40-px dot closer to the border is returned (geometry_cases.last_rows);
  * no pixel of `O.normxcorr2_direct` on the oracle's area mask lies within 1e-7 of the 0.1 threshold, and the direct
    evaluation decides every pixel as the FFT one does: the bit-exact mask comparison rests on no coin toss;
  * mask frames lose no component to the 5x5 opening and none comes out of it thinner than 5 px;
  * the capacity counts (label_cases.expected_capacity) are not `over` at max_markers = 512."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

from oracle import stages as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import geometry_cases as GC                                   # noqa: E402
import label_cases as LC                                      # noqa: E402


def _rim_markers(markers, g, rows):
    xs = [m["center"][0] for m in markers]
    ys = [m["center"][1] for m in markers]
    assert any(x >= g.w - 64 for x in xs), (g.id, "no marker centre in the last 64 columns")
    assert any(y >= g.h - rows for y in ys), (g.id, f"no marker centre in the last {rows} rows")


def test_the_rules_give_the_limits_the_cases_are_named_for():
    """the launchers' rules as geometry_cases restates them, at the sizes the cases sit on."""
    assert GC.stage_rows(512, 2112, 256) == 128 and GC.stage_rows(513, 2112, 256) is None and GC.stage_rows(513, 2112, 768) == 43
    assert GC.stage_rows(1536, 2112, 768) == 128 and GC.stage_rows(1537, 2112, 768) is None
    assert GC.stage_rows(1536, 4096, 768) == 128 and GC.stage_rows(1536, 4096, 256) is None
    assert GC.stage_rows(64, 128, 768) == 1 and GC.stage_rows(64, 128, 256) == 1
    assert GC.stage_rows(2048, 128, 768) == 6 and GC.stage_rows(2049, 128, 768) is None
    assert GC.stage_takes(2048, 128) and not GC.stage_takes(2049, 128) and not GC.stage_takes(1537, 2112)
    assert not GC.stage_takes(2048, 2112)
    # k_stage_lat: with WW >= 33 (G = 1) the tile rule gives R = ceil(H / 64) from 361 rows on, 32 at 2048: the R limit of 128
    # would bind from 8193 rows, far beyond the H limit - 2048 is the tallest frame it takes, and 2049 is not below 2048
    assert GC.lat_rows(2048, 2112) == 32 and GC.lat_rows(2048, 4096) == 32 and GC.lat_rows(2049, 2112) is None
    assert all(GC.lat_rows(h, w) is not None for h in range(64, 2049, 31) for w in (2049, 2112, 4096))
    assert GC.lat_rows(1537, 2112) == 25 and GC.lat_rows(64, 128) == 1
    assert GC.ccl_takes(1537, 2112) and GC.ccl_takes(2048, 2112) and not GC.ccl_takes(2049, 128)
    assert GC.blur16_takes(64, 4096) and GC.blur16_takes(481, 4092) and not GC.blur16_takes(64, 128) and not GC.blur16_takes(481, 128)
    assert [g.case for g in GC.GEOMETRIES] == ["1", "2", "3", "4", "4b", "5", "6", "7", "8", "9", "10", "11", "12", "13"]


@pytest.mark.parametrize("g", GC.PIPELINE, ids=lambda g: g.id)
def test_frames_meet_the_input_conditions(g):
    centres = GC.dot_centres(g.h, g.w)
    d = GC.dot_diameter(g.h)
    # the layout: a centre 2 to 3 px inside each border, one in the last word, one in the last 16 rows
    assert ((centres[:, 1] >= 2) & (centres[:, 1] <= 3)).any() and ((g.h - 1 - centres[:, 1] >= 2) & (g.h - 1 - centres[:, 1] <= 3)).any()
    assert ((centres[:, 0] >= 2) & (centres[:, 0] <= 3)).any() and ((g.w - 1 - centres[:, 0] >= 2) & (g.w - 1 - centres[:, 0] <= 3)).any()
    assert (centres[:, 0] >= 64 * ((g.w - 1) // 64)).any() and (centres[:, 1] >= g.h - 16).any()
    assert g.h <= 1200 or (centres[:, 1] > 1200).any()
    assert g.w <= 1920 or (centres[:, 0] > 1920).any()
    dist = np.hypot(*(centres[:, None, :] - centres[None, :, :]).transpose(2, 0, 1)) + 1e9 * np.eye(len(centres))
    assert dist.min() >= d + 8, (g.id, dist.min())           # (jitter 3 px each: no two dots touch)
    sets = [("gray", GC.gray_frames(g.h, g.w))] + ([("bgr", GC.bgr_frames(g.h, g.w))] if g.bgr else [])
    p = O.branch_params(g.h)
    template = O.gkern(p["tl"], p["tsig"])
    for kind, frames in sets:
        assert frames.shape[:3] == (3, g.h, g.w)
        if kind == "bgr":
            assert (frames[..., 0] != frames[..., 1]).any() and (frames[..., 1] != frames[..., 2]).any()
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
        for i in range(3):
            tag = (g.id, kind, i)
            mask, area = O.find_markers(frames[i])
            for name, plane in (("area", area), ("mask", mask)):
                cut = [plane[0].any(), plane[-1].any(), plane[:, 0].any(), plane[:, -1].any()]
                assert all(cut), (tag, name, "top / bottom / left / right", cut)
            ncc = O.normxcorr2_direct(template, area)
            assert np.abs(ncc - 0.1).min() > 1e-7, (tag, "an NCC pixel within 1e-7 of the threshold: pick another seed")
            assert np.array_equal(ncc > 0.1, mask != 0), tag
            markers = O.marker_center(mask, area)
            assert len(markers) >= (1 if g.case in GC.FEW_MARKERS else 6), (tag, len(markers))
            _rim_markers(markers, g, GC.last_rows(g.h))
            assert not LC.expected_capacity(mask, area, GC.MAX_MARKERS)["over"], tag


@pytest.mark.parametrize("g", GC.MASKS, ids=lambda g: g.id)
def test_mask_frames_meet_the_input_conditions(g):
    h, w = g.h, g.w
    rim, ring = GC.mask_frames(h, w)
    for c in (rim, ring):
        tag = (g.id, c.name)
        assert set(np.unique(c.mask)) == {0, 1} and set(np.unique(c.area)) == {0, 255}
        fg = c.area != 0
        opened = O.morph_open5(fg)
        lab, n = ndimage.label(opened, structure=LC.EIGHT)
        assert n == ndimage.label(fg, structure=LC.EIGHT)[1], (tag, "the opening removed or split a component")
        for sl in ndimage.find_objects(lab):
            assert sl[0].stop - sl[0].start >= 5 and sl[1].stop - sl[1].start >= 5, (tag, sl)
        e = LC.expected_capacity(c.mask, c.area, GC.MAX_MARKERS)
        assert not e["over"], (tag, e)
        assert e["holes"] == (1 if c.name == "ring" else 0), (tag, e)
        markers = O.marker_center(c.mask, c.area)
        assert len(markers) >= 7, (tag, len(markers))
        _rim_markers(markers, g, 16)
    fg = rim.area != 0
    lab, _ = ndimage.label(fg, structure=LC.EIGHT)
    # a component in each corner (the large one may hold the last), one on the last row only, one on the last column only
    assert fg[0, 0] and fg[0, -1] and fg[-1, 0] and fg[-1, -1]
    for line, others in ((lab[-1], (lab[0], lab[:, 0], lab[:, -1])), (lab[:, -1], (lab[0], lab[-1], lab[:, 0]))):
        only = set(np.unique(line)) - {0}
        for o in others:
            only -= set(np.unique(o))
        assert only, (g.id, "no component touches that border alone")
    placed = dict(rim.claims["placed"])
    cx, cy = placed["large"]
    assert cx >= 0.75 * w and cy >= 0.75 * h
    big = lab == lab[int(cy), int(cx)]
    ys, xs = np.nonzero(big.any(axis=1))[0], np.nonzero(big.any(axis=0))[0]
    r768 = LC.stage_tile_rows(h, w, 768)
    assert xs[-1] // 64 - xs[0] // 64 >= 1 and (h < 128 or ys[-1] // r768 - ys[0] // r768 >= 2), (g.id, ys[[0, -1]], xs[[0, -1]])
    tx, ty, at = placed["tall"]
    col = lab[:, tx]
    rows = np.nonzero(col == col[ty])[0]
    assert rows[-1] // r768 - rows[0] // r768 >= 3, (g.id, rows[[0, -1]], r768)
    r128 = 128 in (r768, LC.stage_tile_rows(h, w, 256))
    assert r128 == ("tile_blob" in placed) == (g.case in ("8", "10", "12"))
    if r128:
        x0, y0 = placed["tile_blob"]
        blob = lab == lab[y0 + 64, x0 + 32]
        ys, xs = np.nonzero(blob.any(axis=1))[0], np.nonzero(blob.any(axis=0))[0]
        assert y0 % 128 == 0 and ys[0] < y0 and ys[-1] >= y0 + 128               # every row of the tile, and into both neighbours
        assert blob[y0:y0 + 128].any(axis=1).all()
        assert xs[0] // 64 == xs[-1] // 64 == x0 // 64                           # in one column of words
    (ry, rx), = [p for name, p in ring.claims["placed"] if name == "ring"]
    assert ring.area[ry, rx] == 0 and ring.area[ry, rx + LC.RO - 2] == 255 and ring.mask[ry, rx] == 1
