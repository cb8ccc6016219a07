"""Conditions on the inputs of tests/test_gpu_diameter_edges.py, checked with the helper alone (no GPU): they keep the GPU tests
from passing on frames that lost their edges.  Conditions, not measurements: each states what a frame must contain, and the seeds
and drawings in tests/helpers/diameter_edge_cases.py were chosen so that it does.

Not every kind of noise can meet every condition: 2 x 2 blocks blurred and thresholded leave no single pixel, so the `coarse`
frames are only asked for a line and an interleaved box; `sparse` specks are too small to lie in each other's boxes often, so
the five interleaved components are asked of `white` and `binary` alone."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import diameter_edge_cases as E                               # noqa: E402
import diameter_oracle as D                                   # noqa: E402

MAX_EXTENT = 512                                              # VBS_DIAM_MAX_EXTENT (test_diameter_host.py ties it to the header)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_CAP = int(re.search(r"#define\s+VBS_RUN_CAP\s+(\d+)",     # the labelling kernel's: runs per mask and frame,
                        open(os.path.join(ROOT, "vision-basedsensor_amd", "csrc", "common.h")).read()).group(1))
BACKGROUND_CAP = 1024                                         # ... and components of the background (k_label.hip)


@functools.lru_cache(maxsize=None)
def facts(name, max_markers):
    gray, thr = next((g, t) for n, g, t, m in E.measured_frames() if (n, m) == (name, max_markers))
    mask = E.mask_of(gray, thr)
    return mask, D.contours_of(mask), E.components(mask)


def counts(name, max_markers=512):
    _, allc, comps = facts(name, max_markers)
    return dict(n=len(allc), interleaved=sum(1 for c in comps.values() if c["foreign"]),
                lines=sum(1 for c in allc if c["area2"] == 0 and c["perimeter"] > 0),
                single=sum(1 for c in allc if c["perimeter"] == 0))


NOISE = [n for n, _, _ in E.noise_cases() + E.small_noise_cases()]


def test_neighbourhood_codes_reached():
    codes, noise_codes = set(), set()
    for name, gray, thr, m in E.measured_frames():
        c = E.neighbourhood_codes(facts(name, m)[0])
        codes |= c
        if name in NOISE:
            noise_codes |= c
    print(f"8-neighbourhood codes on foreground pixels: {len(noise_codes)} of 256 over the noise frames, {len(codes)} with the "
          f"hand-made frames")
    assert len(codes) >= 200


@pytest.mark.parametrize("name", NOISE)
def test_noise_frames_keep_their_edges(name):
    c = counts(name)
    print(name, c)
    kind = name.split("-")[0]
    assert c["lines"] >= 1                                    # area2 == 0 with a perimeter
    if kind != "coarse":
        assert c["single"] >= 1                               # perimeter == 0: never a survivor
    if kind in ("white", "binary"):
        assert c["interleaved"] >= 5
    if kind == "coarse":
        assert c["interleaved"] >= 1


def test_line_frames():
    frames = {n: (g, t, d) for n, g, t, d in E.line_frames()}
    H, W = E.GEOMS[1]
    for name in ("horizontal", "vertical"):
        mask, allc, _ = facts("lines-" + name, 512)
        assert np.array_equal(mask, frames[name][2])          # one pixel wide, as drawn
        assert len(allc) == (10 if name == "horizontal" else 7)
        for c in allc:                                        # every pixel but the ends is visited twice
            assert (c["area2"], c["n_diag"]) == (0, 0) and c["n_axis"] >= 6
        assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()
        for a, b in ((63, 64), (127, 128)):
            if name == "horizontal":
                assert (mask[:, a] & mask[:, b]).sum() >= 3       # runs that cross the word seam
                assert (mask[:, a] & ~mask[:, b]).any() and (~mask[:, a] & mask[:, b]).any()   # ... end at it, start at it
            else:
                assert mask[:, a].sum() >= 20 and mask[:, b].sum() >= 20
    mask, allc, _ = facts("lines-diagonal", 512)
    pure = [c for c in allc if (c["area2"], c["n_axis"]) == (0, 0) and c["n_diag"] > 0]
    assert len(allc) == 5 and len(pure) == 3
    assert mask[0, 0] and mask[0, W - 1] and mask[-1].sum() >= 2 and mask[:, 0].any() and mask[:, -1].any()
    d = mask[1:, 1:] & mask[:-1, :-1] & ~mask[1:, :-1] & ~mask[:-1, 1:]      # diagonal necks (x, y) - (x + 1, y + 1)
    a = mask[1:, :-1] & mask[:-1, 1:] & ~mask[1:, 1:] & ~mask[:-1, :-1]      # ... and (x + 1, y) - (x, y + 1)
    assert d[:, 63].any() and d[:, 127].any() and a[:, 63].any() and a[:, 127].any()      # each way across both seams


def test_interleaved_frames():
    for name, gray, thr, boxes in E.interleaved_frames():
        mask, allc, comps = facts("boxes-" + name, 512)
        assert sorted(c["box"] for c in comps.values()) == sorted(boxes.values())
        lab, _ = D.component_pixels(mask)
        for c in comps.values():
            x0, y0, x1, y1 = c["box"]
            if c["box"] in (boxes.get("c_right"), boxes.get("plus")):
                assert x0 & 63 == 0 and x1 & 63 == 63
                # a run of another component cut mid-run by x1: it goes on beyond the box
                assert any(mask[y, x1] and mask[y, x1 + 1] and lab[y, x1] != lab[c["own"][0][1], c["own"][0][0]]
                           for y in range(y0, y1 + 1))
            if c["box"] in (boxes.get("c_left"), boxes.get("plus")):
                assert x0 & 63 == 0                           # ... and by x0: node_of walks back into the word before
                assert any(mask[y, x0] and mask[y, x0 - 1] and lab[y, x0] != lab[c["own"][0][1], c["own"][0][0]]
                           for y in range(y0, y1 + 1))
        assert sum(1 for c in comps.values() if c["foreign"]) >= 1
    # the '+': foreign pixels inside its box lie outside its circle, so taking them as candidates would change the circle
    _, _, comps = facts("boxes-plus", 512)
    plus = next(c for c in comps.values() if c["box"] == (64, 10, 127, 86))
    assert D.exact_mec(plus["own"] + plus["foreign"])[2] > D.exact_mec(plus["own"])[2]


def test_bands_and_dot_grids():
    for name, (_, (bw, bh)) in E.BANDS.items():
        comps = E.components(E.mask_of(*E.band(name)))
        ext = sorted((c["box"][2] - c["box"][0] + 1, c["box"][3] - c["box"][1] + 1) for c in comps.values())
        assert ext == [(10, 10), (bw, bh)], (name, ext)
    assert E.BANDS["at_limit"][1] == (MAX_EXTENT, MAX_EXTENT)
    assert E.BANDS["wide"][1][0] == MAX_EXTENT + 1 and E.BANDS["tall"][1][1] == MAX_EXTENT + 1
    for n in (512, 513, 64, 65):
        allc = D.contours_of(E.mask_of(*E.dots(n)))
        assert len(allc) == n
        assert {(c["area2"], c["n_axis"], c["n_diag"]) for c in allc} == {(-2, 4, 0), (-8, 8, 0)}     # 2 x 2 and 3 x 3
    assert len(D.contours_of(E.mask_of(*E.dots(64, 1)))) == 64
    assert not np.array_equal(E.dots(64)[0], E.dots(64, 1)[0])


def test_no_decision_sits_on_a_filter_boundary_and_measured_frames_fit():
    """The rule `diameter_check.helper_frame` enforces, for both filter settings of the GPU tests; and no frame meant to be
    measured exceeds the extent, the component limits of its engine or the labelling kernel's capacities."""
    for name, gray, thr, max_markers in E.measured_frames():
        mask, allc, comps = facts(name, max_markers)
        for min_area, min_circ in (E.EVERY, E.MID):
            for c in allc:
                assert abs(c["circularity"] - min_circ) > 1e-9 and c["area"] != min_area, (name, c["first"])
        assert len(allc) <= min(max_markers, 512), name
        assert max(max(c["box"][2] - c["box"][0], c["box"][3] - c["box"][1]) + 1 for c in comps.values()) <= MAX_EXTENT, name
        fg_runs, bg_runs, bg_comps = E.capacity(mask)
        assert max(fg_runs, bg_runs) <= RUN_CAP and bg_comps <= BACKGROUND_CAP, name
