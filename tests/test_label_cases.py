"""The labelling case generator (tests/helpers/label_cases.py) makes what each class claims - CPU only."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import label_cases as LC                                      # noqa: E402
from oracle import stages as O                                # noqa: E402

GEOMETRIES = [(64, 128), (300, 200), (450, 480), (480, 640), (481, 136), (700, 1003), (1024, 1280), (1200, 1920), (130, 4096)]


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_cases_have_the_properties_their_class_claims(h, w):
    cases = LC.label_cases(h, w)
    assert {c.cls for c in cases} == {"ragged", "holes", "matching", "overflow"}
    for c in cases:
        assert c.mask.shape == c.area.shape == (h, w) and c.mask.dtype == c.area.dtype == np.uint8
        assert set(np.unique(c.mask)) <= {0, 1} and set(np.unique(c.area)) <= {0, 255}, c.name
        assert c.mask.any(), c.name
        opened = O.morph_open5(c.area != 0)
        _, nb = LC.bounded_background(opened)
        assert LC.holes(opened) == nb, c.name                # Euler number against labelling the complement
        e = LC.expected_capacity(c.mask, c.area, 1024)
        assert e["contours"] == len(O.find_contours_external(opened)), c.name
        assert not LC.expected_capacity(c.mask, c.area, 1024)["over"], c.name
        if c.cls == "ragged":
            for edge in (c.area[0], c.area[-1], c.area[:, 0], c.area[:, -1]):
                assert edge.any(), c.name                    # cut by every border
        if c.cls == "holes":
            assert nb == c.claims["holes"] and (nb > 0 or c.name == "holes_cut"), (c.name, nb, c.claims["holes"])
            lab8, _ = ndimage.label(opened, structure=LC.EIGHT)
            for (y, x) in c.claims["nested"]:                # the nested blob survives the opening, as its own component
                assert opened[y, x] and (lab8 == lab8[y, x]).sum() >= 25, (c.name, y, x)
            bg8, _ = ndimage.label(~opened, structure=LC.EIGHT)
            holes4, _ = LC.bounded_background(opened)
            for (iy, ix, oy, ox) in c.claims["diagonal"]:    # a hole (4-connected), yet 8-connected to the outside
                assert holes4[iy, ix] > 0 and holes4[oy, ox] == 0 and not opened[oy, ox]
                assert bg8[iy, ix] == bg8[0, 0] == bg8[oy, ox]
        if c.name == "holes_cut":
            assert any(n.startswith("cut_bottom") for (n, _, _) in c.claims["placed"])
        if c.cls == "overflow":                              # more opened runs in one row of one word than 3 slots
            op = opened[:, :64]
            assert max(LC.runs(op[y:y + 1]) for y in range(h)) > 3
        if c.cls == "matching":
            assert {"radius_in", "radius_out", "poly_edge"} <= set(c.claims["kinds"]), c.claims["kinds"]
    names = [n for c in cases if c.cls == "holes" for (n, _, _) in c.claims["placed"]]
    assert "word_boundary" in names and "cut_bottom" in names
    if min(h, w) >= 130:
        assert {"double_nest", "diagonal_hole", "ring_blob"} <= set(names)


def test_matching_centres_sit_where_they_claim():
    """each matching centre is on the side of the (minor/10)^2 radius and of the polygon that its kind names."""
    c = [c for c in LC.label_cases(480, 640) if c.cls == "matching"][0]
    opened = O.morph_open5(c.area != 0)
    conts = O.find_contours_external(opened)
    assert set(c.claims["kinds"]) == {"radius_in", "radius_out", "poly_edge", "poly_out", "two_claims"}
    for kind, _, cl in c.claims["placed"]:
        x, y = cl["centre"]
        tests = []
        for cont in conts:
            (ex, ey), (a, b), _ = O.fit_ellipse(cont)
            r = ((x - ex) ** 2 + (y - ey) ** 2) / (min(a, b) / 10) ** 2
            tests.append((r, O.point_polygon_test(cont, (x, y))))
        near = min(tests)
        if kind == "radius_in":
            assert 0.85 <= near[0] < 1 and near[1] > 0
        elif kind == "radius_out":
            assert 1 <= near[0] <= 1.2 and near[1] > 0
        elif kind == "poly_edge":
            assert near[0] < 1 and near[1] == 0
        elif kind == "poly_out":
            assert near[0] < 1 and near[1] < 0
        else:
            assert sum(r < 1 for r, _ in tests) == 2 and sum(r < 1 and p >= 0 for r, p in tests) == 1


@pytest.mark.parametrize("h,w", [(480, 640), (1024, 1280)])
def test_crowded_cases_lie_on_their_side_of_each_limit(h, w):
    limits = {"band_comps": 1024, "open_comps": LC.OPEN_CAP, "band_runs": LC.RUN_CAP, "open_runs": LC.RUN_CAP}
    seen = set()
    for c in LC.crowded_cases(h, w, 1024):
        assert set(np.unique(c.mask)) <= {0, 1} and set(np.unique(c.area)) <= {0, 255}
        e = LC.expected_capacity(c.mask, c.area, 1024)
        if c.name == "mailbox":                              # ten band components, every centroid on one pixel
            centres, _, n = O.band_centroids(c.mask)
            assert n == 10 and (centres == centres[0]).all() and not e["over"]
            continue
        if c.name == "open_segs":                            # nine opened pieces start in a 7-row tile, <= 3 runs per row
            opened = O.morph_open5(c.area != 0)
            for (t, x0) in c.claims["tiles"]:
                tile = opened[t:t + 7, x0:x0 + 64]
                assert ndimage.label(tile, structure=LC.EIGHT)[1] == 9
                assert max(LC.runs(tile[y:y + 1]) for y in range(7)) <= 3
            assert not e["over"]
            continue
        lim, v = limits[c.claims["limit"]], e[c.claims["limit"]]
        if c.claims["over"]:
            assert v > lim and e["over"], (c.name, v)
        else:
            assert 0.85 * lim <= v <= lim and not e["over"], (c.name, v)
        seen.add((c.claims["limit"], c.claims["over"]))
    assert len(seen) == 8                                    # (the sparse frames repeat two limits)


def test_capacity_rule_counts():
    """the counting functions on hand-made masks: runs, Euler number and holes, the 512-contour and 30 720-run edges."""
    z = np.zeros((40, 70), bool)
    z[5, 3:9] = z[5, 11:12] = True
    assert LC.runs(z) == 2
    r = np.zeros((30, 30), bool); r[5:20, 5:20] = True; r[9:13, 9:13] = False
    assert LC.euler8(r) == 0 and LC.holes(r) == 1
    d = np.zeros((10, 10), bool); d[2, 2] = d[3, 3] = True      # diagonal neighbours: one 8-connected component
    assert LC.euler8(d) == 1 and LC.holes(d) == 0
    sq = np.zeros((400, 400), np.uint8)
    for k in range(LC.OPEN_CAP):
        y, x = 8 * (k // 40), 8 * (k % 40)
        sq[y + 2:y + 8, x + 2:x + 8] = 255
    e = LC.expected_capacity(np.zeros_like(sq), sq, 1024)
    assert e["open_comps"] == 512 and not e["over"]
    sq[392:398, 392:398] = 255
    assert LC.expected_capacity(np.zeros_like(sq), sq, 1024)["over"]
