"""CPU tests (no GPU) of the tiling k_stage gives one frame: `vbs_stage_box_geom` exports the very function the kernel calls
(`stage_box_geom`, csrc/stage_common.h) once its pre-scan knows the bounding box of the frame's set bits.  Held here, for
ns = 14 and 8 and for 256 and 768 threads, over boxes at every kind of position: the lanes of a wave hold the row blocks, the
row blocks cover the box's rows, every box pixel dilated by the stencil's reach lies in the window of word columns or at a
true image border, the tiles never get taller than the full-frame ones nor shorter than half of them, the last-row tables
(one entry per tile) never hold more than one entry per thread, and a box that gains nothing gives the full-frame tiling."""
import ctypes as C
import itertools

import pytest

import vbs_amd._lib as L

# width -> words per row: 3, 5, 8, 20, 30, 64 (190 and 1900 are no multiples of 64)
WIDTHS = [190, 320, 512, 1280, 1900, 4096]
HEIGHTS = {190: (484, 100), 320: (600, 480), 512: (481, 450), 1280: (1024,), 1900: (1200,), 4096: (500, 130)}


def geom(h, w, ns, nt, box):
    out = (C.c_int * 12)()
    rc = L.lib().vbs_stage_box_geom(h, w, ns, nt, box[0], box[1], box[2], box[3], out)
    assert rc == L.VBS_OK, (rc, h, w, ns, nt, box)
    full = dict(zip(("WW", "G", "NB", "R"), out[0:4]))
    own = dict(zip(("ja", "WW", "G", "NB", "R", "ylo"), out[4:10]))
    return full, own, out[10], bool(out[11])


def x_edges(w, guard):
    """pixel columns around every word edge that matters: the edge itself +- (guard + 1), and the image borders; for wide
    frames only the first two, the middle and the last two word edges"""
    ww = (w + 63) // 64
    words = range(ww + 1) if ww <= 8 else sorted({0, 1, 2, ww // 2, ww - 2, ww - 1, ww})
    xs = {0, w - 1}
    for e in words:
        for d in (-guard - 1, -guard, -guard + 1, 0, guard - 1, guard, guard + 1):
            for x in (64 * e + d, 64 * e - 1 + d):
                if 0 <= x < w:
                    xs.add(x)
    return sorted(xs)


def y_ranges(h):
    return [(0, 0), (0, h - 1), (h - 1, h - 1), (h // 3, 2 * h // 3), (5, h - 7), (h // 2, h - 1)]


def restated(h, w, nt, guard, full, box):
    """the issue's formulas, restated"""
    xlo, xhi, ylo, yhi = box
    same = dict(ja=0, WW=full["WW"], G=full["G"], NB=full["NB"], R=full["R"], ylo=0)
    if xlo > xhi or ylo > yhi:
        return same
    ja, jb = max(xlo - guard, 0) >> 6, min(xhi + guard, w - 1) >> 6
    wwe = jb - ja + 1
    g = 64 // wwe
    nb = (nt // 64) * g
    r = max(-(-(yhi - ylo + 1) // nb), (full["R"] + 1) // 2)        # never below half the full-frame rows per tile
    return dict(ja=ja, WW=wwe, G=g, NB=nb, R=r, ylo=ylo) if r < full["R"] else same


@pytest.mark.parametrize("nt", [256, 768])
@pytest.mark.parametrize("ns", [14, 8])
@pytest.mark.parametrize("w", WIDTHS)
def test_every_box_position_gives_a_sound_tiling(w, ns, nt):
    guard = ns // 2
    boxed_any = fallback_any = 0
    rows_per_tile = []
    for h in HEIGHTS[w]:
        ww = (w + 63) // 64
        nb_full = (nt // 64) * (64 // ww)
        if -(-h // nb_full) > 128:                            # outside the fused path: the export says so
            out = (C.c_int * 12)()
            assert L.lib().vbs_stage_box_geom(h, w, ns, nt, 0, 0, 0, 0, out) == L.VBS_EINVAL
            continue
        rows_per_tile.append(-(-h // nb_full))
        xs = x_edges(w, guard)
        for (xlo, xhi), (ylo, yhi) in itertools.product(itertools.combinations_with_replacement(xs, 2), y_ranges(h)):
            box = (xlo, xhi, ylo, yhi)
            full, own, gd, boxed = geom(h, w, ns, nt, box)
            assert gd == guard
            assert (full["WW"], full["G"], full["NB"], full["R"]) == (ww, 64 // ww, nb_full, -(-h // nb_full))
            assert own == restated(h, w, nt, guard, full, box), box
            assert own["G"] * own["WW"] <= 64 and own["G"] >= 1
            assert own["NB"] == (nt // 64) * own["G"]
            assert own["NB"] * own["WW"] <= nt                                   # the last-row tables: one entry per tile
            assert 1 <= own["R"] <= full["R"]
            assert own["NB"] * own["R"] >= yhi - own["ylo"] + 1 and own["ylo"] <= ylo    # the row blocks cover the box's rows
            # every box pixel dilated by the guard lies in words ja .. ja + WW - 1, or is cut by a true image border
            assert 64 * own["ja"] <= max(xlo - guard, 0) and 64 * (own["ja"] + own["WW"]) - 1 >= min(xhi + guard, w - 1), box
            assert 0 <= own["ja"] and own["ja"] + own["WW"] <= ww
            if boxed:
                boxed_any += 1
                assert own["ylo"] == ylo and own["R"] < full["R"] and 2 * own["R"] >= full["R"]
            else:
                fallback_any += 1
                assert own == dict(ja=0, WW=ww, G=full["G"], NB=full["NB"], R=full["R"], ylo=0)
    if not rows_per_tile:                                     # (1900x1200 on 256 threads: 150 rows per tile, not the kernel's)
        return
    assert fallback_any > 0
    if max(rows_per_tile) >= 2:                               # (tiles of one row have nothing to gain)
        assert boxed_any > 0


@pytest.mark.parametrize("nt", [256, 768])
@pytest.mark.parametrize("ns", [14, 8])
def test_empty_full_and_one_pixel_frames(ns, nt):
    h, w = 1024, 1280
    full, own, _, boxed = geom(h, w, ns, nt, (0x7FFFFFFF, -1, 0x7FFFFFFF, -1))        # what the kernel's pre-scan leaves of an empty frame
    assert not boxed and own == dict(ja=0, WW=20, G=3, NB=full["NB"], R=full["R"], ylo=0)
    full, own, _, boxed = geom(h, w, ns, nt, (0, w - 1, 0, h - 1))
    assert not boxed and own == dict(ja=0, WW=20, G=3, NB=full["NB"], R=full["R"], ylo=0)
    for x, y in ((0, 0), (w - 1, h - 1), (640, 512), (63, 7), (64, 1000)):
        full, own, guard, boxed = geom(h, w, ns, nt, (x, x, y, y))
        assert boxed and own["ylo"] == y and own["R"] == (full["R"] + 1) // 2
        assert own["ja"] == max(x - guard, 0) >> 6 and own["ja"] + own["WW"] - 1 == min(x + guard, w - 1) >> 6


def test_the_headline_workloads_tile_as_the_design_says():
    """1280x1024, 13x13 dots (columns 178..1103, rows 50..975) on 256 threads: 16 words, four row blocks per wave, 58 rows per
    tile instead of 86; 1920x1200 (columns 373..1548, rows 15..1186) on 768 threads: 20 words, 33 rows instead of 50"""
    full, own, _, boxed = geom(1024, 1280, 14, 256, (178, 1103, 50, 975))
    assert boxed and (full["G"], full["NB"], full["R"]) == (3, 12, 86)
    assert own == dict(ja=2, WW=16, G=4, NB=16, R=58, ylo=50)
    full, own, _, boxed = geom(1200, 1920, 14, 768, (373, 1548, 15, 1186))
    assert boxed and (full["G"], full["NB"], full["R"]) == (2, 24, 50)
    assert own == dict(ja=5, WW=20, G=3, NB=36, R=33, ylo=15)


def test_arguments_outside_the_kernel_are_refused():
    out = (C.c_int * 12)()
    f = L.lib().vbs_stage_box_geom
    assert f(1024, 1280, 14, 256, 0, 0, 0, 0, None) == L.VBS_EINVAL
    assert f(1024, 1280, 10, 256, 0, 0, 0, 0, out) == L.VBS_EINVAL
    assert f(1024, 1280, 14, 512, 0, 0, 0, 0, out) == L.VBS_EINVAL
    assert f(1024, 4160, 14, 768, 0, 0, 0, 0, out) == L.VBS_EINVAL
    assert f(2048, 4096, 14, 768, 0, 0, 0, 0, out) == L.VBS_EINVAL             # 171 rows per tile: more than the row masks hold
