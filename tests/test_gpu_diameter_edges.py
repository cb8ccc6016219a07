"""GPU tests of the marker diameter validation on RAGGED masks (k_diameter.hip; `pytest -m gpu` on an MI355X): the device
against the sequential helper, with the comparisons of tests/helpers/diameter_check.py and nothing weaker - integers, mask bits,
order, pixel counts and boxes exact, the circle rebuilt from the reported support points in fractions and equal to the exact
minimum, float64 columns and statistics within 1e-12 relative.

The inputs come from tests/helpers/diameter_edge_cases.py: noise whose thresholded mask holds 1-px lines, diagonal necks, spurs,
single pixels and components inside each other's bounding boxes; hand-made lines on the word seams and the image border;
interleaved boxes cut mid-run; boxes of exactly VBS_DIAM_MAX_EXTENT and one more; 512 / 513 and max_markers / max_markers + 1
components.  tests/test_diameter_edges_host.py states on the CPU what those frames contain.
"""
import contextlib
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
import diameter_edge_cases as E                               # noqa: E402
import diameter_oracle as D                                   # noqa: E402
from diameter_check import check_frame, run                   # noqa: E402

SCALE = 12.5
_engines = {}


def engine(h, w, max_markers=512, max_batch=4):
    """One engine per geometry and limits for the whole module."""
    from vbs_amd.engine import Engine
    key = (h, w, max_markers, max_batch)
    if key not in _engines:
        _engines[key] = Engine(h, w, max_markers=max_markers, max_batch=max_batch)
    return _engines[key]


@contextlib.contextmanager
def level(thr):
    """`check_frame`, `helper_frame` and `run` read the threshold from the case module."""
    old = K.THRESHOLD
    K.THRESHOLD = thr
    try:
        yield
    finally:
        K.THRESHOLD = old


def groups():
    """The noise and thin-line frames by (H, W, threshold): one batch each."""
    g = {}
    for name, gray, thr in E.noise_cases() + E.small_noise_cases():
        g.setdefault((*gray.shape, thr), []).append((name, gray))
    for name, gray, thr, _ in E.line_frames():
        g.setdefault((*gray.shape, thr), []).append(("lines-" + name, gray))
    return g


GROUPS = groups()
GROUP_IDS = [f"{h}x{w}-t{t}" for h, w, t in GROUPS]


def measure_group(key, min_area, min_circ, offset=0.0):
    """Run one group's frames as one call (several passes of max_batch = 4) and hold every frame to the helper."""
    h, w, thr = key
    frames = np.stack([g for _, g in GROUPS[key]])
    surv_all, rows = [], []
    with level(thr):
        rec, counts, stats, bits = run(engine(h, w), frames, SCALE, offset, min_area, min_circ)
        for i, (name, gray) in enumerate(GROUPS[key]):
            print(name, end=": ")
            assert counts[i] >= 0, (name, counts[i])
            surv = check_frame(gray, rec[i], int(counts[i]), stats[i], bits[i], SCALE, offset, min_area, min_circ)
            surv_all.append(surv)
            rows.append(rec[i, :counts[i]])
    return surv_all, rows


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_every_contour_survives(key):
    """min_area = min_circularity = -1: every component with a perimeter reaches k_diam_circle - lines (area 0), necks, spurs,
    two-point circles, collinear and duplicated candidates, one-row components.  A single pixel (perimeter 0) never appears."""
    surv_all, rows = measure_group(key, *E.EVERY)
    ns = np.concatenate([r[:, 10] for r in rows]).astype(int)
    print(f"{GROUP_IDS[list(GROUPS).index(key)]}: {len(ns)} circles, {int((ns == 2).sum())} on two points, "
          f"{int((ns == 3).sum())} on three")
    assert (ns == 2).any() and (ns == 3).any() and not (ns == 1).any()
    for (name, gray), surv, r in zip(GROUPS[key], surv_all, rows):
        mask = E.mask_of(gray, key[2])
        allc = D.contours_of(mask)
        assert len(surv) == sum(1 for c in allc if c["perimeter"] > 0), name
        assert (r[:, 17] >= 2).all() and (r[:, 5] > 0).all(), name             # pixel count, perimeter
        if not name.startswith("lines-"):
            assert any(c["area2"] == 0 for c in surv), name                      # a line went through the circle
        one_row = [c for c in surv if len({y for _, y in c["chain"]}) == 1]
        if name.startswith(("sparse", "lines-horizontal")):
            assert one_row, name                                                 # a component of a single row


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_mid_filters(key):
    """min_area = 20.25 (areas are multiples of 1/2: no tie), min_circularity = 0.3: long alternating runs of rejected and
    surviving components - the count, the descending-id order and the rank compaction."""
    surv_all, rows = measure_group(key, *E.MID, offset=-0.03)
    kept = rejected = switches = 0
    for (name, gray), surv in zip(GROUPS[key], surv_all):
        allc = D.contours_of(E.mask_of(gray, key[2]))
        firsts = {c["first"] for c in surv}
        flags = [c["first"] in firsts for c in allc]
        kept += sum(flags)
        rejected += len(flags) - sum(flags)
        switches += sum(a != b for a, b in zip(flags, flags[1:]))
    print(f"{kept} kept, {rejected} rejected, {switches} changes between the two along the contour order")
    if key[2] == 127 and key[:2] in E.GEOMS:                  # (the specks of the sparse frames are nearly all under 20.25 px)
        assert kept >= 10 and rejected >= 10 and switches >= 10
    assert rejected > 0


@pytest.mark.parametrize("filt", [E.EVERY, E.MID], ids=["every", "mid"])
def test_interleaved_boxes(filt):
    """Components whose bounding box holds runs of another component, cut mid-run by x0 / x1 on a word seam: check_frame, and
    directly - the circle rebuilt from the reported support points is the exact circle of the component's OWN pixels, and where
    the foreign pixels inside the box would change the circle (the '+'), it is not the union's."""
    cases = E.interleaved_frames()
    h, w = cases[0][1].shape
    with level(E.SHAPE_THRESHOLD):
        rec, counts, stats, bits = run(engine(h, w), np.stack([g for _, g, _, _ in cases]), SCALE, 0.0, *filt)
        told_apart = 0
        for i, (name, gray, thr, boxes) in enumerate(cases):
            print(name, end=": ")
            surv = check_frame(gray, rec[i], int(counts[i]), stats[i], bits[i], SCALE, 0.0, *filt)
            comps = E.components(E.mask_of(gray, thr))
            assert filt != E.EVERY or len(surv) == len(boxes)
            for r, c in zip(rec[i], surv):
                comp = comps[c["first"]]
                ns = int(r[10])
                circle = D.circle_through([(int(r[11 + 2 * k]), int(r[12 + 2 * k])) for k in range(ns)])
                assert circle == D.exact_mec(comp["own"]), (name, c["first"])
                if comp["foreign"]:
                    union = D.exact_mec(comp["own"] + comp["foreign"])
                    if union != D.exact_mec(comp["own"]):
                        assert circle != union
                        told_apart += 1
    print(f"{told_apart} circles that the foreign pixels in their box would have changed")
    assert filt != E.EVERY or told_apart >= 1


def test_extent_at_the_limit_and_one_beyond():
    """A band whose box is exactly VBS_DIAM_MAX_EXTENT x VBS_DIAM_MAX_EXTENT is measured - all 1024 candidate slots in use; one
    of 513 x 300 and one of 300 x 513 get VBS_ECAPACITY and NaN statistics, in either order, and the frame next to them in the
    batch keeps its rows."""
    assert L.DIAM_MAX_EXTENT == 512
    ok, wide, tall = (E.band(n)[0] for n in ("at_limit", "wide", "tall"))
    h, w = E.EXTENT_GEOM
    eng = engine(h, w, max_batch=2)
    with level(E.SHAPE_THRESHOLD):
        rec, counts, stats, bits = run(eng, np.stack([ok, wide]), SCALE, 0.0, *E.EVERY)
        surv = check_frame(ok, rec[0], int(counts[0]), stats[0], bits[0], SCALE, 0.0, *E.EVERY)
        assert len(surv) == 2
        boxes = sorted((int(r[20] - r[18]) + 1, int(r[21] - r[19]) + 1) for r in rec[0, :2])
        assert boxes == [(10, 10), (512, 512)]
        assert counts[1] == L.VBS_ECAPACITY and stats[1][0] == 0 and all(math.isnan(v) for v in stats[1][1:])
        for pair in ((wide, ok), (tall, ok)):
            rec2, counts2, stats2, bits2 = run(eng, np.stack(pair), SCALE, 0.0, *E.EVERY)
            assert counts2[0] == L.VBS_ECAPACITY and stats2[0][0] == 0 and all(math.isnan(v) for v in stats2[0][1:])
            assert counts2[1] == 2 and np.array_equal(rec2[1, :2].view(np.int64), rec[0, :2].view(np.int64))
            assert np.array_equal(stats2[1].view(np.int64), stats[0].view(np.int64)) and np.array_equal(bits2[1], bits[0])
        # with the default filters the band is rejected BEFORE the circle: its extent does not count
        rec3, counts3, stats3, bits3 = run(eng, np.stack([wide, tall]), SCALE)
        for i, g in enumerate((wide, tall)):
            assert len(check_frame(g, rec3[i], int(counts3[i]), stats3[i], bits3[i], SCALE)) == 0


@pytest.mark.parametrize("max_markers,at,over", [(1024, 512, 513), (64, 64, 65)], ids=["512-components", "max_markers-64"])
def test_component_limits(max_markers, at, over):
    """Exactly CCL_OPEN_COMPS = 512 components (max_markers = 1024) and exactly max_markers = 64 are measured; one more is
    reported as VBS_ECAPACITY with NaN statistics.  The reported frame sits between two measured ones, which keep their rows."""
    h, w = E.DOT_GEOM
    first, second, third = E.dots(at)[0], E.dots(over)[0], E.dots(64, 1)[0]
    eng = engine(h, w, max_markers=max_markers)
    with level(E.DOT_THRESHOLD):
        rec, counts, stats, bits = run(eng, np.stack([first, second, third, second, first]), SCALE, 0.0, *E.EVERY)
        assert list(counts) == [at, L.VBS_ECAPACITY, 64, L.VBS_ECAPACITY, at]
        for i in (1, 3):
            assert stats[i][0] == 0 and all(math.isnan(v) for v in stats[i][1:])
        assert len(check_frame(first, rec[0], int(counts[0]), stats[0], bits[0], SCALE, 0.0, *E.EVERY)) == at
        assert len(check_frame(third, rec[2], int(counts[2]), stats[2], bits[2], SCALE, 0.0, *E.EVERY)) == 64
        assert np.array_equal(rec[4, :at].view(np.int64), rec[0, :at].view(np.int64))           # a second pass of the batch
        assert np.array_equal(stats[4].view(np.int64), stats[0].view(np.int64))
        alone, counts1, stats1, _ = run(eng, np.stack([first]), SCALE, 0.0, *E.EVERY)
        assert counts1[0] == at and np.array_equal(alone[0, :at].view(np.int64), rec[0, :at].view(np.int64))


def test_nine_frames_through_a_batch_of_four_twice_and_alone():
    """Three passes, the last one short: every frame against the helper, the same bits in a second run, and every frame run
    alone equal to its rows in the batch."""
    key = (*E.GEOMS[0], 127)
    cases = GROUPS[key]
    assert len(cases) == 9
    frames = np.stack([g for _, g in cases])
    eng = engine(*E.GEOMS[0])
    assert eng.max_batch == 4
    with level(127):
        rec, counts, stats, bits = run(eng, frames, SCALE, 0.02, *E.EVERY)
        rec2, counts2, stats2, bits2 = run(eng, frames, SCALE, 0.02, *E.EVERY)
        assert np.array_equal(counts, counts2) and np.array_equal(stats.view(np.int64), stats2.view(np.int64))
        assert np.array_equal(bits, bits2) and (counts > 5).all()
        for i, (name, gray) in enumerate(cases):
            n = counts[i]
            check_frame(gray, rec[i], int(n), stats[i], bits[i], SCALE, 0.02, *E.EVERY)
            assert np.array_equal(rec[i, :n].view(np.int64), rec2[i, :n].view(np.int64)), name
            r1, c1, s1, b1 = run(eng, frames[i:i + 1], SCALE, 0.02, *E.EVERY)
            assert c1[0] == n and np.array_equal(r1[0, :n].view(np.int64), rec[i, :n].view(np.int64)), name
            assert np.array_equal(s1[0].view(np.int64), stats[i].view(np.int64)) and np.array_equal(b1[0], bits[i]), name


def test_noise_as_a_strided_crop_view_and_as_bgr():
    from oracle import stages as O
    h, w = E.GEOMS[0]
    eng = engine(h, w)
    a, b = E.noise("white", E.GEOMS[0], 0)[0], E.noise("binary", E.GEOMS[0], 0)[0]
    with level(127):
        wide = np.full((2, h + 9, w + 70), 255, np.uint8)         # a crop VIEW: row and frame strides of the wider tensor
        wide[0, 4:4 + h, 35:35 + w], wide[1, 4:4 + h, 35:35 + w] = a, b
        ft = torch.from_numpy(wide).to(eng.device)[:, 4:4 + h, 35:35 + w]
        assert not ft.is_contiguous()
        rec, counts, stats = eng.measure_markers(ft, 127, SCALE, *E.EVERY)
        bits = eng.threshold_bits(ft, 127)
        torch.cuda.synchronize()
        for i, g in enumerate((a, b)):
            check_frame(g, rec[i].cpu().numpy(), int(counts[i]), stats[i].cpu().numpy(), bits[i].cpu().numpy(), SCALE, 0.0,
                        *E.EVERY)
        f = np.stack([K.to_bgr(a, 60), K.to_bgr(b, 61)])
        rec, counts, stats, bits = run(eng, f, SCALE, 0.0, *E.MID)
        for i in range(2):
            check_frame(O.bgr2gray(f[i]), rec[i], int(counts[i]), stats[i], bits[i], SCALE, 0.0, *E.MID)


@pytest.mark.parametrize("geom", E.GEOMS + (E.SMALLEST,), ids=lambda g: f"{g[0]}x{g[1]}")
def test_threshold_bits_on_noise(geom):
    """Every pixel of the reflect-101 border matters on white noise; thresholds 0 and 255 give all-clear and all-set words (the
    bits beyond the width stay clear)."""
    seeds = E.SEEDS["white"] if geom != E.SMALLEST else (0,)
    frames = np.stack([E.noise("white", geom, s)[0] for s in seeds])
    eng = engine(*geom)
    ft = torch.from_numpy(frames).to(eng.device)
    for thr in (0, 127, 254.5, 255):
        bits = eng.threshold_bits(ft, thr).cpu().numpy().view(np.uint64)
        want = np.stack([D.pack_bits(D.threshold_inv(D.blur5_u8(g), thr)) for g in frames])
        assert np.array_equal(bits, want), thr
        if thr == 0:
            assert not want.any()
        if thr == 255:
            assert np.array_equal(want, np.stack([D.pack_bits(np.ones(geom, bool))] * len(frames)))
