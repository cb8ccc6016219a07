"""The pipeline against the CPU oracle (`oracle/stages.py`) at the rim of the frame-size envelope of `vbs_create`
(height >= 64, 128 <= width <= 4096, no upper bound on the height), where the frame size alone decides which kernels run.
Inputs and the launchers' rules restated: tests/helpers/geometry_cases.py (held to their conditions on the CPU by
tests/test_geometry_cases.py).  Tolerances: those of tests/helpers/markers.py - masks, counts and centroids exact, axes
within 1e-3 px, the angle within 0.05 degrees.  `ROUTES` and `_run` are those of tests/test_gpu_labelling_oracle.py.

Geometries (H x W), the limit each sits on and the kernels that ran there on an MI355X (front end | labelling):
   1   64 x  128  both minima, small branch, R = 1 (k_stage: most tiles lie outside the image)
                  k_blur_mfma, k_ncc_mfma | batch k_stage + k_stage_retry; one frame k_stage_lat (each followed by k_label)
   2   64 x 4096  minimum height at maximum width, WW = 64; k_blur16's tiles16 / 8 = 0 clamped to one segment
                  (BGR: k_gray) k_blur16 (the unaligned gray view: k_blur_mfma), k_ncc_mfma | k_stage + k_stage_retry;
                  k_stage_lat; masks on every route
   3  480 x 4096  last small-branch height: k_blur16, k_ncc_mfma | k_stage; k_stage_lat
   4  481 x 4096  first large-branch height (101 taps, NCC 80): (k_gray) k_blur16, k_ncc_mfma | k_stage; k_stage_lat
   4b 481 x 4092  the same with P != W: BGR frames take k_gray's 16-pixel vector pieces with a partial last piece at
                  column 4080 (the view that starts 3 bytes off: its scalar pieces and tail) instead of the flat path of
                  cases 2, 4 and 7: (k_gray) k_blur16, k_ncc_mfma | k_stage; k_stage_lat
   5  481 x  128  large branch in the narrowest frame (every NCC window leaves the image): k_blur_mfma, k_ncc_mfma | k_stage; k_stage_lat
   6 2048 x  128  last height the fast labelling routes accept: k_blur_mfma, k_ncc_mfma | k_stage; k_stage_lat; masks on every route
   7 2049 x  128  first height they all refuse, H % 16 == 1: (k_gray) k_blur_mfma, k_ncc_mfma | k_morph + k_label for every
                  frame: H * NC = 2049 < 65535, but k_ccl refuses H > 2048 as well.  Every forced route falls through to that.
   8  512 x 2112  R = 128 for k_stage's 256-thread instance (WW = 33, one row group per wave): masks on every route
   9  513 x 2112  the 256-thread instance refuses (R = 129), 768 takes over (R = 43): masks on every route
  10 1536 x 2112  R = 128 for the 768-thread instance: masks on every route
  11 1537 x 2112  k_stage refuses for R (129), not for H.  A batch pass takes round 2: k_morph, k_ccl_band + k_ccl_open
                  (H * NC = 1537 * 7 = 10 759 < 65535, so k_ccl runs), k_label.  k_stage_lat's own tile rule accepts this
                  frame (lat_geom: R = 25), so a pass of few frames runs k_stage_lat and k_label; "k_stage_lat did not
                  run" is asserted for the batch pass.
  12 1536 x 4096  R = 128 at WW = 64, the largest frame k_stage accepts: masks on fused, fused768, general
  13 2048 x 2112  k_stage_lat's tile rule (LT_ROWS = 6 rows aimed at, at most LT_CMAX = 16 workgroups of 4 waves): with
                  WW >= 33 a wave holds one row group, R = ceil(H / 64) from 361 rows on - 32 at 2048 rows, and 128 only at
                  8192.  Below 2049 rows the R limit never binds: the tallest frame k_stage_lat accepts at WW >= 33 is 2048
                  rows by the H rule, and "one row more" does not lie below 2048 (2049 rows: case 7).  Masks on `latency`
                  (k_stage_lat) and `fused` (k_stage refuses, R = 171: k_morph, k_ccl_band + k_ccl_open, k_label).

Pipeline passes of three frames are run twice: at the handle's defaults (VBS_OPT_LATENCY_FRAMES = 24: batch and single
frames all take the few-frames route) and with VBS_OPT_LATENCY_FRAMES = 1, which sends the batch to k_stage and a single
frame to k_stage_lat.  All of them must agree bit for bit.  On route `fused256` k_stage_retry (the second chance on 768
threads) is launched only behind a 256-thread k_stage: it ran at 512 x 2112 (R = 128) and not at 513 x 2112."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from oracle import stages as O                                # noqa: E402
from scipy import ndimage                                     # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import geometry_cases as GC                                   # noqa: E402
import label_cases as LC                                      # noqa: E402
from markers import compare_markers                           # noqa: E402
from test_gpu_labelling_oracle import ROUTES, _run            # noqa: E402

STAGE = {"k_stage", "k_stage_retry"}
CCL = {"k_ccl_band", "k_ccl_open"}
FUSED = {"fused", "fused768", "fused256", "latency"}


@pytest.fixture(scope="module")
def oracle():
    """(frames, [(mask, area, markers)]) per (geometry, kind), computed once."""
    made = {}

    def get(g, kind):
        if (g.id, kind) not in made:
            frames = GC.gray_frames(g.h, g.w) if kind == "gray" else GC.bgr_frames(g.h, g.w)
            want = []
            for f in frames:
                om, oa = O.find_markers(f)
                want.append((om, oa, O.marker_center(om, oa)))
            made[(g.id, kind)] = (frames, want)
        return made[(g.id, kind)]
    return get


@pytest.fixture(scope="module")
def mask_oracle():
    made = {}

    def get(g):
        if g.id not in made:
            cases = GC.mask_frames(g.h, g.w)
            for c in cases:
                c.expect = LC.expected_capacity(c.mask, c.area, GC.MAX_MARKERS)
                assert not c.expect["over"]
                c.want = O.marker_center(c.mask, c.area)
                c.bands = ndimage.label(O.band_mask(c.mask))[1]
            made[g.id] = cases
        return made[g.id]
    return get


def _profiled(eng, call):
    eng.profile(True)
    try:
        out = call()
        torch.cuda.synchronize()
        prof = eng.profile_read()
    finally:
        eng.profile(False)
    return out, {k for k, (cnt, _) in prof.items() if cnt > 0}


def _fallthrough(g):
    """(must, never) of a fused route whose launcher refuses the geometry (labelling.hip: round 2, or k_label alone)."""
    if GC.ccl_takes(g.h, g.w):
        return {"k_morph", "k_label"} | CCL, STAGE | {"k_stage_lat"}
    return {"k_morph", "k_label"}, STAGE | CCL | {"k_stage_lat"}


def _route_kernels(g, route):
    """(must run, must not run) for a `ROUTES` entry at this geometry: the table's own sets where the route's launcher
    accepts the frame by its rule, else what it falls through to."""
    takes = {"fused": GC.stage_takes(g.h, g.w), "fused768": GC.stage_takes(g.h, g.w), "fused256": GC.stage_takes(g.h, g.w),
             "latency": GC.lat_rows(g.h, g.w) is not None, "separate": GC.ccl_takes(g.h, g.w), "general": True}[route]
    if takes:
        return ROUTES[route][2], ROUTES[route][3]
    if route == "latency" and GC.stage_takes(g.h, g.w):
        return ROUTES["fused"][2], {"k_stage_lat"} | CCL
    return _fallthrough(g)


def _few_kernels(g):
    """a pass of few frames at the handle's defaults"""
    if GC.lat_rows(g.h, g.w) is not None:
        return {"k_stage_lat", "k_label"}, STAGE | CCL
    return _route_kernels(g, "latency")


def _batch_kernels(g):
    """a batch pass (more frames than VBS_OPT_LATENCY_FRAMES)"""
    if GC.stage_takes(g.h, g.w):
        return {"k_stage"}, CCL | {"k_stage_lat"}
    return _fallthrough(g)


PIPELINE = [(g, "gray") for g in GC.PIPELINE] + [(g, "bgr") for g in GC.BGR]


@pytest.mark.parametrize("g,kind", PIPELINE, ids=lambda v: v.id if isinstance(v, GC.Geometry) else v)
def test_pipeline_equals_the_oracle(g, kind, oracle):
    from vbs_amd.engine import Engine
    from vbs_amd.marker_detection import _det_to_markers
    h, w = g.h, g.w
    frames, want = oracle(g, kind)
    eng = Engine(h, w, max_markers=GC.MAX_MARKERS, max_batch=3)
    try:
        # 1: the front end on three frames at once
        ft = torch.from_numpy(frames).cuda()
        (mask, area), front = _profiled(eng, lambda: eng.find_markers(ft))
        stats = eng.frame_stats(3)
        print(g.id, kind, "front end:", sorted(front))
        for i, (om, oa, _) in enumerate(want):
            assert np.array_equal(area[i].cpu().numpy(), oa), (g.id, kind, i)
            assert np.array_equal(mask[i].cpu().numpy(), om), (g.id, kind, i)
            assert int(stats[i, 0]) == int((oa > 0).sum()) and int(stats[i, 1]) == 0, (g.id, kind, i, stats[i])
        assert ("k_blur16" in front) == GC.blur16_takes(h, w) and ("k_blur_mfma" in front) != GC.blur16_takes(h, w), sorted(front)
        assert ("k_gray" in front) == (kind == "bgr"), sorted(front)
        # 2: the same frames as a strided view of a buffer that starts an odd number of bytes to the left
        buf, cols = GC.padded(frames, left=3 if kind == "gray" else 1)
        view = torch.from_numpy(buf).cuda()[:, :, cols]
        assert (view.data_ptr() - view.untyped_storage().data_ptr()) % 2 == 1 and not view.is_contiguous()
        (m2, a2), front2 = _profiled(eng, lambda: eng.find_markers(view))
        print(g.id, kind, "front end, unaligned view:", sorted(front2))
        assert torch.equal(m2, mask) and torch.equal(a2, area)
        assert "k_blur16" not in front2 or kind == "bgr"      # (gray rows that do not load as aligned dwords: k_blur_mfma)
        # 3 + 4: detections of the batch and of each frame alone, and the route each pass took
        def detect(x):
            _, det, counts = eng.track_to_3d(x, None, want_det=True)
            return det.cpu().numpy(), counts.cpu().numpy()
        (det, counts), ran = _profiled(eng, lambda: detect(ft))
        print(g.id, kind, "few-frames pass of 3:", sorted(ran))
        must, never = _few_kernels(g)
        assert must <= ran and not (never & ran), (g.id, sorted(ran))
        for i, (_, _, markers) in enumerate(want):
            assert counts[i] >= 0, (g.id, kind, i, int(counts[i]))
            compare_markers(_det_to_markers(det[i], int(counts[i])), markers)
        for lat in (24, 1):
            eng.set_option(L.OPT_LATENCY_FRAMES, lat)
            for i in range(3):
                (d1, c1), ran1 = _profiled(eng, lambda: detect(ft[i:i + 1]))
                assert must <= ran1 and not (never & ran1), (g.id, lat, sorted(ran1))
                assert np.array_equal(d1[0], det[i]) and c1[0] == counts[i], (g.id, kind, lat, i)
        print(g.id, kind, "one frame:", sorted(ran1))
        (detb, countsb), ranb = _profiled(eng, lambda: detect(ft))          # VBS_OPT_LATENCY_FRAMES = 1: a batch pass
        print(g.id, kind, "batch pass of 3:", sorted(ranb))
        must, never = _batch_kernels(g)
        assert must <= ranb and not (never & ranb), (g.id, sorted(ranb))
        assert np.array_equal(detb, det) and np.array_equal(countsb, counts), (g.id, kind)
        # the coarse route assertions per case
        if g.case == "7":
            for r in (ran, ran1, ranb):
                assert "k_label" in r and not (r & (STAGE | CCL | {"k_stage_lat"})), sorted(r)
        elif g.case == "11":
            assert "k_label" in ranb and not (ranb & (STAGE | {"k_stage_lat"})), sorted(ranb)
            assert CCL <= ranb                                # (H * NC = 10 759: k_ccl takes the batch)
            assert "k_stage_lat" in ran and "k_stage_lat" in ran1          # (its own rule accepts: module docstring)
        else:
            assert "k_stage" in ranb and not (ranb & CCL), sorted(ranb)
            assert (GC.lat_rows(h, w) is not None) and "k_stage_lat" in ran1, sorted(ran1)
    finally:
        eng.close()


@pytest.mark.parametrize("g", GC.MASKS, ids=lambda g: g.id)
def test_masks_equal_the_oracle_on_the_routes(g, mask_oracle):
    from vbs_amd.engine import Engine
    from vbs_amd.marker_detection import _det_to_markers
    cases = mask_oracle(g)
    n = len(cases)
    eng = Engine(g.h, g.w, max_markers=GC.MAX_MARKERS, max_batch=n)
    try:
        mt = torch.from_numpy(np.stack([c.mask for c in cases])).cuda()
        at = torch.from_numpy(np.stack([c.area for c in cases])).cuda()

        def check(tag, det, counts, st):
            for i, c in enumerate(cases):
                assert counts[i] >= 0, (tag, c.name, int(counts[i]))
                compare_markers(_det_to_markers(det[i], int(counts[i])), c.want)
                assert int(st[i, 5]) == c.bands == c.expect["band_comps"], (tag, c.name, st[i])
                assert int(st[i, 6]) == c.expect["contours"], (tag, c.name, st[i])
                assert int(st[i, 7]) == c.expect["holes"], (tag, c.name, st[i])
                assert int(st[i, 4]) == 0, (tag, c.name, st[i])

        default = None
        if g.routes == ("default",):
            def call():
                det, counts = eng.marker_center(mt, at)
                return det.cpu().numpy(), counts.cpu().numpy()
            default, ran = _profiled(eng, call)
            print(g.id, "default:", sorted(ran))
            must, never = _few_kernels(g)
            assert must <= ran and not (never & ran), (g.id, sorted(ran))
            check((g.id, "default"), default[0], default[1], eng.frame_stats(n))
        for route in (ROUTES if default is not None else g.routes):
            det, counts, st, slow, prof = _run(eng, mt, at, route)
            ran = {k for k, (cnt, _) in prof.items() if cnt > 0}
            print(g.id, route, sorted(ran), "handed on:", [int(s) for s in slow])
            must, never = _route_kernels(g, route)
            assert must <= ran and not (never & ran), (g.id, route, sorted(ran))
            if route == "fused256" and GC.stage_takes(g.h, g.w):
                # launched only behind the 256-thread instance: tells "256 ran" from "256 refused, 768 took over"
                assert ("k_stage_retry" in ran) == (GC.stage_rows(g.h, g.w, 256) is not None), (g.id, sorted(ran))
            check((g.id, route), det, counts, st)
            if route in FUSED and (must, never) == (ROUTES[route][2], ROUTES[route][3]):
                # the fused kernel labelled the rim frame itself and handed the frame with a hole on to k_label
                assert [int(s) for s in slow] == [0, 16 + 4], (g.id, route, slow)
            if default is not None:
                # forcing a route whose launcher refuses falls through: the same rows as at the defaults
                assert np.array_equal(det, default[0]) and np.array_equal(counts, default[1]), (g.id, route)
    finally:
        eng.close()
