"""Every labelling route of `_marker_center` against the CPU oracle (`oracle/stages.py: marker_center`) on ragged, holed,
matching and crowded masks (tests/helpers/label_cases.py).

Routes (`vbs.h`, VBS_OPT_STAGE_IMPL / VBS_OPT_LATENCY_FRAMES): the fused batch kernel k_stage (impl 0: its own choice of
256 / 768 threads, 3: 768 always, 4: 256 wherever the geometry allows), the separate kernels k_morph + k_ccl (impl 1),
the general kernel k_morph + k_label for every frame (impl 2), and the several-workgroups kernel k_stage_lat (a pass of
at most LATENCY_FRAMES frames), which hands on to k_label<ns> that builds its own band and opened planes.  What the
fused kernels cannot take - holes (slow 16 + SLOW_HOLES), tables that overflow (slots 1, mailbox 3, segments 6, records
7, queued unions 8) - goes to k_label; this module checks that it happens and that the result is still the oracle's.
Targeted frames reach single tables: the probe mailbox (3), the opened-mask segments per tile (16 + 6), the component
limits (2, 16 + 2; below max_markers in test_component_limits_below_max_markers_hand_on).  What cannot be required:
  * SLOW_VERTEX (5, a contour vertex of multiplicity > 2) cannot occur after the 5x5 opening
    (test_smallest_opened_components_fit_without_the_degenerate_branch).
  * k_stage_lat has no probe mailbox (its probes are looked up after the resolve), so it never hands on for 3.
  * k_stage_lat's tiles are 5 - 6 rows tall at these geometries (LT_ROWS = 6).  An opened segment that starts below a
    tile's first row lasts at least 5 rows (every opened pixel lies in a 5x5 square), so each of the SG_KO = 3 slots starts
    at most 1 + ceil((R - 1) / 5) = 2 segments in R <= 6 rows: 6 <= SG_SEGMAX = 8, and 16 + 6 cannot occur there.
  * Queued unions (8) were not reached by any layout tried: the queue holds 4096 / 1536 pairs against 2048 / 768 band
    records, and runs that repeat a pair are queued once.  Frames that came close ran out of slots or records first.

Tolerances: those of the tests/test_gpu_parity.py header (tests/helpers/markers.py)."""
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
import label_cases as LC                                      # noqa: E402
from markers import compare_markers                           # noqa: E402

MAX_MARKERS = 1024
GEOMETRIES = [(64, 128), (300, 200), (450, 480), (480, 640), (481, 136), (700, 1003), (1024, 1280), (1200, 1920), (130, 4096)]
CROWDED = {(480, 640), (1024, 1280)}
# name: (VBS_OPT_STAGE_IMPL, VBS_OPT_LATENCY_FRAMES, kernels that must run, kernels that must not)
ROUTES = {
    "fused": (0, 0, {"k_stage", "k_label"}, {"k_ccl_band", "k_ccl_open", "k_stage_lat"}),
    "separate": (1, 0, {"k_morph", "k_ccl_band", "k_ccl_open", "k_label"}, {"k_stage", "k_stage_retry", "k_stage_lat"}),
    "general": (2, 0, {"k_morph", "k_label"}, {"k_stage", "k_stage_retry", "k_stage_lat", "k_ccl_band", "k_ccl_open"}),
    "fused768": (3, 0, {"k_stage", "k_label"}, {"k_ccl_band", "k_ccl_open", "k_stage_lat", "k_stage_retry"}),
    "fused256": (4, 0, {"k_stage", "k_label"}, {"k_ccl_band", "k_ccl_open", "k_stage_lat"}),
    "latency": (0, 32, {"k_stage_lat", "k_label"}, {"k_stage", "k_stage_retry", "k_ccl_band", "k_ccl_open", "k_morph"}),
}
FUSED = {"fused", "fused768", "fused256", "latency"}
OVERFLOW = {1, 3, 6, 7, 8}
K_STAGE = {"fused", "fused768", "fused256"}
# (case, geometries or None = every crowded one) -> (routes, the hand-on reason they must show)
TARGETED = {("mailbox", None): (K_STAGE, 3), ("open_segs", None): (K_STAGE, 16 + 6),
            ("band_comps_sparse_over", (1024, 1280)): (K_STAGE, 2),
            ("open_comps_sparse_over", (1024, 1280)): (FUSED, 16 + 2)}


def _cases(h, w):
    cases = LC.label_cases(h, w)
    if (h, w) in CROWDED:
        cases += LC.crowded_cases(h, w, MAX_MARKERS)
    for c in cases:
        c.expect = LC.expected_capacity(c.mask, c.area, MAX_MARKERS)
        c.want = None if c.expect["over"] else O.marker_center(c.mask, c.area)
        if c.want is not None:
            assert len(O.find_contours_external(O.morph_open5(c.area != 0))) == c.expect["contours"]
    return cases


def _run(eng, mt, at, route):
    """one call on `route`.  For this module's own engines: the C ABI has no option getter, so the options are put back to
    the documented defaults (VBS_OPT_STAGE_IMPL 0, VBS_OPT_LATENCY_FRAMES 24), which is what these engines were made with."""
    impl, lat = ROUTES[route][:2]
    eng.set_option(L.OPT_STAGE_IMPL, impl)
    eng.set_option(L.OPT_LATENCY_FRAMES, lat)
    try:
        eng.profile(True)
        det, counts = eng.marker_center(mt, at)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile(False)
        n = mt.shape[0]
        return det.cpu().numpy(), counts.cpu().numpy(), eng.frame_stats(n), eng.stage_tables(n)["slow"], prof
    finally:
        eng.set_option(L.OPT_STAGE_IMPL, 0)
        eng.set_option(L.OPT_LATENCY_FRAMES, 24)


@pytest.fixture(scope="module")
def engines():
    made = {}
    yield made
    for e in made.values():
        e.close()


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_every_route_equals_the_oracle(h, w, engines):
    from vbs_amd.engine import Engine
    from vbs_amd.marker_detection import _det_to_markers
    cases = _cases(h, w)
    n = len(cases)
    assert n <= 32                                            # one pass, and within the latency route's frame limit
    eng = engines.setdefault((h, w), Engine(h, w, max_markers=MAX_MARKERS, max_batch=n))
    mt = torch.from_numpy(np.stack([c.mask for c in cases])).cuda()
    at = torch.from_numpy(np.stack([c.area for c in cases])).cuda()
    ns = 8 if h <= 480 else 14
    for route, (impl, lat, must, never) in ROUTES.items():
        det, counts, st, slow, prof = _run(eng, mt, at, route)
        ran = {k for k, (cnt, _) in prof.items() if cnt > 0}
        assert must <= ran and not (never & ran), (route, sorted(ran))
        why = {c.name: int(s) for c, s in zip(cases, slow) if s}
        if route in FUSED:
            assert (slow == 16 + 4).any(), (route, why)       # a frame with holes handed on to the general kernel
            assert any((s & 15) in OVERFLOW for s in why.values()), (route, why)      # and one whose tables overflowed
            assert why.get("slots_open") == 16 + 1, (route, why)
            assert all(s & 15 != 5 for s in why.values()), (route, why)
            for (name, geo), (routes, reason) in TARGETED.items():
                if (h, w) in CROWDED and geo in (None, (h, w)) and route in routes:
                    assert why.get(name) == reason, (route, name, why)
        for i, c in enumerate(cases):
            tag = (route, ns, c.name)
            if c.expect["over"]:
                assert int(counts[i]) == L.VBS_ECAPACITY, (tag, int(counts[i]))
                continue
            assert counts[i] >= 0, (tag, int(counts[i]))
            compare_markers(_det_to_markers(det[i], int(counts[i])), c.want)
            assert int(st[i, 5]) == ndimage.label(O.band_mask(c.mask))[1] == c.expect["band_comps"], (tag, st[i])
            assert int(st[i, 6]) == c.expect["contours"], (tag, st[i])     # (components once the holes are filled)
            assert int(st[i, 7]) == c.expect["holes"], (tag, st[i])
            assert int(st[i, 4]) == 0, (tag, st[i])


@pytest.mark.parametrize("h,w", sorted(CROWDED))
def test_crowded_frames_in_the_drop_in(h, w):
    """MarkerTracker._marker_center (its own cached engine: max_markers 1024, one frame per call) raises VbsError for every
    frame beyond a limit and returns the oracle's markers for the frames at 90 % of one."""
    from vbs_amd.marker_detection import MarkerTracker
    checked = 0
    for c in LC.crowded_cases(h, w, MAX_MARKERS):
        if c.claims["over"]:
            with pytest.raises(L.VbsError):
                MarkerTracker._marker_center(c.mask, c.area)
        else:
            compare_markers(MarkerTracker._marker_center(c.mask, c.area), O.marker_center(c.mask, c.area))
            checked += 1
    assert checked >= 4


def test_component_limits_below_max_markers_hand_on():
    """A handle with max_markers = 256: 300 band components or 300 opened ones, spread one or two per tile, are more than
    it holds.  Every fused kernel hands the frame on for its component limit (band 2, opened 16 + 2) - k_stage_lat too,
    whose band limit at max_markers = 1024 is its 1024-node table (a slot reason) - and every route reports
    VBS_ECAPACITY, as k_label's rule says."""
    from vbs_amd.engine import Engine
    h, w, maxm = 1024, 1280, 256
    frames = []
    for draw in ("dot", "sq"):
        mask = np.zeros((h, w), np.uint8); area = np.zeros((h, w), np.uint8)
        for k in range(300):
            y, x = 20 + 50 * (k // 20), 20 + 62 * (k % 20)
            if draw == "dot":
                mask[y, x] = 1
            else:
                area[y:y + 6, x:x + 6] = 255
        mask[h - 30, w - 30] = 1; area[h - 40:h - 20, w - 40:w - 20] = 255
        assert LC.expected_capacity(mask, area, maxm)["over"]
        frames.append((mask, area))
    eng = Engine(h, w, max_markers=maxm, max_batch=2)
    try:
        mt = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
        at = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
        for route in ROUTES:
            _, counts, _, slow, _ = _run(eng, mt, at, route)
            assert (counts == L.VBS_ECAPACITY).all(), (route, counts)
            if route in FUSED:
                assert [int(s) for s in slow] == [2, 16 + 2], (route, slow)
    finally:
        eng.close()


@pytest.mark.parametrize("h,w", [(300, 200), (1024, 1280)])
def test_two_valued_inputs_any_non_zero_value(h, w):
    """{0, 1}, {0, 255} and {0, 7} give the same detection rows on every route."""
    from vbs_amd.engine import Engine
    cases = LC.label_cases(h, w)
    m01 = np.stack([c.mask for c in cases])
    a01 = (np.stack([c.area for c in cases]) != 0).astype(np.uint8)
    eng = Engine(h, w, max_markers=MAX_MARKERS, max_batch=len(cases))
    try:
        for route in ROUTES:
            outs = []
            for v in (1, 255, 7):
                mt, at = torch.from_numpy(m01 * v).cuda(), torch.from_numpy(a01 * v).cuda()
                det, counts = _run(eng, mt, at, route)[:2]
                outs.append((det, counts))
            for det, counts in outs[1:]:
                assert np.array_equal(counts, outs[0][1]) and np.array_equal(det, outs[0][0]), route
            assert (outs[0][1] > 0).any()
    finally:
        eng.close()
