"""The last step of `_marker_center` (k_finalize.hip, row a13) against exact references (tests/helpers/ellipse_oracle.py) on
the frames of tests/helpers/ellipse_cases.py; the caps used here are established on the CPU by tests/test_ellipse_host.py.

  moments    area_first / area_sums of every labelling route equal the traced contour's first pixel and integer vertex
             moments, component by component (paired by first pixel), and the component count is the oracle's.
  fit        the ellipse table (vbs_ellipse_table) against the exact rational fit: cx, cy, w, h within 1 float32 ulp of the
             exact value rounded to float32, at most 1 % of them different at all, the angle mod 180 within max(1 ulp,
             1e-4 degrees) where (h - w) / h >= 1e-3; ok = 0 exactly where the contour has fewer than 5 vertices (no case
             has a singular system).  Why 1 ulp: the normal matrix's condition number stays below 7e5, and 7e5 * 1.1e-16 is
             far below half a float32 ulp, so a float64 solve lands on the correctly rounded value except next to a tie.
             The same on k_finalize_track, through vbs_track_to_3d on synthetic camera frames.
  decisions  det / counts equal oracle.marker_center row by row (centres bit-exact, band label identical), with the parallel
             matching and with the sequential replay; waived only for contours on a decision boundary
             (ellipse_cases.boundary_contours), which are printed; exactly equidistant centres are waived only where the
             device's ellipse centre is not bit for bit the oracle's.
"""
import collections
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from oracle import stages as O                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ellipse_cases as EC                                    # noqa: E402
import ellipse_oracle as E                                    # noqa: E402
from test_gpu_labelling_oracle import ROUTES                  # noqa: E402

MAX_MARKERS = 1024


@pytest.fixture(scope="module")
def engines():
    made = {}
    yield made
    for e, _, _ in made.values():
        e.close()


def _engine(engines, h, w):
    from vbs_amd.engine import Engine
    if (h, w) not in engines:
        fr = EC.frames(h, w)
        eng = Engine(h, w, max_markers=MAX_MARKERS, max_batch=len(fr))
        mt = torch.from_numpy(np.stack([f.mask for f in fr])).cuda()
        at = torch.from_numpy(np.stack([f.area for f in fr])).cuda()
        engines[(h, w)] = (eng, mt, at)
    return engines[(h, w)]


def _run(eng, mt, at, route="fused", seq=False):
    """one call on `route` (options put back to the documented defaults, as in tests/test_gpu_labelling_oracle.py)."""
    impl, lat = ROUTES[route][:2]
    eng.set_option(L.OPT_STAGE_IMPL, impl)
    eng.set_option(L.OPT_LATENCY_FRAMES, lat)
    eng.set_option(L.OPT_FORCE_SEQ_MATCH, 1 if seq else 0)
    try:
        det, counts = eng.marker_center(mt, at)
        torch.cuda.synchronize()
        n = mt.shape[0]
        return det.cpu().numpy(), counts.cpu().numpy(), eng.stage_tables(n), eng.ellipse_table(n)
    finally:
        eng.set_option(L.OPT_STAGE_IMPL, 0)
        eng.set_option(L.OPT_LATENCY_FRAMES, 24)
        eng.set_option(L.OPT_FORCE_SEQ_MATCH, 0)


def _rows(tabs, i, info, w):
    """table row of every contour of frame i, paired by first pixel."""
    na = int(tabs["ncomp"][i, 1])
    assert na == len(info["contours"]), (i, na, len(info["contours"]))
    first = {int(fp): k for k, fp in enumerate(tabs["area_first"][i, :na])}
    assert len(first) == na
    rows = []
    for p in info["per"]:
        key = p["first"][1] * w + p["first"][0]
        assert key in first, (i, p["first"])
        rows.append(first[key])
    return rows


@pytest.mark.parametrize("h,w", EC.GEOMETRIES)
def test_vertex_moments_equal_the_traced_contour_on_every_route(h, w, engines):
    eng, mt, at = _engine(engines, h, w)
    fr = EC.frames(h, w)
    checked = 0
    for route in ROUTES:
        _, counts, tabs, _ = _run(eng, mt, at, route)
        for i, f in enumerate(fr):
            assert counts[i] >= 0, (route, f.name, int(counts[i]))
            info = EC.analyse(f)
            for p, k in zip(info["per"], _rows(tabs, i, info, w)):
                got = [int(v) for v in tabs["area_sums"][i, k, :15]]
                assert got == p["moments"], (route, f.name, p["first"], got, p["moments"])
                checked += 1
    assert checked >= 6 * len(fr)


def _check_fit(ell_row, p, tag, stats, fam):
    """one contour's table row against its exact fit; failures are collected, not raised, so that the figures print."""
    assert int(ell_row[5]) == p["n"], (tag, ell_row[5], p["n"])
    if p["n"] < 5 or p["exact"] is None:
        assert ell_row[6] == 0.0, (tag, ell_row)
        return
    assert ell_row[6] == 1.0, (tag, ell_row)
    for v in ell_row[:5]:
        assert float(np.float32(v)) == v, (tag, ell_row)      # float32 values
    u, dev, tol = E.fit_deviation(tuple(ell_row[:5]), p["exact"])
    s = stats[fam]
    s["n"] += 1
    s["values"] += 4
    s["differ"] += sum(v != 0 for v in u)
    s["ulps"] = [max(a, b) for a, b in zip(s["ulps"], u)]
    if max(u) > 1:
        s["bad"].append((tag, u, tuple(ell_row[:5]), p["oracle"]))
    if dev is not None:
        s["angle"] = max(s["angle"], dev)
        s["angle_ulps"] = max(s["angle_ulps"], dev / E.ulp32(max(abs(ell_row[4]), 1e-3)))
        if dev > tol:
            s["bad"].append((tag, "angle", dev, tol, ell_row[4], p["exact"]["angle_exact"]))


def _new_stats():
    return collections.defaultdict(lambda: dict(n=0, values=0, differ=0, ulps=[0, 0, 0, 0], angle=0.0, angle_ulps=0.0, bad=[]))


def _report(stats, title):
    print(f"\n{title}")
    for fam, s in sorted(stats.items()):
        print(f"  {fam:9s} {s['n']:5d} contours   max ulps cx {s['ulps'][0]} cy {s['ulps'][1]} w {s['ulps'][2]} h {s['ulps'][3]}   "
              f"{s['differ']} of {s['values']} values differ   angle {s['angle']:.2e} deg ({s['angle_ulps']:.2f} ulp)")
    values = sum(s["values"] for s in stats.values())
    differ = sum(s["differ"] for s in stats.values())
    bad = [b for s in stats.values() for b in s["bad"]]
    print(f"  all: {differ} of {values} values differ from the exact value rounded to float32 ({100.0 * differ / max(values, 1):.3f} %)")
    assert not bad, bad[:8]
    assert differ <= 0.01 * values


def test_ellipse_table_equals_the_exact_fit(engines):
    stats = _new_stats()
    for h, w in EC.GEOMETRIES:
        eng, mt, at = _engine(engines, h, w)
        _, counts, tabs, ell = _run(eng, mt, at)
        for i, f in enumerate(EC.frames(h, w)):
            if f.kind != "self":
                continue                                      # (the pieces twins have the same area mask)
            assert counts[i] >= 0
            info = EC.analyse(f)
            for p, k in zip(info["per"], _rows(tabs, i, info, w)):
                _check_fit(ell[i, k], p, (f.name, p["first"]), stats, f.family)
    _report(stats, "k_finalize against the exact fit")


def test_ellipse_table_of_the_fused_finalize_and_track_kernel():
    """vbs_track_to_3d on two synthetic camera frames with a reference table takes k_finalize_track; its ellipse table is
    held to the exact fit of the contours of the area mask the same handle detected."""
    import vbs_amd.synth as S
    from vbs_amd.engine import Engine
    from vbs_amd import ids as I
    from vbs_amd.marker_detection import _det_to_markers
    spec = S.config1()
    frames = S.make_frames(spec, [0, 1], seed=0, channels=3)
    K, dist, R, T = S.default_camera(spec)
    eng = Engine(spec.height, spec.width, max_markers=256, max_batch=2, device=0)
    try:
        ft = torch.from_numpy(frames).cuda()
        _, area = eng.find_markers(ft)
        area = area.cpu().numpy()
        _, det, counts = eng.track_to_3d(ft[:1], None, want_det=True)
        table = I.assign_ids(_det_to_markers(det[0].cpu().numpy(), int(counts[0])), 5, "full", "optimal")
        _, xy = I.reference_arrays(table)
        eng.profile(True)
        eng.track_to_3d(ft, xy, 20.0, L.make_camera(K, dist, R, T, 2.0), 5.0)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile(False)
        assert prof.get("k_finalize_track", (0, 0))[0] > 0 and prof.get("k_finalize", (0, 0))[0] == 0, sorted(prof)
        tabs, ell = eng.stage_tables(2), eng.ellipse_table(2)
        stats = _new_stats()
        for i in range(2):
            f = EC.Frame("synthetic", "self", f"synthetic_{i}", None, area[i])
            info = EC.analyse(f)
            assert len(info["per"]) >= 20
            for p, k in zip(info["per"], _rows(tabs, i, info, spec.width)):
                _check_fit(ell[i, k], p, (f.name, p["first"]), stats, f.family)
        _report(stats, "k_finalize_track against the exact fit")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def wanted():
    """oracle.marker_center of every frame, computed once: (rows, band-centre index of every row)."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            out = []
            for f in EC.frames(h, w):
                res = O.marker_center(f.mask, f.area, return_debug=True)
                out.append((res[0], list(res[1].get("matched", []))))
            made[(h, w)] = out
        return made[(h, w)]
    return get


@pytest.mark.parametrize("h,w", EC.GEOMETRIES)
def test_matching_decisions_equal_the_oracle(h, w, engines, wanted):
    eng, mt, at = _engine(engines, h, w)
    fr = EC.frames(h, w)
    want = wanted(h, w)
    tiles = matched = 0
    waived = collections.Counter()
    for seq in (False, True):
        det, counts, tabs, ell = _run(eng, mt, at, seq=seq)
        for i, f in enumerate(fr):
            assert counts[i] >= 0, (f.name, int(counts[i]))
            info = EC.analyse(f)
            centres = EC.band_centres(f)
            skip = set()                                      # band centres whose decision is waived
            rows_of = _rows(tabs, i, info, w)
            for ci, why in EC.boundary_contours(info, centres).items():
                p = info["per"][ci]
                same = tuple(ell[i, rows_of[ci], :2]) == tuple(p["oracle"][:2])
                if why == "equal" and same:
                    continue                                  # first index wins: held
                cx, cy, wd, ht, _ = p["oracle"]
                d = (centres[:, 0] - cx) ** 2 + (centres[:, 1] - cy) ** 2
                skip |= set(np.nonzero(d <= (max(wd, ht) / 10.0 + 2.0) ** 2)[0].tolist())
                print(f"\nwaived ({'sequential' if seq else 'parallel'}): {f.name} contour at {p['first']}: {why}")
                waived[f.family] += 1
            tiles += len(info["per"])
            rows, idx = want[i]
            got = [(det[i, r], int(det[i, r, 5]) - 1) for r in range(int(counts[i]))]
            got = [(r, b) for r, b in got if b not in skip]
            exp = [(r, b) for r, b in zip(rows, idx) if b not in skip]
            assert len(got) == len(exp), (seq, f.name, len(got), len(exp))
            for (g, gb), (e, eb) in zip(got, exp):
                assert gb == eb, (seq, f.name, gb, eb)        # column 5: the band label
                assert (g[0], g[1]) == tuple(e["center"]), (seq, f.name, g, e)        # bit-exact
                assert centres[gb][0] == g[0] and centres[gb][1] == g[1]
                # the fit behind the row is held by the fit test; here: the row carries that fit's axes and angle
                assert abs(g[2] - e["major_axis"]) <= E.ulp32(e["major_axis"]) and abs(g[3] - e["minor_axis"]) <= E.ulp32(e["minor_axis"])
            matched += len(exp)
    assert matched > 0
    assert sum(waived.values()) <= 0.02 * tiles, (waived, tiles)
    assert waived["minor5"] == 0


@pytest.mark.parametrize("which", sorted(EC.TALL))
def test_moments_at_the_edge_of_64_bits(which):
    """the tall frames of ellipse_cases.tall_frame on every route: where sum y^4 leaves 64 bits the frame is over capacity
    (counts and the status of vbs_frame_stats), below that the moments are the traced contour's and the frame matches."""
    from vbs_amd.engine import Engine
    f = EC.tall_frame(which)
    h, w = f.area.shape
    info = EC.analyse(f, fits=False)
    want = O.marker_center(f.mask, f.area) if which == "near" else None
    eng = Engine(h, w, max_markers=MAX_MARKERS, max_batch=1)
    try:
        mt, at = torch.from_numpy(f.mask[None]).cuda(), torch.from_numpy(f.area[None]).cuda()
        for route in ROUTES:
            for seq in (False, True):
                det, counts, tabs, ell = _run(eng, mt, at, route, seq)
                status = int(eng.frame_stats(1)[0, 2].astype(np.int32))
                if which == "over":
                    assert int(counts[0]) == L.VBS_ECAPACITY and status == L.VBS_ECAPACITY, (route, seq, int(counts[0]), status)
                    continue
                assert int(counts[0]) == len(want) == 1 and status == 0, (route, seq, int(counts[0]), status)
                p, k = info["per"][0], _rows(tabs, 0, info, w)[0]
                assert [int(v) for v in tabs["area_sums"][0, k, :15]] == p["moments"], (route, seq)
                assert ell[0, k, 6] == 1.0 and int(ell[0, k, 5]) == p["n"]
                g, e = det[0, 0], want[0]
                assert (g[0], g[1]) == tuple(e["center"])
                assert abs(g[2] - e["major_axis"]) <= E.ulp32(e["major_axis"]) and abs(g[3] - e["minor_axis"]) <= E.ulp32(e["minor_axis"])
    finally:
        eng.close()
