"""k_stage's per-frame tiling on the GPU: the kernel finds the bounding box of a frame's mask and area bits and spreads its
workgroup over that box alone (csrc/k_stage.hip, `stage_box_geom`).  Nothing it computes may change.  Held here, through the
staged entry (`Engine.marker_center(mask, area)`) on hand-made masks: with VBS_OPT_STAGE_IMPL = 3 and 4 (768 and 256 threads)
every per-component table, detection row and count equals what VBS_OPT_STAGE_IMPL = 1 gives (k_morph + k_ccl, which know no
box), and what the tools' library (libvbs_dbg.so) gives under VBS_STAGE_BBOX_OFF=1 (the full-frame tiling for every frame).

Frames: 190 px wide (three words, the last one cut) and 484 rows for the ns = 14 branch - the smallest at which both thread
counts have tiles of more than one row, so that a box can change them - and 330 x 600 (six words, tiles of 13 and 5 rows).
The ns = 8 branch (190 x 480 here) keeps the full-frame tiling (csrc/k_stage.hip, stage_geom): its frames run all the same,
with the stencil reach of that branch, and must come out as before.  The cases of a geometry run as two passes of 11 and
12 frames; neighbouring frames of a pass take different tilings, an empty frame lies between two occupied ones, and a frame
filled to its borders keeps the full-frame tiling."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

GEOMETRIES = [(484, 190), (480, 190), (600, 330)]
OFF = "VBS_STAGE_BBOX_OFF"
RM, RA = 11, 14                                               # radius of a blob in the mask / in the area mask


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8) * 255


def frame(h, w, blobs=(), mask_only=(), area_only=()):
    m, a = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for cy, cx in blobs:
        m |= disc(h, w, cy, cx, RM)
        a |= disc(h, w, cy, cx, RA)
    for cy, cx in mask_only:
        m |= disc(h, w, cy, cx, RM)
    for cy, cx in area_only:
        a |= disc(h, w, cy, cx, RA)
    return m, a


def passes(h, w):
    """[(name, mask, area)] of the two passes of a geometry"""
    guard = 7 if h > 480 else 4
    mid = h // 2
    edge = []
    # the area disc's first / last column d pixels inside a word edge: d = guard - 1 pulls the neighbouring word into the window
    for d in (guard - 1, guard, guard + 1):
        edge.append((f"left_{d}", *frame(h, w, [(mid, 64 + d + RA), (mid + 70, 64 + d + RA)])))
        edge.append((f"right_{d}", *frame(h, w, [(mid, 127 - d - RA), (mid - 70, 127 - d - RA)])))
    for name, c in (("at_left", (mid, 5)), ("at_right", (mid, w - 6)), ("at_top", (5, w // 2)), ("at_bottom", (h - 6, w // 2))):
        edge.append((name, *frame(h, w, [c])))
    edge.append(("corner", *frame(h, w, [(4, 4), (h - 5, w - 5)])))
    mixed = [("disjoint", *frame(h, w, mask_only=[(100, 40)], area_only=[(h - 130, w - 40)])),
             ("last_rows", *frame(h, w, [(h - 20, 100)])),
             ("word_0", *frame(h, w, [(90, 30), (300, 25)])),
             ("probe_63", *frame(h, w, [(mid, 63), (mid + 40, 127)])),        # the 2x2 cell around a centroid spans two words
             ("probe_edge_word", *frame(h, w, [(mid, 64 + guard + RA), (mid + 3, 64 + guard + RA + 60)])),
             ("occupied_a", *frame(h, w, [(200, 100)])),
             ("empty", *frame(h, w)),
             ("occupied_b", *frame(h, w, [(mid + 100, 150)]))]
    # a thin line below a blob: its band is the line, its centroid's cell reaches one row below the box
    m, a = frame(h, w, [(150, 100)])
    m[260, 70:110] = 255
    a[260, 70:110] = 255
    mixed.append(("line_last_row", m, a))
    # two blobs a tile apart in the same words, touching rows: components that cross row blocks
    m, a = frame(h, w, [(mid - 12, 100), (mid + 12, 100), (mid + 36, 100)])
    mixed.append(("column_of_blobs", m, a))
    grid = [(cy, cx) for cy in range(40, h - 40, 60) for cx in range(40, w - 40, 60)]       # (clear of the two corner blobs)
    mixed.append(("full", *frame(h, w, grid + [(3, 3), (h - 4, w - 4)])))
    mixed.append(("full_shifted", *frame(h, w, [(cy + 9, cx - 5) for cy, cx in grid] + [(3, 3), (h - 4, w - 4)])))
    return edge, mixed


def _dbg_lib():
    """libvbs_dbg.so through `_lib.lib()`'s own loader (signatures and all), without replacing the product library"""
    path = L.LIB_PATH.replace("libvbs.so", "libvbs_dbg.so")
    if not os.path.exists(path):
        import vbs_amd._build as B
        B.build(extra_flags=["-DVBS_DEBUG_KNOBS"], suffix="_dbg")
    saved = (L._lib, L.LIB_PATH)
    L._lib, L.LIB_PATH = None, path
    try:
        return L.lib()
    finally:
        L._lib, L.LIB_PATH = saved


@pytest.fixture(scope="module")
def dbg():
    return _dbg_lib()


def make_engine(lib, h, w, **kw):
    from vbs_amd.engine import Engine
    if lib is None:
        return Engine(h, w, **kw)
    saved = L.lib()
    L._lib = lib
    try:
        return Engine(h, w, **kw)
    finally:
        L._lib = saved


@contextlib.contextmanager
def bbox_off():
    os.environ[OFF] = "1"
    try:
        yield
    finally:
        del os.environ[OFF]


def run(eng, mt, at, impl):
    """one call with VBS_OPT_STAGE_IMPL = impl on the batch kernels (no few-frames route); the options go back to the defaults"""
    eng.set_option(L.OPT_LATENCY_FRAMES, 0)
    eng.set_option(L.OPT_STAGE_IMPL, impl)
    try:
        eng.profile(True)
        det, counts = eng.marker_center(mt, at)
        torch.cuda.synchronize()
        ran = {k for k, (cnt, _) in eng.profile_read().items() if cnt > 0}
        eng.profile(False)
        return det, counts, eng.stage_tables(mt.shape[0]), ran
    finally:
        eng.set_option(L.OPT_STAGE_IMPL, 0)
        eng.set_option(L.OPT_LATENCY_FRAMES, 24)


def same(got, want, names, what):
    (d0, c0, t0, _), (d1, c1, t1, _) = got, want
    assert np.array_equal(t0["slow"], t1["slow"]), (what, t0["slow"], t1["slow"])
    for i, name in enumerate(names):
        nb, na = (int(v) for v in t1["ncomp"][i])
        assert (nb, na) == tuple(int(v) for v in t0["ncomp"][i]), (what, name)
        assert np.array_equal(t0["band_sums"][i][:nb, :3], t1["band_sums"][i][:nb, :3]), (what, name)
        assert np.array_equal(t0["area_first"][i][:na], t1["area_first"][i][:na]), (what, name)
        assert np.array_equal(t0["area_sums"][i][:na, :15], t1["area_sums"][i][:na, :15]), (what, name)
        assert np.array_equal(t0["probe"][i][:nb], t1["probe"][i][:nb]), (what, name)
    assert torch.equal(c0, c1), (what, c0, c1)
    assert torch.equal(d0, d1), what


def tilings(h, w, cases, nt):
    """what the kernel's geometry function makes of every frame of a pass: (boxed, first word, words, rows per tile)"""
    out = []
    for _, m, a in cases:
        ys, xs = np.nonzero(m | a)
        box = (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())) if len(xs) else (0x7FFFFFFF, -1, 0x7FFFFFFF, -1)
        g = (C.c_int * 12)()
        assert L.lib().vbs_stage_box_geom(h, w, 14 if h > 480 else 8, nt, *box, g) == L.VBS_OK
        out.append((bool(g[11]), g[4], g[5], g[8]))
    return out


@pytest.mark.parametrize("h,w", [g for g in GEOMETRIES if g[0] > 480])
def test_the_cases_take_the_tilings_they_are_made_for(h, w):
    """(no kernel runs here: the masks against the exported geometry function, so that the comparisons below mean something)"""
    edge, mixed = passes(h, w)
    names = [n for n, _, _ in edge]
    for nt in (256, 768):
        t = dict(zip(names, tilings(h, w, edge, nt)))
        guard = 7 if h > 480 else 4
        # guard - 1 px inside a word edge: the window takes the neighbouring word; guard and guard + 1: it does not
        assert t[f"left_{guard - 1}"][1] == 0 and t[f"left_{guard}"][1] == 1 and t[f"left_{guard + 1}"][1] == 1
        assert [t[f"right_{d}"][1] + t[f"right_{d}"][2] - 1 for d in (guard - 1, guard, guard + 1)] == [2, 1, 1]
        assert all(t[n][0] for n in names if n != "corner") and not t["corner"][0]
        m = dict(zip([n for n, _, _ in mixed], tilings(h, w, mixed, nt)))
        assert not m["empty"][0] and not m["full"][0] and not m["full_shifted"][0]
        assert m["occupied_a"][0] and m["occupied_b"][0] and m["word_0"][:3] == (True, 0, 1) and m["last_rows"][0]
        assert len({v for v in m.values()}) >= 5                  # neighbouring workgroups of the pass take different tilings


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_tables_and_detections_equal_the_separate_kernels_and_the_full_frame_tiling(h, w, dbg):
    prod = make_engine(None, h, w, max_markers=256, max_batch=16)
    tool = make_engine(dbg, h, w, max_markers=256, max_batch=16)
    try:
        for which, cases in zip(("edge", "mixed"), passes(h, w)):
            names = [n for n, _, _ in cases]
            assert 8 <= len(names) <= 16
            mt = torch.from_numpy(np.stack([m for _, m, _ in cases])).cuda()
            at = torch.from_numpy(np.stack([a for _, _, a in cases])).cuda()
            want = run(prod, mt, at, 1)
            assert {"k_morph", "k_ccl_band", "k_ccl_open"} <= want[3] and "k_stage" not in want[3], sorted(want[3])
            assert int(want[2]["ncomp"][:, 0].max()) >= 2 and int(want[2]["slow"].sum()) == 0
            print(h, w, which, "components (band, opened) per frame:", want[2]["ncomp"].tolist())
            for impl in (3, 4):
                got = run(prod, mt, at, impl)
                assert "k_stage" in got[3] and not ({"k_ccl_band", "k_ccl_open"} & got[3]), sorted(got[3])
                same(got, want, names, (which, impl, "product library"))
                same(run(tool, mt, at, impl), want, names, (which, impl, "tools' library"))
                with bbox_off():
                    off = run(tool, mt, at, impl)
                same(off, want, names, (which, impl, "full-frame tiling"))
                same(got, off, names, (which, impl, "boxed against full-frame"))
    finally:
        prod.close()
        tool.close()


def test_a_reused_workspace_keeps_nothing_of_the_pass_before():
    """the same engine, three passes: blobs all over the frame, then one blob per frame in changing places, then the first
    again - every pass equals a fresh engine's"""
    h, w = 484, 190
    _, mixed = passes(h, w)
    by = {n: (m, a) for n, m, a in mixed}
    order = [["full"] * 8, ["occupied_a", "empty", "occupied_b", "word_0", "last_rows", "empty", "probe_63", "full"], ["full_shifted"] * 8]
    used = make_engine(None, h, w, max_markers=256, max_batch=8)
    try:
        for impl in (4, 3):
            for names in order:
                mt = torch.from_numpy(np.stack([by[n][0] for n in names])).cuda()
                at = torch.from_numpy(np.stack([by[n][1] for n in names])).cuda()
                fresh = make_engine(None, h, w, max_markers=256, max_batch=8)
                try:
                    same(run(used, mt, at, impl), run(fresh, mt, at, impl), names, (impl, names[0]))
                finally:
                    fresh.close()
    finally:
        used.close()
