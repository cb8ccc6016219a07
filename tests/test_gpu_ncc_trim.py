"""k_ncc_mfma's pre-scan on the GPU: the kernel skips the strips and rows whose correlation windows hold no area pixel
and stores zeros there.  Held here: the mask and the `ambiguous` / `exact` counters are those of the untrimmed kernel bit
for bit, the mask equals the float64 map's `> 0.1`, a reused workspace keeps nothing of the pass before, and the fused
path (the benchmark's instance) gives the same tables and the oracle's detections.

How the two kernels are reached.  `vbs_normxcorr2` with a map requested takes the float64 kernel (k_ncc) for map AND mask,
so `eng.normxcorr2(area, want_mask=True)` never runs k_ncc_mfma: the mask under test comes from `vbs_normxcorr2` with
mask only (k_ncc_mfma, the uint8-output instances), the map from a second call.  The untrimmed kernel is the tools'
library (libvbs_dbg.so) under VBS_NCC_TRIM_OFF=1; the same library without the variable trims, as the product one does.

Shapes: 481 x 128 (large template, every window leaves the image), 560 x 320 (interior and border strips), 560 x 244 (width no
multiple of 16), 64 x 128 and 200 x 256 (small template).  Each batch of 13 patterns (helpers/ncc_trim_cases.py) runs frame
by frame (one-frame passes: segments of one or two tiles) and as one pass; 560 x 320 also as one pass of 416 frames, at
which the launch gives every strip one segment (5 word columns x 416 frames >= 2048 workgroups)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import vbs_amd.synth as S                                     # noqa: E402
from vbs_amd import _lib as L                                 # noqa: E402
from oracle import stages as O                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ncc_trim_cases as TC                                   # noqa: E402
from markers import compare_markers                           # noqa: E402

SHAPES = [(481, 128), (560, 320), (560, 244), (64, 128), (200, 256)]
OFF = "VBS_NCC_TRIM_OFF"


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
def trim_off():
    os.environ[OFF] = "1"
    try:
        yield
    finally:
        del os.environ[OFF]


def mfma_mask(eng, area):
    """mask of k_ncc_mfma (vbs_normxcorr2 without a map), and the counters {ambiguous, exact} of the call"""
    mask = torch.empty_like(area)
    eng.ncc_counters(reset=True)
    eng._check(eng.lib.vbs_normxcorr2(eng._h, C.c_void_p(area.data_ptr()), area.shape[0], None, C.c_void_p(mask.data_ptr()),
                                      eng._stream()), "vbs_normxcorr2")
    torch.cuda.synchronize()
    c = eng.ncc_counters()
    return mask, (c["ambiguous"], c["exact"])


@pytest.fixture(scope="module")
def cases():
    """per shape, computed once: names, the area masks on the device, and the float64 map of each (k_ncc)"""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            pats = TC.patterns(h, w)
            area = torch.from_numpy(np.stack([a for _, a in pats])).cuda()
            eng = make_engine(None, h, w, max_batch=len(pats))
            ncc = eng.normxcorr2(area)
            torch.cuda.synchronize()
            eng.close()
            made[(h, w)] = ([n for n, _ in pats], area, ncc)
        return made[(h, w)]
    return get


def check_against_map(mask, ncc, what):
    diff = (ncc > 0.1) != (mask != 0)
    near = bad = 0
    if bool(diff.any()):
        d = (ncc[diff] - 0.1).abs()
        near, bad = int((d <= 1e-10).sum()), int((d > 1e-10).sum())
    print(what, "differing pixels:", bad, "within 1e-10 of the threshold:", near)
    assert bad == 0 and near <= 2, (what, bad, near)


@pytest.mark.parametrize("h,w", SHAPES)
def test_trimmed_mask_and_counters_equal_the_untrimmed_and_the_float64_map(h, w, cases, dbg):
    names, area, ncc = cases(h, w)
    n = area.shape[0]
    prod = make_engine(None, h, w, max_batch=n)
    tool = make_engine(dbg, h, w, max_batch=n)
    try:
        # one pass of the 13 frames
        m_on, c_on = mfma_mask(prod, area)
        m_tool, c_tool = mfma_mask(tool, area)
        with trim_off():
            m_off, c_off = mfma_mask(tool, area)
        print(h, w, "batch counters (ambiguous, exact): trimmed", c_on, "tools' library", c_tool, "untrimmed", c_off)
        assert torch.equal(m_on, m_off) and torch.equal(m_tool, m_off)
        assert c_on == c_off and c_tool == c_off
        check_against_map(m_on, ncc, f"{h}x{w} batch")
        assert int(m_on[names.index("zero")].sum()) == 0
        # frame by frame: the launch cuts a strip into many short segments
        for i, name in enumerate(names):
            a1 = area[i:i + 1]
            m1, c1 = mfma_mask(prod, a1)
            with trim_off():
                m0, c0 = mfma_mask(tool, a1)
            assert torch.equal(m1, m0) and c1 == c0, (name, c1, c0)
            assert torch.equal(m1[0], m_on[i]), name
    finally:
        prod.close()
        tool.close()


def test_one_segment_per_strip_in_a_pass_of_416_frames(cases, dbg):
    h, w = 560, 320
    names, area, ncc = cases(h, w)
    reps = 32
    big = area.repeat(reps, 1, 1)
    assert big.shape[0] == 416
    prod = make_engine(None, h, w, max_batch=big.shape[0])
    tool = make_engine(dbg, h, w, max_batch=big.shape[0])
    try:
        m_on, c_on = mfma_mask(prod, big)
        with trim_off():
            m_off, c_off = mfma_mask(tool, big)
        assert torch.equal(m_on, m_off) and c_on == c_off, (c_on, c_off)
        assert torch.equal(m_on, m_on[:area.shape[0]].repeat(reps, 1, 1))
        check_against_map(m_on[:area.shape[0]], ncc, "560x320, 416 frames")
    finally:
        prod.close()
        tool.close()


def _same_tables(t0, t1):
    for i in range(t0["ncomp"].shape[0]):
        nb, na = (int(v) for v in t0["ncomp"][i])
        assert (nb, na) == tuple(int(v) for v in t1["ncomp"][i])
        assert np.array_equal(t0["band_sums"][i][:nb, :3], t1["band_sums"][i][:nb, :3])
        assert np.array_equal(t0["area_first"][i][:na], t1["area_first"][i][:na])
        assert np.array_equal(t0["area_sums"][i][:na, :15], t1["area_sums"][i][:na, :15])
        assert np.array_equal(t0["probe"][i][:nb], t1["probe"][i][:nb])


def _detect(eng, ft):
    _, det, counts = eng.track_to_3d(ft, None, want_det=True)
    torch.cuda.synchronize()
    return det.cpu().numpy(), counts.cpu().numpy(), eng.stage_tables(ft.shape[0])


@pytest.mark.parametrize("spec", [S.grid_spec(512, 496, 3, 72, 40), S.grid_spec(256, 200, 2, 60, 20)],
                         ids=["512x496", "256x200"])
def test_fused_path_tables_equal_and_detections_are_the_oracles(spec, dbg):
    from vbs_amd.marker_detection import _det_to_markers
    n = 3
    frames = S.make_frames(spec, range(n), seed=2)
    ft = torch.from_numpy(frames).cuda()
    prod = make_engine(None, spec.height, spec.width, max_markers=256, max_batch=n)
    tool = make_engine(dbg, spec.height, spec.width, max_markers=256, max_batch=n)
    try:
        d_on, c_on, t_on = _detect(prod, ft)
        d_tool, c_tool, t_tool = _detect(tool, ft)
        with trim_off():
            d_off, c_off, t_off = _detect(tool, ft)
        assert np.array_equal(c_on, c_off) and np.array_equal(c_tool, c_off) and int(c_on.min()) > 0
        assert np.array_equal(d_on, d_off) and np.array_equal(d_tool, d_off)
        _same_tables(t_on, t_off)
        _same_tables(t_tool, t_off)
        for i in range(n):
            om, oa = O.find_markers(frames[i])
            compare_markers(_det_to_markers(d_on[i], int(c_on[i])), O.marker_center(om, oa))
    finally:
        prod.close()
        tool.close()


def test_a_reused_workspace_keeps_nothing_of_the_pass_before(cases):
    """the rows the kernel skips must be written all the same: all-255 masks first, then the centre disc.  (An all-255
    mask has variance 0 everywhere, so its pass leaves no set bit behind; a pass of discs all over the frame, whose mask has
    bits in every strip, runs between the two so that there is something to keep.)"""
    h, w = 560, 320
    names, area, _ = cases(h, w)
    full = area[names.index("full")].unsqueeze(0).repeat(4, 1, 1).contiguous()
    disc = area[names.index("disc_centre")].unsqueeze(0).repeat(4, 1, 1).contiguous()
    dots = np.zeros((h, w), np.uint8)
    for cy in range(24, h, 48):
        for cx in range(24, w, 48):
            dots |= TC.disc(h, w, cy, cx, 10)
    dots = torch.from_numpy(dots).cuda().unsqueeze(0).repeat(4, 1, 1).contiguous()
    used, fresh = make_engine(None, h, w, max_batch=4), make_engine(None, h, w, max_batch=4)
    try:
        m_full, _ = mfma_mask(used, full)
        assert int(m_full.sum()) == 0
        m_dots, _ = mfma_mask(used, dots)
        # bits where the disc's pass skips: above and below its windows, and in the strips left and right of them
        assert min(int(m_dots[0][:200].sum()), int(m_dots[0][-200:].sum()), int(m_dots[0][:, :64].sum()), int(m_dots[0][:, -64:].sum())) > 0
        m_used, _ = mfma_mask(used, disc)
        m_fresh, _ = mfma_mask(fresh, disc)
        assert torch.equal(m_used, m_fresh) and int(m_fresh.sum()) > 0
    finally:
        used.close()
        fresh.close()
    # the fused path: a pass of marker grids, then a pass of frames with one dot in the centre
    grid, one = S.grid_spec(512, 496, 5, 72, 40), S.grid_spec(512, 496, 1, 72, 40)
    fg = torch.from_numpy(S.make_frames(grid, range(3), seed=4)).cuda()
    fo = torch.from_numpy(S.make_frames(one, range(3), seed=4)).cuda()
    used, fresh = make_engine(None, 496, 512, max_markers=256, max_batch=3), make_engine(None, 496, 512, max_markers=256, max_batch=3)
    try:
        _, c_grid, _ = _detect(used, fg)
        assert int(c_grid.min()) > 1
        d_used, c_used, t_used = _detect(used, fo)
        d_fresh, c_fresh, t_fresh = _detect(fresh, fo)
        assert np.array_equal(c_used, c_fresh) and np.array_equal(d_used, d_fresh) and int(c_fresh.min()) > 0
        _same_tables(t_used, t_fresh)
    finally:
        used.close()
        fresh.close()
