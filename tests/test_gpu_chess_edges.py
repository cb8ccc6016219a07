"""GPU tests of the chessboard corner stage at its edges (csrc/k_chess.hip; `pytest -m gpu` on an MI355X): the device against the
NumPy helper tests/helpers/chess_oracle.py on the inputs of tests/helpers/chess_edge_cases.py, with the comparisons of
tests/test_gpu_chess.py and nothing weaker - response, candidate count, found, peaks and the NaN rows exact, the sub-pixel corners
by `two_class_check` with SAME_ITERS_PX as it stands there.  tests/test_chess_edges_host.py states on the CPU what the inputs
contain: more candidates than k_chess_order keeps and a tie class across the cut, chains beyond their limit, the 16 x 16 and the
2 x 2 pattern, the four rotations of the labelling, peaks on every column and row of a tile, frames below one tile and below the
ring, 65 537 frames in a call, and the windows, zero zones, borders and starts of k_corner_subpix.

`Engine` takes frames of at least 64 x 128; smaller ones go to the C entries directly, with the arguments `Engine` would pass.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import chess_edge_cases as E                                  # noqa: E402
import chess_oracle as CO                                     # noqa: E402
from test_gpu_chess import SAME_ITERS_PX, engine_for, two_class_check     # noqa: E402,F401

CUT_ASKS = [(c["name"], a["pattern"]) for c in E.cut_cases() for a in c["asks"]]
EPS = CO.FINDER_SUBPIX["eps"]


def _entry_find(g, pattern, want_response):
    """vbs_chess_corners on a contiguous uint8 device tensor [n,h,w] of any size, as Engine.find_chessboard_corners calls it."""
    from vbs_amd import _lib as L
    from vbs_amd.analysis import _ptr
    n, h, w = g.shape
    pw, ph = pattern
    dev = g.device
    corners = torch.empty((n, pw * ph, 2), dtype=torch.float64, device=dev)
    peaks = torch.empty((n, pw * ph, 2), dtype=torch.int32, device=dev)
    found = torch.empty((n,), dtype=torch.int32, device=dev)
    ncand = torch.empty((n,), dtype=torch.int32, device=dev)
    resp = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_response else None
    nbytes = int(L.lib().vbs_chess_workspace(n, h, w))
    assert nbytes > 0
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    rc = L.lib().vbs_chess_corners(dev.index or 0, _ptr(g), n, h, w, g.stride(0), g.stride(1), pw, ph, _ptr(corners), _ptr(found),
                                   _ptr(peaks), _ptr(ncand), _ptr(resp), _ptr(ws), None)
    assert rc == L.VBS_OK, rc
    torch.cuda.synchronize()
    return (found, corners, peaks, ncand) + ((resp,) if want_response else ())


def _entry_subpix(g, corners, win, zero_zone, max_iter, eps):
    from vbs_amd import _lib as L
    from vbs_amd.analysis import _ptr
    n, h, w = g.shape
    c = torch.from_numpy(np.array(corners, dtype=np.float64)).to(g.device).reshape(n, -1, 2).contiguous()
    its = torch.zeros((n, c.shape[1]), dtype=torch.int32, device=g.device)
    rc = L.lib().vbs_corner_subpix(g.device.index or 0, _ptr(g), n, h, w, g.stride(0), g.stride(1), _ptr(c), c.shape[1], win[0], win[1],
                                   zero_zone[0], zero_zone[1], max_iter, float(eps), _ptr(its), None)
    assert rc == L.VBS_OK, rc
    torch.cuda.synchronize()
    return c, its


def _batch(frames):
    """One frame or a batch -> a contiguous device tensor [n,h,w] (the cases are read-only arrays: copied first)."""
    f = np.array(frames)
    return torch.from_numpy(f[None] if f.ndim == 2 else f).cuda()


def find(frames, pattern, want_response=True):
    """The finder on one frame or a batch -> device tensors as Engine.find_chessboard_corners returns them."""
    f = _batch(frames)
    if f.shape[1] >= 64 and f.shape[2] >= 128:
        return engine_for(*f.shape[1:]).find_chessboard_corners(f, pattern, want_response=want_response)
    return _entry_find(f, pattern, want_response)


def subpix(frames, corners, win, zero_zone=(-1, -1), max_iter=30, eps=1e-3):
    """k_corner_subpix on one frame or a batch -> (corners float64 [n,k,2], iterations int32 [n,k]) as host arrays."""
    f = _batch(frames)
    if f.shape[1] >= 64 and f.shape[2] >= 128:
        c, its = engine_for(*f.shape[1:]).corner_subpix(f, np.asarray(corners).reshape(len(f), -1, 2), win, zero_zone, max_iter, eps,
                                                        want_iters=True)
    else:
        c, its = _entry_subpix(f, corners, win, zero_zone, max_iter, eps)
    return c.cpu().numpy(), its.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def hold_frame(gray, got, i, want, label):
    """Frame i of a finder result against the helper's dict: the integer outputs exact, NaN exactly where nothing is found, and
    the corners as the peaks through k_corner_subpix (the same bits) held to the helper's by two_class_check."""
    found, corners, peaks, ncand = (t[i].cpu().numpy() for t in got[:4])
    if len(got) > 4:
        assert np.array_equal(got[4][i].cpu().numpy(), want["response"]), label
    assert int(ncand) == want["n_candidates"] and int(found) == want["found"], (label, int(ncand), int(found))
    assert np.array_equal(peaks, want["peaks"]), label
    assert np.isnan(corners).all() == (not want["found"]) and np.isnan(corners).any() == (not want["found"]), label
    if want["found"]:
        again, its = subpix(gray, peaks.astype(np.float64), **CO.FINDER_SUBPIX)
        assert np.array_equal(bits(again[0]), bits(corners)), label
        two_class_check(corners, its[0], want["corners"], want["iters"], EPS, label)


# ---- A: the candidate cut and the ordering -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pattern", CUT_ASKS, ids=[f"{n}-{p[0]}x{p[1]}" for n, p in CUT_ASKS])
def test_candidate_cut_and_ordering(name, pattern):
    """More than VBS_CHESS_MAX_CANDIDATES candidates (the bitwise search, the compaction, the tie rule at the cut), exactly that
    many, one more on either side of the cut, chains beyond their limit, the largest and the smallest pattern."""
    gray = E.cut_by_name(name)["gray"]
    hold_frame(gray, find(gray, pattern), 0, E.helper(name, pattern), f"{name} {pattern}")


@pytest.mark.parametrize("pattern", E.QUADRANT_PATTERNS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_quadrants(pattern):
    """The 8 x 5 board at eight angles as one batch: every rotation of the labelling (`best` of k_chess_order)."""
    frames = E.quadrant_frames()
    got = find(frames, pattern)
    for i, angle in enumerate(E.QUADRANT_ANGLES):
        hold_frame(frames[i], got, i, E.quadrant_helper(i, pattern), f"{angle} degrees {pattern}")


# ---- B: tile seams, small frames, the launch split ---------------------------------------------------------------------
def test_seam_sweep():
    """49 frames in one call: a hard board whose peaks - each decided by the tie rule among four equal pixels - step over every
    column and row of a tile, so every peak sits once next to a seam and reads the neighbouring tile's halo."""
    frames = E.seam_frames()
    got = find(frames, E.SEAM_PATTERN)
    for i, off in enumerate(E.SEAM_OFFSETS):
        hold_frame(frames[i], got, i, E.seam_helper(i), f"offset {off}")


@pytest.mark.parametrize("shape", E.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames(shape):
    """Frames below the ring (no response pixel), below one tile, one tile, one tile and a pixel."""
    gray = E.small_frame(shape)
    hold_frame(gray, find(gray, E.SMALL_PATTERN), 0, CO.find_chessboard_corners(gray, E.SMALL_PATTERN, want=True), f"{shape}")


def test_launch_split():
    """65 537 frames: two launches of k_chess_response (gridDim.z holds 65 535), the second writing at the offsets launch_chess
    works out by hand.  Every frame equals its distinct frame computed alone - the response map too: 65 537 x 36 x 36 int32 are
    340 MB - and the seven distinct frames equal the helper."""
    distinct = E.split_distinct()
    alone = find(distinct, E.SPLIT_PATTERN)
    for i in range(len(distinct)):
        hold_frame(distinct[i], alone, i, E.split_helper(i), f"distinct frame {i}")
    idx = torch.arange(E.SPLIT_FRAMES, device="cuda") % len(distinct)
    frames = _batch(distinct)[idx].contiguous()
    assert frames.shape == (E.SPLIT_FRAMES, 36, 36)
    got = _entry_find(frames, E.SPLIT_PATTERN, True)
    for x, y, what in zip(got, alone, ("found", "corners", "peaks", "n_candidates", "response")):
        x, y = (t.view(torch.int64) if t.dtype == torch.float64 else t for t in (x, y))
        same = (x == y[idx]).reshape(E.SPLIT_FRAMES, -1).all(dim=1)
        assert bool(same.all()), (what, torch.nonzero(~same).reshape(-1)[:8].tolist())


# ---- C: k_corner_subpix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(E.subpix_cases()))
def test_subpix_settings_borders_and_starts(label):
    """Windows up to 15 x 15 and down to 1 x 1, wx != wy, the zero zone on, off and too large, one iteration, eps = 0; patches
    that read the replicated border; starts outside the frame and on its corners; starts that leave their window and go back."""
    gray, starts, kw = E.subpix_cases()[label]
    got, its = subpix(gray, starts, **kw)
    ref, ref_its = E.subpix_helper(label)
    assert np.isfinite(got).all()
    two_class_check(got[0], its[0], ref, ref_its, kw["eps"], label)
    back, ref_back = (bits(got[0]) == bits(starts)).all(axis=1), (bits(ref) == bits(starts)).all(axis=1)
    assert np.array_equal(back, ref_back), label              # the return to the start: the same corners, the same bits
    if label == "survive":
        h, w = gray.shape
        out = lambda p: (p[:, 0] < 0) | (p[:, 0] >= w) | (p[:, 1] < 0) | (p[:, 1] >= h)      # noqa: E731
        assert np.array_equal(out(got[0]), out(ref))           # left outside the frame where the helper leaves them


def test_subpix_leaves_absurd_starts_alone():
    """NaN, infinite and 2e9 starts mixed into a row of valid ones: bit-identical with 0 iterations, and the valid ones as if
    they stood alone."""
    gray = E.near_border()
    pts, frozen = E.survive_starts()
    got, its = subpix(gray, pts, **E._kw((5, 5)))
    assert np.array_equal(bits(got[0][frozen]), bits(pts[frozen])) and (its[0][frozen] == 0).all()
    alone, alone_its = subpix(gray, pts[~frozen], **E._kw((5, 5)))
    assert np.array_equal(bits(got[0][~frozen]), bits(alone[0])) and np.array_equal(its[0][~frozen], alone_its[0])
    assert (its[0][~frozen] >= 1).all()


def test_flat_and_one_dimensional_patches():
    """A determinant of exactly 0 (no gradient, or gradient along one axis): the start comes back after one solve, as the helper
    decides - nothing is said about a position."""
    for name, gray, starts in E.flat_frames():
        ref, ref_its = CO.corner_subpix(gray, starts, **E._kw((5, 5)))
        got, its = subpix(gray, starts, **E._kw((5, 5)))
        assert np.array_equal(bits(got[0]), bits(ref)) and np.array_equal(its[0], ref_its), name
