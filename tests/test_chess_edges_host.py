"""What the edge inputs of tests/helpers/chess_edge_cases.py contain, stated on the CPU with the NumPy helper
(tests/helpers/chess_oracle.py): every case has the property it exists for, so tests/test_gpu_chess_edges.py cannot quietly turn
into a second run of the rendered boards.  As for those boards, no walk decision of any case is a tie (`ties == 0`)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import chess_cases as CC                                      # noqa: E402
import chess_edge_cases as E                                  # noqa: E402
import chess_oracle as CO                                     # noqa: E402
from test_gpu_chess import SAME_ITERS_PX                      # noqa: E402

K = CO.MAX_CANDIDATES
CUT_NAMES = [c["name"] for c in E.cut_cases()]


class _Limited(CO._Walk):
    """The helper's walk, noting whether a chain gave up at its limit (ch_chain's -1)."""
    limited = False

    def chain(self, start, sx, sy, limit):
        out = super().chain(start, sx, sy, limit)
        self.limited |= out is None
        return out


def seeds_leaving_at_the_limit(gray, pattern, seeds):
    """How many of `seeds` (ranks in the kept list) end in the `limit` return of a chain, as order() would walk them."""
    top = CO.strongest(CO.candidates(CO.response(gray)))
    n = 0
    for s in seeds:
        walk = _Limited(top[:int((CO.STRENGTH_RATIO * top[:, 2] >= top[s, 2]).sum()), :2], *pattern)
        assert walk.seed(s) is None or not walk.limited
        n += walk.limited
    return n


@pytest.mark.parametrize("name", CUT_NAMES)
def test_cut_cases(name):
    c = E.cut_by_name(name)
    s = E.sorted_candidates(c["gray"])
    total = len(s)
    for a in c["asks"]:
        r = E.helper(name, a["pattern"])
        assert r["found"] == a["found"] and r["ties"] == 0 and r["n_candidates"] == total, a
        if not a["found"]:
            assert (r["peaks"] == -1).all() and np.isnan(r["corners"]).all()
    cut = f", R at ranks {K - 1} and {K}: {s[K - 1, 2]} and {s[K, 2]}" if total > K else ""
    print(f"{name}: {total} candidates{cut}")
    first = E.helper(name, c["asks"][0]["pattern"])
    resp = first["response"]
    if name == "noise_ground":
        assert total > K
        board = resp[first["peaks"][:, 1], first["peaks"][:, 0]]
        print(f"weakest board corner {board.min()}")
        assert board.min() > s[K - 1, 2]
    elif name == "pure_noise":
        assert total > K
    elif name == "cut_inside_tie_class":
        strong, weak = s[s[:, 0] < 160], s[s[:, 0] >= 160]
        assert len(strong) == 220 and len(weak) == 42 and len(set(strong[:, 2])) == 1 and len(set(weak[:, 2])) == 1
        assert strong[0, 2] > weak[0, 2] and s[K - 1, 2] == s[K, 2] == weak[0, 2]
        # the cut goes through the weak class: by (y, x) its first 36 are the top six rows of the weak board, and they are found
        rows = np.unique(weak[:, 1])
        kept = weak[np.isin(weak[:, 1], rows[:6])]
        assert len(rows) == 7 and np.array_equal(kept, s[220:K])
        assert sorted(map(tuple, first["peaks"])) == sorted(map(tuple, kept[:, :2]))
        print(f"peaks y in {sorted(set(first['peaks'][:, 1]))}")
        # the walk of a strong seed ends at the limit of a chain wherever its row runs along the board's 22 corners
        n = seeds_leaving_at_the_limit(c["gray"], (6, 6), range(220))
        print(f"{n} of the 220 strong seeds leave through the limit of a chain")
        assert n >= 110
    elif name == "exactly_256":
        assert total == K
    elif name == "one_over_weaker":
        assert E.extra_rank(c["gray"]) == (K, K + 1)
    elif name == "one_over_stronger":
        rank, n = E.extra_rank(c["gray"])
        print(f"compression g // {E.one_over_stronger_shrink()} + 60, the extra corner at rank {rank}")
        assert n == K + 1 and rank < K and s[K, 0] < E.BIG["size"][0]          # the one cut away is a corner of the board
    elif name == "row_longer_than_limit":
        assert total == 42
        n = seeds_leaving_at_the_limit(c["gray"], (6, 6), range(total))
        print(f"{n} of the 42 seeds leave through the limit of a chain")
        assert n >= 1
        a, b = E.helper(name, (14, 3))["peaks"], E.helper(name, (3, 14))["peaks"]
        assert sorted(map(tuple, a)) == sorted(map(tuple, b)) and not np.array_equal(a, b)
    elif name == "smallest_pattern":
        assert total == 4
    else:
        raise AssertionError(name)


def test_quadrants():
    """Sixteen found boards, sixteen different first peaks, and each of the four rotations of the labelling chosen at least once."""
    firsts, rotations = set(), []
    for i, angle in enumerate(E.QUADRANT_ANGLES):
        for p in E.QUADRANT_PATTERNS:
            r = E.quadrant_helper(i, p)
            assert r["found"] == 1 and r["ties"] == 0 and r["n_candidates"] == 28
            firsts.add(tuple(r["peaks"][0]))
            rotations.append(E.best_rotation(E.quadrant_frames()[i], p))
    print(f"rotations chosen: {rotations}")
    assert len(firsts) == 16 and set(rotations) == {0, 1, 2, 3}


def test_seam_sweep():
    """Nine candidates and a found board in every frame; every candidate has an equal neighbour in its 9 x 9 neighbourhood, so the
    `before` / `after` rule decides every peak; over the sweep the peaks take every column of a 32-wide and every row of a 16-high
    tile."""
    assert len(E.SEAM_OFFSETS) == len(set(E.SEAM_OFFSETS)) == 49
    xs, ys = set(), set()
    for i in range(len(E.SEAM_OFFSETS)):
        r = E.seam_helper(i)
        assert r["found"] == 1 and r["n_candidates"] == 9 and r["ties"] == 0
        resp = r["response"]
        for x, y, v in r["candidates"]:
            nb = resp[y - 4:y + 5, x - 4:x + 5]
            assert nb.shape == (9, 9) and (nb == v).sum() >= 2
        xs |= set(r["peaks"][:, 0] % 32)
        ys |= set(r["peaks"][:, 1] % 16)
    assert xs == set(range(32)) and ys == set(range(16))


@pytest.mark.parametrize("shape", E.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames(shape):
    assert E.SMALL_SEEDS[shape] == E.first_small_seed(shape)
    r = CO.find_chessboard_corners(E.small_frame(shape), E.SMALL_PATTERN, want=True)
    print(f"{shape}: {r['n_candidates']} candidates")
    assert r["found"] == 0 and r["ties"] == 0
    if min(shape) < 11:
        assert (r["response"] == CO.NEG).all() and r["n_candidates"] == 0
    else:
        assert (r["response"] != CO.NEG).sum() == (shape[0] - 10) * (shape[1] - 10) and r["n_candidates"] >= 1


def test_launch_split_frames():
    """Seven different frames with seven different results, at least four found and at least one refused by the walk itself."""
    d = E.split_distinct()
    assert d.shape == (7, 36, 36) and len({g.tobytes() for g in d}) == 7 and E.SPLIT_FRAMES > 65535 + 1
    res = [E.split_helper(i) for i in range(7)]
    assert all(r["ties"] == 0 for r in res)
    assert sum(r["found"] for r in res) >= 4
    assert any(not r["found"] and r["n_candidates"] >= 4 for r in res)
    assert len({(r["n_candidates"], r["peaks"].tobytes()) for r in res}) == 7


def test_near_border():
    g, r = E.near_border(), E.near_border_helper()
    h, w = g.shape
    p = r["peaks"]
    nearest = min(p[:, 0].min(), p[:, 1].min(), w - 1 - p[:, 0].max(), h - 1 - p[:, 1].max())
    print(f"{w} x {h}, {r['n_candidates']} candidates, nearest peak {nearest} px from a border")
    assert r["found"] == 1 and r["ties"] == 0 and nearest <= E.CROP_MARGIN
    whole = CC.helper_results()["rotated_30"]["peaks"]      # the crop changes nothing but the origin
    assert np.array_equal(p, whole - whole.min(axis=0) + E.CROP_MARGIN)


@pytest.mark.parametrize("label", list(E.subpix_cases()))
def test_subpix_reference_yardstick(label):
    """What the GPU test allows the device, met by the reference alone: summing forwards against summing in reverse moves no
    corner's iteration count and no corner by more than SAME_ITERS_PX."""
    ref, its = E.subpix_helper(label)
    rev, its_rev = E.subpix_helper(label, True)
    gap = np.linalg.norm(ref - rev, axis=1)
    print(f"{label}: forward against reverse {gap.max():.3e} px, iterations {its.min()}..{its.max()}")
    assert np.isfinite(ref).all() and np.array_equal(its, its_rev) and gap.max() <= SAME_ITERS_PX
    gray, starts, kw = E.subpix_cases()[label]
    back = (ref == starts).all(axis=1)
    if label == "return_to_start-win2x2":
        assert back.all() and its.min() >= 2                 # walked, left the window, went back
    elif label == "return_to_start-win5x5":
        assert not back.any()
    elif label == "survive":
        h, w = gray.shape
        assert ((ref[:, 0] < 0) | (ref[:, 0] >= w) | (ref[:, 1] < 0) | (ref[:, 1] >= h)).sum() >= 2     # left outside the frame
        assert ((starts[:, 0] < 0) | (starts[:, 0] >= w) | (starts[:, 1] < 0) | (starts[:, 1] >= h)).sum() == 4
    elif kw["max_iter"] == 1:
        assert (its == 1).all()
    elif kw["eps"] == 0.0:
        assert (its == kw["max_iter"]).all()


def test_window_settings_are_the_ones_meant():
    """The zero zone is on where both sides are >= 0 and smaller than the window, and off in the two cases that say so."""
    on = {E.setting_id(kw): bool((CO._window(*kw["win"], *kw["zero_zone"]) == 0).any()) for kw in E.WINDOW_SETTINGS}
    assert [k for k, v in on.items() if v] == ["win5x3-zone1x0-it30-eps0.001", "win7x7-zone0x0-it30-eps0.001",
                                               "win11x11-zone3x3-it30-eps0.001"]
    assert (CO.MAX_WIN, CO.MAX_WIN) in [kw["win"] for kw in E.WINDOW_SETTINGS]
    pts, frozen = E.survive_starts()
    assert frozen.sum() == 5 and not frozen[[6, 8, 10, 12, 14, 16]].any()


def test_flat_patches():
    """A patch without gradient, or with gradient along one axis only, has a determinant of exactly 0: the helper stops after one
    solve and returns the start."""
    for name, gray, starts in E.flat_frames():
        ref, its = CO.corner_subpix(gray, starts, **E._kw((5, 5)))
        assert np.array_equal(ref.view(np.int64), starts.view(np.int64)) and (its == 1).all(), name
