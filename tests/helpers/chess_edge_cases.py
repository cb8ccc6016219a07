"""Edge inputs for the chessboard corner stage (test infrastructure): frames on which csrc/k_chess.hip takes the branches that
the rendered boards of `chess_cases` never reach - more than VBS_CHESS_MAX_CANDIDATES candidates and a tie class across the cut,
rows longer than the walk's limit, the largest and the smallest pattern, all four rotations of the labelling, peaks on every
column and row of a 32 x 16 tile, frames smaller than a tile or than the ring, 65 537 frames in one call, and the window, zero
zone, border and start positions of k_corner_subpix.

Everything is generated with fixed seeds; `chess_oracle` is the reference as it stands.  tests/test_chess_edges_host.py states,
on the CPU, the property every case exists for, so that none can silently turn into a copy of an old one.
"""
import functools

import numpy as np

import chess_cases as CC
import chess_oracle as CO

GROUND = CC.GROUND
NOISE_SEED = 5


def hard_board(g, nx, ny, sq, lo, hi, x0, y0):
    """Paint an axis-aligned board of nx x ny squares of sq px into g, top-left pixel (x0, y0), no anti-aliasing: square (i, j)
    is `lo` where i + j is even.  Its inner corners lie BETWEEN pixels, so the four pixels round each have the same response."""
    for j in range(ny):
        for i in range(nx):
            g[y0 + j * sq:y0 + (j + 1) * sq, x0 + i * sq:x0 + (i + 1) * sq] = lo if (i + j) % 2 == 0 else hi
    return g


def _frozen(g):
    g = np.ascontiguousarray(g, dtype=np.uint8)
    g.setflags(write=False)
    return g


def _ask(pattern, found):
    return dict(pattern=pattern, found=found)


def _case(name, gray, *asks):
    return dict(name=name, gray=_frozen(gray), asks=asks)


# ---- A: the candidate cut and the ordering -------------------------------------------------------------------------------
def _noise(h, w, seed=NOISE_SEED):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _noise_ground():
    w, h = 320, 240
    Hm = CC.similarity(16, 30, 150.2, 40.4)
    g, _ = CC.render((w, h), (7, 7), Hm)
    box = (Hm @ np.array([[0, 7, 7, 0], [0, 0, 7, 7], [1, 1, 1, 1.0]]))[:2]
    ys, xs = np.mgrid[:h, :w]
    outside = (xs < box[0].min() - 8) | (xs > box[0].max() + 8) | (ys < box[1].min() - 8) | (ys > box[1].max() + 8)
    return np.where(outside, _noise(h, w), g)


def _tie_class():
    g = np.full((300, 280), GROUND, dtype=np.uint8)
    hard_board(g, 11, 23, 12, 0, 255, 10, 10)              # 10 x 22 = 220 inner corners of one response
    hard_board(g, 7, 8, 12, 120, 200, 170, 20)             # 6 x 7 = 42 of one weaker response: 36 of them survive the cut
    return g


BIG = dict(size=(262, 262), squares=(17, 17), Hm=CC.similarity(14, 3, 18, 8))      # 16 x 16 = 256 inner corners
EXTRA_AT = (270, 100)                                     # the 2 x 2-square board in the strip right of the large one
EXTRA_SQ = 12


def _one_over(lo, hi, shrink):
    """The 16 x 16 board in a frame 40 px wider (contrast divided by `shrink` round the ground when shrink > 1), and one more
    corner of levels lo / hi in the free strip."""
    g, _ = CC.render((BIG["size"][0] + 40, BIG["size"][1]), BIG["squares"], BIG["Hm"])
    if shrink > 1:
        g = (g // shrink + 60).astype(np.uint8)
    ground = int(g[0, -1])
    g[:, BIG["size"][0]:] = ground
    return hard_board(g.copy(), 2, 2, EXTRA_SQ, lo, hi, *EXTRA_AT)


def extra_rank(gray):
    """(rank of the extra corner among all candidates by (R desc, y asc, x asc), the number of candidates)."""
    c = CO.candidates(CO.response(gray))
    order = np.lexsort((c[:, 0], c[:, 1], -c[:, 2]))
    mine = np.nonzero(c[order, 0] >= BIG["size"][0])[0]
    assert len(mine) == 1
    return int(mine[0]), len(c)


@functools.lru_cache(maxsize=1)
def one_over_stronger_shrink():
    """The smallest compression g // s + 60 of the large board under which the 0 / 255 extra outranks at least one of its
    corners (the recipe: start at 2 and adjust until the property holds)."""
    for s in range(2, 9):
        rank, total = extra_rank(_one_over(0, 255, s))
        if total == CO.MAX_CANDIDATES + 1 and rank < CO.MAX_CANDIDATES:
            return s
    raise AssertionError("no compression makes the extra corner outrank a board corner")


QUADRANT_ANGLES = (30, 120, 210, 300, 75, 165, 255, 345)


def _quadrant(angle):
    """The board's centre, (4, 2.5) squares, goes to the frame's centre plus a shift of its own per angle (under 6 px): a half turn
    of the centred board would put the corners back on the same pixels."""
    a = np.deg2rad(angle)
    i = QUADRANT_ANGLES.index(angle)
    cx, cy = 109.5 + 0.83 * i, 109.5 - 0.59 * i
    tx = cx - 16 * (np.cos(a) * 4 - np.sin(a) * 2.5)
    ty = cy - 16 * (np.sin(a) * 4 + np.cos(a) * 2.5)
    return CC.render((220, 220), (8, 5), CC.similarity(16, angle, tx, ty))[0]


@functools.lru_cache(maxsize=1)
def cut_cases():
    """Part A: [case]; a case is name, gray, asks = ({pattern, found}, ...)."""
    out = [_case("noise_ground", _noise_ground(), _ask((6, 6), 1)),
           _case("pure_noise", _noise(240, 320), _ask((6, 6), 0)),
           _case("cut_inside_tie_class", _tie_class(), _ask((6, 6), 1), _ask((6, 7), 0), _ask((7, 6), 0)),
           _case("exactly_256", CC.render(BIG["size"], BIG["squares"], BIG["Hm"])[0], _ask((16, 16), 1)),
           _case("one_over_weaker", _one_over(60, 130, 1), _ask((16, 16), 1)),
           _case("one_over_stronger", _one_over(0, 255, one_over_stronger_shrink()), _ask((16, 16), 0)),
           _case("row_longer_than_limit", CC.render((260, 100), (15, 4), CC.similarity(15, 4, 12, 14))[0],
                 _ask((6, 6), 0), _ask((14, 3), 1), _ask((3, 14), 1)),
           _case("smallest_pattern", CC.render((90, 90), (3, 3), CC.similarity(20, 12, 18, 8))[0], _ask((2, 2), 1))]
    return tuple(out)


@functools.lru_cache(maxsize=1)
def quadrant_frames():
    """uint8 [8,220,220]: the 8 x 5 board at QUADRANT_ANGLES."""
    return _frozen(np.stack([_quadrant(a) for a in QUADRANT_ANGLES]))


QUADRANT_PATTERNS = ((7, 4), (4, 7))


def cut_by_name(name):
    return next(c for c in cut_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def helper(name, pattern):
    """The helper (want=True) on a part-A case, computed once per (case, pattern)."""
    return CO.find_chessboard_corners(cut_by_name(name)["gray"], pattern, want=True)


@functools.lru_cache(maxsize=None)
def quadrant_helper(i, pattern):
    return CO.find_chessboard_corners(quadrant_frames()[i], pattern, want=True)


def best_rotation(gray, pattern):
    """Which of the four rotations `chess_oracle.labelled` (the `best` of k_chess_order) chose for the lattice found in `gray`:
    k of np.rot90(grid, -k), read by handing the helper a `labelled` that looks at the grid before passing it on."""
    seen, inner = [], CO.labelled

    def spy(grid, x, y, pw, ph):
        got = inner(grid, x, y, pw, ph)
        g = np.asarray(grid)
        seen.extend(k for k in range(4) if np.rot90(g, -k).shape == (ph, pw) and np.array_equal(np.rot90(g, -k).reshape(-1), got))
        return got

    CO.labelled = spy
    try:
        found, _ = CO.find_chessboard_corners(gray, pattern)
    finally:
        CO.labelled = inner
    assert found and len(seen) == 1
    return seen[0]


def sorted_candidates(gray):
    """All candidates by (R desc, y asc, x asc): int64 [M,3] of (x, y, R)."""
    c = CO.candidates(CO.response(gray))
    return c[np.lexsort((c[:, 0], c[:, 1], -c[:, 2]))]


# ---- B: tile seams, small frames, the launch split ---------------------------------------------------------------------
SEAM_OFFSETS = tuple([(dx, 0) for dx in range(32)] + [(0, dy) for dy in range(1, 16)] + [(31, 15), (17, 9)])
SEAM_PATTERN = (3, 3)


@functools.lru_cache(maxsize=1)
def seam_frames():
    """uint8 [49,96,128]: a 4 x 4-square hard board stepped over every column and row phase of a 32 x 16 tile."""
    out = np.full((len(SEAM_OFFSETS), 96, 128), GROUND, dtype=np.uint8)
    for g, (dx, dy) in zip(out, SEAM_OFFSETS):
        hard_board(g, 4, 4, 12, 30, 220, 20 + dx, 12 + dy)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def seam_helper(i):
    return CO.find_chessboard_corners(seam_frames()[i], SEAM_PATTERN, want=True)


SMALL_SHAPES = ((1, 1), (10, 40), (40, 10), (11, 11), (12, 33), (16, 32), (17, 33))      # (h, w)
# per shape, the first seed of default_rng whose noise has a candidate where one can exist (the host test holds it to that)
SMALL_SEEDS = {(1, 1): 0, (10, 40): 0, (40, 10): 0, (11, 11): 25, (12, 33): 0, (16, 32): 0, (17, 33): 0}
SMALL_PATTERN = (2, 2)


def first_small_seed(shape):
    """The seed SMALL_SEEDS must record: the first whose frame has a candidate (0 for frames with a side below 11)."""
    if min(shape) < 11:
        return 0
    return next(s for s in range(1000) if len(CO.candidates(CO.response(_noise(*shape, seed=s)))))


@functools.lru_cache(maxsize=None)
def small_frame(shape):
    return _frozen(_noise(*shape, seed=SMALL_SEEDS[shape]))


SPLIT_FRAMES = 65537                                      # gridDim.z holds 65 535: a second launch of two frames
SPLIT_PATTERN = (2, 2)


@functools.lru_cache(maxsize=1)
def split_distinct():
    """uint8 [7,36,36]: a 3 x 3-square board of about 8 px at five sub-pixel placements, a 4 x 3-square board (3 x 2 corners: the
    walk refuses it as larger than 2 x 2), and the first placement inverted at a sixty-fourth of the contrast."""
    size = (36, 36)
    place = ((8.0, 0.0, 6.3, 5.6), (8.0, 10.0, 8.4, 4.2), (8.0, -15.0, 4.7, 9.9), (8.5, 25.0, 11.2, 2.1), (7.5, 45.0, 18.1, 2.4))
    out = [CC.render(size, (3, 3), CC.similarity(*p))[0] for p in place]
    out.append(CC.render(size, (4, 3), CC.similarity(8.0, 5.0, 2.5, 6.3))[0])
    out.append(CC.render(size, (3, 3), CC.similarity(*place[0]), invert=True)[0] // 64 + 100)
    return _frozen(np.stack(out))


@functools.lru_cache(maxsize=None)
def split_helper(i):
    return CO.find_chessboard_corners(split_distinct()[i], SPLIT_PATTERN, want=True)


# ---- C: k_corner_subpix ------------------------------------------------------------------------------------------------
def base():
    """(gray, the helper's corners) of `rotated_30`."""
    return CC.by_name("rotated_30")["gray"], CC.helper_results()["rotated_30"]["corners"]


def _kw(win, zero_zone=(-1, -1), max_iter=30, eps=1e-3):
    return dict(win=win, zero_zone=zero_zone, max_iter=max_iter, eps=eps)


WINDOW_SETTINGS = (_kw((15, 15)), _kw((15, 1)), _kw((1, 15)), _kw((1, 1)), _kw((5, 3), (1, 0)), _kw((7, 7), (0, 0)),
                   _kw((11, 11), (3, 3)), _kw((3, 9), (2, -1)), _kw((11, 11), (11, 11)), _kw((5, 5), max_iter=1),
                   _kw((5, 5), max_iter=30, eps=0.0))


def setting_id(kw):
    return "win{}x{}-zone{}x{}-it{}-eps{:g}".format(*kw["win"], *kw["zero_zone"], kw["max_iter"], kw["eps"])


CROP_MARGIN = 6
BORDER_WINDOWS = ((5, 5), (11, 11), (15, 15))


@functools.lru_cache(maxsize=1)
def near_border():
    """`rotated_30` cropped to its peaks +- CROP_MARGIN px (a contiguous copy)."""
    gray = CC.by_name("rotated_30")["gray"]
    p = CC.helper_results()["rotated_30"]["peaks"]
    x0, x1, y0, y1 = p[:, 0].min() - CROP_MARGIN, p[:, 0].max() + CROP_MARGIN, p[:, 1].min() - CROP_MARGIN, p[:, 1].max() + CROP_MARGIN
    return _frozen(gray[y0:y1 + 1, x0:x1 + 1])


@functools.lru_cache(maxsize=1)
def near_border_helper():
    return CO.find_chessboard_corners(near_border(), (6, 6), want=True)


def survive_starts():
    """float64 [k,2] on the cropped image: outside each border, the two corners of the frame, then a row of valid starts with
    NaN, +inf and 2e9 mixed in; and the mask of the rows the kernel must leave bit-identical with iters = 0."""
    h, w = near_border().shape
    valid = near_border_helper()["corners"][:6]
    rows = [(-2.5, 30.0), (w + 1.5, 40.0), (30.0, -0.5), (50.0, h + 3.0), (0.0, 0.0), (np.nextafter(w, 0.0), np.nextafter(h, 0.0)),
            valid[0], (np.nan, 40.0), valid[1], (50.0, np.inf), valid[2], (2e9, 30.0), valid[3], (np.nan, np.nan), valid[4],
            (30.0, -2e9), valid[5]]
    pts = np.array(rows, dtype=np.float64)
    return pts, ~(np.abs(pts) < 1e9).all(axis=1)


def flat_frames():
    """[(name, gray 40 x 50, starts)]: a uniform frame and a vertical step edge; starts inside and on the edges, with fractions
    that are exact in binary (the bilinear patch is then exact, and a flat direction gives a determinant of exactly 0)."""
    flat = np.full((40, 50), 128, dtype=np.uint8)
    step = np.zeros((40, 50), dtype=np.uint8)
    step[:, 25:] = 200
    starts = np.array([(20.0, 20.0), (24.5, 10.25), (25.0, 30.5), (0.0, 0.0), (49.0, 39.0), (49.5, 12.0), (12.75, 39.5), (0.0, 20.0),
                       (26.25, 0.0)])
    return (("uniform", _frozen(flat), starts), ("step_edge", _frozen(step), starts))


RETURN_OFFSET = (2.6, -2.3)


def return_starts():
    return base()[1] + np.array(RETURN_OFFSET)


@functools.lru_cache(maxsize=1)
def subpix_cases():
    """Every part-C run that is held to the helper by position: {label: (gray, finite starts float64 [k,2], keywords)}."""
    gray, corners = base()
    out = {setting_id(kw): (gray, corners, kw) for kw in WINDOW_SETTINGS}
    for win in BORDER_WINDOWS:
        out["near_border-win{}x{}".format(*win)] = (near_border(), near_border_helper()["corners"], _kw(win))
    pts, frozen = survive_starts()
    out["survive"] = (near_border(), pts[~frozen], _kw((5, 5)))
    out["return_to_start-win2x2"] = (gray, return_starts(), _kw((2, 2)))
    out["return_to_start-win5x5"] = (gray, return_starts(), _kw((5, 5)))
    return out


@functools.lru_cache(maxsize=None)
def subpix_helper(label, reverse=False):
    """(refined, iterations) of the helper on a part-C case, computed once; `reverse` sums in the opposite order."""
    gray, starts, kw = subpix_cases()[label]
    return CO.corner_subpix(gray, starts, reverse=reverse, **kw)
