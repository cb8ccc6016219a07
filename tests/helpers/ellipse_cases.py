"""Frames for the last step of `_marker_center` (contour-vertex moments, ellipse fit, centre matching): area masks built from
small tiles, and masks that put band centroids where the matching has to decide.  CPU only.

A frame is (mask uint8 {0, 1}, area uint8 {0, 255}) like tests/helpers/label_cases.py.  Tiles are placed with a gap of at
least 6 background pixels, so neither the 5x5 opening nor the contours of two tiles interact; mask pieces are 1 to 4 pixels
and at least 2 pixels apart, so each is one band component whose centroid is the piece's (the band filter keeps every pixel of
a blob smaller than its window).

Every family is built with mask = area (`kind` "self": the one band centroid of a tile is its own), and - except `squares2`
and `large` - once more with mask pieces (`kind` "pieces"): per tile copy one piece whose centroid lies on the quarter- /
third-pixel lattice (fractions 0, 1/4, 1/3, 1/2, 2/3, 3/4, in the pairs the pieces below can produce) inside the disc of
radius minor / 10 about the oracle's ellipse centre, chosen so that the copies of a tile reach different branches of
`inside_polygon`; every second copy gets a second piece (nearest wins; the farther one comes first in raster order where
possible, and exactly equidistant pairs are taken where a tile has them: first index wins).  A centre can never be claimed by
two contours: the polygons of two external contours are disjoint (their pixels are not 8-adjacent), so the sequential replay
of k_finalize is reached only through VBS_OPT_FORCE_SEQ_MATCH.  Contours that must not match (fewer than 5 vertices, minor
axis below 5) get a piece at their centre all the same.

`frames(geometry)` returns the list for one of GEOMETRIES; `analyse(frame)` the per-contour references (cached on the frame).
"""
import functools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import stages as O

import ellipse_oracle as E

GEOMETRIES = [(64, 128), (480, 640), (520, 640), (130, 4096), (1200, 1920)]
MAX_COMPONENTS = 400                       # per frame: below CCL_OPEN_COMPS = 512
MAX_FRAMES = 32                            # per geometry
GAP = 6


@dataclass
class Tile:
    family: str
    name: str
    shape: np.ndarray                      # bool, cropped to its bounding box


@dataclass
class Frame:
    family: str
    kind: str                              # "self" | "pieces"
    name: str
    mask: np.ndarray
    area: np.ndarray
    tiles: List[Tuple[Tile, int, int]] = field(default_factory=list)      # (tile, y0, x0) of the bounding box (may be clipped)
    info: Optional[dict] = None
    placed: List[dict] = field(default_factory=list)                      # pieces: contour index, centroid, branch, decision


# ---------------------------------------------------------------------------------------------------------------------
# tiles
def _crop(m: np.ndarray) -> np.ndarray:
    ys, xs = np.nonzero(m)
    return m[ys.min():ys.max() + 1, xs.min():xs.max() + 1]


def squares(offsets) -> np.ndarray:
    m = np.zeros((24, 24), bool)
    m[9:14, 9:14] = True
    for dx, dy in offsets:
        m[9 + dy:14 + dy, 9 + dx:14 + dx] = True
    return _crop(m)


def digitised_ellipse(a: float, b: float, angle, cx: float = 0.0, cy: float = 0.0) -> np.ndarray:
    """pixels (x, y) with ((u / a)^2 + (v / b)^2 <= 1), (u, v) the pixel centre in the ellipse's axes; the centre is
    (cx, cy) plus an integer.  angle: radians, or "p45" / "m45" for exactly +-45 degrees (u, v from integer sums), 0 and
    "90" exact as well."""
    r = int(math.ceil(max(a, b))) + 2
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    x, y = xx - cx, yy - cy
    if angle in ("p45", "m45"):
        sg = 1.0 if angle == "p45" else -1.0
        u2, v2 = (x + sg * y) ** 2 / 2.0, (y - sg * x) ** 2 / 2.0
    elif angle == "90":
        u2, v2 = y * y, x * x
    else:
        c, s = math.cos(angle), math.sin(angle)
        u2, v2 = (x * c + y * s) ** 2, (y * c - x * s) ** 2
    m = u2 / (a * a) + v2 / (b * b) <= 1.0
    return _crop(m) if m.any() else m[:1, :1]


ANGLES = [0.0, "90", "p45", "m45", 0.05, 0.2, 0.4, 0.6, 1.0, 1.3, 1.52, 1.62, 1.9, 2.3, 2.7, 3.09]
AXES = [(4.5, 3.2), (6.0, 3.2), (7.3, 4.5), (9.0, 6.0), (12.5, 4.5), (12.5, 9.0), (16.0, 7.3), (20.0, 3.2), (20.0, 12.5),
        (20.0, 16.0)]


@functools.lru_cache(maxsize=None)
def tiles_squares2() -> List[Tile]:
    return [Tile("squares2", f"sq2_{dx}_{dy}", squares([(dx, dy)])) for dy in range(-6, 7) for dx in range(-6, 7)]


@functools.lru_cache(maxsize=None)
def tiles_squares3(count: int = 300, seed: int = 11) -> List[Tile]:
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < count:
        o = tuple(sorted((int(rng.integers(-6, 7)), int(rng.integers(-6, 7))) for _ in range(2)))
        if o in seen:
            continue
        seen.add(o)
        m = squares(o)
        if ndimage.label(m, structure=np.ones((3, 3), bool))[1] != 1:
            continue
        out.append(Tile("squares3", "sq3_%d_%d_%d_%d" % (o[0] + o[1]), m))
    return out + [Tile("squares3", "sq3_%d_%d_%d_%d" % (o[0] + o[1]), squares(o)) for o in RARE if o not in seen]


# unions found by a search over all pairs of offsets (not part of the seeded sample): the ellipse centre lies within
# minor / 10 of a convex corner (one pixel of the cell), or of a pinch between two squares that touch at a corner
RARE = [((-1, 5), (5, -1)), ((1, -5), (6, -6)), ((1, 5), (6, 6)), ((5, 1), (6, 6)), ((-6, -6), (-1, -5)), ((-1, -5), (5, 1)),
        ((-6, -5), (-5, 5)), ((-5, 5), (6, 4)), ((-5, 5), (-2, 6)), ((-5, 5), (6, 0)), ((-5, -5), (6, -6)), ((-6, -1), (5, 5)),
        ((5, 5), (6, -5)), ((-5, -5), (2, 6))]


@functools.lru_cache(maxsize=None)
def tiles_ellipses() -> List[Tile]:
    out = []
    for k, (a, b) in enumerate(AXES):
        for j, ang in enumerate(ANGLES):
            sym = ang in (0.0, "90", "p45", "m45")
            # exactly symmetric digitisations: centre on a pixel centre or a pixel corner; the others off both
            cx, cy = ((0.0, 0.0) if (k + j) % 2 else (0.5, 0.5)) if sym else (0.3 + 0.07 * j, 0.6 - 0.05 * k)
            out.append(Tile("ellipses", f"el_{a}_{b}_{ang}", digitised_ellipse(a, b, ang, cx, cy)))
    for r in (3.2, 5.0, 8.5, 13.0, 20.0):                                  # circles, and near-circles 99.5 / 100
        out.append(Tile("ellipses", f"circle_{r}", digitised_ellipse(r, r, 0.0, 0.0, 0.0)))
        out.append(Tile("ellipses", f"circle_{r}_off", digitised_ellipse(r, r, 0.0, 0.37, 0.21)))
    for a in (10.0, 20.0):
        for ang in (0.0, "90", 0.7):
            out.append(Tile("ellipses", f"near_{a}_{ang}", digitised_ellipse(a, a * 0.995, ang, 0.0, 0.0)))
    for a, b in ((100.0, 2.7), (110.0, 3.0), (60.0, 3.3)):                 # aspect ratios up to about 40
        for ang in (0.0, "90", 0.015):
            out.append(Tile("ellipses", f"thin_{a}_{b}_{ang}", digitised_ellipse(a, b, ang, 0.0, 0.5)))
    return out


@functools.lru_cache(maxsize=None)
def tiles_minor5() -> List[Tile]:
    """shapes whose exact minor axis falls in [4.9, 5.1]: a scan over the minor semi-axis of tilted ellipses (upright ones
    jump from 4.x to 5.8 as their opened core gains a row), one tile per distinct opened outline."""
    out, shapes, outlines = [], set(), set()
    for a in (9.0, 10.0, 12.0):
        for ang in (0.2, 0.3, 1.2, 1.4):
            for cxy in ((0.0, 0.0), (0.5, 0.5), (0.3, 0.1)):
                for b100 in range(260, 300, 2):
                    m = digitised_ellipse(a, b100 / 100.0, ang, *cxy)
                    if (m.shape, m.tobytes()) in shapes:
                        continue
                    shapes.add((m.shape, m.tobytes()))
                    c = O.find_contours_external(O.morph_open5(np.pad(m, 4)))
                    if len(c) != 1 or len(c[0]) < 5 or c[0].tobytes() in outlines:
                        continue
                    outlines.add(c[0].tobytes())
                    ex = E.exact_fit(c[0])
                    if ex is not None and 4.9 <= float(ex["w_exact"]) <= 5.1:
                        out.append(Tile("minor5", f"m5_{a}_{b100 / 100.0}_{ang}_{cxy[0]}", m))
    return out


def reach(t: Tile) -> set:
    """the (branch, decision) pairs a piece can reach on the tile standing alone in the interior of a frame."""
    f = Frame("x", "self", "x", None, np.pad(t.shape, 8))
    info = analyse(f)
    out = set()
    for ci, p in enumerate(info["per"]):
        if p["oracle"] is not None and min(p["oracle"][2:4]) >= 5.0:
            out |= {(c[3], c[4]) for c in candidates(info, ci, *f.area.shape)}
    return out


@functools.lru_cache(maxsize=None)
def tiles_border() -> List[Tile]:
    """for every (branch, decision) the first two unions of three squares that reach it, and six small ellipses."""
    pick, count = {}, {}
    for t in tiles_squares3():
        for lab in sorted(reach(t)):
            if lab[0] != "four" and count.get(lab, 0) < 2:
                count[lab] = count.get(lab, 0) + 1
                pick.setdefault(t.name, t)
    el = [t for t in tiles_ellipses() if max(t.shape.shape) <= 28][::9][:6]
    return [Tile("border", t.name, t.shape) for t in list(pick.values()) + el]


# ---------------------------------------------------------------------------------------------------------------------
# frames
def _blank(h, w):
    return np.zeros((h, w), bool)


def _ncomp(m: np.ndarray) -> int:
    from scipy import ndimage
    return int(ndimage.label(m, structure=np.ones((3, 3), bool))[1])


def _pack(h: int, w: int, tiles: List[Tile], family: str, limit: int = MAX_COMPONENTS - 20) -> List[Frame]:
    """shelves, left to right and top to bottom, GAP pixels between boxes and to the frame's edges."""
    frames, cur, x, y, shelf, n = [], None, GAP, GAP, 0, 0
    for t in sorted(tiles, key=lambda t: -t.shape.shape[0]):
        th, tw = t.shape.shape
        assert th + 2 * GAP <= h and tw + 2 * GAP <= w, (t.name, h, w)
        if cur is not None and x + tw + GAP > w:
            x, y, shelf = GAP, y + shelf + GAP, 0
        if cur is None or y + th + GAP > h or n + _ncomp(t.shape) > limit:
            cur = Frame(family, "self", f"{family}_{len(frames)}", None, _blank(h, w))
            frames.append(cur)
            x, y, shelf, n = GAP, GAP, 0, 0
        cur.area[y:y + th, x:x + tw] |= t.shape
        cur.tiles.append((t, y, x))
        x, shelf, n = x + tw + GAP, max(shelf, th), n + _ncomp(t.shape)
    return frames


def _border_frames(h: int, w: int, tiles: List[Tile]) -> List[Frame]:
    """six tiles per frame: the corners and the middles of the long edges.  First every tile twice, flush with its edges
    (the outline is the interior one); then every tile once more, pushed 1, 2, 3 pixels or half its size out of the frame,
    so that the opening meets 4- and 3-thick remains and ellipse centres reach the first and last two rows and columns."""
    frames = []
    slots = [(t, 0) for t in tiles for _ in range(2)] + [(t, 1 + k % 4) for k, t in enumerate(tiles)]
    for k in range(0, len(slots), 6):
        f = Frame("border", "self", f"border_{len(frames)}", None, _blank(h, w))
        for slot, (t, push) in enumerate(slots[k:k + 6]):
            th, tw = t.shape.shape
            px, py = (tw // 2, th // 2) if push == 4 else (push, push)
            col, row = slot % 3, slot // 3
            x0 = (-px, (w - tw) // 2, w - tw + px)[col]
            y0 = -py if row == 0 else h - th + py
            ys, xs = max(0, y0), max(0, x0)
            ye, xe = min(h, y0 + th), min(w, x0 + tw)
            f.area[ys:ye, xs:xe] |= t.shape[ys - y0:ye - y0, xs - x0:xe - x0]
            f.tiles.append((t, y0, x0))
        frames.append(f)
    return frames


NOTCHES = ((6.0, 1), (6.2, 1), (6.3, 1), (6.4, 1), (6.6, 1), (6.8, 1))


def _notch_frames(h: int, w: int) -> List[Frame]:
    """cells in rows or columns 0 to 1 (and the last two).  A contour whose minor axis reaches 5 keeps its ellipse centre
    two pixels and more inside the frame unless the frame's edge cuts the shape in half, so: discs centred on the frame's
    edges and corners, with a notch of 1 or 2 pixels at the edge, which the opening keeps (its squares may hang over the
    edge).  Their ellipse centres lie 2 to 4 pixels from the edge, and some of the disc of radius minor / 10 about them
    reaches row / column 1.  The cells it reaches there are whole, on-row and on-column ones: searches over clipped unions of
    three squares and over notch widths, depths and radii found no contour whose disc holds a three-of-four or a diagonal
    cell in the first two rows or columns."""
    frames = []
    yy, xx = np.mgrid[0:h, 0:w]
    for k, (r, nd) in enumerate(NOTCHES):
        f = Frame("border", "self", f"border_notch_{k}", None, _blank(h, w))
        o = 0.5 * (k % 2)
        for cx, cy in ((-0.5, -0.5), (44 + o, -0.5), (-0.5, 36 + o), (w - 0.5, 30 - o), (88 - o, h - 0.5), (w - 0.5, h - 0.5),
                       (w - 0.5, -0.5)):
            f.area |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
            x0, y0 = int(math.floor(min(max(cx, 0), w - 1))), int(math.floor(min(max(cy, 0), h - 1)))
            nw, dp = nd if isinstance(nd, tuple) else (nd, nd)
            xs = slice(x0, x0 + nw) if cx < w - 1 else slice(w - nw, w)
            ys = slice(y0, y0 + nw) if cy < h - 1 else slice(h - nw, h)
            if 0 <= cx < w - 1:                         # on the top / bottom edge: the notch opens to that edge
                ys = slice(0, dp) if cy < 0 else slice(h - dp, h)
            if 0 <= cy < h - 1:
                xs = slice(0, dp) if cx < 0 else slice(w - dp, w)
            f.area[ys, xs] = False
        frames.append(f)
    return frames


def _large(h: int, w: int) -> List[Frame]:
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    if (h, w) == (130, 4096):
        a, b, th = 2030.0, 55.0, 0.002
        x, y = xx - 2047.3, yy - 64.6
        u, v = x * math.cos(th) + y * math.sin(th), y * math.cos(th) - x * math.sin(th)
        out.append(("thin", (u / a) ** 2 + (v / b) ** 2 <= 1.0))
    else:
        a, b, th = 860.0, 530.0, 0.4
        x, y = xx - 959.3, yy - 599.6
        u, v = x * math.cos(th) + y * math.sin(th), y * math.cos(th) - x * math.sin(th)
        out.append(("ellipse", (u / a) ** 2 + (v / b) ** 2 <= 1.0))
        # a band of the same extent whose four edges step diagonally: a pixel per row (column) for 7, then back
        saw_y, saw_x = (yy.astype(np.int64) % 7), (xx.astype(np.int64) % 7)
        out.append(("sawtooth", (xx >= 100 + saw_y) & (xx <= 1810 + saw_y) & (yy >= 60 + saw_x) & (yy <= 1130 + saw_x)))
    frames = []
    for name, m in out:
        f = Frame("large", "self", f"large_{name}", None, m)
        frames.append(f)
    return frames


def _finish_self(f: Frame) -> Frame:
    f.mask = f.area.astype(np.uint8)
    f.area = f.area.astype(np.uint8) * 255
    return f


# ---------------------------------------------------------------------------------------------------------------------
# references per frame
TALL = {"near": 5000, "over": 7800}


def tall_frame(which: str) -> Frame:
    """The range of the int64 moments: a 24-pixel bar over the whole height of a 128-pixel-wide frame whose edges
    run at a slope of 1/2 - a pixel sideways every second row, which the 5x5 opening keeps and which makes every border
    pixel a contour vertex - to and fro.  With 7800 rows sum y^4 about the first pixel passes 2^63 ("over": every route
    must report VBS_ECAPACITY); with 5000 rows it is a seventh of that and the moments must be exact ("near").  The mask
    is a single pixel in the middle of the bar."""
    h, w = TALL[which], 128
    ph = np.arange(h) % 80
    x0 = 30 + np.where(ph < 40, ph // 2, (79 - ph) // 2)
    xx = np.arange(w)[None, :]
    area = (xx >= x0[:, None]) & (xx < x0[:, None] + 24)
    f = _finish_self(Frame("tall", "self", f"tall_{which}", None, area))
    f.mask = np.zeros((h, w), np.uint8)                    # one band centroid, beside the ellipse centre
    f.mask[h // 2, x0[h // 2] + 11] = 1
    return f


def moment_guard(moments, h: int, w: int) -> float:
    """the quantity k_finalize holds below 9e18: n + sum x^2 (w - 1)^2 + sum y^2 (h - 1)^2, an upper bound of every |sum|."""
    return float(moments[0] + moments[3] * (w - 1) ** 2 + moments[5] * (h - 1) ** 2)


def analyse(f: Frame, fits: bool = True) -> dict:
    """opened mask, contours (oracle order), id image, and per contour: first pixel, moments, oracle fit, exact fit."""
    if f.info is not None:
        return f.info
    opened = O.morph_open5(np.asarray(f.area) != 0)
    contours = O.find_contours_external(opened)
    per = []
    for c in contours:
        fp = E.first_pixel(c)
        d = dict(first=fp, n=len(c), moments=E.vertex_moments(c, fp), oracle=None, exact=None)
        if len(c) >= 5 and fits:
            (cx, cy), (w, h), ang = O.fit_ellipse(c)
            d["oracle"] = (cx, cy, w, h, ang)
            d["exact"] = E.exact_fit(c)
        per.append(d)
    f.info = dict(opened=opened, contours=contours, ids=E.contour_id_image(opened, contours), per=per)
    return f.info


# pieces: pixels (x, y) relative to a base pixel; every rotation / reflection is generated below
_BASE_PIECES = {"single": [(0, 0)], "domino": [(0, 0), (1, 0)], "ltromino": [(0, 0), (1, 0), (0, 1)],
                "bar4": [(0, 0), (1, 0), (2, 0), (3, 0)], "ltetromino": [(0, 0), (0, 1), (0, 2), (1, 2)],
                "ttetromino": [(0, 0), (1, 0), (2, 0), (1, 1)]}


def _orientations():
    out = {}
    for name, px in _BASE_PIECES.items():
        for rot in range(4):
            for flip in (False, True):
                q = px
                for _ in range(rot):
                    q = [(-y, x) for x, y in q]
                if flip:
                    q = [(-x, y) for x, y in q]
                mx, my = min(x for x, _ in q), min(y for _, y in q)
                q = tuple(sorted((x - mx, y - my) for x, y in q))
                out.setdefault(q, name)
    return out


PIECES = _orientations()                    # {pixels: name}


def candidates(info: dict, ci: int, h: int, w: int, reach: float = 1.0):
    """[(pixels (absolute), centroid (x, y), d2, branch, decision)] for contour ci: every piece position whose centroid lies
    within `reach` * minor / 10 of the oracle's ellipse centre (strictly inside for reach = 1, like the reference's `<`)."""
    p = info["per"][ci]
    cx, cy, wd, ht, _ = p["oracle"]
    rad = min(wd, ht) / 10.0 * reach
    cid = len(info["contours"]) - 1 - ci
    out = []
    for px, name in PIECES.items():
        n = len(px)
        ox, oy = sum(x for x, _ in px) / n, sum(y for _, y in px) / n
        for by in range(int(math.floor(cy - rad - oy)), int(math.ceil(cy + rad - oy)) + 1):
            for bx in range(int(math.floor(cx - rad - ox)), int(math.ceil(cx + rad - ox)) + 1):
                absx = [(bx + x, by + y) for x, y in px]
                if any(not (0 <= x < w and 0 <= y < h) for x, y in absx):
                    continue
                # the centroid as the pipeline forms it: integer sums, one division
                gx, gy = sum(x for x, _ in absx) / n, sum(y for _, y in absx) / n
                d2 = (gx - cx) ** 2 + (gy - cy) ** 2
                if not d2 < rad * rad:
                    continue
                ids, fx, fy = E.cell_and_fraction(info["opened"], info["ids"], (gx, gy))
                br, dec = E.cell_branch(ids, fx, fy, cid)
                out.append((tuple(absx), (gx, gy), d2, br, dec, name))
    return out


def _free(mask: np.ndarray, px) -> bool:
    h, w = mask.shape
    for x, y in px:
        if mask[max(0, y - 2):y + 3, max(0, x - 2):x + 3].any():
            return False
    return True


def place_pieces(f: Frame, seen: Dict, copy_of: Dict[int, int]) -> Frame:
    """the "pieces" twin of a "self" frame: the same area, mask pieces chosen per contour.  `seen` counts (branch, decision)
    over everything placed so far (rare ones are preferred); copy_of[ci] = which copy of its tile contour ci is."""
    info = analyse(f)
    h, w = f.area.shape
    g = Frame(f.family, "pieces", f.name + "_pieces", np.zeros((h, w), np.uint8), f.area, f.tiles, info)
    for ci, p in enumerate(info["per"]):
        if p["oracle"] is None or min(p["oracle"][2:4]) < 5.0:
            cx, cy = (p["oracle"][:2] if p["oracle"] else np.asarray(info["contours"][ci]).reshape(-1, 2).mean(0))
            px = [(int(round(cx)), int(round(cy)))]
            if 0 <= px[0][0] < w and 0 <= px[0][1] < h and _free(g.mask, px):
                g.mask[px[0][1], px[0][0]] = 1
                g.placed.append(dict(contour=ci, centroid=(float(px[0][0]), float(px[0][1])), branch="no_fit", decision=False))
            continue
        cand = [c for c in candidates(info, ci, h, w) if _free(g.mask, c[0])]
        if not cand:
            continue
        k = copy_of.get(ci, 0)
        edge = "notch" in f.name                           # there: a centroid in rows / columns 0 to 1 before anything else
        cand.sort(key=lambda c: (not (edge and min(c[1]) < 2.0), seen.get((c[3], c[4]), 0), c[2]))
        first = cand[0]
        chosen = [first]
        if k % 2 == 1:                                     # two pieces: exactly equidistant ones if the tile has a pair, else
            def apart(a, b):                               # the rarest-branch piece and a farther one that raster order puts first
                return all(max(abs(xa - xb), abs(ya - yb)) >= 2 for xa, ya in a[0] for xb, yb in b[0])
            inside = sorted((c for c in cand if c[4]), key=lambda c: c[2])
            pair = next(((a, b) for i, a in enumerate(inside) for b in inside[i + 1:i + 40]
                         if a[2] == b[2] and a[2] > 0 and apart(a, b)), None)
            if pair and ci % 2 == 0:
                chosen = list(pair)
            else:
                far = [c for c in inside if c[2] > first[2] and apart(c, first)]
                chosen += sorted(far, key=lambda c: (c[0][0][1], c[0][0][0]))[:1]
        for c in chosen:
            for x, y in c[0]:
                g.mask[y, x] = 1
            seen[(c[3], c[4])] = seen.get((c[3], c[4]), 0) + 1
            g.placed.append(dict(contour=ci, centroid=c[1], branch=c[3], decision=c[4], d2=c[2], piece=c[5],
                                 second=c is not chosen[0]))
    return g


def _copies(tiles: List[Tile], k: int) -> List[Tile]:
    return [t for t in tiles for _ in range(k)]


def _copy_index(f: Frame) -> Dict[int, int]:
    """contour index -> running copy number of its tile within the frame (contours found by their tile's box)."""
    info = analyse(f)
    count: Dict[str, int] = {}
    box = []
    for t, y0, x0 in f.tiles:
        box.append((y0, x0, y0 + t.shape.shape[0], x0 + t.shape.shape[1], count.get(t.name, 0)))
        count[t.name] = count.get(t.name, 0) + 1
    out = {}
    for ci, p in enumerate(info["per"]):
        x, y = p["first"]
        for y0, x0, y1, x1, k in box:
            if y0 <= y < y1 and x0 <= x < x1:
                out[ci] = k
                break
    return out


_CACHE: Dict[Tuple[int, int], List[Frame]] = {}


def frames(h: int, w: int) -> List[Frame]:
    """every frame of geometry (h, w): "self" frames first, then their "pieces" twins."""
    if (h, w) in _CACHE:
        return _CACHE[(h, w)]
    if (h, w) in ((130, 4096), (1200, 1920)):
        out = [_finish_self(f) for f in _large(h, w)]
    else:
        if (h, w) == (64, 128):
            selfs = _border_frames(h, w, tiles_border())[:MAX_FRAMES // 2 - 6] + _notch_frames(h, w)
        elif (h, w) == (480, 640):
            selfs = (_pack(h, w, tiles_squares2(), "squares2") + _pack(h, w, _copies(tiles_squares3(), 3), "squares3")
                     + _pack(h, w, _copies(tiles_ellipses(), 2), "ellipses") + _pack(h, w, _copies(tiles_minor5(), 2), "minor5"))
        else:                                              # the large-image parameter set (window 14), one copy of each
            selfs = (_pack(h, w, tiles_squares3()[:150], "squares3") + _pack(h, w, tiles_ellipses(), "ellipses")
                     + _pack(h, w, tiles_minor5(), "minor5"))
        seen: Dict = {}
        twins = [place_pieces(f, seen, _copy_index(f)) for f in selfs if f.family != "squares2"]
        out = [_finish_self(f) for f in selfs] + twins
        for g in twins:
            g.area = np.where(np.asarray(g.area) != 0, 255, 0).astype(np.uint8)
    assert len(out) <= MAX_FRAMES, len(out)
    for f in out:
        assert len(analyse(f)["contours"]) <= MAX_COMPONENTS
    _CACHE[(h, w)] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
def band_centres(f: Frame) -> np.ndarray:
    """the band centroids of the frame's mask as (x, y) float64 rows, in the reference's order."""
    c, _, n = O.band_centroids(f.mask)
    return np.asarray(c, np.float64).reshape(-1, 2)[:, ::-1] if n else np.zeros((0, 2))


def boundary_contours(info: dict, centres: np.ndarray, rel: float = 1e-9) -> Dict[int, str]:
    """contours on a decision boundary -> why: "minor" (exact minor axis within 1 float32 ulp of 5), "thr" (a centre's squared
    distance within `rel` of the threshold), "near" (two admissible centres within `rel` of each other, not equal) or "equal"
    (exactly equidistant: the first index wins, which holds only for the very same ellipse centre)."""
    out = {}
    for ci, p in enumerate(info["per"]):
        if p["oracle"] is None:
            continue
        cx, cy, w, h, _ = p["oracle"]
        if abs(float(p["exact"]["w_exact"]) - 5.0) <= E.ulp32(5.0):
            out[ci] = "minor"
            continue
        minor = min(w, h)
        if minor < 5.0 or not len(centres):
            continue
        thr = (minor / 10.0) ** 2
        d = (centres[:, 0] - cx) ** 2 + (centres[:, 1] - cy) ** 2
        if (np.abs(d - thr) <= rel * thr).any():
            out[ci] = "thr"
            continue
        near = [(float(d[i]), i) for i in np.nonzero(d < thr)[0]
                if O.point_polygon_test(info["contours"][ci], tuple(centres[i])) >= 0]
        near.sort()
        if len(near) >= 2 and near[1][0] - near[0][0] <= rel * near[1][0]:
            out[ci] = "equal" if near[1][0] == near[0][0] else "near"
    return out
