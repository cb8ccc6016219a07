"""Mask / area-mask cases for the labelling stage of `_marker_center` (band mask -> components -> 5x5 opening -> external
contours -> ellipse fits -> centre matching), and the capacity outcome each one must have.  CPU only: NumPy, SciPy and
the oracle's own restatements.

`label_cases(h, w, seed)` returns a list of `Case`: `mask` uint8 {0, 1} and `area` uint8 {0, 255} of shape (h, w) - the
two-valued inputs `vbs_marker_center` takes - a class (`ragged`, `holes`, `matching`, `crowded`), a name, and the
properties the class claims (checked by tests/test_label_cases.py, relied on by tests/test_gpu_labelling_oracle.py).

Capacity rule (`expected_capacity`), restated from the general labelling kernel k_label.hip, which every route hands a
frame to when its own tables give out, so that the rule is the same on every route:
  * k_label.hip:335  `nruns > VBS_RUN_CAP` (30 720, common.h:16) for any mask it labels -> VBS_ECAPACITY.  The masks
    are the band mask, the opened area mask and - only when the opened mask has holes - its complement.  A run is a
    maximal horizontal run of 1-pixels in one row.
  * k_label.hip:407  band components > max_markers; opened components > max_markers, > 1024, or
    `ncomp * NMOM * 8 > sizeof(parent) / 2` (NMOM = 15, parent = u32[VBS_RUN_CAP]: 15 * 8 * ncomp > 61 440, that is more
    than 512 contours); components of the complement > 1024 -> VBS_ECAPACITY.
Holes are background components (4-connected, the complement of 8-connected components as cv2.findContours sees them)
that do not touch the image border: components - Euler number, the count the kernels test.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np
from scipy import ndimage

from oracle import stages as O

RUN_CAP = 30720              # VBS_RUN_CAP, common.h:16
OPEN_CAP = 512               # 61 440 / (NMOM * 8), k_label.hip:407
COMP_CAP = 1024              # k_label.hip:407 (the complement's components; max_markers is at most 1024 too)

EIGHT = np.ones((3, 3), bool)


@dataclass
class Case:
    cls: str
    name: str
    mask: np.ndarray
    area: np.ndarray
    claims: Dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------------------------------
# counts
def runs(fg: np.ndarray) -> int:
    """maximal horizontal runs of 1-pixels (the union-find nodes of k_label)."""
    b = np.asarray(fg, bool)
    return int(b[:, 0].sum() + (b[:, 1:] & ~b[:, :-1]).sum())


def euler8(fg: np.ndarray) -> int:
    """Euler number of the 8-connected foreground by bit-quad counting (Gray 1971), zero outside the image."""
    f = np.pad(np.asarray(fg, bool), 1).astype(np.int32)
    q = f[:-1, :-1] + f[:-1, 1:] + f[1:, :-1] + f[1:, 1:]
    diag = (q == 2) & (f[:-1, :-1] == f[1:, 1:])
    n1, n3, nd = int((q == 1).sum()), int((q == 3).sum()), int(diag.sum())
    assert (n1 - n3 - 2 * nd) % 4 == 0
    return (n1 - n3 - 2 * nd) // 4


def holes(fg: np.ndarray) -> int:
    """components - Euler number (the kernels' test for a frame with holes)."""
    return int(ndimage.label(fg, structure=EIGHT)[1]) - euler8(fg)


def bounded_background(fg: np.ndarray) -> Tuple[np.ndarray, int]:
    """(labels, count) of the 4-connected background components that do not touch the border: the holes, by labelling."""
    lab, n = ndimage.label(~np.asarray(fg, bool))
    edge = set(np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])).tolist()) - {0}
    keep = [i for i in range(1, n + 1) if i not in edge]
    out = np.zeros_like(lab)
    for k, i in enumerate(keep, 1):
        out[lab == i] = k
    return out, len(keep)


def expected_capacity(mask: np.ndarray, area: np.ndarray, max_markers: int) -> Dict:
    """The counts k_label sees for one frame and whether it must report VBS_ECAPACITY (rule: module docstring)."""
    band = O.band_mask(mask)
    opened = O.morph_open5(area != 0)
    e = {"band_runs": runs(band), "open_runs": runs(opened), "band_comps": int(ndimage.label(band)[1]),
         "open_comps": int(ndimage.label(opened, structure=EIGHT)[1]), "holes": holes(opened)}
    e["bg_runs"] = runs(~opened) if e["holes"] else 0
    e["bg_comps"] = int(ndimage.label(~opened)[1]) if e["holes"] else 0
    # external contours = components of the opened mask once its holes are filled (what vbs_frame_stats field 6 reports)
    e["contours"] = int(ndimage.label(opened | (bounded_background(opened)[0] > 0), structure=EIGHT)[1]) if e["holes"] \
        else e["open_comps"]
    e["over"] = (e["band_runs"] > RUN_CAP or e["open_runs"] > RUN_CAP or e["bg_runs"] > RUN_CAP
                 or e["band_comps"] > max_markers or e["open_comps"] > min(max_markers, OPEN_CAP)
                 or e["bg_comps"] > COMP_CAP)
    return e


# ---------------------------------------------------------------------------------------------------------------------
# drawing
class _Canvas:
    """one frame under construction; features are placed where their box (plus a margin) is still free."""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.area = np.zeros((h, w), bool)
        self.mask = np.zeros((h, w), bool)
        self.used = np.zeros((h, w), bool)
        self.yy, self.xx = np.mgrid[0:h, 0:w]
        self.placed: List[str] = []

    def free(self, y0, y1, x0, x1, margin=3):
        y0, y1, x0, x1 = max(0, y0 - margin), min(self.h, y1 + margin), max(0, x0 - margin), min(self.w, x1 + margin)
        return y0 < y1 and x0 < x1 and not self.used[y0:y1, x0:x1].any()

    def take(self, y0, y1, x0, x1):
        self.used[max(0, y0):max(0, y1), max(0, x0):max(0, x1)] = True

    def disc(self, cy, cx, r):
        return (self.yy - cy) ** 2 + (self.xx - cx) ** 2 <= r * r

    def ring(self, cy, cx, ri, ro):
        d = (self.yy - cy) ** 2 + (self.xx - cx) ** 2
        return (d <= ro * ro) & (d > ri * ri)

    def centre(self, cy, cx):
        """a band component whose centroid is exactly (cx, cy) (integer or half-integer): 1, 2 or 4 pixels (the erosion of
        the band filter removes all of them, so the band is the blob itself)."""
        ys = [int(np.floor(cy))] + ([int(np.floor(cy)) + 1] if cy != np.floor(cy) else [])
        xs = [int(np.floor(cx))] + ([int(np.floor(cx)) + 1] if cx != np.floor(cx) else [])
        for y in ys:
            for x in xs:
                self.mask[y, x] = True

    def out(self, cls, name, **claims):
        return Case(cls, name, self.mask.astype(np.uint8), (self.area * 255).astype(np.uint8), dict(claims, placed=list(self.placed)))


def _place(cv: _Canvas, size, at=None, step=None):
    """(cy, cx) of a free box of `size` (half-extent) - at `at` if given and free, else the first free grid position."""
    if at is not None:
        cy, cx = at
        return (cy, cx) if cv.free(cy - size, cy + size + 1, cx - size, cx + size + 1) else None
    step = step or max(4, size // 2)
    for cy in range(size + 1, cv.h - size - 1, step):
        for cx in range(size + 1, cv.w - size - 1, step):
            if cv.free(cy - size, cy + size + 1, cx - size, cx + size + 1):
                return cy, cx
    return None


def _ellipse(cv, cx, cy, a, b, th):
    u = (cv.xx - cx) * np.cos(th) + (cv.yy - cy) * np.sin(th)
    v = -(cv.xx - cx) * np.sin(th) + (cv.yy - cy) * np.cos(th)
    return (u / a) ** 2 + (v / b) ** 2 <= 1


def ragged(h, w, rng, k):
    """overlapping rotated ellipses as the route-against-route tests draw them (mask: the same ellipse at 0.7), four of
    them centred on the four borders."""
    cv = _Canvas(h, w)
    s = min(h, w)
    amax = max(6.0, min(40.0, s / 4))
    centres = [(rng.uniform(0, h), 0.0), (rng.uniform(0, h), w - 1.0), (0.0, rng.uniform(0, w)), (h - 1.0, rng.uniform(0, w))]
    centres += [(rng.uniform(0, h), rng.uniform(0, w)) for _ in range(int(rng.integers(6, 30)))]
    for (cy, cx) in centres:
        a, b, th = rng.uniform(4, amax), rng.uniform(4, amax), rng.uniform(0, np.pi)
        cv.area |= _ellipse(cv, cx, cy, a, b, th)
        cv.mask |= _ellipse(cv, cx, cy, 0.7 * a, 0.7 * b, th)
    return cv.out("ragged", f"ragged{k}", borders=4)


# hole features: (half-extent, draw(cv, cy, cx) -> claims)
RO, RI = 22, 12                 # a ring's outer / inner radius

def _ring(cv, cy, cx):
    cv.area |= cv.ring(cy, cx, RI, RO)
    cv.centre(cy, cx)                                    # band centre inside the hole
    return {"holes": 1}


def _ring_blob(cv, cy, cx):
    cv.area |= cv.ring(cy, cx, RI, RO) | cv.disc(cy + 2, cx - 1, 5)
    cv.centre(cy + 2, cx - 1)                            # band centre inside the nested blob
    return {"holes": 1, "nested": [(cy + 2, cx - 1)]}


def _double_nest(cv, cy, cx):
    cv.area |= cv.ring(cy, cx, 24, 32) | cv.ring(cy, cx, 11, 18) | cv.disc(cy, cx + 1, 5)
    cv.centre(cy, cx + 1.5)                              # inside the innermost blob
    return {"holes": 2, "nested": [(cy, cx + 1)]}


def _diagonal_hole(cv, cy, cx):
    """a square frame of 6-px bars whose top bar and right bar meet only at a corner: the enclosed background touches the
    outside diagonally only - a hole under the 4-connected background (8-connected foreground)."""
    t, y0, x0 = 6, cy - 14, cx - 14
    y1, xc = y0 + 28, x0 + 22
    a = cv.area
    a[y0:y0 + t, x0:xc] = True                           # top bar, ends at column xc - 1
    a[y0 + t:y1, xc:xc + t] = True                       # right bar, starts one row below the top bar
    a[y1 - t:y1, x0:xc + t] = True
    a[y0:y1, x0:x0 + t] = True
    cv.centre(cy + 0.5, cx - 3)
    return {"holes": 1, "diagonal": (y0 + t, xc - 1, y0 + t - 1, xc)}     # (inside pixel, outside pixel)


def _cut_ring(side):
    def draw(cv, cy, cx):
        cv.area |= cv.ring(cy, cx, RI, RO)
        iy, ix = min(max(cy, 2), cv.h - 3), min(max(cx, 2), cv.w - 3)
        cv.centre(iy, ix)                                # band centre in the open gap: no hole, outside the contour
        return {"holes": 0}
    return draw


def _holes_frames(h, w):
    frames = []
    # 1: holes and nesting, wherever they fit
    cv = _Canvas(h, w)
    for name, size, draw in (("ring", RO, _ring), ("ring_blob", RO, _ring_blob), ("double_nest", 32, _double_nest),
                             ("diagonal_hole", 15, _diagonal_hole), ("ring_blob", RO, _ring_blob)):
        p = _place(cv, size + 1)
        if p is None:
            continue
        claims = draw(cv, *p)
        cv.take(p[0] - size - 1, p[0] + size + 2, p[1] - size - 1, p[1] + size + 2)
        cv.placed.append((name, p, claims))
    frames.append(cv.out("holes", "holes_nested"))
    # 2: at word boundaries, in the last partial word, on rows 0 and H-1
    cv = _Canvas(h, w)
    spots = [("word_boundary", (h // 2, 64 * k)) for k in range(1, (w - RO) // 64 + 1)]
    spots += [("last_word", (h // 2, w - 1 - RO)), ("row0", (RO, w // 2)), ("rowH1", (h - 1 - RO, w // 3)),
              ("row0_word", (RO, 64)), ("rowH1_last", (h - 1 - RO, w - 1 - RO))]
    for name, at in spots:
        if not (RO <= at[0] <= h - 1 - RO and RO <= at[1] <= w - 1 - RO):
            continue
        p = _place(cv, RO, at=at)
        if p is None:
            continue
        claims = _ring(cv, *p) if len(cv.placed) % 2 == 0 else _ring_blob(cv, *p)
        cv.take(p[0] - RO, p[0] + RO + 1, p[1] - RO, p[1] + RO + 1)
        cv.placed.append((name, p, claims))
    frames.append(cv.out("holes", "holes_edges"))
    # 3: rings cut by each border (their gap is open to the outside: no hole), two rings inside as well
    cv = _Canvas(h, w)
    for name, at in (("cut_bottom", (h + 2, (2 * w) // 3)), ("cut_left", (h // 2, -3)), ("cut_top", (-3, w // 3)),
                     ("cut_right", (h // 3, w + 2)), ("cut_bottom2", (h + 5, w // 6))):
        cy, cx = at
        if not cv.free(cy - RO, cy + RO + 1, cx - RO, cx + RO + 1):
            continue
        claims = _cut_ring(name)(cv, cy, cx)
        cv.take(cy - RO, cy + RO + 1, cx - RO, cx + RO + 1)
        cv.placed.append((name, (cy, cx), claims))
    for name, draw in (("ring", _ring), ("ring_blob", _ring_blob)):
        p = _place(cv, RO + 1)
        if p is not None:
            claims = draw(cv, *p)
            cv.take(p[0] - RO - 1, p[0] + RO + 2, p[1] - RO - 1, p[1] + RO + 2)
            cv.placed.append((name, p, claims))
    frames.append(cv.out("holes", "holes_cut"))
    # 4: exactly one hole and nothing else, a frame every fused kernel takes up to the hole test
    cv = _Canvas(h, w)
    p = (h // 2, w // 2)
    cv.placed.append(("ring", p, _ring(cv, *p)))
    frames.append(cv.out("holes", "hole_one"))
    for f in frames:
        f.claims["holes"] = sum(c.get("holes", 0) for (_, _, c) in f.claims["placed"])
        f.claims["nested"] = [q for (_, _, c) in f.claims["placed"] for q in c.get("nested", [])]
        f.claims["diagonal"] = [c["diagonal"] for (_, _, c) in f.claims["placed"] if "diagonal" in c]
    return frames


def _matching_frame(h, w):
    """centres just inside / just outside the (minor/10)^2 radius and the polygon of one contour, and a centre inside the
    thresholds of two contours (a C-shaped ring and the blob in its mouth) that only one polygon holds.  Two external
    contours of a 5x5-opened mask never both hold one point (their components are not 8-connected), so a centre claimed by
    two contours cannot arise through `_marker_center`."""
    cv = _Canvas(h, w)
    claims = []

    def fit_of(shape):
        cs = O.find_contours_external(O.morph_open5(shape))
        assert len(cs) == 1
        (ex, ey), (a, b), _ = O.fit_ellipse(cs[0])
        return cs[0], ex, ey, min(a, b)

    def pick(cont, ex, ey, minor, want_in_radius, want_poly, lo, hi):
        thr = (minor / 10) ** 2
        best = None
        for dy2 in range(-24, 25):
            for dx2 in range(-24, 25):
                x, y = np.floor(ex * 2) / 2 + dx2 / 2, np.floor(ey * 2) / 2 + dy2 / 2
                d = (x - ex) ** 2 + (y - ey) ** 2
                r = d / thr
                pp = O.point_polygon_test(cont, (x, y))
                if (d < thr) == want_in_radius and want_poly(pp) and lo <= r <= hi:
                    if best is None or abs(r - 1) < best[0]:
                        best = (abs(r - 1), x, y)
        return best

    R = min(26, (min(h, w) - 8) // 4)
    for kind in ("radius_in", "radius_out", "poly_edge", "poly_out", "two_claims"):
        size = R + 2
        p = _place(cv, size)
        if p is None or R < 10:
            continue
        cy, cx = p
        if kind in ("radius_in", "radius_out"):
            shape = cv.disc(cy, cx, R)
            cont, ex, ey, minor = fit_of(shape)
            b = pick(cont, ex, ey, minor, kind == "radius_in", lambda t: t > 0, *((0.85, 1.0) if kind == "radius_in" else (1.0, 1.2)))
        elif kind in ("poly_edge", "poly_out"):
            shape = cv.disc(cy, cx, R) & ~((cv.xx >= cx) & (np.abs(cv.yy - cy) <= 3))     # a slot from the rim to the centre
            cont, ex, ey, minor = fit_of(shape)
            b = pick(cont, ex, ey, minor, True, (lambda t: t == 0) if kind == "poly_edge" else (lambda t: t < 0), 0.0, 1.0)
        else:
            shape = cv.ring(cy, cx, R - 8, R) & ~((cv.xx >= cx) & (np.abs(cv.yy - cy) <= 5))   # a C open to the right ...
            blob = cv.disc(cy, cx + 2, 6)                                                      # ... and a blob in its mouth
            ca, exa, eya, mina = fit_of(shape)
            cb, exb, eyb, minb = fit_of(blob)
            thr_a, thr_b = (mina / 10) ** 2, (minb / 10) ** 2
            b = None
            for dy2 in range(-16, 17):
                for dx2 in range(-16, 17):
                    x, y = cx + 2 + dx2 / 2, cy + dy2 / 2
                    if (x - exa) ** 2 + (y - eya) ** 2 < thr_a and (x - exb) ** 2 + (y - eyb) ** 2 < thr_b \
                            and O.point_polygon_test(cb, (x, y)) > 0:
                        b = (0, x, y)
                        break
                if b:
                    break
            shape = shape | blob
        if b is None:
            continue
        cv.area |= shape
        cv.centre(b[2], b[1])
        cv.take(cy - size, cy + size + 1, cx - size, cx + size + 1)
        cv.placed.append((kind, (cy, cx), {"centre": (b[1], b[2])}))
        claims.append(kind)
    return cv.out("matching", "matching", kinds=claims)


def _slots_frame(h, w):
    """opened bars five pixels wide and one apart across the first 64-px word: more segments alive in one row of a tile than
    the opened-mask walk of the fused kernels has slots (SG_KO = 3, stage_common.h), so they hand the frame on (16 + 1)."""
    cv = _Canvas(h, w)
    rows = min(h - 4, 24)
    for x in range(1, min(w, 64) - 5, 6):
        cv.area[2:2 + rows, x:x + 5] = True
    cv.centre(2 + rows // 2, 3)                          # a band centre inside the first bar
    return cv.out("overflow", "slots_open")


def label_cases(h: int, w: int, seed: int = 0) -> List[Case]:
    """ragged, holes and matching cases for one geometry, and one frame that overflows the fused kernels' slots."""
    rng = np.random.default_rng(seed * 7919 + h * 31 + w)
    out = [ragged(h, w, rng, k) for k in range(2)]
    out += _holes_frames(h, w)
    out.append(_matching_frame(h, w))
    out.append(_slots_frame(h, w))
    return out


def stage_tile_rows(h: int, w: int, nt: int) -> int:
    """rows R of the tile one thread of k_stage walks (k_stage.hip stage_geom): nt threads hold (nt / 64) * (64 / WW) row
    blocks of WW = ceil(w / 64) words."""
    ww = -(-w // 64)
    nb = (nt // 64) * (64 // ww)
    return -(-h // nb)


def _segs_pattern(cv, t, x0):
    """three lanes of 5x5 squares in one word column (x0 .. x0 + 54) around tile row t: each lane has a square ending on row
    t, one on rows t+1 .. t+5 and one on rows t+6 .. t+10, each shifted 6 px right of the one before (never 8-adjacent).
    At most three runs are alive in a row, but a tile that starts on row t and has at least 7 rows starts nine segments of
    the opened mask: more than the SG_SEGMAX = 8 a thread can hold (16 + SLOW_SEGS)."""
    for lane in range(3):
        for k, y in enumerate((t - 4, t + 1, t + 6)):
            x = x0 + 19 * lane + 6 * k
            cv.area[y:y + 5, x:x + 5] = True


def _mailbox_frame(cv, spacing, k=10):
    """k concentric rings three pixels thick in the mask, `spacing` px apart: k band components whose centroids are all the
    frame's centre pixel.  Each centroid posts a probe request for the rows iy and iy + 1 to the thread that owns the pixel,
    k > ST_MB_CAP = 8 requests in one row: the band walk's mailbox overflows (SLOW_MAILBOX) although no tile holds more
    than a few ring arcs."""
    cy, cx = cv.h // 2, cv.w // 2
    d2 = (cv.yy - cy) ** 2 + (cv.xx - cx) ** 2
    for i in range(k):
        r = 14 + spacing * i
        cv.mask |= (d2 > (r - 1.5) ** 2) & (d2 <= (r + 1.5) ** 2)
    cv.area |= cv.disc(cy, cx, 8)


# ---------------------------------------------------------------------------------------------------------------------
# crowded frames: each one aims at one limit, just beyond it or at 90 % of it
def _grid(h, w, n, pitch, margin=16):
    """top-left corners of n cells of a pitch x pitch grid inside the frame."""
    ys = range(margin, h - margin - pitch, pitch)
    xs = range(margin, w - margin - pitch, pitch)
    cells = [(y, x) for y in ys for x in xs]
    assert len(cells) >= n, (h, w, n, pitch, len(cells))
    return cells[:n]


def _markers(cv, k=3):
    """k plain markers in the bottom-right corner (an opened disc holding a band centre), so that crowded frames that stay
    inside their limits still produce detections."""
    for i in range(k):
        cy, cx = cv.h - 40, cv.w - 40 - 60 * i
        cv.area |= cv.disc(cy, cx, 14)
        cv.mask |= cv.disc(cy, cx, 9)


def crowded_cases(h: int, w: int, max_markers: int = 1024) -> List[Case]:
    """frames just beyond each capacity limit and at 90 % of it, and frames aimed at single tables of the fused kernels:
    the probe mailbox, the opened-mask segments per tile, and the component limits met by components spread thinly enough
    that no tile's slots give out first.  Needs room: 480 x 640 and larger."""
    out = []
    cv = _Canvas(h, w)
    _mailbox_frame(cv, 22)
    out.append(cv.out("crowded", "mailbox", limit=None, over=False))
    cv = _Canvas(h, w)
    at = []
    for i, nt in enumerate((768, 256)):
        r = stage_tile_rows(h, w, nt)
        t = r * max(1, (h // 3) // r)                     # a tile's first row, well inside the frame
        _segs_pattern(cv, t, 64 * (2 + 2 * i) + 2)
        at.append((t, 64 * (2 + 2 * i)))
    _markers(cv)
    out.append(cv.out("crowded", "open_segs", limit=None, over=False, tiles=at))
    # components spread one or two per tile: the fused kernels' component limits (SLOW_NCOMP), then k_label's
    for name, n, draw in (("band_comps_sparse_over", max_markers + 40, "dot"), ("open_comps_sparse_over", OPEN_CAP + 20, "sq")):
        cv = _Canvas(h, w)
        pitch = int(np.sqrt((h - 100) * (w - 40) / n))
        for (y, x) in _grid(h - 80, w, n, pitch, margin=10):
            if draw == "dot":
                cv.mask[y, x] = True
            else:
                cv.area[y:y + 6, x:x + 6] = True
        _markers(cv)
        out.append(cv.out("crowded", name, limit=name[:10], over=True))
    reserve = 80                                              # bottom rows kept for the markers
    hh = h - reserve
    for over in (True, False):
        tag = "over" if over else "90"
        # band components: isolated pixels (each one its own band component)
        n = max_markers + 40 if over else int(0.9 * max_markers)
        cv = _Canvas(h, w)
        for (y, x) in _grid(hh, w, n, 3):
            cv.mask[y, x] = True
        _markers(cv)
        out.append(cv.out("crowded", f"band_comps_{tag}", limit="band_comps", over=over))
        # opened components: 6x6 squares (they survive the opening; 4-vertex contours are not fitted)
        n = OPEN_CAP + 20 if over else int(0.9 * OPEN_CAP)
        cv = _Canvas(h, w)
        for (y, x) in _grid(hh, w, n, 9):
            cv.area[y:y + 6, x:x + 6] = True
        _markers(cv)
        out.append(cv.out("crowded", f"open_comps_{tag}", limit="open_comps", over=over))
        # band runs: vertical lines one pixel wide (a run per line per row, a component per line)
        lines = min(500, (w - 40) // 2)
        target = RUN_CAP + 1000 if over else int(0.9 * RUN_CAP)
        rows = -(-target // lines)
        assert rows <= hh - 40, (h, w)
        cv = _Canvas(h, w)
        cv.mask[20:20 + rows, 20:20 + 2 * lines:2] = True
        _markers(cv)
        out.append(cv.out("crowded", f"band_runs_{tag}", limit="band_runs", over=over))
        # opened runs: bars five pixels wide, one pixel apart
        bars = (w - 40) // 6
        target = RUN_CAP + 1000 if over else int(0.9 * RUN_CAP)
        rows = -(-target // bars)
        assert rows <= hh - 40, (h, w)
        cv = _Canvas(h, w)
        for k in range(bars):
            cv.area[20:20 + rows, 20 + 6 * k:25 + 6 * k] = True
        _markers(cv)
        out.append(cv.out("crowded", f"open_runs_{tag}", limit="open_runs", over=over))
    return out
