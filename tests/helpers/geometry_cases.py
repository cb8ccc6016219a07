"""Inputs and expectations for the rim of the frame-size envelope of `vbs_create` (height >= 64, 128 <= width <= 4096, no
upper bound on the height).  CPU only: NumPy, the frame synthesiser and the launchers' geometry rules restated as plain
integer arithmetic.  tests/test_geometry_cases.py holds the inputs to the properties tests/test_gpu_geometry_edges.py
relies on.

Geometry rules (restated from the launchers so that a test can say which kernels a frame size must reach):
  * `stage_rows(h, w, nt)`     k_stage.hip `stage_geom`: tiles of R = ceil(h / ((nt / 64) * (64 / WW))) rows, refused for
                               h > 2048 or R > 128.
  * `lat_rows(h, w)`           k_stage_lat.hip `lat_geom`: NW = ceil(h / (LT_ROWS * G)), C = clamp(ceil(NW / 4), 1, LT_CMAX),
                               R = ceil(h / (4 * C * G)), refused for h > 2048 or R > 128.  With G >= 1 and C = 16 the
                               R limit would bind from h = 8193 on: below 2049 rows it never does, the h rule is the only
                               refusal (case 13).
  * `ccl_takes(h, w)`          k_ccl.hip `ccl_layout`: h <= 2048 and h * NC < 65535, NC = ceil(WW / min(WW, 5)).
  * `blur16_takes(h, w)`       k_blur16.hip `blur16_takes` for a dense, aligned frame: from 176 (small branch) / 240 columns,
                               width a multiple of 4.
"""
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

import vbs_amd.synth as S

sys.path.insert(0, os.path.dirname(__file__))
import label_cases as LC                                      # noqa: E402

MAX_MARKERS = 512
LT_ROWS, LT_CMAX = 6, 16                                      # k_stage_lat.hip
SEED = 1                                                      # one at which every input condition holds (tests/test_geometry_cases.py)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules
def words(w: int) -> int:
    return -(-w // 64)


def stage_rows(h: int, w: int, nt: int) -> Optional[int]:
    """rows per tile of k_stage's `nt`-thread instance, None where `stage_geom` refuses."""
    r = LC.stage_tile_rows(h, w, nt)
    return None if h > 2048 or r > 128 else r


def stage_takes(h: int, w: int) -> bool:
    """`launch_stage`: one of the two instances accepts (the 256-thread one hands over to 768 where it refuses)."""
    return stage_rows(h, w, 768) is not None


def lat_rows(h: int, w: int) -> Optional[int]:
    g = 64 // words(w)
    nw = -(-h // (LT_ROWS * g))
    c = min(max(-(-nw // 4), 1), LT_CMAX)
    r = -(-h // (4 * c * g))
    return None if h > 2048 or r > 128 else r


def ccl_takes(h: int, w: int) -> bool:
    ww = words(w)
    nc = -(-ww // min(ww, 5))
    return h <= 2048 and h * nc < 65535


def blur16_takes(h: int, w: int) -> bool:
    return w >= (176 if h <= 480 else 240) and w % 4 == 0


# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    case: str                    # case number of the module docstring of tests/test_gpu_geometry_edges.py ("4b": case 4 at a width that is no multiple of 64)
    h: int
    w: int
    why: str
    pipeline: bool = False
    bgr: bool = False
    routes: Tuple[str, ...] = ()     # mask check: names of tests/test_gpu_labelling_oracle.py ROUTES; ("default",) = untouched options

    @property
    def id(self) -> str:
        return f"{self.case}-{self.h}x{self.w}"


EVERY = ("fused", "separate", "general", "fused768", "fused256", "latency")
GEOMETRIES = [
    Geometry("1", 64, 128, "both minima; small branch; k_blur_mfma; R = 1", pipeline=True),
    Geometry("2", 64, 4096, "minimum height at maximum width; k_blur16 with nseg clamped from 0; WW = 64", pipeline=True, bgr=True,
             routes=EVERY),
    Geometry("3", 480, 4096, "last small-branch height at full width", pipeline=True),
    Geometry("4", 481, 4096, "first large-branch height at full width", pipeline=True, bgr=True),
    Geometry("4b", 481, 4092, "case 4 with P != W (a multiple of 4: k_blur16 still takes it; BGR: k_gray's vector pieces with a partial tail)",
             pipeline=True, bgr=True),
    Geometry("5", 481, 128, "large branch in the narrowest frame", pipeline=True),
    Geometry("6", 2048, 128, "last height the fast labelling routes accept", pipeline=True, routes=EVERY),
    Geometry("7", 2049, 128, "first height they all refuse; H % 16 == 1", pipeline=True, bgr=True, routes=("default",)),
    Geometry("8", 512, 2112, "R = 128 for k_stage's 256-thread instance (WW = 33)", routes=EVERY),
    Geometry("9", 513, 2112, "the 256-thread instance refuses, 768 takes over", routes=EVERY),
    Geometry("10", 1536, 2112, "R = 128 for the 768-thread instance", routes=EVERY),
    Geometry("11", 1537, 2112, "k_stage refuses for R, not for H", pipeline=True, routes=("default",)),
    Geometry("12", 1536, 4096, "R = 128 at WW = 64: the largest frame k_stage accepts", routes=("fused", "fused768", "general")),
    Geometry("13", 2048, 2112, "the tallest frame k_stage_lat accepts at WW >= 33 (its R is 32: only the H rule binds)",
             routes=("latency", "fused")),
]
BY_ID = {g.id: g for g in GEOMETRIES}
PIPELINE = [g for g in GEOMETRIES if g.pipeline]
BGR = [g for g in GEOMETRIES if g.bgr]
MASKS = [g for g in GEOMETRIES if g.routes]
FEW_MARKERS = {"1", "5"}         # geometries too small for six whole dots: one marker is the minimum there


# ---------------------------------------------------------------------------------------------------------------------
# frames
def dot_diameter(h: int) -> int:
    return 20 if h <= 480 else 40


def dot_centres(h: int, w: int) -> np.ndarray:
    """about a dozen dot centres (x, y) in px: one 2.5 px inside each border, one whole dot near each corner (the top right
    one with its centre in the row's last 64-pixel word), one with its centre in the last 16 rows, the rest spread (beyond
    row 1200 / column 1920 where the frame has them)."""
    d = dot_diameter(h)
    r = d // 2
    m = r + 6                                                 # a whole dot's centre stays this far inside (3 px jitter)
    if (h, w) == (64, 128):
        # six dots are all that fit: cut by the top, left, right and bottom border, one whole in the last word, one whole
        # with its centre in the last 16 rows
        return np.array([(40, 2.5), (2.5, 34), (124.5, 26), (100, 60.5), (80, 22), (52, 51)], np.float64)
    if w == 128:
        # a column of dots (40 px across in 128 columns)
        c = [(64, 2.5), (26, 60), (w - 27, 60), (2.5, int(0.3 * h)), (w - 3.5, int(0.42 * h)), (64, int(0.55 * h)),
             (64, int(0.68 * h)), (26, h - 90), (w - 27, h - 90), (30, h - 25), (100, h - 3.5)]
        if h > 1000:
            c += [(40, int(0.8 * h)), (90, int(0.9 * h))]
        return np.array(c, np.float64)
    lo, hi = m, h - 1 - m

    def cy(f):
        return float(min(max(int(f * h), lo), hi))
    xl, xr = 2 * r + 13.5, w - 2 * r - 14.5                   # the corner dots next to the left / right border dot
    c = [(2.5, cy(0.5)), (xl, lo), (xl + d + 10, hi), (int(0.2 * w), 2.5), (int(0.35 * w), cy(0.3)), (int(0.5 * w), cy(0.8)),
         (int(0.62 * w), h - 3.5), (int(0.75 * w), cy(0.45)), (int(0.93 * w), cy(0.7)), (xr - d - 10, h - 12), (xr, lo),
         (w - 3.5, cy(0.55))]
    if d == 40:
        c.append((int(0.86 * w), h - 25))                     # the lowest whole dot a 40-px dot can be (see LAST_ROWS)
    return np.array(c, np.float64)


def last_rows(h: int) -> int:
    """rows from the bottom within which a returned marker's centre must lie.  16 in the small branch.  In the large
    branch a 40-px dot whose centre lies in the last 16 rows is cut by 5 px or more, and the oracle returns no marker for
    a dot cut by more than about 1 px (its ellipse centre and its band centroid part by more than minor / 10).  The lowest
    whole dot has its centre 25 rows from the bottom, 22 to 28 with the jitter of 3 px, and a band centroid within a pixel
    of that: 29 there.  Both masks still reach the last row (the border condition), and the mask frames have a marker in
    the last 16 rows at every geometry."""
    return 16 if h <= 480 else 29


def frame_spec(h: int, w: int) -> S.FrameSpec:
    c16 = np.round(dot_centres(h, w) * 16).astype(np.int64)
    return S.FrameSpec(w, h, c16, dot_diameter(h) * 16, name=f"rim_{h}x{w}")


def gray_frames(h: int, w: int) -> np.ndarray:
    """frames 0 to 2 of the spec (frame 0 without jitter, 1 and 2 with: the cut dots move): uint8 [3, h, w]."""
    return S.make_frames(frame_spec(h, w), [0, 1, 2], seed=SEED)


def bgr_frames(h: int, w: int) -> np.ndarray:
    """the same frames with B, G and R all different (as test_bgr_weights_and_dog_wrap builds them): uint8 [3, h, w, 3]."""
    g = gray_frames(h, w)
    return np.stack([np.clip(g.astype(int) + d, 0, 255) for d in (7, -9, 3)], axis=-1).astype(np.uint8)


def padded(frames: np.ndarray, left: int = 3, right: int = 5) -> Tuple[np.ndarray, slice]:
    """(buffer, column slice): the frames inside a buffer with `left` more pixels in front of every row and `right` behind,
    filled with a value no frame has much of.  Gray: an odd byte offset for left = 3; BGR: take left = 1 (3 bytes)."""
    pad = [(0, 0), (0, 0), (left, right)] + [(0, 0)] * (frames.ndim - 3)
    return np.pad(frames, pad, constant_values=113), slice(left, left + frames.shape[2])


# ---------------------------------------------------------------------------------------------------------------------
# masks
class _Planes:
    """one frame under construction.  Shapes are evaluated inside their own bounding window only: at 1536 x 4096 a
    full-frame coordinate grid per shape costs more than the oracle does."""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.area = np.zeros((h, w), bool)
        self.mask = np.zeros((h, w), bool)

    def window(self, cx, cy, ex, ey):
        y0, y1 = max(0, int(np.floor(cy - ey)) - 1), min(self.h, int(np.ceil(cy + ey)) + 2)
        x0, x1 = max(0, int(np.floor(cx - ex)) - 1), min(self.w, int(np.ceil(cx + ex)) + 2)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        return (slice(y0, y1), slice(x0, x1)), yy, xx

    def ellipse(self, cx, cy, a, b, th):
        """(window, pixels) of the filled ellipse of tests/helpers/label_cases.py `_ellipse`."""
        ex, ey = np.hypot(a * np.cos(th), b * np.sin(th)), np.hypot(a * np.sin(th), b * np.cos(th))
        win, yy, xx = self.window(cx, cy, ex, ey)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        return win, (u / a) ** 2 + (v / b) ** 2 <= 1

    def clear(self, win, margin=4):
        """no area pixel yet in the window (plus a margin): what is drawn there stays a component of its own."""
        ys, xs = win
        return not self.area[max(0, ys.start - margin):ys.stop + margin, max(0, xs.start - margin):xs.stop + margin].any()

    def draw(self, cx, cy, a, b, th, must=True):
        """a filled ellipse into `area`, the same at 0.6 of the axes into `mask` - if its window is still clear."""
        win, e = self.ellipse(cx, cy, a, b, th)
        if not e.any() or not self.clear(win):
            assert not must, (self.h, self.w, cx, cy, a, b)
            return False
        self.area[win] |= e
        win, e = self.ellipse(cx, cy, 0.6 * a, 0.6 * b, th)
        self.mask[win] |= e
        return True

    def ring(self, cy, cx):
        """label_cases' ring (outer / inner radius RO / RI) with a one-pixel band centre inside the hole."""
        win, yy, xx = self.window(cx, cy, LC.RO, LC.RO)
        assert self.clear(win)
        d = (yy - cy) ** 2 + (xx - cx) ** 2
        self.area[win] |= (d <= LC.RO * LC.RO) & (d > LC.RI * LC.RI)
        self.mask[cy, cx] = True

    def out(self, cls, name, placed):
        return LC.Case(cls, name, self.mask.astype(np.uint8), (self.area * 255).astype(np.uint8), {"placed": placed})


def _fillers(cv, us):
    """small whole ellipses along the longer axis (fractions `us`), alternating between two lines across the shorter one
    (left out where something lies there already), and two that the input conditions need: one with its centre in the
    last 64 columns, one in the last 16 rows."""
    h, w = cv.h, cv.w
    for k, u in enumerate(us):
        v = (0.3, 0.62)[k % 2]
        cx, cy = (u * w, min(max(v * h, 12), h - 13)) if w >= h else (min(max(v * w, 16), w - 17), u * h)
        cv.draw(int(cx), int(cy), 12, 8, 0.5 * k, must=False)
    cv.draw(w - 34, int(0.7 * h) if w >= h else int(0.62 * h), 12, 8, 0.3)                # centre in the last 64 columns
    cv.draw(int(0.27 * w) if w >= h else int(0.7 * w), h - 9, 14 if w >= h else 12, 6, 0.0)    # and in the last 16 rows


def mask_frames(h: int, w: int) -> List[LC.Case]:
    """two `Case`s (mask {0, 1}, area {0, 255}): rotated filled ellipses at the rim, and one ring among plain blobs."""
    s = min(h, w)
    r768, r256 = LC.stage_tile_rows(h, w, 768), LC.stage_tile_rows(h, w, 256)
    wide = w >= h
    cv = _Planes(h, w)
    # the large one first (everything else keeps clear of it): centre in the last quarter of both axes
    cv.draw(0.8 * w, 0.8 * h, 0.45 * s, 0.12 * s, 0.6)
    placed = [("large", (0.8 * w, 0.8 * h))]
    ca, cb = min(14.0, s / 6), min(10.0, s / 9)
    for (cx, cy) in ((0, 0), (w - 1, 0), (0, h - 1)):                                      # corners: both borders
        cv.draw(cx, cy, ca, cb, 0.0)
    cv.draw(w - 1, h - 1, ca, cb, 0.0, must=False)            # (in a frame about as tall as wide the large one holds that corner)
    if wide:
        cv.draw(int(0.2 * w), h - 4, 12, 8, 0.3)                                           # the last row only
        cv.draw(w - 4, int(0.3 * h) if h > 64 else 32, 8, min(10, h / 8), 0.0)             # the last column only
    else:
        cv.draw(int(0.4 * w), h - 4, 10, 8, 0.0)
        cv.draw(w - 4, int(0.2 * h), 8, 12, 0.0)
    # tall and thin (9 px): across at least three tile boundaries of the 768-thread instance
    at = min(2 * r768 + 4, (h - 8) // 2)
    tx, ty = (int(0.42 * w), max(at + 4, int(0.35 * h))) if wide else (w // 2, int(0.42 * h))
    cv.draw(tx, ty, at, 4, np.pi / 2)
    assert (ty + at) // r768 - (ty - at) // r768 >= 3, (h, w, r768)
    placed.append(("tall", (tx, ty, at)))
    if 128 in (r768, r256):
        # a blob that fills the whole height of tile 1 (rows 128 .. 255) in one 64-pixel column of words
        y0, x0 = 128, 64 * (int(0.55 * w) // 64)
        win, e = cv.ellipse(x0 + 32, y0 + 63.5, 72, 27, np.pi / 2)
        assert cv.clear(win) and win[1].start >= x0 and win[1].stop <= x0 + 64
        cv.area[win] |= e
        cv.area[y0:y0 + 128, x0 + 8:x0 + 56] = True
        win, e = cv.ellipse(x0 + 32, y0 + 63.5, 40, 14, np.pi / 2)
        cv.mask[win] |= e
        placed.append(("tile_blob", (x0, y0)))
    _fillers(cv, (0.06, 0.12, 0.33, 0.5, 0.62, 0.7, 0.9))
    rim = cv.out("rim", "rim", placed)
    # frame 2: one ring (a hole: every fused kernel hands the frame on to k_label) among plain blobs
    cv = _Planes(h, w)
    ry, rx = (min(max(int(0.5 * h), LC.RO + 2), h - LC.RO - 3), int(0.6 * w)) if wide else (int(0.6 * h), w // 2)
    cv.ring(ry, rx)
    _fillers(cv, (0.05, 0.15, 0.25, 0.35, 0.45, 0.75, 0.85, 0.95))
    return [rim, cv.out("holes", "ring", [("ring", (ry, rx))])]
