"""Sequential restatement of `code/Precision_Validation/DiameterValidation.py` (`main` :218, `measure_markers` :113-144) for
the tests of the device path: test infrastructure, not product code.

Contours come from `oracle.stages.find_contours_external` (the restated `cv2.findContours(RETR_EXTERNAL, ...)`), the blur
is `oracle.stages.gaussian_blur_u8`'s arithmetic with OpenCV's fixed 5-tap kernel; added here are the shoelace area, the chain
length and an EXACT minimum enclosing circle over `fractions.Fraction` / Python integers.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from oracle import stages as O

TAPS5 = np.array([16, 64, 96, 64, 16], dtype=np.int64)      # (1, 4, 6, 4, 1) / 16 in 8 fractional bits
SQRT2 = math.sqrt(2.0)


def blur5_u8(gray: np.ndarray) -> np.ndarray:
    """`cv2.GaussianBlur(gray, (5, 5), 0)` in the fixed-point model of `oracle.stages.gaussian_blur_u8`."""
    g = gray.astype(np.int64)
    h = ndimage.correlate1d(g, TAPS5, axis=1, mode="mirror")
    v = ndimage.correlate1d(h, TAPS5, axis=0, mode="mirror")
    return ((v + 32768) >> 16).astype(np.uint8)


def threshold_inv(blur: np.ndarray, threshold: float) -> np.ndarray:
    """`cv2.threshold(img, t, 255, THRESH_BINARY_INV)` on uint8 as a boolean mask: img <= floor(t)."""
    return blur.astype(np.int64) <= math.floor(threshold)


def pack_bits(mask: np.ndarray) -> np.ndarray:
    """[H, W] bool -> [H, ceil(W / 64)] uint64, bit x % 64 of word x // 64 = pixel x."""
    H, W = mask.shape
    ww = (W + 63) // 64
    m = np.zeros((H, ww * 64), dtype=np.uint64)
    m[:, :W] = mask
    return (m.reshape(H, ww, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def chain_measures(chain: np.ndarray):
    """Full (unapproximated) closed border chain [k, 2] -> (area2, n_axis, n_diag): twice the signed shoelace area through the
    pixel centres and the numbers of unit and diagonal steps.  `cv2.contourArea` = |area2| / 2 and `cv2.arcLength(cnt, True)`
    = n_axis + n_diag sqrt 2 (CHAIN_APPROX_SIMPLE only drops collinear points, which changes neither)."""
    pts = [(int(x), int(y)) for x, y in chain]
    k = len(pts)
    if k < 2:
        return 0, 0, 0
    area2 = n_axis = n_diag = 0
    for i in range(k):
        (x0, y0), (x1, y1) = pts[i], pts[(i + 1) % k]
        dx, dy = x1 - x0, y1 - y0
        assert max(abs(dx), abs(dy)) == 1, "not a chain"
        area2 += x0 * y1 - x1 * y0
        if dx and dy:
            n_diag += 1
        else:
            n_axis += 1
    return area2, n_axis, n_diag


def fill_holes(fg: np.ndarray) -> np.ndarray:
    """Background regions (4-connected) that do not reach the image edge become foreground: what RETR_EXTERNAL ignores."""
    return ndimage.binary_fill_holes(fg)


# ---- exact minimum enclosing circle ----------------------------------------------------------------------------------------

def _hull(points):
    pts = sorted(set(points))
    if len(pts) <= 2:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1])
                                     - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out

    lo, up = half(pts), half(reversed(pts))
    return lo[:-1] + up[:-1]


def circle_through(support):
    """Exact circle (cx, cy, r2) as Fractions with the 1, 2 or 3 given integer points on its boundary (2: as a diameter)."""
    s = [(int(x), int(y)) for x, y in support]
    if len(s) == 1:
        return Fraction(s[0][0]), Fraction(s[0][1]), Fraction(0)
    if len(s) == 2:
        (ax, ay), (bx, by) = s
        return Fraction(ax + bx, 2), Fraction(ay + by, 2), Fraction((ax - bx) ** 2 + (ay - by) ** 2, 4)
    (ax, ay), (bx, by), (cx, cy) = s
    bx, by, cx, cy = bx - ax, by - ay, cx - ax, cy - ay
    d = 2 * (bx * cy - by * cx)
    assert d != 0, "collinear support"
    ux = Fraction(cy * (bx * bx + by * by) - by * (cx * cx + cy * cy), d)
    uy = Fraction(bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by), d)
    return ax + ux, ay + uy, ux * ux + uy * uy


def _inside(c, p):
    return (p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2 <= c[2]


def exact_mec(points):
    """Minimum enclosing circle of integer points, exact: (cx, cy, r2) as Fractions.  Incremental construction over the
    convex hull's vertices (the circle of a set is that of its hull)."""
    pts = _hull([(int(x), int(y)) for x, y in points])
    c = circle_through(pts[:1])
    for i in range(1, len(pts)):
        if _inside(c, pts[i]):
            continue
        c = circle_through([pts[i]])
        for j in range(i):
            if _inside(c, pts[j]):
                continue
            c = circle_through([pts[i], pts[j]])
            for k in range(j):
                if not _inside(c, pts[k]):
                    c = circle_through([pts[i], pts[j], pts[k]])
    return c


# ---- the whole of measure_markers --------------------------------------------------------------------------------------------

def contours_of(mask: np.ndarray):
    """Every external contour of a boolean mask in findContours' order: dicts with the full chain, the integer measures, the
    first pixel and the float64 area / perimeter / circularity."""
    out = []
    for chain in O.find_contours_external(mask, approx_simple=False):
        area2, n_axis, n_diag = chain_measures(chain)
        per = n_axis + n_diag * SQRT2
        area = abs(area2) / 2.0
        out.append(dict(chain=chain, area2=area2, n_axis=n_axis, n_diag=n_diag, first=(int(chain[0][0]), int(chain[0][1])),
                        area=area, perimeter=per, circularity=(4.0 * math.pi * area) / (per * per) if per > 0 else 0.0))
    return out


def measure_gray(gray: np.ndarray, threshold: float, scale: float, min_area: float = 100, min_circularity: float = 0.85,
                 offset_mm: float = 0.0):
    """`main` :218 + `measure_markers`: (mask, all contours, survivors).  A survivor also carries the exact circle (`mec` =
    (cx, cy, r2) as Fractions), the correctly rounded radius / centre and `diameter_mm`."""
    mask = threshold_inv(blur5_u8(gray), threshold)
    allc = contours_of(mask)
    surv = []
    for c in allc:
        if c["area"] < min_area or c["perimeter"] == 0 or c["circularity"] < min_circularity:
            continue
        cx, cy, r2 = exact_mec(c["chain"])
        c = dict(c, mec=(cx, cy, r2), cx=float(cx), cy=float(cy), radius=math.sqrt(r2))
        c["diameter_mm"] = (c["radius"] * 2) / scale + offset_mm
        surv.append(c)
    return mask, allc, surv


def component_pixels(mask: np.ndarray):
    """Labels (8-connected) of the hole-filled mask: (label image, n)."""
    return ndimage.label(fill_holes(mask), structure=np.ones((3, 3)))


def axis_ratio(chain) -> float:
    """Minor / major axis of a border chain from the covariance of its points: ~1 for a disc, b / a for an ellipse."""
    p = np.asarray(chain, dtype=np.float64).reshape(-1, 2)
    w = np.linalg.eigvalsh(np.cov(p.T))
    return float(np.sqrt(w[0] / w[1]))
