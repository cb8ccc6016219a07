"""Exact references for the last step of `_marker_center` (k_finalize.hip): the contour-vertex moments, the two least-squares
fits of cv2.fitEllipse solved in rational arithmetic, and the 2x2 pixel cell `inside_polygon` decides from.  CPU only.

`exact_fit` restates `oracle.stages.fit_ellipse` with every rounding but the last removed:
  (i)  min sum (-A x^2 - B y^2 - C x y + D x + E y - 10000)^2 over the vertices gives the conic, its gradient's zero the centre;
  (ii) min sum (A x^2 + B y^2 + C x y - 1)^2 about that centre gives axes and angle.
Both are solved through their normal equations in `fractions.Fraction` from integer power sums, so the only roundings left
are the closing square roots (to 2^-200), the atan2 (float64) and the float32 roundings of the five results.

Origin.  Scaling the coordinates by s maps the family of (i) onto itself (A / s^2, D / s), so the scale enters neither fit.
A translation does: (i) has a fixed right-hand side and no constant term, and moving the origin by t moves the fitted
centre by up to 0.65 |t| on unions of two squares (1e-2 |t| and less on digitised ellipses; tests/test_ellipse_host.py
measures it).  The origin is therefore part of what cv2 computes, and `exact_fit` takes cv2's: the float32 mean of the
vertices from a running float32 sum (`mean32`), exactly as a rational.  The kernel rounds the exact sum once instead;
the two means are the same float32 value whenever the coordinate sums stay below 2^24 (every case but `large`).

The branch `|g3[2]| > 1e-8` of the reference is taken on the SCALED coefficients (g3 / scale^2), and the scale of the
kernel is not cv2's.  With g2 != 0 both branches give t = hypot(g2, g1 - g0) or t = g1 - g0; these differ (by sign, which
swaps the axes and turns the ellipse by 90 degrees) only when g1 < g0.  `exact_fit` evaluates the test at both scales and
reports in `branch_differs` when they disagree; an exactly symmetric outline has g2 = 0 and takes the second branch at
every scale.
"""
import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# (a, b) of S[1..14] as fit_ellipse_moments reads them; S[0] = n
ORDER = ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4))
MIN_EPS = Fraction(1, 10 ** 8)
FOUR_OVER_PI = 1.2732395447351628            # the kernel's constant


def vertex_moments(contour, first_pixel) -> List[int]:
    """[n, sum (x - ax)^a (y - ay)^b for (a, b) in ORDER] as Python ints; first_pixel = (ax, ay)."""
    ax, ay = int(first_pixel[0]), int(first_pixel[1])
    pts = [(int(x) - ax, int(y) - ay) for x, y in np.asarray(contour).reshape(-1, 2)]
    return [len(pts)] + [sum(x ** a * y ** b for x, y in pts) for a, b in ORDER]


def first_pixel(contour) -> Tuple[int, int]:
    """the contour's first raster pixel (x, y): smallest y, then smallest x (where the border following starts)."""
    c = np.asarray(contour).reshape(-1, 2)
    y = int(c[:, 1].min())
    return int(c[c[:, 1] == y, 0].min()), y


# ---------------------------------------------------------------------------------------------------------------------
def f32_round(q: Fraction) -> float:
    """q rounded once to the nearest float32 (ties to even), as a Python float; |q| within float32's normal range or 0."""
    if q == 0:
        return 0.0
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e < 127
    m = a / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    fl = m.numerator // m.denominator
    r = m - fl
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl & 1):
        fl += 1
    return s * float(fl) * 2.0 ** (e - 23)


def sqrt_fraction(q: Fraction, bits: int = 200) -> Fraction:
    """sqrt(q) to a relative 2^-bits (rounded down)."""
    assert q >= 0
    if q == 0:
        return Fraction(0)
    k = bits + max(0, q.denominator.bit_length() - q.numerator.bit_length())
    return Fraction(math.isqrt((q.numerator << (2 * k)) // q.denominator), 1 << k)


def ulps32(a: float, b: float) -> int:
    """distance of two float32 values in units of the last place (same sign or zero)."""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7FFFFFFF) for v in (ia, ib))
    return abs(ia - ib)


def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def _solve(A: List[List[Fraction]], b: List[Fraction]) -> Optional[List[Fraction]]:
    n = len(b)
    A = [row[:] + [b[i]] for i, row in enumerate(A)]
    for c in range(n):
        p = next((r for r in range(c, n) if A[r][c] != 0), None)
        if p is None:
            return None
        A[c], A[p] = A[p], A[c]
        for r in range(c + 1, n):
            if A[r][c] != 0:
                f = A[r][c] / A[c][c]
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    x = [Fraction(0)] * n
    for c in range(n - 1, -1, -1):
        x[c] = (A[c][n] - sum(A[c][k] * x[k] for k in range(c + 1, n))) / A[c][c]
    return x


def _moments(pts: Sequence[Tuple[Fraction, Fraction]]) -> Dict[Tuple[int, int], Fraction]:
    m = {}
    for a in range(5):
        for b in range(5 - a):
            m[a, b] = sum((x ** a * y ** b for x, y in pts), Fraction(0))
    return m


def mean32(contour, running: bool = True) -> Tuple[float, float]:
    """the float32 mean of the vertices: from a running float32 sum like cv2's Point2f accumulation (running), or from the
    exact sum rounded once like the kernel."""
    c = np.asarray(contour).reshape(-1, 2)
    n = np.float32(len(c))
    if running:
        s = np.zeros(2, np.float32)
        for p in c.astype(np.float32):
            s = (s + p).astype(np.float32)
    else:
        s = np.array([int(c[:, 0].sum()), int(c[:, 1].sum())], np.float64).astype(np.float32)
    m = (s / n).astype(np.float32)
    return float(m[0]), float(m[1])


def exact_conic(contour, origin=None):
    """steps (i) and (ii) in Fractions about `origin` (default: cv2's float32 mean): (centre (absolute), g3, ..) or None."""
    pts = [(Fraction(int(x)), Fraction(int(y))) for x, y in np.asarray(contour).reshape(-1, 2)]
    if origin is None:
        origin = mean32(contour)
    ox, oy = Fraction(origin[0]), Fraction(origin[1])
    q = [(x - ox, y - oy) for x, y in pts]
    m = _moments(q)
    A = [[m[4, 0], m[2, 2], m[3, 1], -m[3, 0], -m[2, 1]],
         [m[2, 2], m[0, 4], m[1, 3], -m[1, 2], -m[0, 3]],
         [m[3, 1], m[1, 3], m[2, 2], -m[2, 1], -m[1, 2]],
         [-m[3, 0], -m[1, 2], -m[2, 1], m[2, 0], m[1, 1]],
         [-m[2, 1], -m[0, 3], -m[1, 2], m[1, 1], m[0, 2]]]
    g = _solve(A, [-10000 * m[2, 0], -10000 * m[0, 2], -10000 * m[1, 1], 10000 * m[1, 0], 10000 * m[0, 1]])
    if g is None:
        return None
    det = 4 * g[0] * g[1] - g[2] * g[2]
    if det == 0:
        return None
    r0 = (2 * g[1] * g[3] - g[2] * g[4]) / det
    r1 = (2 * g[0] * g[4] - g[2] * g[3]) / det
    mu = _moments([(x - r0, y - r1) for x, y in q])
    g3 = _solve([[mu[4, 0], mu[2, 2], mu[3, 1]], [mu[2, 2], mu[0, 4], mu[1, 3]], [mu[3, 1], mu[1, 3], mu[2, 2]]],
                [mu[2, 0], mu[0, 2], mu[1, 1]])
    if g3 is None:
        return None
    return (ox + r0, oy + r1), g3, q, m


def scales(contour) -> Tuple[float, float]:
    """(cv2's scale 100 / sum(|x| + |y|), the kernel's 100 / (n sqrt(r2) 4 / pi)) about the float32 mean."""
    c = np.asarray(contour, np.float64).reshape(-1, 2)
    n = len(c)
    d = c - np.array(mean32(contour))
    s = float(np.abs(d).sum())
    r2 = float((d * d).sum() / n)
    return 100.0 / s, 100.0 / (n * math.sqrt(r2) * FOUR_OVER_PI)


def exact_fit(contour, origin=None):
    """dict(cx, cy, w, h, angle: float32 values as Python floats, w <= h; w_exact, h_exact, cx_exact, cy_exact: Fractions
    (axes to 2^-200); angle_exact: float64 degrees; aniso: (h - w) / h; branch_differs; cond_degenerate) or None where
    one of the two systems, or the conic's 2x2 centre system, is singular."""
    r = exact_conic(contour, origin)
    if r is None:
        return None
    (cx, cy), g3, _, _ = r
    s_cv, s_k = scales(contour)
    g0, g1, g2 = g3
    ang = -0.5 * math.atan2(float(g2), float(g1 - g0)) if (g2 != 0 or g1 != g0) else -0.5 * math.atan2(0.0, 0.0)
    big = [abs(g2) / Fraction(s) ** 2 > MIN_EPS for s in (s_cv, s_k)]
    out_by_branch = []
    for first in (True, False):
        t = sqrt_fraction(g2 * g2 + (g1 - g0) ** 2) if first else g1 - g0
        r2, r3 = abs(g0 + g1 - t), abs(g0 + g1 + t)
        out_by_branch.append((r2, r3))
    r2, r3 = out_by_branch[0 if big[0] else 1]
    # (r > min_eps on the scaled coefficient, else the reference leaves r itself: a degenerate conic, not an ellipse)
    degenerate = any(v / Fraction(s) ** 2 <= MIN_EPS for v in (r2, r3) for s in (s_cv, s_k))
    if degenerate or r2 == 0 or r3 == 0:
        return None
    wq = 2 * sqrt_fraction(2 / r2)
    hq = 2 * sqrt_fraction(2 / r3)
    w32, h32 = f32_round(wq), f32_round(hq)
    deg = ang * 180.0 / math.pi
    a32 = float(np.float32(deg))
    if w32 > h32:
        w32, h32, wq, hq = h32, w32, hq, wq
        deg = 90.0 + deg
        a32 = float(np.float32(deg))
    if a32 < -180:
        a32 = float(np.float32(np.float32(a32) + np.float32(360)))
    if a32 > 360:
        a32 = float(np.float32(np.float32(a32) - np.float32(360)))
    return dict(cx=f32_round(cx), cy=f32_round(cy), w=w32, h=h32, angle=a32, cx_exact=cx, cy_exact=cy, w_exact=wq,
                h_exact=hq, angle_exact=deg, aniso=float((hq - wq) / hq),
                branch_differs=(big[0] != big[1]) and out_by_branch[0] != out_by_branch[1])


# ---------------------------------------------------------------------------------------------------------------------
BG = 0xFFFF


def contour_id_image(opened: np.ndarray, contours) -> np.ndarray:
    """uint16 image: for every pixel of `opened` the id the kernels give its component = raster order of first pixels
    (contour i of the oracle's list, which is in reverse order, has id len - 1 - i); 0xFFFF elsewhere."""
    from scipy import ndimage
    lab, n = ndimage.label(opened, structure=np.ones((3, 3), bool))
    assert n == len(contours)
    out = np.full(opened.shape, BG, np.uint16)
    for i, c in enumerate(contours):
        x, y = first_pixel(c)
        out[lab == lab[y, x]] = len(contours) - 1 - i
    return out


def cell_and_fraction(opened, id_image, pt):
    """(ids of (x, y), (x+1, y), (x, y+1), (x+1, y+1), fx, fy) for the float32-rounded point: what inside_polygon is given."""
    H, W = id_image.shape
    xf, yf = np.float32(pt[0]), np.float32(pt[1])
    x0, y0 = int(np.floor(xf)), int(np.floor(yf))
    fx, fy = np.float32(xf - np.floor(xf)), np.float32(yf - np.floor(yf))
    ids = [int(id_image[y, x]) if 0 <= x < W and 0 <= y < H and opened[y, x] else BG
           for x, y in ((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))]
    return ids, fx, fy


def cell_branch(ids, fx, fy, cid) -> Tuple[str, bool]:
    """(name of the branch of inside_polygon the cell reaches for component cid, its decision); float32 arithmetic."""
    one = np.float32(1)
    c00, c10, c01, c11 = (i == cid for i in ids)
    if fx == 0 and fy == 0:
        return "vertex", c00
    if fy == 0:
        return "on_row", c00 and c10
    if fx == 0:
        return "on_col", c00 and c01
    cnt = c00 + c10 + c01 + c11
    if cnt == 4:
        return "four", True
    if cnt == 3:
        if not c11:
            return "three_no11", bool(np.float32(fx + fy) <= one)
        if not c00:
            return "three_no00", bool(np.float32(fx + fy) >= one)
        if not c10:
            return "three_no10", bool(fy >= fx)
        return "three_no01", bool(fx >= fy)
    if cnt == 2:
        if c00 and c11:
            return "diag_main", bool(fx == fy)
        if c10 and c01:
            return "diag_anti", bool(np.float32(fx + fy) == one)
        return "two_side", False
    return ("one" if cnt == 1 else "zero"), False


# ---------------------------------------------------------------------------------------------------------------------
ANISO_MIN = 1e-3                             # below this (h - w) / h only the axes are held, not the angle
ANGLE_FLOOR = 1e-4                           # degrees: kappa * eps / ANISO_MIN = 7e5 * 1.1e-16 / 1e-3 rad = 4.4e-6 degrees, rounded up


def fit_deviation(got, ex) -> Tuple[List[int], Optional[float], float]:
    """got = (cx, cy, w, h, angle) float32 values; ex = exact_fit's dict.  -> (ulps of cx, cy, w, h from the exact value
    rounded to float32; the angle's deviation mod 180 in degrees or None below ANISO_MIN; the angle's tolerance)."""
    u = [ulps32(got[i], ex[k]) for i, k in enumerate(("cx", "cy", "w", "h"))]
    if ex["aniso"] < ANISO_MIN:
        return u, None, 0.0
    dev = abs((got[4] - ex["angle_exact"] + 90.0) % 180.0 - 90.0)
    return u, dev, max(ulp32(max(abs(ex["angle"]), abs(got[4]))), ANGLE_FLOOR)
