"""Area masks for the tests of k_ncc_mfma's pre-scan (the kernel runs its 16-row steps only where a strip's correlation
windows can hold an area pixel), and a NumPy restatement of the rule that decides what is skipped.

The rule, per 16-column strip (first column xw) and 16-row tile (first row y0): the tile's windows cover the rows
y0 + lo .. y0 + 15 + hi and the columns xw + lo .. xw + 15 + hi; a tile whose cover holds no area pixel is `dead`.  The
kernel skips a subset of the dead tiles whatever its segmentation (a segment drops the dead tiles in front of its first
and behind its last occupied row; segments of one tile drop every dead tile), so a mask that is zero on every dead tile
is one no segmentation can change."""
import numpy as np

from oracle import stages as O


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8) * 255


def patterns(h, w, seed=5):
    """[(name, area mask uint8 {0, 255} [h, w])]: the 13 frames of one batch."""
    z = np.zeros((h, w), np.uint8)
    out = [("zero", z.copy()), ("full", np.full((h, w), 255, np.uint8))]
    for name, (y, x) in (("px_tl", (0, 0)), ("px_tr", (0, w - 1)), ("px_bl", (h - 1, 0)), ("px_br", (h - 1, w - 1)),
                         ("px_centre", (h // 2, w // 2))):
        a = z.copy()
        a[y, x] = 255
        out.append((name, a))
    out.append(("disc_centre", disc(h, w, h // 2, w // 2, 20)))
    # 20 px left of a 16-column boundary: the strip right of the boundary holds no area pixel of its own, its windows do
    out.append(("disc_left_of_boundary", disc(h, w, h // 2, 16 * (w // 32) - 20, 12)))
    for name, y in (("row_first", 0), ("row_last", h - 1)):
        a = z.copy()
        a[y, :] = 255
        out.append((name, a))
    a = z.copy()
    a[h // 2, w - 1] = 255
    out.append(("px_last_column", a))
    rng = np.random.default_rng(seed)
    out.append(("specks", (rng.random((h, w)) < 1e-4).astype(np.uint8) * 255))
    return out


def dead_pixels(area, l):
    """bool [h, w]: the pixels of the dead tiles (see the module's text) of one area mask."""
    h, w = area.shape
    lo, hi = O.ncc_window(l)
    occ = area != 0
    dead = np.zeros((h, w), bool)
    for xw in range(0, w, 16):
        cols = occ[:, max(xw + lo, 0):min(xw + 15 + hi, w - 1) + 1]
        rows = cols.any(axis=1)
        for y0 in range(0, h, 16):
            if not rows[max(y0 + lo, 0):min(y0 + 15 + hi, h - 1) + 1].any():
                dead[y0:y0 + 16, xw:xw + 16] = True
    return dead


def oracle_mask(area):
    p = O.branch_params(area.shape[0])
    return O.normxcorr2_direct(O.gkern(p["tl"], p["tsig"]), area) > 0.1
