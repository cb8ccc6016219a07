"""Synthetic validation shots for the diameter tests: dark shapes on a bright, noisy background (test infrastructure).

`shot(H, W, seed)` places, on a jittered grid so that nothing touches by accident: discs of 15-40 px diameter (anti-aliased
edge), ellipses on both sides of the 0.85 circularity threshold, specks under 100 px, rings and discs with a bright hole, and -
at the image edge - discs cut by it; `board=True` adds a chessboard of touching dark squares (one 8-connected blob of
circularity far below pi / 4).  Grey levels: shapes ~40, background ~200, Gaussian noise of `noise` levels; with threshold 120
the blurred noise never crosses.
"""
import numpy as np

THRESHOLD = 120


def _ellipse(img, cx, cy, a, b, ang, level, soft=0.8):
    H, W = img.shape
    r = int(max(a, b) + 3)
    y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r + 1), max(0, int(cx) - r), min(W, int(cx) + r + 1)
    yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
    d = (np.sqrt((u / a) ** 2 + (v / b) ** 2) - 1.0) * min(a, b)        # ~ signed distance to the edge in px
    cov = np.clip(0.5 - d / soft, 0.0, 1.0)
    img[y0:y1, x0:x1] = img[y0:y1, x0:x1] * (1 - cov) + level * cov


def shot(H, W, seed, board=False, noise=6.0, pitch=56, kinds="DDDDEeSRHD"):
    """float image -> uint8 [H, W].  kinds (cycled over the grid cells, shuffled): D disc, E ellipse with circularity above
    0.85, e ellipse below it, S speck, R ring, H disc with a hole."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 200.0)
    cells = [(gx, gy) for gy in range(pitch // 2 + 4, H - pitch // 2, pitch) for gx in range(pitch // 2 + 4, W - pitch // 2, pitch)]
    bx0 = by0 = bx1 = by1 = -1
    if board:
        sq, nsq = 22, 6
        bx0, by0 = W // 2 - sq * nsq // 2, H // 2 - sq * nsq // 2
        bx1, by1 = bx0 + sq * nsq, by0 + sq * nsq
        for r in range(nsq):
            for c in range(nsq):
                if (r + c) % 2 == 0:
                    img[by0 + r * sq:by0 + (r + 1) * sq + 1, bx0 + c * sq:bx0 + (c + 1) * sq + 1] = 40.0   # corners overlap: they touch
    order = rng.permutation(len(cells))
    for n, ci in enumerate(order):
        gx, gy = cells[ci]
        if bx0 - pitch // 2 - 4 < gx < bx1 + pitch // 2 + 4 and by0 - pitch // 2 - 4 < gy < by1 + pitch // 2 + 4:
            continue
        cx, cy = gx + rng.uniform(-4, 4), gy + rng.uniform(-4, 4)
        k = kinds[n % len(kinds)]
        rad = rng.uniform(7.5, 20.0)
        if k == "D":
            _ellipse(img, cx, cy, rad, rad, 0.0, 40.0)
        elif k == "E":
            _ellipse(img, cx, cy, rad, rad * rng.uniform(0.8, 0.95), rng.uniform(0, np.pi), 40.0)
        elif k == "e":
            _ellipse(img, cx, cy, max(rad, 12.0), max(rad, 12.0) * rng.uniform(0.3, 0.5), rng.uniform(0, np.pi), 40.0)
        elif k == "S":
            _ellipse(img, cx, cy, rng.uniform(1.5, 4.5), rng.uniform(1.5, 4.5), 0.0, 40.0)
        elif k == "R":
            _ellipse(img, cx, cy, max(rad, 12.0), max(rad, 12.0), 0.0, 40.0)
            _ellipse(img, cx, cy, max(rad, 12.0) - 4.0, max(rad, 12.0) - 4.0, 0.0, 200.0)
        elif k == "H":
            _ellipse(img, cx, cy, max(rad, 12.0), max(rad, 12.0), 0.0, 40.0)
            _ellipse(img, cx + 2, cy - 1, 3.0, 2.5, 0.3, 200.0)
    # discs cut by each image edge
    _ellipse(img, 3.0, H * 0.3, 14.0, 14.0, 0.0, 40.0)
    _ellipse(img, W - 5.0, H * 0.7, 16.0, 16.0, 0.0, 40.0)
    _ellipse(img, W * 0.3, 2.0, 13.0, 13.0, 0.0, 40.0)
    _ellipse(img, W * 0.62, H - 4.0, 17.0, 17.0, 0.0, 40.0)
    img += rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def to_bgr(gray, seed):
    """A BGR frame whose channels differ by a few levels (so that the conversion's coefficients matter)."""
    rng = np.random.default_rng(seed)
    f = np.stack([gray.astype(np.int64) + rng.integers(-6, 7, gray.shape) for _ in range(3)], axis=-1)
    return np.clip(f, 0, 255).astype(np.uint8)
