"""Rendered markers for the tests of `vbs_refine_markers`: a supersampled renderer for ellipses with blur, gain, offset and seeded
noise, the seeded accuracy set, and table rows in `vbs_track`'s format."""
import math

import numpy as np
from scipy import ndimage

TABLE_COLS = 10
# The accuracy of the rule on `accuracy_set()` below (seed 2023: 128 markers, contrasts 200/60 and 120/90, sigma 0 and 1 px,
# noise 1.5 levels, ratio 0.85 .. 1, starts off by up to 1 px a coordinate and 1.5 px in diameter), as the RESTATEMENT gives it:
# the largest |major' - 2a|, |d_area - 2 sqrt(ab)| and centre error, in px.  The bounds are 1.5 x these maxima; the margin covers
# a change of seed (seeds 1 and 2 give 0.225 / 0.189 / 0.102 and 0.269 / 0.166 / 0.129), not a change of rule.  DESIGN 4.24
# carries the same figures.
MEASURED_MAX = {"major": 0.25957487719986716, "d_area": 0.19090408942589931, "centre": 0.09931781553131606}
BOUND = {k: 1.5 * v for k, v in MEASURED_MAX.items()}          # 0.389, 0.286, 0.149 px
SS = 8                                                       # sub-pixels a side


def coverage(h, w, cx, cy, a, b, theta_deg=0.0):
    """The share of every pixel of an [h, w] frame inside the ellipse of semi-axes a >= b whose MAJOR axis points along
    theta_deg (from +x towards +y, y down); pixel (x, y) is the square [x - 0.5, x + 0.5] x [y - 0.5, y + 0.5]."""
    pad = int(math.ceil(a)) + 2
    xa, xb = max(int(cx) - pad, 0), min(int(cx) + pad + 1, w)
    ya, yb = max(int(cy) - pad, 0), min(int(cy) + pad + 1, h)
    sub = (np.arange(SS) + 0.5) / SS - 0.5
    xs = (np.arange(xa, xb)[:, None] + sub[None, :]).reshape(-1) - cx
    ys = (np.arange(ya, yb)[:, None] + sub[None, :]).reshape(-1) - cy
    t = math.radians(theta_deg)
    X, Y = np.meshgrid(xs, ys)
    u, v = X * math.cos(t) + Y * math.sin(t), -X * math.sin(t) + Y * math.cos(t)
    inside = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    out = np.zeros((h, w))
    out[ya:yb, xa:xb] = inside.reshape(yb - ya, SS, xb - xa, SS).mean(axis=(1, 3))
    return out


def render(h, w, markers, bg=200.0, fg=60.0, sigma=0.0, gain=1.0, offset=0.0, noise=0.0, seed=0):
    """uint8 [h, w]: `markers` = (cx, cy, a, b, theta_deg) each, level fg on bg, a Gaussian blur of `sigma` px, gain v + offset,
    then seeded Gaussian noise of `noise` levels, rounded and clipped."""
    cov = np.zeros((h, w))
    for m in markers:
        cov = np.maximum(cov, coverage(h, w, *m))
    img = bg + (fg - bg) * cov
    if sigma > 0:
        img = ndimage.gaussian_filter(img, sigma, mode="nearest")
    img = gain * img + offset
    if noise > 0:
        img = img + noise * np.random.default_rng(seed).standard_normal((h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def row(cx, cy, major, minor=None, angle=0.0, flags=1, det_index=0, xyz=(0.0, 0.0, 0.0)):
    """One table row as `vbs_track` writes it."""
    return np.array([flags, cx, cy, major, major if minor is None else minor, angle, xyz[0], xyz[1], xyz[2], det_index],
                    dtype=np.float32)


def accuracy_set(seed=2023, per_group=32, size=64):
    """The seeded accuracy set: per_group markers for each of contrast (200/60, 120/90) x sigma (0, 1) - 128 at the default -
    each alone on its own frame: semi-axis a in 7 .. 9 px, ratio b / a in 0.85 .. 1, any direction, the centre anywhere in the
    middle pixel, noise 1.5 levels; the start is off by up to +-1 px in each centre coordinate and +-1.5 px in diameter.
    -> list of dicts: gray, row (the perturbed start), cx, cy, a, b, theta, bg, fg, sigma."""
    rng = np.random.default_rng(seed)
    out = []
    for bg, fg in ((200.0, 60.0), (120.0, 90.0)):
        for sigma in (0.0, 1.0):
            for _ in range(per_group):
                a = rng.uniform(7.0, 9.0)
                b = a * rng.uniform(0.85, 1.0)
                cx, cy = size / 2 + rng.uniform(-0.5, 0.5), size / 2 + rng.uniform(-0.5, 0.5)
                theta = rng.uniform(0.0, 180.0)
                gray = render(size, size, [(cx, cy, a, b, theta)], bg, fg, sigma, noise=1.5, seed=int(rng.integers(1 << 30)))
                start = row(cx + rng.uniform(-1.0, 1.0), cy + rng.uniform(-1.0, 1.0), 2 * a + rng.uniform(-1.5, 1.5))
                out.append({"gray": gray, "row": start, "cx": cx, "cy": cy, "a": a, "b": b, "theta": theta, "bg": bg, "fg": fg,
                            "sigma": sigma})
    return out
