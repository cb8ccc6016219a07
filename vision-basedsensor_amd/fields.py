"""Grids and weights for `engine.field_map_f64` (NumPy only).  The device smoother divides by the sum of the weights it could
use, so a weight matrix needs no normalisation here; it is computed on the host, as the FIR's taps are (`filters.py`), so that no
`exp` of the device enters a result."""
import numpy as np


def _nodes(nodes_xy):
    a = np.asarray(nodes_xy, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError("nodes_xy must be [m >= 1, 2]")
    return a


def grid_over(nodes_xy, shape=(64, 64), margin=0.0):
    """A regular grid over the bounding box of the finite nodes, widened by `margin` on every side.  `shape` = (rows, columns):
    rows run along y, columns along x.  Returns (grid_xy float64 [rows * columns, 2], row-major - p = row * columns + column, x
    fastest - and the area of one cell, dx * dy; an axis with one point has spacing 1)."""
    a = _nodes(nodes_xy)
    ny, nx = int(shape[0]), int(shape[1])
    if ny < 1 or nx < 1:
        raise ValueError("shape must be (rows >= 1, columns >= 1)")
    if not (np.isfinite(float(margin)) and float(margin) >= 0.0):
        raise ValueError("margin must be finite and >= 0")
    fin = a[np.isfinite(a).all(axis=1)]
    if fin.shape[0] < 1:
        raise ValueError("no node has finite coordinates")
    lo, hi = fin.min(axis=0) - float(margin), fin.max(axis=0) + float(margin)
    xs = np.linspace(lo[0], hi[0], nx) if nx > 1 else np.array([(lo[0] + hi[0]) / 2])
    ys = np.linspace(lo[1], hi[1], ny) if ny > 1 else np.array([(lo[1] + hi[1]) / 2])
    dx = (hi[0] - lo[0]) / (nx - 1) if nx > 1 and hi[0] > lo[0] else 1.0
    dy = (hi[1] - lo[1]) / (ny - 1) if ny > 1 and hi[1] > lo[1] else 1.0
    gx, gy = np.meshgrid(xs, ys)                                # [ny, nx]: x fastest
    return np.ascontiguousarray(np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)), float(dx * dy)


def default_bandwidth(nodes_xy):
    """The median distance of a finite node to its nearest finite neighbour (1.0 for fewer than two nodes)."""
    a = _nodes(nodes_xy)
    fin = a[np.isfinite(a).all(axis=1)]
    if fin.shape[0] < 2:
        return 1.0
    d2 = ((fin[:, None, :] - fin[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return float(np.median(np.sqrt(d2.min(axis=1))))


def gaussian_weights(nodes_xy, grid_xy, bandwidth, cutoff=3.0):
    """W float64 [P, m] = exp(-r^2 / 2 h^2) with r the distance of grid point p to node m and h = `bandwidth`; EXACTLY 0 beyond
    r > cutoff * h and for a node with a non-finite coordinate (a slot that has no position gets no weight)."""
    a = _nodes(nodes_xy)
    g = np.asarray(grid_xy, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 2 or g.shape[0] < 1:
        raise ValueError("grid_xy must be [P >= 1, 2]")
    h, c = float(bandwidth), float(cutoff)
    if not (np.isfinite(h) and h > 0.0 and np.isfinite(c) and c > 0.0):
        raise ValueError("bandwidth and cutoff must be finite and > 0")
    fin = np.isfinite(a).all(axis=1)
    safe = np.where(fin[:, None], a, 0.0)
    r2 = (g[:, None, 0] - safe[None, :, 0]) ** 2 + (g[:, None, 1] - safe[None, :, 1]) ** 2
    w = np.exp(-r2 / (2.0 * h * h))
    keep = fin[None, :] & (r2 <= (c * h) * (c * h))
    return np.ascontiguousarray(np.where(keep, w, 0.0))


def row_sums(W):
    """wsum float64 [P]: the full row sums of W, added in ascending m from 0.0 (one rounded add per slot)."""
    w = np.asarray(W, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("W must be [P, m]")
    acc = np.zeros(w.shape[0], dtype=np.float64)
    for m in range(w.shape[1]):
        acc = acc + w[:, m]
    return acc
