"""Host-side companions of `analysis.shape_series`: the default length scale of a marker field, the kind of surface a
row of `shape` describes, and its radii of curvature.  NumPy only; nothing here touches a device."""
import math

import numpy as np

SHAPE_COLS = 24
(DEGREE, COUNT, N_USED, MX, MY, MZ, C0, A, B, P, Q, R, RMS_PLANE, RMS, H, K, K1, K2, DIR_DEG, APEX, APEX_X, APEX_Y, APEX_Z,
 DEPTH) = range(SHAPE_COLS)
SHAPE_COLUMNS = ("degree", "count", "n_used", "mx", "my", "mz", "c0", "a", "b", "p", "q", "r", "rms_plane", "rms", "H", "K", "k1", "k2",
                 "dir_deg", "apex", "apex_x", "apex_y", "apex_z", "depth")
# `kind`: what the signs of K and H say (z up: a bowl is curved upwards everywhere, its apex the lowest point)
KIND_NONE, KIND_PLANE, KIND_BOWL, KIND_DOME, KIND_SADDLE, KIND_RIDGE = range(6)
KIND_NAMES = ("none", "plane", "bowl", "dome", "saddle", "ridge")


def default_length(ref_xyz, slots=None):
    """The length `shape_series` scales x and y by when none is given: the root of the mean squared distance of the selected
    reference (x, y) from their mean, length = sqrt(fsum((x - mx)^2 + (y - my)^2) / k) with mx = fsum(x) / k, my = fsum(y) / k over
    the k selected rows whose x and y are finite (`math.fsum`: exactly rounded sums, so the value does not depend on the order of
    the slots).  ValueError where that is not a positive finite number (no row, or all rows on one point)."""
    xy = np.asarray(ref_xyz, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] < 2:
        raise ValueError("ref_xyz must be [m, 3]")
    if slots is not None:
        xy = xy[np.asarray(slots, dtype=np.int64).reshape(-1)]
    xy = xy[np.isfinite(xy[:, 0]) & np.isfinite(xy[:, 1])]
    k = xy.shape[0]
    if k < 1:
        raise ValueError("default_length: no selected reference position is finite")
    mx, my = math.fsum(xy[:, 0].tolist()) / k, math.fsum(xy[:, 1].tolist()) / k
    dx, dy = xy[:, 0] - mx, xy[:, 1] - my
    length = math.sqrt(math.fsum((dx * dx + dy * dy).tolist()) / k)
    if not (math.isfinite(length) and length > 0.0):
        raise ValueError("default_length: the selected reference positions do not span a length; pass `length`")
    return length


def _rows(shape):
    s = np.asarray(shape, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != SHAPE_COLS:
        raise ValueError(f"shape must be [N, {SHAPE_COLS}] (`shape_series`)")
    return s


def kind(shape, apex_rel=1e-6):
    """An integer code per frame from the degree and the signs of K and H: KIND_NONE (degree 0), KIND_PLANE (degree 1), and at
    degree 2 KIND_RIDGE where |K| fails the entry's test |K| > apex_rel (p^2 + 2 q^2 + r^2) - one curvature is zero to that
    measure: a ridge, a trough or no curvature at all - else KIND_SADDLE (K < 0), KIND_BOWL (K > 0, H > 0: curved upwards, the apex
    is the lowest point) or KIND_DOME (K > 0, H < 0).  `apex_rel`: the value `shape_series` was called with."""
    s = _rows(shape)
    p, q, r = s[:, P], s[:, Q], s[:, R]
    curved = np.abs(s[:, K]) > float(apex_rel) * ((p * p + 2.0 * (q * q)) + r * r)
    two = np.where(~curved, KIND_RIDGE, np.where(s[:, K] < 0.0, KIND_SADDLE, np.where(s[:, H] > 0.0, KIND_BOWL, KIND_DOME)))
    return np.where(s[:, DEGREE] == 2.0, two, np.where(s[:, DEGREE] == 1.0, KIND_PLANE, KIND_NONE)).astype(np.int64)


def radius(shape):
    """The radii of curvature 1 / k1 and 1 / k2 with their validity: -> (radius [N, 2] (signed like the curvature; NaN where not
    valid), valid [N, 2] = the frame has degree 2 and that curvature is not zero)."""
    s = _rows(shape)
    k = s[:, [K1, K2]]
    valid = (s[:, DEGREE] == 2.0)[:, None] & (k != 0.0) & np.isfinite(k)
    return np.where(valid, 1.0 / np.where(valid, k, 1.0), np.nan), valid
