"""Cameras, points and tables the uncertainty tests share (`tests/test_uncert_host.py`, `tests/test_gpu_uncert.py`)."""
import numpy as np

import uncert_oracle as U

FLAG_TRACKED, FLAG_XYZ = 1, 2
DIST = np.array([-0.28, 0.09, 1e-3, -5e-4, -0.01])


def _rot(a, b):
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    return Rz @ Rx


def camera(size=(640, 480), distorted=True, exact=False, R=None, T=(3.0, -2.0, 40.0), dmm=2.0):
    """(K, dist, R, T, dmm).  `exact`: fx + fy is a power of two and dmm = 2, so f_avg, dmm / f_avg and f_avg^2 are exact in
    float32 and the solve IS the smooth function (the forward mode and the complex step then differ by rounding only)."""
    W, H = size
    if exact:
        fx, fy = (500.0, 524.0) if W <= 640 else (2000.0, 2096.0)
        dmm = 2.0
    else:
        f = 600.0 if W <= 640 else 1500.0
        fx, fy = f * 1.01, f * 0.99
    K = np.array([[fx, 0.0, W / 2 + 3.3], [0.0, fy, H / 2 - 2.1], [0.0, 0.0, 1.0]])
    return (K, DIST if distorted else np.zeros(5), _rot(0.3, 0.2) if R is None else np.asarray(R, dtype=np.float64),
            np.asarray(T, dtype=np.float64), dmm)


def points(cam, size):
    """uvd [N, 3] (float32 values): from the principal point's neighbourhood out to the frame corners, diameters 5 .. 40 px."""
    W, H = size
    K = np.asarray(cam[0], dtype=np.float32)
    cx, cy = float(K[0, 2]), float(K[1, 2])
    pts = []
    for d in (5.0, 9.5, 16.0, 40.0):
        for u, v in ((cx + 0.01, cy - 0.02), (cx + 3.0, cy + 1.0), (W / 3, H / 3), (0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0),
                     (W - 1.0, H - 1.0), (W * 0.8, H * 0.6)):
            pts.append((u, v, d))
    return np.array(pts, dtype=np.float32).astype(np.float64)


def table(cam, n, m, size=(640, 480), seed=0, move=None, noise=(0.05, 0.05), poison=True, gaps=True):
    """A float32 table [n, m, 10] with everything the entries have to step around: about 20 % untracked rows (the reference
    frame included), rows below 5 px with and without the XYZ flag, one row exactly on the principal point (Rr < 1e-6) that
    carries the flag, XYZ flags cleared on good rows as `despike_table` clears them, and NaN / 1e30 in every cell that must not
    be read (all of an untracked row, columns 4, 5, 9 everywhere, X Y Z of a row without the flag).  `move` [n, m, 3] is added to
    (Cx, Cy, major)."""
    rng = np.random.default_rng(seed)
    W, H = size
    c = U.Cam(*cam)
    side = int(np.ceil(np.sqrt(m)))
    gx, gy = np.meshgrid(np.linspace(0.1 * W, 0.9 * W, side), np.linspace(0.1 * H, 0.9 * H, side))
    base = np.stack([gx.ravel()[:m], gy.ravel()[:m], np.full(m, 14.0)], axis=1)
    o = base[None] + rng.normal(size=(n, m, 3)) * np.array([noise[0], noise[0], noise[1]])
    if move is not None:
        o = o + move
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 1:4] = o
    tracked = rng.random((n, m)) >= 0.2 if gaps else np.ones((n, m), dtype=bool)
    if gaps and n * m >= 8:
        small = rng.random((n, m)) < 0.08
        t[small, 3] = 4.0
        f, s = n // 2, m // 2
        t[f, s, 1], t[f, s, 2], t[f, s, 3] = c.cx32, c.cy32, 14.0  # on the principal point
        tracked[f, s] = True
    P, X, ok = U.primal(c, t[..., 1].ravel().astype(np.float64), t[..., 2].ravel().astype(np.float64),
                        t[..., 3].ravel().astype(np.float64))
    t[..., 6:9] = X.reshape(n, m, 3)
    xyz = tracked & ok.reshape(n, m) & (t[..., 3] >= 5.0)
    if gaps and n * m >= 8:
        xyz &= rng.random((n, m)) >= 0.05                         # despiked
        xyz |= tracked & (t[..., 3] < 5.0) & (rng.random((n, m)) < 0.5)     # solved with a smaller gate: the entry's own gate decides
        xyz[n // 2, m // 2] = True
    t[..., 0] = tracked * FLAG_TRACKED + xyz * FLAG_XYZ
    if poison:
        bad = np.where(rng.random((n, m)) < 0.5, np.float32(np.nan), np.float32(1e30))
        for col in (4, 5, 9):
            t[..., col] = bad
        for col in (6, 7, 8):
            t[..., col] = np.where(xyz, t[..., col], bad)
        for col in (1, 2, 3):
            t[..., col] = np.where(tracked, t[..., col], bad)
    return t


def factor(q, seed=0):
    """A camera factor [16, q] of plausible sizes: q = 0 none, 1 dmm only, 5 the pose's w and T0, T1, 16 dense."""
    rng = np.random.default_rng(100 + seed)
    scale = np.array([0.5, 0.5, 0.3, 0.3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-3, 1e-4, 1e-4, 1e-4, 0.02, 0.02, 0.05, 0.01])
    L = np.zeros((16, q))
    if q == 1:
        L[15, 0] = scale[15]
    elif q == 5:
        for j, k in enumerate((9, 10, 11, 12, 13)):
            L[k, j] = scale[k]
    elif q > 0:
        L = np.tril(rng.normal(size=(16, 16)))[:, :q] * scale[:, None]
    return L
