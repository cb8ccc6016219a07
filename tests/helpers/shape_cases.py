"""Recordings and point sets the tests of `vbs_shape_series` share (`tests/test_shape_host.py`, `tests/test_gpu_shape.py`): seeded
and small.  Two ways to an end point: a table whose X, Y, Z columns move (the general recordings: P = ref + scale d), and a table
whose Z column alone carries a prescribed height over float64 reference positions (`table_of_heights`: P = (ref_x, ref_y, dz), so a
test can put the markers exactly where it wants them - on a line, on a circle - whatever float32 would do to such coordinates)."""
import numpy as np

import pose_oracle as PO
import posecov_cases as PC
import uncert_oracle as U

FLAG_TRACKED, FLAG_XYZ = 1, 2
PIXEL_SIGMA = 0.05             # px, centre and diameter: the pixel-noise level of the uncertainty tests (row f21)
# the first five rings of the sensor's published layout (radius mm, count, first angle deg): 61 markers at its pitch of about 3.4 mm
RINGS61 = ((0.0, 1, 0.0), (3.49, 6, 30.0), (6.92, 12, 0.0), (10.23, 18, 10.0), (13.37, 24, 0.0))


def ring61():
    """[61, 3] reference positions of a flat field (Z = 0)."""
    pts = []
    for radius, count, a0 in RINGS61:
        for k in range(count):
            a = np.deg2rad(a0 + 360.0 * k / count)
            pts.append((radius * np.cos(a), radius * np.sin(a), 0.0))
    return np.asarray(pts, dtype=np.float64)


def rms_length(xy):
    """The rms radius of points [k, 2] about their mean (what `shapes.default_length` computes, in plain NumPy)."""
    d = np.asarray(xy, dtype=np.float64) - np.mean(xy, axis=0)
    return float(np.sqrt((d * d).sum(axis=1).mean()))


# ---- point sets for the fit itself -----------------------------------------------------------------------------------------------------
def irregular_xy(m, seed=0, angle_deg=0.0, offset=(0.0, 0.0), pitch=2.0):
    """m positions on a jittered square grid, rotated by `angle_deg` and moved to `offset`."""
    rng = np.random.default_rng(1000 + seed)
    side = int(np.ceil(np.sqrt(m)))
    i = np.arange(m)
    xy = np.stack([(i % side - (side - 1) / 2) * pitch, (i // side - (side - 1) / 2) * pitch], axis=1)
    xy = xy + rng.uniform(-0.3, 0.3, size=xy.shape) * pitch
    a = np.deg2rad(angle_deg)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return xy @ rot.T + np.asarray(offset, dtype=np.float64)[None]


def quadric_z(xy, centre, coeffs):
    """z = c0 + a x + b y + (p x x + 2 q x y + r y y) / 2 in x, y counted from `centre`; coeffs = (c0, a, b, p, q, r)."""
    x, y = xy[:, 0] - centre[0], xy[:, 1] - centre[1]
    c0, a, b, p, q, r = coeffs
    return c0 + a * x + b * y + (p * x * x + 2.0 * q * x * y + r * y * y) / 2.0


def table_of_heights(ref_xy, dz, missing=None):
    """-> dict(table float32 [1 + F, m, 10], ref_disp, ref_xyz, start = 0): frame 0 is the start (all zeros, every slot seen), frame
    1 + f has Z = dz[f] (float32) and X = Y = 0, so with scale 1 in plane mode the end points are (ref_x, ref_y, (double)float32(dz)).
    `missing` [F, m]: rows without VBS_FLAG_XYZ, holding NaN."""
    dz = np.atleast_2d(np.asarray(dz, dtype=np.float64))
    F, m = dz.shape
    t = np.zeros((1 + F, m, 10), dtype=np.float32)
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    t[1:, :, 8] = dz.astype(np.float32)
    if missing is not None:
        dead = np.concatenate([np.zeros((1, m), dtype=bool), np.asarray(missing, dtype=bool)])
        t[..., 0][dead] = FLAG_TRACKED
        t[..., 6:9][dead] = np.nan
    ref_disp = np.zeros((m, 4))
    ref_disp[:, 0] = 1.0
    ref_xyz = np.concatenate([np.asarray(ref_xy, dtype=np.float64), np.zeros((m, 1))], axis=1)
    return dict(table=t, ref_disp=ref_disp, ref_xyz=ref_xyz, start=0)


def degeneracies():
    """name -> (ref_xy [m, 2], dz [m], missing [m], min_count, the degree the entry must report or ('max', d))."""
    rng = np.random.default_rng(77)
    out = {}
    xy = irregular_xy(16, 3)
    z = quadric_z(xy, (0.3, -0.2), (0.1, 0.02, -0.03, 0.05, 0.01, 0.04)) + rng.normal(size=16) * 0.01
    for k in (0, 1, 2):
        out[f"count {k}"] = (xy, z, np.arange(16) >= k, 9, 0)
    for k in (3, 4, 5):
        out[f"count {k}"] = (xy, z, np.arange(16) >= k, 9, 1)
    out["count 8 < min_count 9"] = (xy, z, np.arange(16) >= 8, 9, 1)
    out["count 8 >= min_count 6"] = (xy, z, np.arange(16) >= 8, 6, 2)
    out["count 16"] = (xy, z, np.zeros(16, dtype=bool), 9, 2)
    t = np.linspace(-5.0, 5.0, 16)
    out["collinear"] = (np.stack([1.0 + 0.6 * t, -2.0 + 0.8 * t], axis=1), 0.05 * t * t, np.zeros(16, dtype=bool), 9, 0)
    out["a line in u only"] = (np.stack([t, np.full(16, 1.25)], axis=1), 0.05 * t * t, np.zeros(16, dtype=bool), 9, ("max", 1))
    a = 2.0 * np.pi * np.arange(12) / 12 + 0.1
    circ = np.stack([3.0 + 4.0 * np.cos(a), -1.0 + 4.0 * np.sin(a)], axis=1)
    out["12 markers on a circle"] = (circ, 0.02 * circ[:, 0] - 0.01 * circ[:, 1] + rng.normal(size=12) * 0.01,
                                     np.zeros(12, dtype=bool), 9, 1)
    return out


def rejection_sets():
    """name -> (ref_xy, dz, min_count, reject_k): 30 markers on a noisy bowl with one gross outlier (slot 11), and 9 markers whose
    kept set cannot hold degree 2 at min_count 9."""
    rng = np.random.default_rng(78)
    xy = irregular_xy(30, 5)
    z = quadric_z(xy, (0.0, 0.0), (-0.4, 0.01, 0.02, 0.06, -0.01, 0.05)) + rng.normal(size=30) * 0.005
    z[11] += 1.5
    xy9 = irregular_xy(9, 6)
    z9 = quadric_z(xy9, (0.0, 0.0), (-0.4, 0.01, 0.02, 0.06, -0.01, 0.05)) + rng.normal(size=9) * 0.005
    return {"outlier": (xy, z, 9, 3.0), "too few kept": (xy9, z9, 9, 1.0)}


# ---- general recordings (the GPU cases) ----------------------------------------------------------------------------------------------
def recording(n, m, start, seed=0, drop=0.1, outliers=0, empty_frame=None, bad_ref=0.05):
    """-> dict(table float32 [n, m, 10], ref_disp [m, 4], ref_xyz [m, 3], start, length): markers at a jittered grid with a shallow
    dome in Z; frame f presses a bowl of growing depth into them, with noise on all axes.  A fraction `drop` of the rows (not in
    the start frame) has no 3-D point; a fraction `bad_ref` of the slots has ref_disp flag 0.  Every cell the contract says is not
    read holds NaN or a huge value: columns 1 - 5 and 9 everywhere, X Y Z of rows without the flag, ref_disp and ref_xyz of a slot
    whose flag is 0 (1e300 there: float64).  `outliers` slots per frame (from frame 2 on) are lifted by 3.5; `empty_frame` loses
    every row."""
    rng = np.random.default_rng(4000 + seed)
    ref = PO.grid_ref(m)
    ref[:, :2] += rng.uniform(-0.4, 0.4, size=(m, 2))
    xyz = np.broadcast_to(ref[None], (n, m, 3)).copy()
    r2 = ((ref[:, :2] - np.array([0.7, -0.4])) ** 2).sum(axis=1)
    span = max(float(np.sqrt(r2.max())), 1.0)
    for f in range(n):
        depth = 0.15 * (f + 1)
        xyz[f, :, 2] += -depth * np.exp(-r2 / (0.5 * span * span))
        xyz[f] += rng.normal(size=(m, 3)) * np.array([0.01, 0.01, 0.004])
        if f >= 2 and outliers:
            xyz[f, rng.choice(m, size=min(outliers, m), replace=False), 2] += 3.5
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    t[..., 6:9] = xyz.astype(np.float32)
    junk = lambda shape: np.where(rng.random(shape) < 0.5, np.float32(np.nan), np.float32(1e30)).astype(np.float32)   # noqa: E731
    for col in (1, 2, 3, 4, 5, 9):
        t[..., col] = junk((n, m))
    dead = rng.random((n, m)) < drop
    dead[start] = False
    if empty_frame is not None:
        dead[empty_frame] = True
    k = int(dead.sum())
    t[..., 0][dead] = (rng.random(k) < 0.5).astype(np.float32) * FLAG_TRACKED
    t[..., 6:9][dead] = junk((k, 3))
    bad = rng.random(m) < bad_ref
    ref_disp = np.concatenate([np.ones((m, 1)), rng.normal(size=(m, 3)) * 0.05], axis=1)
    big = lambda shape: np.where(rng.random(shape) < 0.5, np.nan, 1e300)       # noqa: E731
    ref_disp[bad] = np.concatenate([np.zeros((int(bad.sum()), 1)), big((int(bad.sum()), 3))], axis=1)
    ref_xyz = ref.copy()
    ref_xyz[bad] = big((int(bad.sum()), 3))
    good = ~bad
    length = rms_length(ref[good, :2]) if good.sum() >= 2 and rms_length(ref[good, :2]) > 0 else 1.0
    return dict(table=t, ref_disp=ref_disp, ref_xyz=ref_xyz, start=start, length=length)


# ---- a rendered spherical cap ------------------------------------------------------------------------------------------------------------
def cap_heights(ref, R, centre, depth):
    """dZ [m] of a flat field pressed by a sphere of radius R whose lowest point is `depth` below the field at `centre` (x, y): the
    field follows the sphere, dz = -depth + (R - sqrt(R R - rho rho)), rho the distance from the centre."""
    rho2 = (ref[:, 0] - centre[0]) ** 2 + (ref[:, 1] - centre[1]) ** 2
    return -depth + (R - np.sqrt(R * R - rho2))


def cap_recording(cam, ref, R, centres, depths, seed=0, pixel_sigma=PIXEL_SIGMA):
    """A float32 table [1 + F, m, 10] rendered through the camera as `posecov_cases.tilted_recording` renders its own: frame 0 the
    flat field at rest, frame 1 + f the cap of `depths[f]` at `centres[f]`; the pixel columns carry Gaussian noise of
    `pixel_sigma` px and X, Y, Z are their solve.  R: one radius or one per frame.  -> table."""
    rng = np.random.default_rng(1900 + seed)
    c = U.Cam(*cam)
    F, m = len(depths), ref.shape[0]
    Rs = np.broadcast_to(np.asarray(R, dtype=np.float64), (F,))
    t = np.zeros((1 + F, m, 10), dtype=np.float32)
    for f in range(1 + F):
        X = ref.copy()
        if f:
            X[:, 2] += cap_heights(ref, float(Rs[f - 1]), centres[f - 1], depths[f - 1])
        t[f, :, 1:4] = PC.observe(c, X) + rng.normal(size=(m, 3)) * pixel_sigma
    _, Xs, ok = U.primal(c, t[..., 1].ravel().astype(np.float64), t[..., 2].ravel().astype(np.float64),
                         t[..., 3].ravel().astype(np.float64))
    assert ok.all()
    t[..., 6:9] = Xs.reshape(1 + F, m, 3)
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    return t
