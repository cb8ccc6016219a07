"""Point sets and recordings the tests of `vbs_rigid_series` share (`tests/test_rigid_host.py`, `tests/test_gpu_rigid.py`): seeded
and small.  A recording is a float32 table whose X, Y, Z columns carry a moved copy of a layout, and a `source` [m, 4] = (flag, X, Y,
Z) the frames are registered to; every cell the contract says is not read holds NaN or a huge value."""
import numpy as np

FLAG_TRACKED, FLAG_XYZ = 1, 2
# the sensor's published layout (radius mm, count, first angle deg): 65 markers, the four outer ones on the axes
RINGS65 = ((0.0, 1, 0.0), (3.49, 6, 30.0), (6.92, 12, 0.0), (10.23, 18, 10.0), (13.37, 24, 0.0), (16.29, 4, 0.0))
SHELL_RISE, SHELL_RADIUS = 5.47, 16.29                          # the shell rises 5.47 mm over a radius of 16.29 mm


def layout65(shell=True):
    """[65, 3]: the ring layout, Z on the sphere through the rim that rises SHELL_RISE over SHELL_RADIUS (0 with shell=False)."""
    pts = []
    for radius, count, a0 in RINGS65:
        for k in range(count):
            a = np.deg2rad(a0 + 360.0 * k / count)
            pts.append((radius * np.cos(a), radius * np.sin(a)))
    xy = np.asarray(pts, dtype=np.float64)
    z = np.zeros(len(pts))
    if shell:
        big = (SHELL_RADIUS ** 2 + SHELL_RISE ** 2) / (2.0 * SHELL_RISE)
        z = np.sqrt(big * big - (xy ** 2).sum(axis=1)) - (big - SHELL_RISE)
    return np.column_stack([xy, z])


def flat_grid(m, pitch=2.0, seed=None):
    """m positions on a square grid in the plane Z = 0, jittered in the plane with a seed."""
    side = int(np.ceil(np.sqrt(m)))
    i = np.arange(m)
    xy = np.stack([(i % side - (side - 1) / 2) * pitch, (i // side - (side - 1) / 2) * pitch], axis=1).astype(np.float64)
    if seed is not None:
        xy = xy + np.random.default_rng(700 + seed).uniform(-0.3, 0.3, size=xy.shape) * pitch
    return np.column_stack([xy, np.zeros(m)])


def rotation(axis, angle_deg):
    """The rotation by `angle_deg` about `axis` (Rodrigues); exactly 180 degrees is 2 a a' - I, without a rounded sine."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    if angle_deg == 180.0:
        return 2.0 * np.outer(a, a) - np.eye(3)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(angle_deg)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def swing_twist(tilt_deg, azimuth_deg, twist_deg):
    """Twist about z, then a swing that leans the normal by `tilt_deg` towards `azimuth_deg`: R (0, 0, 1) = (sin t cos a, sin t sin a,
    cos t), the conventions of the columns tilt_deg, azimuth_deg and twist_deg."""
    az = np.deg2rad(azimuth_deg)
    return rotation((-np.sin(az), np.cos(az), 0.0), tilt_deg) @ rotation((0.0, 0.0, 1.0), twist_deg)


def source_of(layout, bad=None):
    """source [m, 4] of a layout; the slots of `bad` get flag 0 and 1e300 / NaN in their coordinates."""
    m = layout.shape[0]
    src = np.concatenate([np.ones((m, 1)), np.asarray(layout, dtype=np.float64)], axis=1)
    if bad is not None and np.any(bad):
        k = int(np.sum(bad))
        src[bad] = np.concatenate([np.zeros((k, 1)), np.where(np.arange(3 * k).reshape(k, 3) % 2 == 0, np.nan, 1e300)], axis=1)
    return src


def table_of_points(P, missing=None, seed=0):
    """float32 table [F, m, 10] with X, Y, Z = P [F, m, 3]: both flags set, NaN / 1e30 in the columns 1 - 5 and 9, which the entry
    never reads; rows of `missing` [F, m] lose VBS_FLAG_XYZ and hold NaN / 1e30 in X, Y, Z."""
    rng = np.random.default_rng(900 + seed)
    P = np.asarray(P, dtype=np.float64)
    F, m = P.shape[:2]
    junk = lambda shape: np.where(rng.random(shape) < 0.5, np.float32(np.nan), np.float32(1e30)).astype(np.float32)   # noqa: E731
    t = np.zeros((F, m, 10), dtype=np.float32)
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    t[..., 6:9] = P.astype(np.float32)
    for col in (1, 2, 3, 4, 5, 9):
        t[..., col] = junk((F, m))
    if missing is not None:
        dead = np.asarray(missing, dtype=bool)
        k = int(dead.sum())
        t[..., 0][dead] = (rng.random(k) < 0.5).astype(np.float32) * FLAG_TRACKED
        t[..., 6:9][dead] = junk((k, 3))
    return t


def moved(layout, R, t, s=1.0):
    return s * (np.asarray(layout) @ np.asarray(R).T) + np.asarray(t, dtype=np.float64)


def recording(n, m, seed=0, drop=0.1, outliers=0, empty_frame=None, bad_src=0.05, scale=1.0):
    """-> dict(table, source, layout, poses): a jittered grid on a shallow dome; frame f is the layout rotated by 1.5 f degrees about
    an oblique axis, shifted and scaled by `scale` ** f, with noise of 0.01 mm.  A share `drop` of the rows has no 3-D point, a share
    `bad_src` of the slots has source flag 0, `outliers` slots per frame (from frame 1 on) are moved by 2.5 mm, `empty_frame` loses
    every row."""
    rng = np.random.default_rng(5000 + seed)
    lay = flat_grid(m, 2.0, seed)
    lay[:, 2] = 0.9 - 0.004 * (lay[:, :2] ** 2).sum(axis=1)
    P = np.empty((n, m, 3))
    poses = []
    for f in range(n):
        R, t, s = rotation((0.3, -0.5, 0.8), 1.5 * f), np.array([0.2 * f, -0.1 * f, 0.05 * f]), scale ** f
        poses.append((R, t, s))
        P[f] = moved(lay, R, t, s) + rng.normal(size=(m, 3)) * 0.01
        if f >= 1 and outliers:
            P[f, rng.choice(m, size=min(outliers, m), replace=False)] += np.array([1.5, -1.0, 1.7])
    dead = rng.random((n, m)) < drop
    if empty_frame is not None:
        dead[empty_frame] = True
    bad = rng.random(m) < bad_src
    return dict(table=table_of_points(P, dead, seed), source=source_of(lay, bad), layout=lay, poses=poses)


def tilt_twist_recording(n, tilt_end=2.0, twist_end=3.0, azimuth=35.0, noise=0.02, gaps=0.03, seed=0, dimple=None):
    """The 65-marker shell tilted 0 -> `tilt_end` degrees towards `azimuth` and twisted 0 -> `twist_end` degrees about its normal
    along n frames, about its own centroid, with `noise` mm on every coordinate and a share `gaps` of the rows missing.  `dimple` =
    (x, y, depth, width): a Gaussian dimple pressed along -Z of the layout BEFORE the motion, growing linearly with the frame.
    -> dict(table, source, layout, tilt [n], twist [n], azimuth)."""
    rng = np.random.default_rng(6000 + seed)
    lay = layout65()
    centre = lay.mean(axis=0)
    tilt, twist = np.linspace(0.0, tilt_end, n), np.linspace(0.0, twist_end, n)
    P = np.empty((n, 65, 3))
    for f in range(n):
        body = lay.copy()
        if dimple is not None:
            x, y, depth, width = dimple
            body[:, 2] -= (depth * f / max(n - 1, 1)) * np.exp(-((lay[:, 0] - x) ** 2 + (lay[:, 1] - y) ** 2) / (2.0 * width * width))
        P[f] = moved(body - centre, swing_twist(tilt[f], azimuth, twist[f]), centre) + rng.normal(size=(65, 3)) * noise
    dead = rng.random((n, 65)) < gaps
    dead[0] = False
    return dict(table=table_of_points(P, dead, seed), source=source_of(lay), layout=lay, tilt=tilt, twist=twist, azimuth=azimuth)
