"""Scenes and recordings the tests of `vbs_rigid_ml_series` share (`tests/test_rigid_ml_host.py`, `tests/test_gpu_rigid_ml.py`): the
`layout65` shell and the `recording` grids of `rigid_cases`, with a covariance per 3-D point built as a needle along its viewing ray,
    Sigma = sigma_lat^2 (I - u u') + (h sigma_rel)^2 u u',        u = (X - cam) / h,   h = |X - cam|,
about a stated camera centre.  Every cell the contract says is not read holds NaN, 1e30 or 1e300."""
import numpy as np

import rigid_cases as RC
import rigid_oracle as RO

CAM = np.array([0.0, 0.0, 45.0])                                # the camera centre, 45 mm above the layout's plane
SIGMA_LAT, SIGMA_REL = 0.0035, 0.14 / 45.0                      # mm across the ray; along it, relative to the distance
_COLS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def needle(X, cam=CAM, sigma_lat=SIGMA_LAT, sigma_rel=SIGMA_REL):
    """[..., 3] points -> [..., 3, 3] covariances."""
    X = np.asarray(X, dtype=np.float64)
    v = X - np.asarray(cam, dtype=np.float64)
    h = np.sqrt((v * v).sum(axis=-1))
    u = v / h[..., None]
    uu = u[..., :, None] * u[..., None, :]
    return sigma_lat ** 2 * (np.eye(3) - uu) + ((h * sigma_rel) ** 2)[..., None, None] * uu


def cov7(S, flag=None):
    """[..., 3, 3] -> the record [..., 7] = (flag, xx, xy, xz, yy, yz, zz); rows with flag 0 hold NaN / 1e300."""
    S = np.asarray(S, dtype=np.float64)
    out = np.ones(S.shape[:-2] + (7,))
    for k, (i, j) in enumerate(_COLS):
        out[..., 1 + k] = S[..., i, j]
    if flag is not None:
        dead = ~np.asarray(flag, dtype=bool)
        junk = np.where(np.arange(6) % 2 == 0, np.nan, 1e300)
        out[dead] = np.concatenate([[0.0], junk])
    return out


def draw(rng, S):
    """One draw of N(0, S) per covariance of S [..., 3, 3]."""
    Lc = np.linalg.cholesky(S)
    return (Lc @ rng.normal(size=S.shape[:-1] + (1,)))[..., 0]


def scene(n, seed=0, tilt=1.0, twist=1.5, azimuth=35.0, sigma_lat=SIGMA_LAT, sigma_rel=SIGMA_REL, isotropic=None, slots=None):
    """n independent draws of ONE motion of the 65-marker shell (tilt and twist in degrees about its centroid, a shift of
    (0.02, -0.01, 0.03) mm) seen from `CAM`: -> dict(table [n, k, 10], source [k, 4], cov [n, k, 7], S [n, k, 3, 3], R, c, qm, layout).
    `isotropic`: a sigma, for equal isotropic covariances instead of needles.  `slots`: the layout rows kept."""
    rng = np.random.default_rng(8000 + seed)
    lay = RC.layout65()
    if slots is not None:
        lay = lay[np.asarray(slots)]
    qm = lay.mean(axis=0)
    R = RC.swing_twist(tilt, azimuth, twist)
    c = qm + np.array([0.02, -0.01, 0.03])
    X = (lay - qm) @ R.T + c
    S1 = needle(X, CAM, sigma_lat, sigma_rel) if isotropic is None else np.broadcast_to(isotropic ** 2 * np.eye(3), (len(lay), 3, 3))
    S = np.broadcast_to(S1, (n,) + S1.shape).copy()
    P = X[None] + draw(rng, S)
    table = RC.table_of_points(P, None, seed)
    # the table is float32: its rounding (1e-6 mm at 20 mm) is three orders below sigma_lat
    return dict(table=table, source=RC.source_of(lay), cov=cov7(S), S=S, R=R, c=c, qm=qm, layout=lay)


def start_of(k, reject_k=0.0, frame_range=None):
    """The start records of a case by the restatement of `vbs_rigid_series` (with_scale off) -> (rigid, residual)."""
    rigid, _, res = RO.rigid_series(k["table"], k["source"], None, False, reject_k, frame_range=frame_range)
    return rigid, res


def recording(n, m, seed=0, reject_k=0.0, with_source_cov=False, drop=0.1, cov_dead=0.05, singular=2, outliers=0):
    """A `rigid_cases.recording` with needles about a camera 60 mm above the grid, a share `cov_dead` of cov flags of 0, `singular`
    slots per frame whose covariance has a zero pivot, frame 1 (where there is one) without a start (every row lost) and frame 2 with
    two usable covariances only, so that it ends in flag 1.  -> the dict of `rigid_cases.recording` plus cov [n, m, 7], source_cov
    [m, 7] or None, rigid_clean, residual_clean (the restated start), rigid, residual (the same with every cell that is not read
    overwritten: `poison_start`) and reject_k."""
    small = m < 10
    k = RC.recording(n, m, seed=seed, drop=0.0 if small else drop, outliers=outliers, empty_frame=1 if n > 1 else None,
                     bad_src=0.0 if small else 0.05)
    rng = np.random.default_rng(8100 + seed)
    cam = np.array([0.0, 0.0, 60.0])
    P = k["table"][..., 6:9].astype(np.float64)
    P = np.where(np.isfinite(P) & (np.abs(P) < 1e6), P, 1.0)        # (rows without a point get a covariance nobody reads)
    S = needle(P, cam, 0.004, 0.003)
    alive = np.ones((n, m), dtype=bool) if small else rng.random((n, m)) >= cov_dead
    if not small:
        for f in range(n):
            for s in rng.choice(m, size=min(singular, m), replace=False):
                S[f, s] = np.diag([1e-4, 0.0, 1e-4]) if s % 2 else np.zeros((3, 3))
    if n > 2:
        alive[2] = False
        alive[2, :2] = True
    k["cov"] = cov7(S, alive)
    k["source_cov"] = None
    if with_source_cov:
        ok = np.ones(m, dtype=bool) if small else rng.random(m) >= 0.03
        k["source_cov"] = cov7(needle(k["layout"], cam, 0.004, 0.003), ok)
    k["reject_k"] = reject_k
    k["rigid_clean"], k["residual_clean"] = start_of(k, reject_k)
    k["rigid"], k["residual"] = poison_start(k["rigid_clean"], k["residual_clean"], seed)
    return k


READ_COLS = (0, 3, 4, 5, 9, 10, 11, 12, 22, 23, 24)             # of a row of `rigid` with a start: flag, qm, the quaternion, t


def poison_start(rigid, residual, seed=0):
    """Copies of the start records with NaN / 1e30 / 1e300 in every cell the contract says is not read: of `rigid` everything but
    `READ_COLS` in a row with a start and everything but the flag in a row without one; of `residual` the columns 1 - 3 of every
    row.  The restatement and the device are both handed these."""
    rng = np.random.default_rng(8200 + seed)
    junk = lambda shape: rng.choice(np.array([np.nan, 1e30, 1e300, -1e300]), size=shape)              # noqa: E731
    rg, rs = np.array(rigid, dtype=np.float64), np.array(residual, dtype=np.float64)
    keep = np.zeros(rg.shape, dtype=bool)
    keep[:, READ_COLS] = rg[:, :1] != 0.0
    keep[:, 0] = True
    rg = np.where(keep, rg, junk(rg.shape))
    rs[..., 1:] = junk(rs[..., 1:].shape)
    return rg, rs
