"""Host side of the uncertainty of the 3-D solve (`vbs_uncert_cov`, `vbs_uncert_total`), NumPy only: the factor of
the camera's covariance the entries take, the covariance of a set of poses, the isotropic observation covariance.

The camera vector theta has 16 entries: fx, fy, cx, cy, k1, k2, p1, p2, k3, w0, w1, w2, T0, T1, T2, dmm - w a small rotation on
the camera side, R_wc' = exp([w]x) R_wc.  The device never sees Sigma_theta as a matrix: it takes L [16, q] with Sigma_theta =
L L' and pushes every column through the solve as one direction, so whatever it builds from them is a sum of squares.
"""
import numpy as np

N_THETA = 16
THETA = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "w0", "w1", "w2", "T0", "T1", "T2", "dmm")
# the error constant of `camera_factor(cov=..)`: every entry of L L' - cov is at most CHOL_EPS trace(cov) for a positive definite cov
# (Cholesky's backward error gamma_(n+1) |L| |L'|, and no entry of |L| |L'| exceeds ||L||_F^2 = trace(cov))
CHOL_EPS = (N_THETA + 1) * 2.0 ** -53


def obs_cov(sigma_centre, sigma_diameter):
    """The isotropic shortcut: [6] = uu, uv, ud, vv, vd, dd of (Cx, Cy, major) with independent errors."""
    sc, sd = float(sigma_centre), float(sigma_diameter)
    if not (np.isfinite(sc) and np.isfinite(sd) and sc >= 0.0 and sd >= 0.0):
        raise ValueError("sigma_centre and sigma_diameter must be finite and >= 0")
    return np.array([sc * sc, 0.0, 0.0, sc * sc, 0.0, sd * sd])


def _pivoted_cholesky(cov):
    """cov = L L' for a symmetric positive semidefinite matrix, largest remaining diagonal first; a pivot <= 0 ends it (what is
    left is zero up to rounding, or the matrix was not semidefinite: the directions are dropped)."""
    A = np.array(cov, dtype=np.float64)
    n = A.shape[0]
    cols = []
    for _ in range(n):
        dg = np.diag(A)
        p = int(np.argmax(dg))
        if not dg[p] > 0.0:
            break
        col = A[:, p] / np.sqrt(dg[p])
        cols.append(col)
        A = A - np.outer(col, col)
        A[p, :] = 0.0
        A[:, p] = 0.0
    return np.stack(cols, axis=1) if cols else np.zeros((n, 0))


def camera_factor(std_intrinsics=None, omega_std=None, t_std=None, diameter_std=None, cov=None):
    """L [16, q] with Sigma_theta = L L'.  Either the diagonal inputs - `std_intrinsics` [9] (fx fy cx cy k1 k2 p1 p2 k3, as
    `calibrate_camera_points` returns them), `omega_std` [3] (rad), `t_std` [3], `diameter_std` (mm); None = exact - which give a
    diagonal factor with its zero columns dropped, or a full symmetric 16 x 16 `cov`, factored by a pivoted Cholesky that drops
    pivots <= 0.  A `cov` that is not symmetric, or anything non-finite or negative, is refused."""
    if cov is not None:
        if any(v is not None for v in (std_intrinsics, omega_std, t_std, diameter_std)):
            raise ValueError("either cov or the diagonal inputs")
        S = np.asarray(cov, dtype=np.float64)
        if S.shape != (N_THETA, N_THETA) or not np.isfinite(S).all():
            raise ValueError(f"cov must be a finite [{N_THETA}, {N_THETA}] matrix")
        if not np.array_equal(S, S.T):
            raise ValueError("cov must be symmetric")
        return _pivoted_cholesky(S)
    sd = np.zeros(N_THETA)
    for lo, size, v, what in ((0, 9, std_intrinsics, "std_intrinsics"), (9, 3, omega_std, "omega_std"), (12, 3, t_std, "t_std"),
                              (15, 1, diameter_std, "diameter_std")):
        if v is None:
            continue
        a = np.asarray(v, dtype=np.float64).reshape(-1)
        if a.size != size or not np.isfinite(a).all() or (a < 0.0).any():
            raise ValueError(f"{what} must be {size} finite values >= 0")
        sd[lo:lo + size] = a
    keep = np.nonzero(sd > 0.0)[0]
    Lf = np.zeros((N_THETA, keep.size))
    Lf[keep, np.arange(keep.size)] = sd[keep]
    return Lf


def _log_so3(R):
    """The rotation vector of a rotation matrix (angles below pi)."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    s = float(np.linalg.norm(w))                                   # sin(angle)
    c = (np.trace(R) - 1.0) / 2.0
    ang = float(np.arctan2(s, c))
    return w if s < 1e-12 else w * (ang / s)


def _exp_so3(w):
    w = np.asarray(w, dtype=np.float64)
    a = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if a < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(a) / a) * K + ((1.0 - np.cos(a)) / (a * a)) * (K @ K)


def mean_pose(R_list, T_list):
    """The mean of K poses: R_mean the chordal mean (the rotation nearest the mean matrix), T_mean the mean translation."""
    Rs = np.asarray(R_list, dtype=np.float64).reshape(-1, 3, 3)
    Ts = np.asarray(T_list, dtype=np.float64).reshape(-1, 3)
    if Rs.shape[0] != Ts.shape[0] or Rs.shape[0] < 1:
        raise ValueError("K >= 1 rotations [K, 3, 3] and translations [K, 3]")
    U, _, Vt = np.linalg.svd(Rs.mean(axis=0))
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt, Ts.mean(axis=0)


def pose_scatter(R_list, T_list):
    """The scatter of K >= 2 poses (R_k world -> camera, T_k), as `calibrate_recording` produces them, mapped into theta: with
    the `mean_pose`, w_k = log(R_k R_mean'), T_k - T_mean.  Returns the [6, 6] sample covariance (ddof 1) of (w, T) - rows and
    columns 9 .. 14 of Sigma_theta (`embed_pose_cov`)."""
    Rs = np.asarray(R_list, dtype=np.float64).reshape(-1, 3, 3)
    Ts = np.asarray(T_list, dtype=np.float64).reshape(-1, 3)
    if Rs.shape[0] != Ts.shape[0] or Rs.shape[0] < 2:
        raise ValueError("pose_scatter needs K >= 2 rotations [K, 3, 3] and translations [K, 3]")
    Rm, Tm = mean_pose(Rs, Ts)
    x = np.array([np.concatenate([_log_so3(Rk @ Rm.T), Tk - Tm]) for Rk, Tk in zip(Rs, Ts)])
    x = x - x.mean(axis=0)
    return x.T @ x / (Rs.shape[0] - 1.0)


def embed_pose_cov(cov6, base=None):
    """A 16 x 16 Sigma_theta with `cov6` (of w, T) in rows and columns 9 .. 14, on top of `base` (default zeros)."""
    S = np.zeros((N_THETA, N_THETA)) if base is None else np.array(base, dtype=np.float64)
    S[9:15, 9:15] = S[9:15, 9:15] + np.asarray(cov6, dtype=np.float64)
    return S
