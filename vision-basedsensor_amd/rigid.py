"""Host-side companions of `analysis.rigid_series`: the point set a recording is registered to, the rotation nearest
to a filtered matrix, the angles of a rotation, the share of the motion that is rigid and the kind of motion a row of `rigid`
describes; and of `analysis.rigid_ml_series`: the standard deviations of the weighted pose, its covariance referred to
another point and the chi-squared check.  NumPy only; nothing here touches a device."""
import math

import numpy as np

RIGID_COLS, RIGID_SWEEPS = 33, 8
(FLAG, COUNT, N_USED, QMX, QMY, QMZ, PMX, PMY, PMZ, QW, QX, QY, QZ, R00, R01, R02, R10, R11, R12, R20, R21, R22, TX, TY, TZ, SCALE,
 RMS, RMS0, ANGLE_DEG, TILT_DEG, AZIMUTH_DEG, TWIST_DEG, GAP) = range(RIGID_COLS)
RIGID_COLUMNS = ("flag", "count", "n_used", "qmx", "qmy", "qmz", "pmx", "pmy", "pmz", "qw", "qx", "qy", "qz", "r00", "r01", "r02", "r10",
                 "r11", "r12", "r20", "r21", "r22", "tx", "ty", "tz", "scale", "rms", "rms0", "angle_deg", "tilt_deg", "azimuth_deg",
                 "twist_deg", "gap")
RIGID_ML_COLS, RIGID_ML_PCOV_COLS = 40, 22
(ML_FLAG, ML_N_START, ML_N_USED, ML_STEPS, ML_QW, ML_QX, ML_QY, ML_QZ) = range(8)
(ML_R00, ML_TX, ML_CX, ML_QMX, ML_CHI2, ML_DOF, ML_CHI2_START, ML_STEP_ROT, ML_STEP_C, ML_ANGLE_DEG, ML_TILT_DEG, ML_AZIMUTH_DEG,
 ML_TWIST_DEG, ML_NXX, ML_NXY, ML_NYY, ML_T2_TILT, ML_VAR_TWIST) = (8, 17, 20, 23, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39)
KIND_NONE, KIND_STILL, KIND_SHIFT, KIND_TILT, KIND_TWIST, KIND_MIXED = range(6)
KIND_NAMES = ("none", "still", "shift", "tilt", "twist", "mixed")
_DEG = 57.29577951308232
_FLAG_XYZ = 2
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def source_from_table(table, frame):
    """`source` [m, 4] from frame `frame` of a table [n, m, 10] (host array or tensor): flag = 1 where the row carries
    VBS_FLAG_XYZ, X, Y, Z the float64 of its float32 columns 6 - 8 (0 where it does not)."""
    t = table.detach().cpu().numpy() if hasattr(table, "detach") else np.asarray(table)
    if t.ndim != 3 or t.shape[2] != 10:
        raise ValueError("table must be [n, m, 10]")
    if int(frame) != frame or not (0 <= int(frame) < t.shape[0]):
        raise ValueError(f"frame {frame} outside the table's {t.shape[0]} frames")
    row = t[int(frame)].astype(np.float32)
    ok = (np.nan_to_num(row[:, 0], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) & _FLAG_XYZ) != 0
    src = np.zeros((t.shape[1], 4))
    src[:, 0] = ok
    src[:, 1:] = np.where(ok[:, None], row[:, 6:9].astype(np.float64), 0.0)
    return src


def source_from_layout(xyz, valid=None):
    """`source` [m, 4] from a layout [m, 3]: flag = 1 where `valid` (all rows by default) and the three coordinates are finite."""
    p = np.asarray(xyz, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("layout must be [m, 3]")
    ok = np.isfinite(p).all(axis=1)
    if valid is not None:
        v = np.asarray(valid).astype(bool).reshape(-1)
        if v.shape[0] != p.shape[0]:
            raise ValueError("valid must have one entry per layout row")
        ok = ok & v
    src = np.zeros((p.shape[0], 4))
    src[:, 0] = ok
    src[:, 1:] = np.where(ok[:, None], p, 0.0)
    return src


def _leading_quaternion(H):
    """Horn's N of H [3][3] (H[i][j] = sum q_i p_j), `vbs_rigid_series`'s cyclic Jacobi and eigenvector rule -> (w, x, y, z)."""
    (Hxx, Hxy, Hxz), (Hyx, Hyy, Hyz), (Hzx, Hzy, Hzz) = [[float(v) for v in r] for r in H]
    T = [[0.0] * 4 for _ in range(4)]
    T[0][0], T[1][1], T[2][2], T[3][3] = (Hxx + Hyy) + Hzz, (Hxx - Hyy) - Hzz, (Hyy - Hxx) - Hzz, (Hzz - Hxx) - Hyy
    T[0][1], T[0][2], T[0][3] = Hyz - Hzy, Hzx - Hxz, Hxy - Hyx
    T[1][2], T[1][3], T[2][3] = Hxy + Hyx, Hzx + Hxz, Hyz + Hzy
    for p, q in _PAIRS:
        T[q][p] = T[p][q]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(RIGID_SWEEPS):
        for p, q in _PAIRS:
            apq = T[p][q]
            if apq == 0.0:
                continue
            theta = (T[q][q] - T[p][p]) / (2.0 * apq)
            tt = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            cs = 1.0 / math.sqrt(tt * tt + 1.0)
            sn = tt * cs
            for k in range(4):
                x, y = T[k][p], T[k][q]
                T[k][p], T[k][q] = cs * x - sn * y, sn * x + cs * y
            for k in range(4):
                x, y = T[p][k], T[q][k]
                T[p][k], T[q][k] = cs * x - sn * y, sn * x + cs * y
            for k in range(4):
                x, y = V[k][p], V[k][q]
                V[k][p], V[k][q] = cs * x - sn * y, sn * x + cs * y
            T[p][q] = T[q][p] = 0.0
    k = 0
    for i in range(1, 4):
        if T[i][i] > T[k][k]:
            k = i
    v = [V[i][k] for i in range(4)]
    nr = math.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
    w, x, y, z = v[0] / nr, v[1] / nr, v[2] / nr, v[3] / nr
    first = x if x != 0.0 else (y if y != 0.0 else z)
    if w < 0.0 or (w == 0.0 and first < 0.0):
        w, x, y, z = -w, -x, -y, -z
    return w, x, y, z


def _rotation(w, x, y, z):
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def nearest_rotation(M):
    """The rotation nearest to every 3 x 3 matrix of M [..., 3, 3] in the Frobenius sense: the R that maximises trace(R' M), by the
    N, the Jacobi and the eigenvector rule of `vbs_rigid_series` with H = M' - always proper, no determinant fix.  It turns a
    FILTERED `coef` back into rotations (trends are taken from filtered matrices, never from filtered angles or quaternions).  A
    matrix that is not finite gives NaN."""
    A = np.asarray(M, dtype=np.float64)
    if A.ndim < 2 or A.shape[-2:] != (3, 3):
        raise ValueError("M must be [..., 3, 3]")
    flat = A.reshape(-1, 3, 3)
    out = np.full(flat.shape, np.nan)
    for i, m in enumerate(flat):
        if np.isfinite(m).all():
            out[i] = _rotation(*_leading_quaternion(m.T))
    return out.reshape(A.shape)


def angles(R):
    """Columns 28 - 31 of `rigid` from rotations R [..., 3, 3]: -> [..., 4] = angle_deg, tilt_deg, azimuth_deg, twist_deg.  The angle
    and the twist come from the quaternion of R (the `nearest_rotation` rule, so a matrix that is only nearly a rotation is fine)."""
    A = np.asarray(R, dtype=np.float64)
    if A.ndim < 2 or A.shape[-2:] != (3, 3):
        raise ValueError("R must be [..., 3, 3]")
    flat = A.reshape(-1, 3, 3)
    out = np.full((flat.shape[0], 4), np.nan)
    for i, m in enumerate(flat):
        if not np.isfinite(m).all():
            continue
        w, x, y, z = _leading_quaternion(m.T)
        out[i] = ((2.0 * math.atan2(math.sqrt((x * x + y * y) + z * z), w)) * _DEG,
                  math.atan2(math.sqrt(m[0, 2] * m[0, 2] + m[1, 2] * m[1, 2]), m[2, 2]) * _DEG,
                  math.atan2(m[1, 2], m[0, 2]) * _DEG, (2.0 * math.atan2(z, w)) * _DEG)
    return out.reshape(A.shape[:-2] + (4,))


def rigid_share(rms, rms0):
    """1 - SSR / SS0 = 1 - (rms / rms0)^2: the share of the squared displacement P - Q that the rigid motion explains (NaN where
    rms0 is 0: nothing moved)."""
    a, b = np.asarray(rms, dtype=np.float64), np.asarray(rms0, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(b > 0.0, 1.0 - (a / np.where(b > 0.0, b, 1.0)) ** 2, np.nan)


def _rows(rigid):
    r = np.asarray(rigid, dtype=np.float64)
    if r.ndim == 1:
        r = r[None]
    if r.ndim != 2 or r.shape[1] != RIGID_COLS:
        raise ValueError(f"rigid must be [N, {RIGID_COLS}] (`rigid_series`)")
    return r


def kind(row, shift_mm=0.05, tilt_deg=0.1, twist_deg=0.1):
    """An integer code per row of `rigid`: KIND_NONE (flag 0), else by what exceeds its threshold - the shift of the centroid
    |pm - qm| > `shift_mm`, tilt_deg > `tilt_deg`, |twist_deg| > `twist_deg`: none of them KIND_STILL, exactly one KIND_SHIFT /
    KIND_TILT / KIND_TWIST, more than one KIND_MIXED.  The thresholds are arguments: they depend on the noise of the recording."""
    r = _rows(row)
    d = r[:, PMX:PMZ + 1] - r[:, QMX:QMZ + 1]
    shift = np.sqrt((d * d).sum(axis=1)) > float(shift_mm)
    tilt = r[:, TILT_DEG] > float(tilt_deg)
    twist = np.abs(r[:, TWIST_DEG]) > float(twist_deg)
    k = shift.astype(np.int64) + tilt + twist
    one = np.where(shift, KIND_SHIFT, np.where(tilt, KIND_TILT, KIND_TWIST))
    out = np.where(k == 0, KIND_STILL, np.where(k == 1, one, KIND_MIXED))
    return np.where(r[:, FLAG] == 0.0, KIND_NONE, out).astype(np.int64)


# ---- the weighted pose (`rigid_ml_series`) --------------------------------------------------------------------------------------------
def _ml_rows(ml, pcov=None):
    a = np.asarray(ml, dtype=np.float64)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != RIGID_ML_COLS:
        raise ValueError(f"ml must be [N, {RIGID_ML_COLS}] (`rigid_ml_series`)")
    if pcov is None:
        return a
    c = np.asarray(pcov, dtype=np.float64)
    if c.ndim == 1:
        c = c[None]
    if c.shape != (a.shape[0], RIGID_ML_PCOV_COLS):
        raise ValueError(f"pcov must be [N, {RIGID_ML_PCOV_COLS}], one row per row of ml")
    return a, c


def pose_covariance(pcov):
    """The symmetric [N, 6, 6] over (omega in rad, c in mm) from the rows of `pcov` (NaN where its flag is 0)."""
    c = np.asarray(pcov, dtype=np.float64)
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or c.shape[1] != RIGID_ML_PCOV_COLS:
        raise ValueError(f"pcov must be [N, {RIGID_ML_PCOV_COLS}] (`rigid_ml_series`)")
    out = np.full((c.shape[0], 6, 6), np.nan)
    at = 1
    for i in range(6):
        for j in range(i, 6):
            out[:, i, j] = out[:, j, i] = c[:, at]
            at += 1
    out[c[:, 0] == 0.0] = np.nan
    return out


def pose_sigma(ml, pcov):
    """-> (sigma_rot_deg [N, 3], sigma_c [N, 3]): the standard deviations of the three components of the rotation error omega, in
    degrees, and of the centre c = the image of qm, in mm (NaN where the frame has no weighted fit).  Components 0 and 1 of omega
    carry the tilt, component 2 the twist, for a body whose normal is near z."""
    a, _ = _ml_rows(ml, pcov)
    Cm = pose_covariance(pcov)
    d = np.stack([Cm[:, k, k] for k in range(6)], axis=1)
    with np.errstate(all="ignore"):
        sg = np.sqrt(d)
    return sg[:, :3] * _DEG, sg[:, 3:]


def move_centre(pcov, ml, point):
    """The covariance [N, 6, 6] of (omega, the image of `point`) from that of (omega, c = the image of qm): with lever = R (point -
    qm) the image is c + R (point - qm), and to first order  d image = dc + omega x lever = dc - [lever]x omega.  R and qm are the
    frame's own, read from its row of `ml` (`pcov` does not carry them).  `point` = qm is the identity; `point` = the origin gives
    the covariance of (omega, t).  `point` is [3], or [N, 3] with one point per frame."""
    a, _ = _ml_rows(ml, pcov)
    Cm = pose_covariance(pcov)
    Rm, qm = a[:, ML_R00:ML_R00 + 9].reshape(-1, 3, 3), a[:, ML_QMX:ML_QMX + 3]
    pt = np.asarray(point, dtype=np.float64)
    if pt.shape not in ((3,), (a.shape[0], 3)):
        raise ValueError("point must be [3] or [N, 3]")
    lever = np.einsum("nij,nj->ni", Rm, pt.reshape(-1, 3) - qm)
    T = np.zeros((Cm.shape[0], 6, 6))
    T[:, np.arange(6), np.arange(6)] = 1.0
    # -[lever]x
    T[:, 3, 1], T[:, 3, 2] = lever[:, 2], -lever[:, 1]
    T[:, 4, 0], T[:, 4, 2] = -lever[:, 2], lever[:, 0]
    T[:, 5, 0], T[:, 5, 1] = lever[:, 1], -lever[:, 0]
    return np.einsum("nij,njk,nlk->nil", T, Cm, T)


def consistent(ml, k=3.0):
    """[N] bool: chi2 lies within dof +- k sqrt(2 dof), the k-sigma band of a chi-squared variable - the frame's residuals are what
    the noise model predicts for a rigid body.  False where the frame has no weighted fit or dof < 1."""
    a = _ml_rows(ml)
    dof = a[:, ML_DOF]
    ok = (a[:, ML_FLAG] == 2.0) & (dof >= 1.0)
    with np.errstate(all="ignore"):
        return ok & (np.abs(a[:, ML_CHI2] - dof) <= float(k) * np.sqrt(2.0 * np.where(ok, dof, 1.0)))
