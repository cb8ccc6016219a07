"""NumPy / Python float64 restatement of `vbs_rigid_series` (include/vbs.h; csrc/k_rigid.hip), operand for operand: the side the GPU
tests hold `rigid`, `coef` and `residual` to BIT FOR BIT in everything but the six columns that pass through a root or an arc
tangent last (4 ulp).  Every sum over slots is `pose_oracle.lane_fold` (lane l adds slots l, l + 64, .. ascending, then the fold
32 .. 1); the matrix N, the cyclic Jacobi, the quaternion, the rotation, the scale and the translation are scalar IEEE double
operations in the stated order (a Python float is one; nothing here contracts); what is done per slot is done on NumPy arrays, whose
ufuncs do not contract either.

The independent side (`svd_fit`) solves the same problem by another algorithm: `np.linalg.svd` of the 3 x 3 with the determinant
fix and Umeyama's scale.  `tests/test_rigid_host.py` holds the restatement to it."""
import math

import numpy as np

import pose_oracle as PO

RIGID_COLS, GROUP, SWEEPS = 33, 4, 8
DEG = 57.29577951308232
ULP_COLS = (26, 27, 28, 29, 30, 31)                             # rms, rms0, angle, tilt, azimuth, twist
EXACT_COLS = tuple(c for c in range(RIGID_COLS) if c not in ULP_COLS)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _sum(v, pred):
    return float(PO.lane_fold(np.asarray(v, dtype=np.float64)[None], np.asarray(pred)[None])[0])


def horn_matrix(H):
    """N [4][4] from H [3][3] (H[i][j] = sum q_i p_j), the lower triangle mirrored."""
    (Hxx, Hxy, Hxz), (Hyx, Hyy, Hyz), (Hzx, Hzy, Hzz) = H
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0], N[1][1], N[2][2], N[3][3] = (Hxx + Hyy) + Hzz, (Hxx - Hyy) - Hzz, (Hyy - Hxx) - Hzz, (Hzz - Hxx) - Hyy
    N[0][1], N[0][2], N[0][3] = Hyz - Hzy, Hzx - Hxz, Hxy - Hyx
    N[1][2], N[1][3], N[2][3] = Hxy + Hyx, Hzx + Hxz, Hyz + Hzy
    for p, q in PAIRS:
        N[q][p] = N[p][q]
    return N


def jacobi(N, sweeps=SWEEPS):
    """`sweeps` sweeps of the cyclic Jacobi of `k_modes_ritz` from V = I -> (T, V) as lists of Python floats."""
    T = [[float(x) for x in row] for row in N]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
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
    return T, V


def quaternion(H, sweeps=SWEEPS):
    """-> ((w, x, y, z), lam - d2, T): the leading eigenvector of N as a unit quaternion with w >= 0."""
    T, V = jacobi(horn_matrix(H), sweeps)
    k = 0
    for i in range(1, 4):
        if T[i][i] > T[k][k]:
            k = i
    d2 = None
    for i in range(4):
        if i != k and (d2 is None or T[i][i] > d2):
            d2 = T[i][i]
    v = [V[i][k] for i in range(4)]
    nn = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]
    nr = math.sqrt(nn)
    w, x, y, z = v[0] / nr, v[1] / nr, v[2] / nr, v[3] / nr
    first = x if x != 0.0 else (y if y != 0.0 else z)
    if w < 0.0 or (w == 0.0 and first < 0.0):
        w, x, y, z = -w, -x, -y, -z
    return (w, x, y, z), T[k][k] - d2, T


def rotation(quat):
    w, x, y, z = quat
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def fit(Q, P, pred, with_scale=False, gap_rel=1e-6, sweeps=SWEEPS):
    """The fit of one set of one frame: Q, P [m, 3], pred [m] -> dict(count, qm, pm, exists, gap, quat, R, t, s, H, T)."""
    pred = np.asarray(pred, dtype=bool)
    c = int(pred.sum())
    out = dict(count=c, qm=[0.0] * 3, pm=[0.0] * 3, exists=False, gap=0.0)
    if c == 0:
        return out
    n = float(c)
    out["qm"] = qm = [_sum(Q[:, k], pred) / n for k in range(3)]
    out["pm"] = pm = [_sum(P[:, k], pred) / n for k in range(3)]
    if c < 3:
        return out
    with np.errstate(all="ignore"):
        q = [np.where(pred, Q[:, k] - qm[k], 0.0) for k in range(3)]
        p = [np.where(pred, P[:, k] - pm[k], 0.0) for k in range(3)]
    H = [[_sum(q[i] * p[j], pred) for j in range(3)] for i in range(3)]
    sqq = _sum((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2], pred)
    spp = _sum((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2], pred)
    quat, lead, T = quaternion(H, sweeps)
    den = sqq + spp
    if not den > 0.0:
        return out
    out["gap"] = gap = lead / den
    out.update(H=H, T=T, sqq=sqq, spp=spp)
    if not gap > gap_rel:
        return out
    R = rotation(quat)
    s = 1.0
    if with_scale and sqq > 0.0:
        D = None
        for j in range(3):
            for i in range(3):
                term = R[j][i] * H[i][j]
                D = term if D is None else D + term
        s = D / sqq
    t = [pm[i] - s * ((R[i][0] * qm[0] + R[i][1] * qm[1]) + R[i][2] * qm[2]) for i in range(3)]
    out.update(exists=True, quat=quat, R=R, t=t, s=s)
    return out


def residuals(Q, P, pred, f):
    """e [m, 3] and e . e [m] of the slots of `pred` against the fit f (0 elsewhere)."""
    R, t, s = f["R"], f["t"], f["s"]
    with np.errstate(all="ignore"):
        e = [np.where(pred, P[:, i] - (s * ((R[i][0] * Q[:, 0] + R[i][1] * Q[:, 1]) + R[i][2] * Q[:, 2]) + t[i]), 0.0) for i in range(3)]
    return np.stack(e, axis=1), (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def _ss0(Q, P, pred):
    with np.errstate(all="ignore"):
        d = [np.where(pred, P[:, k] - Q[:, k], 0.0) for k in range(3)]
    return _sum((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], pred)


def frame(Q, P, common, with_scale=False, reject_k=0.0, gap_rel=1e-6, sweeps=SWEEPS):
    """One frame: Q, P [m, 3], common [m] -> (rigid row [33], coef [4, 4], residual [m, 4], used [m])."""
    m = P.shape[0]
    common = np.asarray(common, dtype=bool)
    row, coef, res = np.zeros(RIGID_COLS), np.zeros((4, 4)), np.zeros((m, 4))
    f = fit(Q, P, common, with_scale, gap_rel, sweeps)
    used, flag = common, 0.0
    row[1] = row[2] = f["count"]
    row[3:6], row[6:9], row[32] = f["qm"], f["pm"], f["gap"]
    if not f["exists"]:
        return row, coef, res, used
    flag = 1.0
    e, ee = residuals(Q, P, used, f)
    ssr = _sum(ee, used)
    if reject_k > 0.0 and ssr > 0.0:
        thr = (reject_k * reject_k) * (ssr / float(f["count"]))
        keep = common & (ee <= thr)
        if int(keep.sum()) < f["count"]:
            f2 = fit(Q, P, keep, with_scale, gap_rel, sweeps)
            if f2["exists"]:
                f, used, flag = f2, keep, 2.0
                e, ee = residuals(Q, P, used, f)
                ssr = _sum(ee, used)
    ss0 = _ss0(Q, P, used)
    nu = float(used.sum())
    w, x, y, z = f["quat"]
    R = f["R"]
    row[0], row[2] = flag, nu
    row[3:6], row[6:9], row[9:13] = f["qm"], f["pm"], f["quat"]
    row[13:22], row[22:25], row[25] = [R[i][j] for i in range(3) for j in range(3)], f["t"], f["s"]
    row[26], row[27] = math.sqrt(ssr / nu), math.sqrt(ss0 / nu)
    row[28] = (2.0 * math.atan2(math.sqrt((x * x + y * y) + z * z), w)) * DEG
    row[29] = math.atan2(math.sqrt(R[0][2] * R[0][2] + R[1][2] * R[1][2]), R[2][2]) * DEG
    row[30] = math.atan2(R[1][2], R[0][2]) * DEG
    row[31] = (2.0 * math.atan2(z, w)) * DEG
    row[32] = f["gap"]
    for i in range(3):
        coef[i] = (flag, R[i][0], R[i][1], R[i][2])
    coef[3] = (flag, f["t"][0], f["t"][1], f["t"][2])
    res[:, 0] = used
    res[:, 1:] = np.where(used[:, None], e, 0.0)
    return row, coef, res, used


def common_points(table, source, mask=None, frame_range=None):
    """-> (Q [m, 3], P [F, m, 3], common [F, m]): the common rule of the entry."""
    t, src = np.asarray(table), np.asarray(source, dtype=np.float64)
    n, m = t.shape[:2]
    fa, fb = (0, n) if frame_range is None else frame_range
    sel = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    sel = sel & (src[:, 0] != 0)
    xyz = (np.nan_to_num(t[fa:fb, :, 0], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) & 2) != 0
    return src[:, 1:4], t[fa:fb, :, 6:9].astype(np.float64), xyz & sel[None]


def rigid_series(table, source, mask=None, with_scale=False, reject_k=0.0, gap_rel=1e-6, frame_range=None, sweeps=SWEEPS):
    """vbs_rigid_series: -> (rigid [F, 33], coef [F, 4, 4], residual [F, m, 4])."""
    Q, P, common = common_points(table, source, mask, frame_range)
    F, m = common.shape
    rigid, coef, res = np.zeros((F, RIGID_COLS)), np.zeros((F, 4, 4)), np.zeros((F, m, 4))
    for f in range(F):
        rigid[f], coef[f], res[f], _ = frame(Q, P[f], common[f], bool(with_scale), float(reject_k), float(gap_rel), sweeps)
    return rigid, coef, res


# ---- the independent side -----------------------------------------------------------------------------------------------------------
def svd_fit(Q, P, with_scale=False):
    """Kabsch / Umeyama on points Q, P [k, 3]: -> (R, t, s) with P ~ s R Q + t, by `np.linalg.svd` and the determinant fix."""
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    qm, pm = Q.mean(axis=0), P.mean(axis=0)
    q, p = Q - qm, P - pm
    U, S, Vt = np.linalg.svd(p.T @ q)                            # sum p q'
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    s = float((S * d).sum() / (q * q).sum()) if with_scale else 1.0
    return R, pm - s * (R @ qm), s


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def _bits_equal(g, w, what):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    assert g.shape == w.shape and g.dtype == np.float64, (what, g.shape, w.shape, g.dtype)
    diff = g.view(np.uint64) != w.view(np.uint64)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} entries differ in bits, first at {list(at)}: {g[at]!r} != {w[at]!r}")


def check(got, want, what=""):
    """(rigid, coef, residual) of the device (None = not asked for) against the restatement's: everything bit for bit, +0 and -0
    told apart, but the columns `ULP_COLS` of rigid (4 ulp).  No entry is skipped or masked, and no output may hold a NaN."""
    rigid, coef, res = got
    if rigid is not None:
        g = np.asarray(rigid)
        assert g.shape == want[0].shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "rigid", g.shape)
        _bits_equal(g[:, EXACT_COLS], want[0][:, EXACT_COLS], f"{what}: rigid (exact columns)")
        for col in ULP_COLS:
            u = PO.ulps(g[:, col], want[0][:, col])
            assert (u <= 4).all(), f"{what}: rigid column {col} off by {int(u.max())} ulp in frame {int(u.argmax())}"
    if coef is not None:
        assert not np.isnan(np.asarray(coef)).any(), (what, "coef")
        _bits_equal(np.asarray(coef), want[1], f"{what}: coef")
    if res is not None:
        assert not np.isnan(np.asarray(res)).any(), (what, "residual")
        _bits_equal(np.asarray(res), want[2], f"{what}: residual")
