"""NumPy / Python float64 restatement of `vbs_rigid_ml_series` (include/vbs.h; csrc/k_rigid_ml.hip), operand for operand: the side the
GPU tests hold `ml`, `pcov`, `coef` and `mahal` to BIT FOR BIT in everything but the four angle columns, which pass through an arc
tangent last (4 ulp).  Every sum over slots is `pose_oracle.lane_fold` (lane l adds slots l, l + 64, .. ascending, then the fold
32 .. 1); what is done per slot is done on NumPy arrays, whose ufuncs do not contract; the 6 x 6, the step and the columns are
scalar IEEE double operations in the stated order (a Python float is one).

The independent side (`scipy_fit`, `numeric_cov`) solves the same problem by another route: `scipy.optimize.least_squares` on the
whitened residuals with the rotation as a rotation vector (Rodrigues, sines and cosines), and central differences of that
residual.  `tests/test_rigid_ml_host.py` holds the restatement to them."""
import math

import numpy as np

import pose_oracle as PO
import rigid_oracle as RO

ML_COLS, PCOV_COLS, GROUP, MAX_ITERS = 40, 22, 4, 16
DEG = RO.DEG
ULP_COLS = (31, 32, 33, 34)                                     # angle, tilt, azimuth, twist
EXACT_COLS = tuple(c for c in range(ML_COLS) if c not in ULP_COLS)
(FLAG, N_START, N_USED, STEPS, QW, QX, QY, QZ) = range(8)
R0, T0, C0, QM0, CHI2, DOF, CHI2_START, STEP_ROT, STEP_C, ANGLE, TILT, AZIMUTH, TWIST, NXX, NXY, NYY, T2_TILT, VAR_TWIST = (
    8, 17, 20, 23, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39)


def _sums(vals, pred):
    """The lane fold of every array of `vals` over the slots of `pred` -> a list of Python floats."""
    v = np.stack([np.asarray(a, dtype=np.float64) for a in vals])
    return [float(x) for x in PO.lane_fold(v, np.broadcast_to(np.asarray(pred), v.shape))]


def upper_index(i, j):
    """Where entry (i, j), i <= j, of the 6 x 6 sits among the 21 of `pcov`."""
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


# ---- the LDL' of fit_math.h, on scalars (N = 6) and on arrays over slots (N = 3) --------------------------------------------------------
def ldl_factor(A, piv_rel):
    """-> (npass, L, d) for a list-of-lists A of Python floats."""
    n = len(A)
    L = [[0.0] * n for _ in range(n)]
    c = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        dj = A[j][j]
        for k in range(j):
            dj = dj - L[j][k] * c[j][k]
        if not dj > piv_rel * A[j][j]:
            return j, L, d
        d[j] = dj
        for i in range(j + 1, n):
            cij = A[i][j]
            for k in range(j):
                cij = cij - L[j][k] * c[i][k]
            c[i][j] = cij
            L[i][j] = cij / dj
    return n, L, d


def ldl_solve(L, d, b):
    """ldl_forward then ldl_back over the whole system (scalars or arrays)."""
    n = len(d)
    z, y = [None] * n, [None] * n
    for i in range(n):
        zi = b[i]
        for k in range(i):
            zi = zi - L[i][k] * z[k]
        z[i] = zi
        y[i] = zi / d[i]
    x = [None] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def ldl3_arrays(S, piv_rel):
    """The 3 x 3 of every slot at once: S[i][j] arrays -> (ok, L, d); entries of slots that fail hold whatever IEEE makes of them."""
    with np.errstate(all="ignore"):
        d0 = S[0][0]
        ok = d0 > piv_rel * S[0][0]
        c10, c20 = S[1][0], S[2][0]
        L10, L20 = c10 / d0, c20 / d0
        d1 = S[1][1] - L10 * c10
        ok = ok & (d1 > piv_rel * S[1][1])
        c21 = S[2][1] - L10 * c20
        L21 = c21 / d1
        d2 = (S[2][2] - L20 * c20) - L21 * c21
        ok = ok & (d2 > piv_rel * S[2][2])
    zero = np.zeros_like(d0)
    return ok, [[zero, zero, zero], [L10, zero, zero], [L20, L21, zero]], [d0, d1, d2]


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------
def sweep(Q, P, covP, covQ, flags, R, c, qm, piv_rel):
    """One sweep at the pose (R, c): Q, P [m, 3]; covP [m, 7]; covQ [m, 7] or None; flags [m] = begun and both covariance flags set.
    -> dict(used [m], dist [m], N [6], M [9], W [6], g [6], chi2, n_used)."""
    m = Q.shape[0]
    with np.errstate(all="ignore"):
        S = [[None] * 3 for _ in range(3)]
        idx = {(0, 0): 1, (0, 1): 2, (0, 2): 3, (1, 1): 4, (1, 2): 5, (2, 2): 6}
        for (i, j), col in idx.items():
            S[i][j] = S[j][i] = np.where(flags, covP[:, col], 0.0)
        if covQ is not None:
            G = [[None] * 3 for _ in range(3)]
            for (i, j), col in idx.items():
                G[i][j] = G[j][i] = np.where(flags, covQ[:, col], 0.0)
            T = [[(R[i][0] * G[0][j] + R[i][1] * G[1][j]) + R[i][2] * G[2][j] for j in range(3)] for i in range(3)]
            for i in range(3):
                for j in range(i, 3):
                    rs = (T[i][0] * R[j][0] + T[i][1] * R[j][1]) + T[i][2] * R[j][2]
                    S[i][j] = S[j][i] = S[i][j] + rs
        ok, L, d = ldl3_arrays(S, piv_rel)
        used = flags & ok
        dq = [np.where(used, Q[:, k] - qm[k], 0.0) for k in range(3)]
        y = [(R[i][0] * dq[0] + R[i][1] * dq[1]) + R[i][2] * dq[2] for i in range(3)]
        e = [np.where(used, P[:, i], 0.0) - (y[i] + c[i]) for i in range(3)]
        W = [[None] * 3 for _ in range(3)]
        one, zero = np.ones(m), np.zeros(m)
        for j in range(3):
            x = ldl_solve(L, d, [one if k == j else zero for k in range(3)])
            for i in range(j + 1):
                W[i][j] = W[j][i] = x[i]
        u = [(W[i][0] * e[0] + W[i][1] * e[1]) + W[i][2] * e[2] for i in range(3)]
        M = [[W[i][2] * y[1] - W[i][1] * y[2], W[i][0] * y[2] - W[i][2] * y[0], W[i][1] * y[0] - W[i][0] * y[1]] for i in range(3)]
        dist = (e[0] * u[0] + e[1] * u[1]) + e[2] * u[2]
        N = [M[2][0] * y[1] - M[1][0] * y[2], M[2][1] * y[1] - M[1][1] * y[2], M[2][2] * y[1] - M[1][2] * y[2],
             M[0][1] * y[2] - M[2][1] * y[0], M[0][2] * y[2] - M[2][2] * y[0], M[1][2] * y[0] - M[0][2] * y[1]]
        g = [u[2] * y[1] - u[1] * y[2], u[0] * y[2] - u[2] * y[0], u[1] * y[0] - u[0] * y[1], u[0], u[1], u[2]]
        Wu = [W[0][0], W[0][1], W[0][2], W[1][1], W[1][2], W[2][2]]
    vals = N + [M[i][j] for i in range(3) for j in range(3)] + Wu + g + [dist]
    sums = _sums(vals, used)                                     # the 28 sums, one fold each
    return dict(used=used, dist=np.where(used, dist, 0.0), N=sums[0:6], M=sums[6:15], W=sums[15:21], g=sums[21:27], chi2=sums[27],
                n_used=int(used.sum()))


def normal_matrix(s):
    """A [6][6] over (omega, c) from a sweep's sums."""
    A = [[0.0] * 6 for _ in range(6)]
    n = s["N"]
    A[0][0], A[0][1], A[0][2], A[1][1], A[1][2], A[2][2] = n
    for i in range(3):
        for j in range(3):
            A[j][3 + i] = s["M"][i * 3 + j]
    w = s["W"]
    A[3][3], A[3][4], A[3][5], A[4][4], A[4][5], A[5][5] = w
    for i in range(6):
        for j in range(i):
            A[i][j] = A[j][i]
    return A


def max_abs(a, b, c):
    s = abs(a)
    if abs(b) > s:
        s = abs(b)
    if abs(c) > s:
        s = abs(c)
    return s


def step_pose(quat, c, x):
    """q <- (1, omega / 2) / |.| (x) q, renormalised, the sign rule; c <- c + dc."""
    h0, h1, h2 = 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    hn = math.sqrt(((1.0 + h0 * h0) + h1 * h1) + h2 * h2)
    aw, ax, ay, az = 1.0 / hn, h0 / hn, h1 / hn, h2 / hn
    bw, bx, by, bz = quat
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    xq = ((aw * bx + ax * bw) + ay * bz) - az * by
    yq = ((aw * by - ax * bz) + ay * bw) + az * bx
    zq = ((aw * bz + ax * by) - ay * bx) + az * bw
    nr = math.sqrt(((w * w + xq * xq) + yq * yq) + zq * zq)
    w, xq, yq, zq = w / nr, xq / nr, yq / nr, zq / nr
    first = xq if xq != 0.0 else (yq if yq != 0.0 else zq)
    if w < 0.0 or (w == 0.0 and first < 0.0):
        w, xq, yq, zq = -w, -xq, -yq, -zq
    return (w, xq, yq, zq), [c[0] + x[3], c[1] + x[4], c[2] + x[5]]


def frame(Q, P, covP, covQ, start, begun, iters=8, piv_rel=1e-12, trace=None):
    """One frame: Q, P [m, 3]; covP [m, 7]; covQ [m, 7] or None; start [33] a row of `rigid`; begun [m] = residual[:, 0] != 0.
    -> (ml [40], pcov [22], coef [4, 4], mahal [m, 3]).  `trace`: a list that receives (step_rot, step_c) of every step."""
    m = P.shape[0]
    ml, pcov, coef, mahal = np.zeros(ML_COLS), np.zeros(PCOV_COLS), np.zeros((4, 4)), np.zeros((m, 3))
    if start[0] == 0.0:
        return ml, pcov, coef, mahal
    with np.errstate(all="ignore"):
        flags = begun & (covP[:, 0] != 0.0)
        if covQ is not None:
            flags = flags & (covQ[:, 0] != 0.0)
    q0 = tuple(float(v) for v in start[9:13])
    qm = [float(v) for v in start[3:6]]
    R = RO.rotation(q0)
    c0 = [((R[i][0] * qm[0] + R[i][1] * qm[1]) + R[i][2] * qm[2]) + float(start[22 + i]) for i in range(3)]
    quat, c = q0, list(c0)
    flag, it, step_rot, step_c = 2, 0, 0.0, 0.0
    C = [0.0] * 21
    dist0 = np.zeros(m)
    while True:
        s = sweep(Q, P, covP, covQ, flags, R, c, qm, piv_rel)
        if it == 0:
            chi2_start, dist0 = s["chi2"], s["dist"]
        npass, L, d = (0, None, None)
        if s["n_used"] >= 3:
            npass, L, d = ldl_factor(normal_matrix(s), piv_rel)
        if npass < 6:
            flag, step_rot, step_c = 1, 0.0, 0.0
            quat, c, R = q0, list(c0), RO.rotation(q0)
            s = sweep(Q, P, covP, covQ, flags, R, c, qm, piv_rel)
            chi2_start = s["chi2"]
            break
        if it == iters:
            for j in range(6):
                x = ldl_solve(L, d, [1.0 if k == j else 0.0 for k in range(6)])
                for i in range(j + 1):
                    C[upper_index(i, j)] = x[i]
            break
        x = ldl_solve(L, d, s["g"])
        quat, c = step_pose(quat, c, x)
        R = RO.rotation(quat)
        step_rot, step_c = max_abs(x[0], x[1], x[2]), max_abs(x[3], x[4], x[5])
        if trace is not None:
            trace.append((step_rot, step_c))
        it += 1
    used = s["used"]
    mahal[:, 0] = used
    mahal[:, 1] = s["dist"]
    mahal[:, 2] = s["dist"] if flag == 1 else np.where(used, dist0, 0.0)
    t = [c[i] - ((R[i][0] * qm[0] + R[i][1] * qm[1]) + R[i][2] * qm[2]) for i in range(3)]
    w, x, y, z = quat
    ml[0:4] = flag, int(begun.sum()), s["n_used"], it
    ml[4:8] = quat
    ml[8:17] = [R[i][j] for i in range(3) for j in range(3)]
    ml[17:20], ml[20:23], ml[23:26] = t, c, qm
    ml[26], ml[27], ml[28], ml[29], ml[30] = s["chi2"], float(3 * s["n_used"] - 6), chi2_start, step_rot, step_c
    ml[31] = (2.0 * math.atan2(math.sqrt((x * x + y * y) + z * z), w)) * DEG
    ml[32] = math.atan2(math.sqrt(R[0][2] * R[0][2] + R[1][2] * R[1][2]), R[2][2]) * DEG
    ml[33] = math.atan2(R[1][2], R[0][2]) * DEG
    ml[34] = (2.0 * math.atan2(z, w)) * DEG
    if flag == 2:
        n0, n1, n2 = R[0][2], R[1][2], R[2][2]
        s00, s01, s02, s11, s12, s22 = C[0], C[1], C[2], C[6], C[7], C[11]
        a0, a1, a2 = n2 * s01 - n1 * s02, n2 * s11 - n1 * s12, n2 * s12 - n1 * s22
        b0, b2 = n0 * s02 - n2 * s00, n0 * s22 - n2 * s02
        nxx, nxy, nyy = a1 * n2 - a2 * n1, a2 * n0 - a0 * n2, b2 * n0 - b0 * n2
        t2 = 0.0
        if nxx > 0.0:
            l = nxy / nxx
            d2, z2 = nyy - l * nxy, n1 - l * n0
            if d2 > piv_rel * nyy:
                t2 = (n0 * n0) / nxx + (z2 * z2) / d2
        v0, v1 = (s00 * n0 + s01 * n1) + s02 * n2, (s01 * n0 + s11 * n1) + s12 * n2
        v2 = (s02 * n0 + s12 * n1) + s22 * n2
        ml[35:40] = nxx, nxy, nyy, t2, (n0 * v0 + n1 * v1) + n2 * v2
        pcov[0] = 1.0
        pcov[1:] = C
    for i in range(3):
        coef[i] = (flag, R[i][0], R[i][1], R[i][2])
    coef[3] = (flag, t[0], t[1], t[2])
    return ml, pcov, coef, mahal


def rigid_ml_series(table, source, cov, rigid, residual, source_cov=None, iters=8, piv_rel=1e-12, frame_range=None, traces=None):
    """vbs_rigid_ml_series: -> (ml [F, 40], pcov [F, 22], coef [F, 4, 4], mahal [F, m, 3]); cov, rigid and residual cover the frames
    of `frame_range` alone."""
    t, src = np.asarray(table), np.asarray(source, dtype=np.float64)
    n, m = t.shape[:2]
    fa, fb = (0, n) if frame_range is None else frame_range
    F = fb - fa
    cov, rigid, residual = np.asarray(cov), np.asarray(rigid), np.asarray(residual)
    assert cov.shape == (F, m, 7) and rigid.shape == (F, 33) and residual.shape == (F, m, 4)
    covQ = None if source_cov is None else np.asarray(source_cov, dtype=np.float64)
    P = t[fa:fb, :, 6:9].astype(np.float64)
    ml, pcov, coef, mahal = np.zeros((F, ML_COLS)), np.zeros((F, PCOV_COLS)), np.zeros((F, 4, 4)), np.zeros((F, m, 3))
    for f in range(F):
        tr = None if traces is None else []
        with np.errstate(all="ignore"):
            begun = residual[f, :, 0] != 0.0
        ml[f], pcov[f], coef[f], mahal[f] = frame(src[:, 1:4], P[f], cov[f], covQ, rigid[f], begun, iters, piv_rel, tr)
        if traces is not None:
            traces.append(tr)
    return ml, pcov, coef, mahal


# ---- the independent side ---------------------------------------------------------------------------------------------------------------
def full_cov(c7):
    """[.., 7] -> [.., 3, 3]."""
    c7 = np.asarray(c7, dtype=np.float64)
    out = np.empty(c7.shape[:-1] + (3, 3))
    for (i, j), col in {(0, 0): 1, (0, 1): 2, (0, 2): 3, (1, 1): 4, (1, 2): 5, (2, 2): 6}.items():
        out[..., i, j] = out[..., j, i] = c7[..., col]
    return out


def rodrigues(r):
    th = float(np.linalg.norm(r))
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def whitened(params, Rbase, Q, P, SP, SQ, qm):
    """The whitened residuals of the pose R = exp([r]x) Rbase, c: chol(S_i)^-1 e_i stacked, by LAPACK."""
    R = rodrigues(params[:3]) @ Rbase
    e = P - ((Q - qm) @ R.T + params[3:6])
    S = SP if SQ is None else SP + R @ SQ @ R.T
    Lc = np.linalg.cholesky(S)
    return np.concatenate([np.linalg.solve(Lc[i], e[i]) for i in range(len(e))])


def scipy_fit(Q, P, SP, SQ, qm, R0, c0):
    """-> (R, c, cov [6, 6], chi2): `least_squares` (Levenberg-Marquardt, a central-difference Jacobian) from (R0, c0); the covariance is (J'J)^-1 with J by central differences of the
    whitened residual at the optimum, the weights held (as Gauss-Newton holds them)."""
    from scipy.optimize import least_squares
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    R, c = np.asarray(R0, dtype=np.float64), np.asarray(c0, dtype=np.float64)
    for _ in range(6):                                           # restarted about the last rotation until it stops moving
        fun = lambda p: whitened(p, R, Q, P, SP, SQ, qm)        # noqa: E731
        jac = lambda p: np.stack([(fun(p + d) - fun(p - d)) / 2e-6 for d in 1e-6 * np.eye(6)], axis=1)   # noqa: E731
        sol = least_squares(fun, np.concatenate([np.zeros(3), c]), jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        R, c = rodrigues(sol.x[:3]) @ R, sol.x[3:6]
        if np.abs(sol.x[:3]).max() < 1e-14:
            break
    return R, c, numeric_cov(Q, P, SP, SQ, qm, R, c), float((sol.fun ** 2).sum())


def numeric_cov(Q, P, SP, SQ, qm, R, c, h=1e-6):
    """(J'J)^-1 at (R, c) for a left perturbation exp([w]x) R, the weights held at S(R)."""
    S = SP if SQ is None else SP + R @ SQ @ R.T
    Lc = np.linalg.cholesky(S)

    def res(p):
        Rp = rodrigues(p[:3]) @ R
        e = P - ((Q - qm) @ Rp.T + c + p[3:6])
        return np.concatenate([np.linalg.solve(Lc[i], e[i]) for i in range(len(e))])

    J = np.empty((3 * len(P), 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        J[:, k] = (res(d) - res(-d)) / (2.0 * h)
    return np.linalg.inv(J.T @ J)


def pcov_matrix(row):
    """A row of `pcov` -> the symmetric [6, 6]."""
    Cm = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            Cm[i, j] = Cm[j, i] = row[1 + upper_index(i, j)]
    return Cm


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------
def check(got, want, what=""):
    """(ml, pcov, coef, mahal) of the device (None = not asked for) against the restatement's: everything bit for bit, +0 and -0 told
    apart, but the columns `ULP_COLS` of ml (4 ulp).  No entry is skipped or masked, and no output may hold a NaN."""
    ml, pcov, coef, mahal = got
    if ml is not None:
        g = np.asarray(ml)
        assert g.shape == want[0].shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "ml", g.shape)
        RO._bits_equal(g[:, EXACT_COLS], want[0][:, EXACT_COLS], f"{what}: ml (exact columns {EXACT_COLS})")
        for col in ULP_COLS:
            u = PO.ulps(g[:, col], want[0][:, col])
            assert (u <= 4).all(), f"{what}: ml column {col} off by {int(u.max())} ulp in frame {int(u.argmax())}"
    for name, g, w in (("pcov", pcov, want[1]), ("coef", coef, want[2]), ("mahal", mahal, want[3])):
        if g is not None:
            assert not np.isnan(np.asarray(g)).any(), (what, name)
            RO._bits_equal(np.asarray(g), w, f"{what}: {name}")
