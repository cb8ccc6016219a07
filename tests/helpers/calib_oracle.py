"""Oracle of the device camera calibration (csrc/k_calib.hip, csrc/calib_math.h): NumPy float64, no torch.

`solve` repeats the device's steps - homography per view (Hartley-normalised normal equations with h33 = 1, 5 Gauss-Newton steps),
cv2's closed form for the focal lengths over the active views, a pose per view, Levenberg-Marquardt in the Schur form with the
device's damping schedule, stopping rule and left-multiplied pose update - operation for operation in IEEE float64: the sums run
per lane and then through the wave's xor-butterfly, the Cholesky loops are the device's, and no step calls the maths library
beyond sqrt (the pose step takes its Rodrigues coefficients from their series), so that the path of the fit, its accept / reject
decisions and its iteration count can be compared for equality.  `optimum` is the INDEPENDENT fit:
scipy.optimize.least_squares(method="lm") over all 9 + 6 V parameters with Rodrigues-vector poses, every tolerance at machine
epsilon, started from the helper's initial values.  Also the case generator of tests/test_calib_host.py and tests/test_gpu_calib.py."""
import functools

import numpy as np

FEW_VIEWS, DEGENERATE = 1, 2
H_GN_STEPS, POLAR_STEPS, LM_EPS, LAMBDA0, LAMBDA_FAIL = 5, 8, 1e-11, 1e-3, 1e10
SIZE = (640, 480)
K_TRUE = (820.0, 815.0, 325.0, 236.0)
DIST_A = (-0.12, 0.06, 0.0011, -0.0008, 0.01)
DIST_B = (-0.25, 0.1, 0.001, -0.002, 0.0)


# ---- calib_math.h and k_calib.hip, operation for operation ----------------------------------------------------------------------
# A wave's lanes take the points lane + 64 k: arrays of shape [4, 64] (`_lanes`), summed per lane over k, then over the lanes by
# the xor-butterfly (`_butterfly`), which leaves every lane with the same bits.
PER = 4
_LANE = np.arange(64)


def _lanes(a, n):
    out = np.zeros(PER * 64)
    out[:n] = a
    return out.reshape(PER, 64)


def _butterfly(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v[..., 0]


def _lane_sum(terms, valid):
    """terms [..., 4, 64] -> [...]: acc = acc + term for the valid points of a lane in k order, then the butterfly."""
    acc = np.zeros(terms.shape[:-2] + (64,))
    for k in range(PER):
        acc = np.where(valid[k], acc + terms[..., k, :], acc)
    return _butterfly(acc)


def tri(n, p, q):
    return p * n - (p * (p - 1)) // 2 + (q - p)


def _eliminate8(A):
    """pnp_eliminate8 on the augmented 8 x 9 system: (h, ok)."""
    A = A.copy()
    amax = np.abs(A[:, :8]).max()
    pmin = np.inf
    for k in range(8):
        piv = k + int(np.argmax(np.abs(A[k:, k])))       # the first maximum, as the device's strict >
        best = abs(A[piv, k])
        A[[k, piv]] = A[[piv, k]]
        pmin = min(pmin, best)
        pv = A[k, k] if best > 0.0 else 1.0
        for r in range(k + 1, 8):
            A[r, k + 1:] = A[r, k + 1:] - (A[r, k] / pv) * A[k, k + 1:]
    if not pmin > 1e-9 * amax:
        return np.zeros(8), False
    h = np.zeros(8)
    for i in range(7, -1, -1):
        v = A[i, 8]
        for j in range(i + 1, 8):
            v = v - A[i, j] * h[j]
        h[i] = v / A[i, i]
    return h, True


def _h_solve(ju, jv, bu, bv, valid):
    """calib_h_accumulate over the points, the sums over the wave, calib_h_solve."""
    terms = [ju[i] * ju[j] + jv[i] * jv[j] for i in range(8) for j in range(i, 8)] + [ju[i] * bu + jv[i] * bv for i in range(8)]
    acc = _lane_sum(np.array(terms), valid)
    A = np.zeros((8, 9))
    q = 0
    for i in range(8):
        for j in range(i, 8):
            A[i, j] = A[j, i] = acc[q]
            q += 1
        A[i, 8] = acc[36 + i]
    return _eliminate8(A)


def homography(obj, img):
    """k_calib_homography for one view: (H [9] with H[8] = 1, ok).  obj [N,2], img [N,2]."""
    with np.errstate(all="ignore"):
        n = len(obj)
        dn = float(n)
        valid = _lanes(np.ones(n), n) > 0
        X, Y, x, y = _lanes(obj[:, 0], n), _lanes(obj[:, 1], n), _lanes(img[:, 0], n), _lanes(img[:, 1], n)
        mxo, myo, mxi, myi = (_lane_sum(q, valid) / dn for q in (X, Y, x, y))
        a, b, c, d = X - mxo, Y - myo, x - mxi, y - myi
        so = np.sqrt(2.0) / (_lane_sum(np.sqrt(a * a + b * b), valid) / dn)
        si = np.sqrt(2.0) / (_lane_sum(np.sqrt(c * c + d * d), valid) / dn)
        X, Y, x, y = so * (X - mxo), so * (Y - myo), si * (x - mxi), si * (y - myi)
        one, zero = np.ones_like(X), np.zeros_like(X)
        h, oks = _h_solve([X, Y, one, zero, zero, zero, -(x * X), -(x * Y)], [zero, zero, zero, X, Y, one, -(y * X), -(y * Y)], x, y, valid)
        sxx, sxy, syy = _lane_sum(x * x, valid), _lane_sum(x * y, valid), _lane_sum(y * y, valid)
        ok = bool(np.isfinite(so) and np.isfinite(si) and sxx * syy - sxy * sxy > 1e-9 * (sxx * syy)) and oks
        for _ in range(H_GN_STEPS):
            iw = 1.0 / ((h[6] * X + h[7] * Y) + 1.0)
            u, v = ((h[0] * X + h[1] * Y) + h[2]) * iw, ((h[3] * X + h[4] * Y) + h[5]) * iw
            dh, okd = _h_solve([X * iw, Y * iw, iw, zero, zero, zero, -(u * X) * iw, -(u * Y) * iw],
                               [zero, zero, zero, X * iw, Y * iw, iw, -(v * X) * iw, -(v * Y) * iw], x - u, y - v, valid)
            ok = okd and ok
            h = h + dh
        G = np.zeros(9)
        for r, (ga, gb, gc) in enumerate(((h[0], h[1], h[2]), (h[3], h[4], h[5]), (h[6], h[7], 1.0))):
            G[3 * r], G[3 * r + 1], G[3 * r + 2] = ga * so, gb * so, gc - (ga * (so * mxo) + gb * (so * myo))
        isi = 1.0 / si
        F = np.zeros(9)
        for j in range(3):
            F[j] = G[j] * isi + mxi * G[6 + j]
            F[3 + j] = G[3 + j] * isi + myi * G[6 + j]
            F[6 + j] = G[6 + j]
        H = F / F[8]
        return H, bool(ok and F[8] > 0.0 and np.isfinite(H).all())


def init_focal(Hs, size):
    """calib_init_rows over the homographies [k,9] in order, calib_init_focal: (fx, fy, cx, cy, ok)."""
    cx, cy = (float(size[0]) - 1.0) * 0.5, (float(size[1]) - 1.0) * 0.5
    m = [0.0] * 5
    with np.errstate(all="ignore"):
        for H in Hs:
            h = [H[0] - cx * H[6], H[3] - cy * H[6], H[6]]
            v = [H[1] - cx * H[7], H[4] - cy * H[7], H[7]]
            d1, d2 = [0.0] * 3, [0.0] * 3
            nh = nv = n1 = n2 = 0.0
            for j in range(3):
                d1[j], d2[j] = (h[j] + v[j]) * 0.5, (h[j] - v[j]) * 0.5
                nh, nv, n1, n2 = nh + h[j] * h[j], nv + v[j] * v[j], n1 + d1[j] * d1[j], n2 + d2[j] * d2[j]
            nh, nv, n1, n2 = 1.0 / np.sqrt(nh), 1.0 / np.sqrt(nv), 1.0 / np.sqrt(n1), 1.0 / np.sqrt(n2)
            h, v, d1, d2 = [q * nh for q in h], [q * nv for q in v], [q * n1 for q in d1], [q * n2 for q in d2]
            a0, b0, c0 = h[0] * v[0], h[1] * v[1], -(h[2] * v[2])
            a1, b1, c1 = d1[0] * d2[0], d1[1] * d2[1], -(d1[2] * d2[2])
            m = [m[0] + (a0 * a0 + a1 * a1), m[1] + (a0 * b0 + a1 * b1), m[2] + (b0 * b0 + b1 * b1),
                 m[3] + (a0 * c0 + a1 * c1), m[4] + (b0 * c0 + b1 * c1)]
        det = m[0] * m[2] - m[1] * m[1]
        if not det > 1e-9 * (m[0] * m[2]):
            return 0.0, 0.0, cx, cy, False
        a, b = (m[3] * m[2] - m[1] * m[4]) / det, (m[0] * m[4] - m[1] * m[3]) / det
        if not (a > 0.0 and b > 0.0 and np.isfinite(a) and np.isfinite(b)):
            return 0.0, 0.0, cx, cy, False
        fx, fy = np.sqrt(abs(1.0 / a)), np.sqrt(abs(1.0 / b))
        return fx, fy, cx, cy, bool(np.isfinite(fx) and np.isfinite(fy))


def polar(M):
    """pnp_polar on M [9]: (M, ok)."""
    M = list(M)
    for _ in range(POLAR_STEPS):
        C = [M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6],
             M[2] * M[7] - M[1] * M[8], M[0] * M[8] - M[2] * M[6], M[1] * M[6] - M[0] * M[7],
             M[1] * M[5] - M[2] * M[4], M[2] * M[3] - M[0] * M[5], M[0] * M[4] - M[1] * M[3]]
        det = (M[0] * C[0] + M[1] * C[1]) + M[2] * C[2]
        if not det > 1e-12:
            return np.array(M), False
        M = [0.5 * (M[i] + C[i] / det) for i in range(9)]
    return np.array(M), True


def init_pose(H, fx, fy, cx, cy):
    """calib_init_pose: (R [3,3], t [3], ok)."""
    with np.errstate(all="ignore"):
        M = [0.0] * 9
        for j in range(3):
            M[j], M[3 + j], M[6 + j] = (H[j] - cx * H[6 + j]) / fx, (H[3 + j] - cy * H[6 + j]) / fy, H[6 + j]
        n1 = np.sqrt((M[0] * M[0] + M[3] * M[3]) + M[6] * M[6])
        n2 = np.sqrt((M[1] * M[1] + M[4] * M[4]) + M[7] * M[7])
        sc = 0.5 * (n1 + n2)
        if not sc > 0.0:
            return np.eye(3), np.zeros(3), False
        sc = 1.0 / sc
        t = np.array([M[2] * sc, M[5] * sc, M[8] * sc])
        for i in (0, 3, 6, 1, 4, 7):
            M[i] = M[i] * sc
        M[2] = M[3] * M[7] - M[6] * M[4]
        M[5] = M[6] * M[1] - M[0] * M[7]
        M[8] = M[0] * M[4] - M[3] * M[1]
        R, ok = polar(M)
        return R.reshape(3, 3), t, bool(ok and t[2] > 0.0 and np.isfinite(R).all() and np.isfinite(t).all())


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx + 0.5 * Kx @ Kx
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1 - np.cos(th)) / th ** 2) * Kx @ Kx


def rotation_vector(R):
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    return w * (th / (2.0 * s)) if s > 1e-12 else 0.5 * w


def _to_camera(R, t, X, Y):
    """pnp_to_camera with Z = 0; R = 9 values, t = 3."""
    return [((R[3 * i] * X + R[3 * i + 1] * Y) + R[3 * i + 2] * 0.0) + t[i] for i in range(3)]


def _project(cam, R, t, X, Y):
    """pnp_project on arrays of points: (u, v, z)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    Pc = _to_camera(R, t, X, Y)
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * rad + 2.0 * p1 * xy) + p2 * (r2 + 2.0 * x2)
    yd = (y * rad + p1 * (r2 + 2.0 * y2)) + 2.0 * p2 * xy
    return fx * xd + cx, fy * yd + cy, Pc[2]


def project(cam, R, t, obj):
    """(u, v, z) of the board points obj [N,2] for R [3,3], t [3]."""
    return _project(cam, np.asarray(R).reshape(9), t, obj[:, 0], obj[:, 1])


def _point_terms(cam, R, t, X, Y, uo, vo):
    """pnp_pixel_jacobian and calib_intrinsic_columns on arrays of points: ru, rv, Iu [9], Iv [9], Pu [6], Pv [6], front."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    Pc = _to_camera(R, t, X, Y)
    iz = 1.0 / Pc[2]
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    drad = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1
    xd = (x * rad + 2.0 * p1 * xy) + p2 * (r2 + 2.0 * x2)
    yd = (y * rad + p1 * (r2 + 2.0 * y2)) + 2.0 * p2 * xy
    ru, rv = (fx * xd + cx) - uo, (fy * yd + cy) - vo
    dxx = fx * (((rad + 2.0 * x2 * drad) + 2.0 * p1 * y) + 6.0 * p2 * x)
    dxy = fx * ((2.0 * xy * drad + 2.0 * p1 * x) + 2.0 * p2 * y)
    dyx = fy * ((2.0 * xy * drad + 2.0 * p1 * x) + 2.0 * p2 * y)
    dyy = fy * (((rad + 2.0 * y2 * drad) + 6.0 * p1 * y) + 2.0 * p2 * x)
    ax, ay, az = dxx * iz, dxy * iz, -(dxx * x + dxy * y) * iz
    bx, by, bz = dyx * iz, dyy * iz, -(dyx * x + dyy * y) * iz
    Pu = [ay * -Pc[2] + az * Pc[1], ax * Pc[2] + az * -Pc[0], ax * -Pc[1] + ay * Pc[0], ax, ay, az]
    Pv = [by * -Pc[2] + bz * Pc[1], bx * Pc[2] + bz * -Pc[0], bx * -Pc[1] + by * Pc[0], bx, by, bz]
    r4 = r2 * r2
    r6 = r4 * r2
    one, zero = np.ones_like(x), np.zeros_like(x)
    Iu = [xd, zero, one, zero, fx * (x * r2), fx * (x * r4), fx * (2.0 * xy), fx * (r2 + 2.0 * x2), fx * (x * r6)]
    Iv = [zero, yd, zero, one, fy * (y * r2), fy * (y * r4), fy * (r2 + 2.0 * y2), fy * (2.0 * xy), fy * (y * r6)]
    return ru, rv, Iu, Iv, Pu, Pv, Pc[2] > 0.0


def jacobian(cam, R, t, obj, img):
    """One view, for the dense fit: residuals r [2N] (u rows then v rows), J_intrinsic [2N,9], J_pose [2N,6] (left-multiplied
    step: rotation, then translation), ok (every point in front)."""
    ru, rv, Iu, Iv, Pu, Pv, front = _point_terms(cam, np.asarray(R).reshape(9), t, obj[:, 0], obj[:, 1], img[:, 0], img[:, 1])
    return (np.concatenate([ru, rv]), np.vstack([np.column_stack(Iu), np.column_stack(Iv)]),
            np.vstack([np.column_stack(Pu), np.column_stack(Pv)]), bool(front.all()))


def view_costs(cam, Rs, ts, obj, imgs):
    """Squared pixel error of every view (plain NumPy sums: for checks of returned parameters, not the device's order)."""
    out = np.zeros(len(Rs))
    with np.errstate(all="ignore"):
        for a, (R, t, img) in enumerate(zip(Rs, ts, imgs)):
            u, v, z = project(cam, R, t, obj)
            out[a] = ((u - img[:, 0]) ** 2 + (v - img[:, 1]) ** 2).sum() if (z > 0.0).all() else np.inf
    return out


class _Problem:
    """The state k_calib_refine keeps in LDS and registers, and its passes."""

    def __init__(self, obj, imgs):
        self.n, self.k = len(obj), len(imgs)
        self.valid = _lanes(np.ones(self.n), self.n) > 0
        self.X, self.Y = _lanes(obj[:, 0], self.n), _lanes(obj[:, 1], self.n)
        self.uo = [_lanes(im[:, 0], self.n) for im in imgs]
        self.vo = [_lanes(im[:, 1], self.n) for im in imgs]

    def cost_pass(self, cam, R, t):
        """calib_pass<false>: vcost [k]."""
        vcost = np.zeros(self.k)
        for a in range(self.k):
            u, v, z = _project(cam, R[a], t[a], self.X, self.Y)
            du, dv = u - self.uo[a], v - self.vo[a]
            vcost[a] = _lane_sum(np.where(z > 0.0, du * du + dv * dv, np.inf), self.valid)
        return vcost

    def jacobian_pass(self, cam, R, t):
        """calib_pass<true>: (A [54], blk [k,81], vcost [k])."""
        blk, vcost, part = np.zeros((self.k, 81)), np.zeros(self.k), np.zeros((4, 54))
        for a in range(self.k):
            ru, rv, Iu, Iv, Pu, Pv, front = _point_terms(cam, R[a], t[a], self.X, self.Y, self.uo[a], self.vo[a])
            live = self.valid & front
            tv = ([Iu[i] * Pu[j] + Iv[i] * Pv[j] for i in range(9) for j in range(6)] +
                  [Pu[i] * Pu[j] + Pv[i] * Pv[j] for i in range(6) for j in range(i, 6)] + [Pu[i] * ru + Pv[i] * rv for i in range(6)])
            blk[a] = _lane_sum(np.array(tv), live)
            cost = np.zeros(64)
            for k in range(PER):
                cost = np.where(self.valid[k], np.where(front[k], cost + (ru[k] * ru[k] + rv[k] * rv[k]), np.inf), cost)
            vcost[a] = _butterfly(cost)
            ta = [Iu[i] * Iu[j] + Iv[i] * Iv[j] for i in range(9) for j in range(i, 9)] + [Iu[i] * ru + Iv[i] * rv for i in range(9)]
            part[a % 4] = part[a % 4] + _lane_sum(np.array(ta), live)
        return ((part[0] + part[1]) + part[2]) + part[3], blk, vcost


def _sym6(Ci):
    """[..., 21] -> [6][6] of arrays."""
    return [[Ci[..., tri(6, min(p, q), max(p, q))] for q in range(6)] for p in range(6)]


def inverse6(C, lam):
    """calib_inverse6 for every view at once: C [k,21] -> (Ci [k,21], ok [k])."""
    M = [[None] * 6 for _ in range(6)]
    L = [[None] * 6 for _ in range(6)]
    Li = [[None] * 6 for _ in range(6)]
    q = 0
    for i in range(6):
        for j in range(i, 6):
            M[i][j] = M[j][i] = C[:, q]
            q += 1
    for i in range(6):
        M[i][i] = M[i][i] + lam * M[i][i]
    ok = np.ones(len(C), dtype=bool)
    for j in range(6):
        s = M[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        bad = ~(s > 0.0)
        ok &= ~bad
        ljj = np.sqrt(np.where(bad, 1.0, s))
        L[j][j] = ljj
        for i in range(j + 1, 6):
            v = M[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / ljj
    for j in range(6):
        Li[j][j] = 1.0 / L[j][j]
        for i in range(j + 1, 6):
            v = np.zeros(len(C))
            for k in range(j, i):
                v = v - L[i][k] * Li[k][j]
            Li[i][j] = v / L[i][i]
    Ci = np.zeros((len(C), 21))
    q = 0
    for i in range(6):
        for j in range(i, 6):
            v = np.zeros(len(C))
            for k in range(j, 6):
                v = v + Li[k][i] * Li[k][j]
            Ci[:, q] = v
            q += 1
    return Ci, ok


_SCHUR_I = np.array([i for i in range(9) for j in range(i, 9)] + list(range(9)))
_SCHUR_J = np.array([j for i in range(9) for j in range(i, 9)] + [-1] * 9)


def schur(A, lam, blk, ci):
    """calib_schur_entry for the 54 entries at once: S = upper triangle (45) then the right-hand side (9)."""
    s = A.copy()
    diag = (_SCHUR_I == _SCHUR_J)
    s = np.where(diag, s + lam * s, s)
    for a in range(len(blk)):
        B, g = blk[a, :54].reshape(9, 6), blk[a, 75:81]
        b = B[_SCHUR_I]                                                        # [54,6]
        c = np.where((_SCHUR_J >= 0)[:, None], B[np.maximum(_SCHUR_J, 0)], g[None, :])
        Cf = _sym6(ci[a])
        quad = np.zeros(54)
        for p in range(6):
            w = np.zeros(54)
            for q in range(6):
                w = w + Cf[p][q] * c[:, q]
            quad = quad + b[:, p] * w
        s = s - quad
    return s


def solve9(S):
    """calib_solve9: (dA [9], diag S^-1 [9], ok)."""
    N = 9
    L = np.zeros((N, N))
    Li = np.zeros((N, N))
    ok = True
    for j in range(N):
        s = S[tri(N, j, j)]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if not s > 0.0:
            ok, s = False, 1.0
        ljj = np.sqrt(s)
        L[j, j] = ljj
        for i in range(j + 1, N):
            v = S[tri(N, j, i)]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / ljj
    y, dA, inv_diag = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        v = -S[45 + i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(N - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, N):
            v = v - L[k, i] * dA[k]
        dA[i] = v / L[i, i]
    for j in range(N):
        Li[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, N):
            v = 0.0
            for k in range(j, i):
                v = v - L[i, k] * Li[k, j]
            Li[i, j] = v / L[i, i]
    for i in range(N):
        v = 0.0
        for k in range(i, N):
            v = v + Li[k, i] * Li[k, i]
        inv_diag[i] = v
    return dA, inv_diag, bool(ok and np.isfinite(dA).all())


def factor(A, blk, lam):
    """calib_factor: (dA, ci, diag S^-1) or None when a factorisation fails."""
    with np.errstate(all="ignore"):
        ci, ok = inverse6(blk[:, 54:75], lam)
        if not ok.all():
            return None
        dA, inv_diag, ok9 = solve9(schur(A, lam, blk, ci))
    return (dA, ci, inv_diag) if ok9 else None


def back_substitute(blk, ci, dA):
    """calib_back_substitute for every view: d [k,6]."""
    r = []
    for p in range(6):
        v = blk[:, 75 + p]
        for i in range(9):
            v = v + blk[:, 6 * i + p] * dA[i]
        r.append(v)
    Cf = _sym6(ci)
    d = np.zeros((len(blk), 6))
    for p in range(6):
        w = np.zeros(len(blk))
        for q in range(6):
            w = w + Cf[p][q] * r[q]
        d[:, p] = -w
    return d


def apply_step(d, R, t):
    """calib_apply_step for every view: d [k,6], R [k,9], t [k,3] -> (R, t).  The Rodrigues coefficients by their series."""
    wx, wy, wz = d[:, 0], d[:, 1], d[:, 2]
    th2 = wx * wx + wy * wy + wz * wz
    sa, sb = np.ones_like(th2), np.ones_like(th2)
    for k in range(12, 0, -1):
        sa = 1.0 - th2 / float((2 * k) * (2 * k + 1)) * sa
        sb = 1.0 - th2 / float((2 * k + 1) * (2 * k + 2)) * sb
    with np.errstate(all="ignore"):
        th = np.sqrt(th2)
        a = np.where(th2 <= 1.0, sa, np.sin(th) / th)
        b = np.where(th2 <= 1.0, 0.5 * sb, (1.0 - np.cos(th)) / th2)
    E = [1.0 + b * (wx * wx - th2), b * (wx * wy) - a * wz, b * (wx * wz) + a * wy,
         b * (wx * wy) + a * wz, 1.0 + b * (wy * wy - th2), b * (wy * wz) - a * wx,
         b * (wx * wz) - a * wy, b * (wy * wz) + a * wx, 1.0 + b * (wz * wz - th2)]
    Rn, tn = np.zeros_like(R), np.zeros_like(t)
    for i in range(3):
        for j in range(3):
            Rn[:, 3 * i + j] = (E[3 * i] * R[:, j] + E[3 * i + 1] * R[:, 3 + j]) + E[3 * i + 2] * R[:, 6 + j]
        tn[:, i] = ((E[3 * i] * t[:, 0] + E[3 * i + 1] * t[:, 1]) + E[3 * i + 2] * t[:, 2]) + d[:, 3 + i]
    return Rn, tn


def _seq_sum(v):
    s = 0.0
    for x in v:
        s = s + x
    return s


def initial(obj, imgs, size, Hs=None):
    """The device's starting point over the given views: dict(status, cam [9], R list, t list, H [k,9])."""
    if Hs is None:
        hv = [homography(obj, img) for img in imgs]
        if not all(ok for _, ok in hv):
            return dict(status=DEGENERATE)
        Hs = np.array([H for H, _ in hv])
    fx, fy, cx, cy, ok = init_focal(Hs, size)
    if not ok:
        return dict(status=DEGENERATE)
    poses = [init_pose(H, fx, fy, cx, cy) for H in Hs]
    if not all(p[2] for p in poses):
        return dict(status=DEGENERATE)
    return dict(status=0, cam=np.array([fx, fy, cx, cy, 0, 0, 0, 0, 0.0]), R=[p[0] for p in poses], t=[p[1] for p in poses], H=Hs)


def solve(obj, imgs, size, active=None, max_iter=30):
    """k_calib_refine for one problem over the views `active` (indices, default all) of imgs [V,N,2]: dict(status, cam [9],
    R, t (lists over the active views), cost, view_cost, rms, view_rms, std_intrinsics, iterations, init)."""
    obj = np.asarray(obj, dtype=np.float64)[:, :2]
    active = list(range(len(imgs))) if active is None else list(active)
    hv = [homography(obj, np.asarray(imgs[v], dtype=np.float64)) for v in active]
    if len(active) < 3:
        return dict(status=FEW_VIEWS)
    if not all(ok for _, ok in hv):
        return dict(status=DEGENERATE)
    im = [np.asarray(imgs[v], dtype=np.float64) for v in active]
    init = initial(obj, im, size, np.array([H for H, _ in hv]))
    if init["status"]:
        return dict(status=DEGENERATE)
    n, k = len(obj), len(active)
    P = _Problem(obj, im)
    cam = init["cam"].copy()
    R, t = np.array([r.reshape(9) for r in init["R"]]), np.array(init["t"])
    lam, iters, fresh = LAMBDA0, 0, True
    A = blk = vc = cost = None
    with np.errstate(all="ignore"):
        for it in range(max_iter + 1):
            if fresh:
                A, blk, vc = P.jacobian_pass(cam, R, t)
                cost = _seq_sum(vc)
                fresh = False
                if not np.isfinite(cost):
                    return dict(status=DEGENERATE)
            if it == max_iter:
                break
            f = factor(A, blk, lam)
            if f is None:
                iters += 1
                lam = lam * 10.0
                if lam > LAMBDA_FAIL:
                    return dict(status=DEGENERATE)
                continue
            dA, ci, _ = f
            d = back_substitute(blk, ci, dA)
            dm = max(np.abs(dA).max(), np.where(np.isfinite(d), np.abs(d), np.inf).max())
            if not dm >= LM_EPS:
                break
            iters += 1
            cam_t = cam + dA
            Rt, tt = apply_step(d, R, t)
            cost_t = _seq_sum(P.cost_pass(cam_t, Rt, tt))
            if cost_t <= cost:
                lam = max(lam * 0.1, 1e-15)
                cam, R, t, fresh = cam_t, Rt, tt, True
            else:
                lam = min(lam * 10.0, 1e15)
        f = factor(A, blk, 0.0)
        points = float(k) * float(n)
        dof = 2.0 * points - float(9 + 6 * k)
        std = np.sqrt((cost / dof) * f[2]) if f is not None and dof > 0.0 else np.full(9, np.nan)
        return dict(status=0, cam=cam, R=[r.reshape(3, 3) for r in R], t=[x for x in t], cost=cost, view_cost=vc,
                    rms=np.sqrt(cost / points), view_rms=np.sqrt(vc / float(n)), std_intrinsics=std, iterations=iters, init=init,
                    active=active)


# ---- the independent optimum -----------------------------------------------------------------------------------------------------
def _left_jacobian(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + 0.5 * Kx
    return np.eye(3) + ((1 - np.cos(th)) / th ** 2) * Kx + ((th - np.sin(th)) / th ** 3) * Kx @ Kx


def optimum(obj, imgs, init):
    """scipy least_squares(method="lm") over cam [9] and (rotation vector, t) per view, from `init` (of `initial` / `solve`): dict(
    cam, R, t, cost, view_cost, success, cond = condition number of the column-scaled Jacobian, std_intrinsics from
    sigma^2 diag (J^T J)^-1 at the optimum)."""
    from scipy.optimize import least_squares
    obj = np.asarray(obj, dtype=np.float64)[:, :2]
    k, n = len(imgs), len(obj)
    x0 = np.concatenate([init["cam"]] + [np.concatenate([rotation_vector(R), t]) for R, t in zip(init["R"], init["t"])])

    def both(x):
        r, J = np.zeros(2 * n * k), np.zeros((2 * n * k, 9 + 6 * k))
        for a in range(k):
            w, t = x[9 + 6 * a:12 + 6 * a], x[12 + 6 * a:15 + 6 * a]
            R = rodrigues(w)
            # a step dw of the rotation vector is the left step J_l(w) dw; the translation t' = E t + dt moves with it, so the
            # Rodrigues-vector parametrisation (t independent of w) takes dt = -[J_l dw]x t out again
            ra, Ji, Jp, _ = jacobian(x[:9], R, t, obj, imgs[a])
            Jl = _left_jacobian(w)
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
            rows = slice(2 * n * a, 2 * n * (a + 1))
            r[rows], J[rows, :9] = ra, Ji
            J[rows, 9 + 6 * a:12 + 6 * a] = (Jp[:, :3] + Jp[:, 3:] @ tx) @ Jl
            J[rows, 12 + 6 * a:15 + 6 * a] = Jp[:, 3:]
        return r, J

    eps = np.finfo(np.float64).eps
    res = least_squares(lambda x: both(x)[0], x0, jac=lambda x: both(x)[1], method="lm", x_scale="jac", xtol=eps, ftol=eps, gtol=eps,
                        max_nfev=2000)
    r, J = both(res.x)
    sv = np.linalg.svd(J / np.linalg.norm(J, axis=0), compute_uv=False)
    cov = np.linalg.inv(J.T @ J)
    cost = float(r @ r)
    dof = 2 * n * k - (9 + 6 * k)
    e2 = (r.reshape(k, 2, n) ** 2).sum(axis=1)
    return dict(cam=res.x[:9].copy(), R=[rodrigues(res.x[9 + 6 * a:12 + 6 * a]) for a in range(k)],
                t=[res.x[12 + 6 * a:15 + 6 * a].copy() for a in range(k)], cost=cost, view_cost=e2.sum(axis=1),
                success=bool(res.success and res.status > 0), cond=float(sv[0] / sv[-1]),
                std_intrinsics=np.sqrt((cost / dof) * np.diag(cov)[:9]) if dof > 0 else np.full(9, np.nan))


def reprojection_gap(cam_a, R_a, t_a, cam_b, R_b, t_b, obj):
    """Largest distance (px) between the two parameter sets' projections of the board over all views."""
    obj = np.asarray(obj, dtype=np.float64)[:, :2]
    worst = 0.0
    for Ra, ta, Rb, tb in zip(R_a, t_a, R_b, t_b):
        ua, va, _ = project(cam_a, Ra, ta, obj)
        ub, vb, _ = project(cam_b, Rb, tb, obj)
        worst = max(worst, float(np.hypot(ua - ub, va - vb).max()))
    return worst


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) * 0.5
    s = 0.5 * np.linalg.norm(Ra.T @ Rb - (Ra.T @ Rb).T) / np.sqrt(2.0)
    return float(np.degrees(np.arctan2(s, c)))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def board(pattern, square=3.0):
    """`intrinsic_calibration.object_points`: float32 [pw*ph,3]."""
    objp = np.zeros((pattern[0] * pattern[1], 3), np.float32)
    objp[:, :2] = np.mgrid[:pattern[0], :pattern[1]].T.reshape(-1, 2) * square
    return objp


def make_case(name, views, pattern, dist, noise, seed, square=3.0):
    """Views of one board under random poses (tilts up to +-35 degrees about x and y, any rotation about z up to +-30), redrawn
    until every corner lies inside the image with a margin of 5 px; Gaussian pixel noise; corners through float32."""
    rng = np.random.default_rng(seed)
    objp = board(pattern, square)
    obj = objp[:, :2].astype(np.float64)
    cam = np.array(K_TRUE + tuple(dist))
    centre = obj.mean(axis=0)
    extent = np.ptp(obj, axis=0).max() + square
    Rs, ts, imgs = [], [], []
    while len(Rs) < views:
        ax, ay, az = np.radians(rng.uniform(-35, 35)), np.radians(rng.uniform(-35, 35)), np.radians(rng.uniform(-30, 30))
        R = rodrigues([0, 0, az]) @ rodrigues([0, ay, 0]) @ rodrigues([ax, 0, 0])
        z = K_TRUE[0] * extent / rng.uniform(200.0, 380.0)
        t = np.array([rng.uniform(-0.25, 0.25) * z * 0.6, rng.uniform(-0.2, 0.2) * z * 0.5, z]) - R[:, :2] @ centre
        u, v, zc = project(cam, R, t, obj)
        if (zc > 0).all() and u.min() > 5 and v.min() > 5 and u.max() < SIZE[0] - 6 and v.max() < SIZE[1] - 6:
            Rs.append(R)
            ts.append(t)
            uv = np.column_stack([u, v]) + (rng.normal(0.0, noise, (len(u), 2)) if noise else 0.0)
            imgs.append(uv.astype(np.float32).astype(np.float64))
    return dict(name=name, objp=objp, obj=obj, imgs=np.array(imgs), size=SIZE, cam=cam, R=Rs, t=ts, noise=noise, pattern=pattern)


CASES = (("three_exact", 3, (6, 6), (0, 0, 0, 0, 0), 0.0, 11),      # (seed 1: the helper ends 1.08e-9 BELOW scipy, past the host test's 1e-9)
         ("three_distorted", 3, (6, 6), DIST_A, 0.05, 2),
         ("five_views", 5, (6, 6), DIST_A, 0.1, 3),
         ("eight_7x4", 8, (7, 4), DIST_B, 0.3, 4),
         ("four_13x5", 4, (13, 5), DIST_A, 0.1, 5),
         ("three_16x16", 3, (16, 16), DIST_A, 0.1, 6),
         ("sixtyfour_4x3", 64, (4, 3), DIST_A, 0.1, 7))


@functools.lru_cache(maxsize=1)
def cases():
    """Every regular case with the helper's solution (`sol`) and the independent optimum (`opt`), computed once per process."""
    out = []
    for name, views, pattern, dist, noise, seed in CASES:
        c = make_case(name, views, pattern, dist, noise, seed, square=3.0 if pattern != (16, 16) else 1.5)
        c["sol"] = solve(c["obj"], c["imgs"], c["size"])
        c["opt"] = optimum(c["obj"], c["imgs"], c["sol"]["init"]) if c["sol"]["status"] == 0 else None
        out.append(c)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def collinear_view(c):
    """Corners of a view that all lie on one line: the board's points mapped to the line through the view's first two corners."""
    img = c["imgs"][0]
    p, q = img[0], img[-1]
    s = np.linspace(0.0, 1.0, len(img))[:, None]
    return (p + s * (q - p)).astype(np.float32).astype(np.float64)


def fronto_parallel_views(c, k=3):
    """k views of the board seen fronto-parallel (rotations about the optical axis only): 1 / f^2 is not determined."""
    out = []
    for j in range(k):
        R = rodrigues([0, 0, np.radians(20.0 * j)])
        t = np.array([-4.0 + j, -5.0, 60.0 + 5 * j])
        u, v, _ = project(c["cam"], R, t, c["obj"])
        out.append(np.column_stack([u, v]).astype(np.float32).astype(np.float64))
    return np.array(out)


# ---- end to end: rendered boards for calibrate_camera(dir, ..., calibrate="device") ------------------------------------------------
E2E_K = (300.0, 300.0, 101.0, 78.0)
# Largest gap of fx, fy, cx, cy to the rendered K when the HELPER calibrates the corners that the helper chain (finder + (11,11)
# refinement) finds in the four rendered boards below: measured on the CPU by tests/test_calib_host.py::test_rendered_boards_record;
# the finder's 0.1-0.15 px corner error (chess_cases.HELPER_ERR_PX) sets it, not this solver.  The device is held to 2 x that.
E2E_HELPER_K_GAP_PX = 1.2508


@functools.lru_cache(maxsize=1)
def rendered_boards():
    """Four 6 x 6 boards (7 x 7 squares of 3 mm) under tilted poses through K = E2E_K, no distortion, in 203 x 157 crops."""
    import chess_cases as CC                              # (needs chess_oracle: imported only here)
    fx, fy, cx, cy = E2E_K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    out = []
    for tilt in ((18.0, -12.0, 5.0), (-20.0, 15.0, -8.0), (12.0, 22.0, 12.0), (-15.0, -18.0, 0.0)):
        R = rodrigues([0, 0, np.radians(tilt[2])]) @ rodrigues([0, np.radians(tilt[1]), 0]) @ rodrigues([np.radians(tilt[0]), 0, 0])
        t = np.array([0.0, 0.0, 50.0]) - R[:, :2] @ np.array([10.5, 10.5])
        Hm = Km @ np.column_stack([R[:, 0] * 3.0, R[:, 1] * 3.0, t])       # board coordinates in squares
        gray, corners = CC.render((203, 157), (7, 7), Hm / Hm[2, 2])
        out.append((gray, corners))
    return tuple(out)


def padded(gray):
    """An image whose `crop_image` (1/8 left and right, 1/16 top) is `gray`."""
    h, w = gray.shape
    W, Hh = w * 4 // 3 + 8, h * 16 // 15 + 8
    for ww in range(w, 2 * w):
        if ww - 2 * int(ww / 8) == w:
            W = ww
            break
    for hh in range(h, 2 * h):
        if hh - int(hh / 16) == h:
            Hh = hh
            break
    out = np.full((Hh, W), 190, dtype=np.uint8)
    out[int(Hh / 16):, int(W / 8):int(W / 8) + w] = gray
    return out
