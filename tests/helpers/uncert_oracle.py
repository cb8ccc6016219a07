"""NumPy float64 restatement of the uncertainty entries (`include/vbs.h`: vbs_uncert_points, vbs_uncert_cov, vbs_uncert_total,
vbs_pixel_noise; csrc/k_uncert.hip), the side the GPU tests hold every output to BIT FOR BIT: the forward mode in the kernel's
operation order, the covariance products, the LDL' and the per-frame fold.  Every array expression below is elementwise IEEE
float64 (NumPy fuses nothing), written operand for operand as the kernel writes it.

A second, independent form of the model is `model_complex`: the solve written once for complex128 and differentiated by the
complex step (h = 1e-30), which has no truncation error.  It is the smooth function; the solve's three float32 constants
(f_avg, dmm / f_avg, f_avg^2) make the forward mode differ from it by about 1e-7 relative unless they are exact in float32.

A camera is (K [3,3], dist [5], R [3,3], T [3], dmm) taken as float32, as `vbs_camera` holds it.
"""
import numpy as np

FLAG_TRACKED, FLAG_XYZ = 1, 2
NCAM, NSEED = 16, 19
COV_COLS, DCOV_COLS, TOTAL_COLS, NOISE_COLS, GROUP = 7, 8, 8, 10, 4
THETA = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "w0", "w1", "w2", "T0", "T1", "T2", "dmm")


class Cam:
    def __init__(self, K, dist, R, T, dmm=2.0):
        K = np.asarray(K, dtype=np.float32).reshape(3, 3)
        self.fx32, self.fy32, self.cx32, self.cy32 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        d = np.zeros(5, dtype=np.float32)
        dd = np.asarray(dist, dtype=np.float32).ravel()[:5]
        d[:dd.size] = dd
        self.k = d.astype(np.float64)
        self.has_dist = bool((d != 0).any())
        self.R = np.asarray(R, dtype=np.float32).reshape(3, 3).astype(np.float64)
        self.T = np.asarray(T, dtype=np.float32).reshape(3).astype(np.float64)
        self.dmm32 = np.float32(dmm)
        self.fx, self.fy, self.cx, self.cy = (np.float64(v) for v in (self.fx32, self.fy32, self.cx32, self.cy32))
        self.f_avg32 = np.float32((self.fx32 + self.fy32) / np.float32(2.0))
        self.k32 = np.float32(self.dmm32 / self.f_avg32)
        self.f2_32 = np.float32(self.f_avg32 * self.f_avg32)

    def theta(self):
        """The camera vector in float64 (w = 0)."""
        return np.array([self.fx, self.fy, self.cx, self.cy, *self.k, 0.0, 0.0, 0.0, *self.T, np.float64(self.dmm32)])


# ---- the model as executed, and its tangents ------------------------------------------------------------------------------------------
def primal(c, u0, v0, d):
    """undistort_point + solve_marker on arrays [N] -> (P, X [N,3], ok [N]); X is zeros where Rr < 1e-6."""
    u0, v0, d = (np.asarray(a, dtype=np.float64) for a in (u0, v0, d))
    with np.errstate(all="ignore"):
        x0, y0 = (u0 - c.cx) / c.fx, (v0 - c.cy) / c.fy
        x, y = x0, y0
        xi, yi = [], []
        for _ in range(5):
            xi.append(x); yi.append(y)
            if c.has_dist:
                r2 = x * x + y * y
                icd = 1.0 / (1.0 + ((c.k[4] * r2 + c.k[1]) * r2 + c.k[0]) * r2)
                dxx = 2.0 * c.k[2] * x * y + c.k[3] * (r2 + 2.0 * x * x)
                dyy = c.k[2] * (r2 + 2.0 * y * y) + 2.0 * c.k[3] * x * y
                x, y = (x0 - dxx) * icd, (y0 - dyy) * icd
        u, v = x * c.fx + c.cx, y * c.fy + c.cy
        P = dict(xi=xi, yi=yi, xe=x, ye=y)
        P["du"], P["dv"] = u - c.cx, v - c.cy
        P["Rr"] = np.sqrt(P["du"] * P["du"] + P["dv"] * P["dv"])
        P["fa"], P["kk"] = np.float64(c.f_avg32), np.float64(c.k32)
        P["S"] = np.sqrt(P["Rr"] * P["Rr"] + np.float64(c.f2_32))
        d_eff = P["kk"] * P["S"]
        P["q"] = d_eff / d
        P["h"] = P["fa"] * P["q"]
        P["a0"], P["a1"] = P["h"] * P["du"] / c.fx, P["h"] * P["dv"] / c.fy
        P["pc"] = [P["a0"] - c.T[0], P["a1"] - c.T[1], P["h"] - c.T[2]]
        X = np.stack([c.R[0, i] * P["pc"][0] + c.R[1, i] * P["pc"][1] + c.R[2, i] * P["pc"][2] for i in range(3)], axis=-1)
        near = P["Rr"] < 1e-6
        X = np.where(near[..., None], 0.0, X)
        ok = ~near & np.isfinite(X).all(axis=-1)
    return P, X, ok


def push(c, P, d, s):
    """The directional derivative of X along the seed s [19] (`unc_push`) -> [N, 3]; meaningful where the row is ok."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        x0, y0 = P["xi"][0], P["yi"][0]
        tx0, ty0 = ((s[16] - s[2]) - x0 * s[0]) / c.fx, ((s[17] - s[3]) - y0 * s[1]) / c.fy
        tx, ty = tx0, ty0
        if c.has_dist:
            k = c.k
            for it in range(5):
                x, y = P["xi"][it], P["yi"][it]
                r2, tr2 = x * x + y * y, 2.0 * (x * tx + y * ty)
                a = k[4] * r2 + k[1]
                b = a * r2 + k[0]
                icd = 1.0 / (1.0 + b * r2)
                ta = (s[8] * r2 + k[4] * tr2) + s[5]
                tb = (ta * r2 + a * tr2) + s[4]
                tc = tb * r2 + b * tr2
                ticd = -((tc * icd) * icd)
                xy, txy = x * y, tx * y + x * ty
                ax, ay = r2 + 2.0 * x * x, r2 + 2.0 * y * y
                tax, tay = tr2 + 4.0 * (x * tx), tr2 + 4.0 * (y * ty)
                dxx = 2.0 * k[2] * x * y + k[3] * ax
                dyy = k[2] * ay + 2.0 * k[3] * x * y
                tdxx = 2.0 * (s[6] * xy + k[2] * txy) + (s[7] * ax + k[3] * tax)
                tdyy = (s[6] * ay + k[2] * tay) + 2.0 * (s[7] * xy + k[3] * txy)
                tx, ty = (tx0 - tdxx) * icd + (x0 - dxx) * ticd, (ty0 - tdyy) * icd + (y0 - dyy) * ticd
        tdu, tdv = tx * c.fx + P["xe"] * s[0], ty * c.fy + P["ye"] * s[1]
        tRr = (P["du"] * tdu + P["dv"] * tdv) / P["Rr"]
        tfa = 0.5 * (s[0] + s[1])
        tkk = (s[15] - P["kk"] * tfa) / P["fa"]
        tS = (P["Rr"] * tRr + P["fa"] * tfa) / P["S"]
        tde = tkk * P["S"] + P["kk"] * tS
        tq = (tde - P["q"] * s[18]) / d
        th = tfa * P["q"] + P["fa"] * tq
        ta0 = ((th * P["du"] + P["h"] * tdu) - P["a0"] * s[0]) / c.fx
        ta1 = ((th * P["dv"] + P["h"] * tdv) - P["a1"] * s[1]) / c.fy
        pc = P["pc"]
        p0 = (ta0 - s[12]) + (pc[1] * s[11] - pc[2] * s[10])
        p1 = (ta1 - s[13]) + (pc[2] * s[9] - pc[0] * s[11])
        p2 = (th - s[14]) + (pc[0] * s[10] - pc[1] * s[9])
        return np.stack([c.R[0, i] * p0 + c.R[1, i] * p1 + c.R[2, i] * p2 for i in range(3)], axis=-1)


def unit(k):
    s = np.zeros(NSEED)
    s[k] = 1.0
    return s


def jacobians(c, uvd):
    """vbs_uncert_points: -> xyz [N,3], J_obs [N,3,3], J_cam [N,3,16], ok int32 [N]."""
    uvd = np.asarray(uvd, dtype=np.float64).reshape(-1, 3)
    P, X, ok = primal(c, uvd[:, 0], uvd[:, 1], uvd[:, 2])
    J = np.stack([np.where(ok[:, None], push(c, P, uvd[:, 2], unit(k)), 0.0) for k in range(NSEED)], axis=-1)
    return X, J[:, :, NCAM:], J[:, :, :NCAM], ok.astype(np.int32)


def obs_product(A, S6):
    """xx, xy, xz, yy, yz, zz of A S A' (`unc_obs_cov`): A [N,3,3], S6 [N or 1, 6] -> [N, 6]."""
    S6 = np.asarray(S6, dtype=np.float64).reshape(-1, 6)
    S = [[S6[:, 0], S6[:, 1], S6[:, 2]], [S6[:, 1], S6[:, 3], S6[:, 4]], [S6[:, 2], S6[:, 4], S6[:, 5]]]
    M = [[A[:, i, 0] * S[0][k] + A[:, i, 1] * S[1][k] + A[:, i, 2] * S[2][k] for k in range(3)] for i in range(3)]
    return np.stack([M[i][0] * A[:, j, 0] + M[i][1] * A[:, j, 1] + M[i][2] * A[:, j, 2] for i in range(3) for j in range(i, 3)], axis=-1)


def _rows(c, rows, min_size, obs, L):
    """What a kernel forms for table rows [N,10] (obs [N or 1, 6], L [16,q]): usable [N], the observation part [N,6], G [N,q,3]."""
    rows = np.asarray(rows)
    flags = rows[:, 0].astype(np.int64)
    d = rows[:, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        gate = ((flags & FLAG_XYZ) != 0) & (d >= min_size)
    # a row that must not be read is not read: its cells may hold NaN or 1e30
    u0 = np.where(gate, rows[:, 1].astype(np.float64), 0.0)
    v0 = np.where(gate, rows[:, 2].astype(np.float64), 0.0)
    dd = np.where(gate, d, 1.0)
    P, _, ok = primal(c, u0, v0, dd)
    ok &= gate
    A = np.stack([push(c, P, dd, unit(NCAM + k)) for k in range(3)], axis=-1)
    part = np.where(ok[:, None], obs_product(A, obs), 0.0)
    q = L.shape[1]
    G = np.zeros((rows.shape[0], q, 3))
    for col in range(q):
        s = np.zeros(NSEED)
        s[:NCAM] = L[:, col]
        G[:, col] = np.where(ok[:, None], push(c, P, dd, s), 0.0)
    return ok, part, G


def _factor(L):
    return np.zeros((NCAM, 0)) if L is None else np.asarray(L, dtype=np.float64).reshape(NCAM, -1)


def _obs(obs, m):
    o = np.asarray(obs, dtype=np.float64).reshape(-1, 6)
    return np.broadcast_to(o, (m, 6)) if o.shape[0] == 1 else o


def _outer_add(acc, g):
    """acc [N,6] + g g' entry by entry, in the kernel's order."""
    e = 0
    for i in range(3):
        for j in range(i, 3):
            acc[:, e] = acc[:, e] + g[:, i] * g[:, j]
            e += 1


def solve3d_cov(table, c, obs, L=None, ref_frame=None, min_size=5.0, piv_rel=1e-12, frame_range=None):
    """vbs_uncert_cov: -> (cov [F,m,7], dcov [F,m,8] or None)."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    a, b = (0, n) if frame_range is None else frame_range
    L, obs = _factor(L), _obs(obs, m)
    q = L.shape[1]
    F = b - a
    ok, part, G = _rows(c, t[a:b].reshape(F * m, -1), min_size, np.tile(obs, (F, 1)), L)
    sx = part.copy()
    for col in range(q):
        _outer_add(sx, G[:, col])
    cov = np.concatenate([ok[:, None].astype(np.float64), sx], axis=1).reshape(F, m, COV_COLS)
    if ref_frame is None:
        return cov, None
    ok0, part0, G0 = _rows(c, t[ref_frame], min_size, obs, L)
    ok0, part0, G0 = np.tile(ok0, F), np.tile(part0, (F, 1)), np.tile(G0, (F, 1, 1))
    both = ok & ok0
    sd = part + part0
    for col in range(q):
        _outer_add(sd, G[:, col] - G0[:, col])
    sd = np.where(both[:, None], sd, 0.0)
    rows = t[a:b].reshape(F * m, -1)
    ref = np.tile(t[ref_frame], (F, 1))
    with np.errstate(all="ignore"):
        D = [np.where(both, rows[:, 6 + k].astype(np.float64), 0.0) - np.where(both, ref[:, 6 + k].astype(np.float64), 0.0)
             for k in range(3)]
        thr = piv_rel * ((sd[:, 0] + sd[:, 3]) + sd[:, 5])
        d1 = sd[:, 0]
        v1 = both & (d1 > thr)
        l21, l31 = sd[:, 1] / d1, sd[:, 2] / d1
        d2 = sd[:, 3] - l21 * sd[:, 1]
        v2 = v1 & (d2 > thr)
        w = sd[:, 4] - l21 * sd[:, 2]
        l32 = w / d2
        d3 = (sd[:, 5] - l31 * sd[:, 2]) - l32 * w
        v3 = v2 & (d3 > thr)
        z1 = D[0]
        z2 = D[1] - l21 * z1
        z3 = (D[2] - l31 * z1) - l32 * z2
        t2 = (z1 * z1 / d1 + z2 * z2 / d2) + z3 * z3 / d3
    t2 = np.where(v3, t2, 0.0)
    flag = np.where(both, np.where(v3, 3.0, 1.0), 0.0)
    dcov = np.concatenate([flag[:, None], sd, t2[:, None]], axis=1).reshape(F, m, DCOV_COLS)
    return cov, dcov


def fold_down(lane):
    """The fold of wave_fold.h over 64 lane values [..., 64] -> [...]."""
    v = np.array(lane, dtype=np.float64)
    off = 32
    while off >= 1:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def lane_sums(x, use):
    """Lane l adds the used entries of x [m] at l, l + 64, .. ascending from 0.0; then the fold."""
    lanes = np.zeros(64)
    for i in range(x.shape[0]):
        if use[i]:
            lanes[i % 64] = lanes[i % 64] + x[i]
    return fold_down(lanes)


def solve3d_total(table, c, obs, L=None, ref_frame=0, slots=None, min_size=5.0, frame_range=None):
    """vbs_uncert_total: -> total [F, 8]; `slots` a boolean mask [m] or None."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    a, b = (0, n) if frame_range is None else frame_range
    L, obs = _factor(L), _obs(obs, m)
    q = L.shape[1]
    ok0, part0, G0 = _rows(c, t[ref_frame], min_size, obs, L)
    want = ok0 if slots is None else ok0 & np.asarray(slots, dtype=bool)
    out = np.zeros((b - a, TOTAL_COLS))
    for f in range(a, b):
        ok, part, G = _rows(c, t[f], min_size, obs, L)
        use = ok & want
        cnt = int(use.sum())
        o = out[f - a]
        o[0] = cnt
        o[1] = 1.0 if want.sum() >= 1 and cnt == want.sum() else 0.0
        so = [lane_sums(part[:, e] + part0[:, e], use) for e in (0, 3, 5)]
        cam = [0.0, 0.0, 0.0]
        for col in range(q):
            for k in range(3):
                bk = lane_sums(G[:, col, k] - G0[:, col, k], use)
                cam[k] = cam[k] + bk * bk
        for k in range(3):
            o[2 + k] = so[k] + cam[k]
            o[5 + k] = cam[k]
    return out


def pixel_noise(table, frame_range=None):
    """vbs_pixel_noise: -> [m, 10]."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    a, b = (0, n) if frame_range is None else frame_range
    out = np.zeros((m, NOISE_COLS))
    tr = (t[a:b, :, 0].astype(np.int64) & FLAG_TRACKED) != 0
    x = t[a:b, :, 1:4].astype(np.float64)
    for i in range(m):
        v = x[tr[:, i], i]
        cnt = v.shape[0]
        s = np.zeros(3)
        for r in v:
            s = s + r
        mu = s / cnt if cnt else np.zeros(3)
        cc = np.zeros(6)
        for r in v:
            e = r - mu
            cc = cc + np.array([e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2], e[2] * e[2]])
        out[i, 0] = cnt
        out[i, 1:4] = mu
        out[i, 4:] = cc / (cnt - 1.0) if cnt > 1 else 0.0
    return out


# ---- the independent form: the smooth model for complex128, differentiated by the complex step --------------------------------------
def model_complex(theta, o, R, has_dist):
    """X [3] of the observation o = (Cx, Cy, major) under the camera vector theta [16]; any of them may be complex."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = theta[:9]
    w, T, dmm = theta[9:12], theta[12:15], theta[15]
    x0, y0 = (o[0] - cx) / fx, (o[1] - cy) / fy
    x, y = x0, y0
    if has_dist:
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dxx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dyy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dxx) * icd, (y0 - dyy) * icd
    du, dv = x * fx, y * fy
    f_avg = (fx + fy) / 2.0
    Rr2 = du * du + dv * dv
    h = f_avg * ((dmm / f_avg) * np.sqrt(Rr2 + f_avg * f_avg) / o[2])
    pc = np.array([h * du / fx - T[0], h * dv / fy - T[1], h - T[2]])
    # R_wc' = exp([w]x) R_wc to first order: X = R_wc^T (I - [w]x) pc = R^T (pc - w x pc)
    pc = pc - np.array([w[1] * pc[2] - w[2] * pc[1], w[2] * pc[0] - w[0] * pc[2], w[0] * pc[1] - w[1] * pc[0]])
    return np.asarray(R, dtype=np.float64).T @ pc


def jacobian_complex_step_theta(theta, o, R, has_dist, h=1e-30):
    """J_cam [3,16] of the smooth model at a float64 camera vector theta and observation o [3]."""
    th, o = np.asarray(theta).astype(np.complex128), np.asarray(o, dtype=np.complex128)
    Jc = np.zeros((3, NCAM))
    for k in range(NCAM):
        tk = th.copy()
        tk[k] += 1j * h
        Jc[:, k] = model_complex(tk, o, R, has_dist).imag / h
    return Jc


def jacobian_complex_step(c, o, h=1e-30):
    """(J_obs [3,3], J_cam [3,16]) of the smooth model at camera c and observation o [3]."""
    th, o = c.theta().astype(np.complex128), np.asarray(o, dtype=np.complex128)
    Jo = np.zeros((3, 3))
    for k in range(3):
        ok = o.copy()
        ok[k] += 1j * h
        Jo[:, k] = model_complex(th, ok, c.R, c.has_dist).imag / h
    return Jo, jacobian_complex_step_theta(th, o, c.R, c.has_dist, h)
