"""NumPy / Python float64 restatement of `vbs_sphere_series` (include/vbs.h; csrc/k_sphere.hip), operand for operand: the side the GPU
tests hold `sphere`, `radial` and `decomp` to BIT FOR BIT in everything but the five columns that pass through a root or an arc
tangent last (4 ulp, the project's rule).  Every sum over slots is `pose_oracle.lane_fold` (lane l adds slots l, l + 64, ..
ascending, then the fold 32 .. 1); the LDL', the cyclic Jacobi and the plane are scalar IEEE double operations in the stated order (a
Python float is one; nothing here contracts); what is done per slot is done on NumPy arrays, whose ufuncs do not contract either.

The INTERIOR roots - R = sqrt(R2), sqrt(r2) in rho and in the depths, the Jacobi's, the normalisations - feed exact columns.  IEEE
requires sqrt to be correctly rounded, `math.sqrt` / `np.sqrt` are, and the device's float64 sqrt is as well (k_rigid's interior
roots have been bit-equal since that entry exists), so these columns are held in bits and `check` carries no widened bound; should
a device ever round a root otherwise, the bound for the columns downstream of it has to be DERIVED from 4 ulp of that root (rho and
the depths: 4 ulp of sqrt(r2), i.e. 4 * 2^-52 * R absolute), never guessed.

`margins()` gives, for one frame, the relative distance of every DECISION (membership, pivot, R2 > 0, gap, rejection, orientation)
from its threshold: the case makers assert that it is far above what 4 ulp of a root can move (2^-50), so the restatement alone
decides every case.

The independent side is `geometric_fit` (`scipy.optimize.least_squares` on |P - C| - R) and `svd_plane` (`np.linalg.svd`);
`tests/test_sphere_host.py` holds the restatement to them."""
import math

import numpy as np

import pose_oracle as PO

SPHERE_COLS, GROUP, SWEEPS = 31, 4, 6
DEG = 57.29577951308232
ULP_COLS = (8, 23, 24, 25, 29)                                  # rms_fit, spot_radius, tilt_deg, azimuth_deg, plane_rms
EXACT_COLS = tuple(c for c in range(SPHERE_COLS) if c not in ULP_COLS)
PAIRS = ((0, 1), (0, 2), (1, 2))
(FLAG, N_FIT, N_FIT_USED, REJECTED, CX, CY, CZ, RADIUS, RMS_FIT, N_USED, N_CONTACT, CMX, CMY, CMZ, DEPTH_SUM, DEPTH_MEAN, DEPTH_MAX,
 DEEPEST, NX, NY, NZ, DIST, OFFSET, SPOT_RADIUS, TILT_DEG, AZIMUTH_DEG, SX, SY, SZ, PLANE_RMS, GAP) = range(SPHERE_COLS)
MIN_MARGIN = 1e-9                                               # every decision of every case is at least this far (relatively) from flipping


def _sum(v, pred):
    return float(PO.lane_fold(np.asarray(v, dtype=np.float64)[None], np.asarray(pred)[None])[0])


def _rel(a, b):
    """The relative distance of a comparison a <> b from equality."""
    s = max(abs(a), abs(b))
    return abs(a - b) / s if s > 0.0 else 0.0


def dist2(P, C):
    with np.errstate(all="ignore"):
        dx, dy, dz = P[:, 0] - C[0], P[:, 1] - C[1], P[:, 2] - C[2]
        return (dx * dx + dy * dy) + dz * dz


def solve(N, g, piv_rel, margin=None):
    """LDL' in basis order, all four pivots must pass -> beta [4] or None."""
    Lm = [[0.0] * 4 for _ in range(4)]
    c = [[0.0] * 4 for _ in range(4)]
    d = []
    for j in range(4):
        dj = N[j][j]
        for k in range(j):
            dj = dj - Lm[j][k] * c[j][k]
        if margin is not None:
            margin.append(("pivot", _rel(dj, piv_rel * N[j][j])))
        if not dj > piv_rel * N[j][j]:
            return None
        d.append(dj)
        for i in range(j + 1, 4):
            cij = N[i][j]
            for k in range(j):
                cij = cij - Lm[j][k] * c[i][k]
            c[i][j], Lm[i][j] = cij, cij / dj
    z, y = [], []
    for i in range(4):
        zi = g[i]
        for k in range(i):
            zi = zi - Lm[i][k] * z[k]
        z.append(zi)
        y.append(zi / d[i])
    beta = [0.0] * 4
    for i in range(3, -1, -1):
        b = y[i]
        for k in range(i + 1, 4):
            b = b - Lm[k][i] * beta[k]
        beta[i] = b
    return beta


def fit(P, pred, piv_rel=1e-9, margin=None):
    """The fit of one set of one frame: P [m, 3], pred [m] -> dict(count, exists, C, R, rho, ssr)."""
    pred = np.asarray(pred, dtype=bool)
    c = int(pred.sum())
    out = dict(count=c, exists=False)
    if c < 4:
        return out
    n = float(c)
    pm = [_sum(P[:, k], pred) / n for k in range(3)]
    with np.errstate(all="ignore"):
        u = [np.where(pred, P[:, k] - pm[k], 0.0) for k in range(3)]
        s = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    Sx, Sy, Sz = (_sum(u[k], pred) for k in range(3))
    Sxx, Sxy, Sxz = _sum(u[0] * u[0], pred), _sum(u[0] * u[1], pred), _sum(u[0] * u[2], pred)
    Syy, Syz, Szz = _sum(u[1] * u[1], pred), _sum(u[1] * u[2], pred), _sum(u[2] * u[2], pred)
    Ss = _sum(s, pred)
    Sxs, Sys, Szs = (_sum(u[k] * s, pred) for k in range(3))
    N = [[Sxx, Sxy, Sxz, Sx], [Sxy, Syy, Syz, Sy], [Sxz, Syz, Szz, Sz], [Sx, Sy, Sz, n]]
    beta = solve(N, [Sxs, Sys, Szs, Ss], piv_rel, margin)
    if beta is None:
        return out
    cx, cy, cz = beta[0] / 2.0, beta[1] / 2.0, beta[2] / 2.0
    cc = (cx * cx + cy * cy) + cz * cz
    R2 = beta[3] + cc
    if margin is not None:
        margin.append(("R2", abs(R2) / max(abs(beta[3]), cc, 1e-300)))
    if not R2 > 0.0:
        return out
    C, R = [pm[0] + cx, pm[1] + cy, pm[2] + cz], math.sqrt(R2)
    with np.errstate(all="ignore"):
        rho = np.where(pred, np.sqrt(dist2(P, C)) - R, 0.0)
    out.update(exists=True, C=C, R=R, rho=rho, ssr=_sum(rho * rho, pred), N=N)
    return out


def jacobi3(A, sweeps=SWEEPS):
    """`sweeps` sweeps of the cyclic Jacobi of `k_modes_ritz` on a symmetric 3 x 3 from V = I -> (T, V) as lists of Python floats."""
    T = [[float(x) for x in row] for row in A]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = T[p][q]
            if apq == 0.0:
                continue
            theta = (T[q][q] - T[p][p]) / (2.0 * apq)
            tt = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            cs = 1.0 / math.sqrt(tt * tt + 1.0)
            sn = tt * cs
            for k in range(3):
                x, y = T[k][p], T[k][q]
                T[k][p], T[k][q] = cs * x - sn * y, sn * x + cs * y
            for k in range(3):
                x, y = T[p][k], T[q][k]
                T[p][k], T[q][k] = cs * x - sn * y, sn * x + cs * y
            for k in range(3):
                x, y = V[k][p], V[k][q]
                V[k][p], V[k][q] = cs * x - sn * y, sn * x + cs * y
            T[p][q] = T[q][p] = 0.0
    return T, V


def plane(P, contact, C, gap_rel=1e-3, sweeps=SWEEPS, margin=None):
    """The plane through the contact slots alone -> dict(cm, exists, gap, n, dist, lmin, T); needs a contact slot."""
    nc = int(contact.sum())
    ncd = float(nc)
    cm = [_sum(P[:, k], contact) / ncd for k in range(3)]
    out = dict(cm=cm, exists=False, gap=0.0)
    if nc < 3:
        return out
    with np.errstate(all="ignore"):
        q = [np.where(contact, P[:, k] - cm[k], 0.0) for k in range(3)]
    Axx, Axy, Axz = _sum(q[0] * q[0], contact), _sum(q[0] * q[1], contact), _sum(q[0] * q[2], contact)
    Ayy, Ayz, Azz = _sum(q[1] * q[1], contact), _sum(q[1] * q[2], contact), _sum(q[2] * q[2], contact)
    tr = (Axx + Ayy) + Azz
    if not tr > 0.0:
        return out
    T, V = jacobi3([[Axx, Axy, Axz], [Axy, Ayy, Ayz], [Axz, Ayz, Azz]], sweeps)
    k = 0
    for i in range(1, 3):
        if T[i][i] < T[k][k]:
            k = i
    l1 = None
    for i in range(3):
        if i != k and (l1 is None or T[i][i] < l1):
            l1 = T[i][i]
    out["gap"] = gap = (l1 - T[k][k]) / tr
    out["T"] = T
    v = [V[i][k] for i in range(3)]
    nr = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    nx, ny, nz = v[0] / nr, v[1] / nr, v[2] / nr
    dd = (nx * (C[0] - cm[0]) + ny * (C[1] - cm[1])) + nz * (C[2] - cm[2])
    if dd < 0.0:
        nx, ny, nz, dd = -nx, -ny, -nz, -dd
    if margin is not None:
        margin.append(("gap", _rel(gap, gap_rel)))
        if gap > gap_rel:
            margin.append(("dist", dd / max(math.sqrt(dist2(np.asarray([cm]), C)[0]), 1e-300)))
    if gap > gap_rel and dd > 0.0:
        out.update(exists=True, n=[nx, ny, nz], dist=dd, lmin=T[k][k])
    return out


def frame(P, fit_pred, use_pred, given=None, Q=None, q_ok=None, contact_depth=0.1, piv_rel=1e-9, gap_rel=1e-3, reject_k=0.0,
          sweeps=SWEEPS, margin=None):
    """One frame: P [m, 3]; fit_pred, use_pred [m] -> (sphere row [31], radial [m, 2], decomp [m, 4] (zeros without Q))."""
    m = P.shape[0]
    fit_pred, use_pred = np.asarray(fit_pred, dtype=bool), np.asarray(use_pred, dtype=bool)
    row, rad, dec = np.zeros(SPHERE_COLS), np.zeros((m, 2)), np.zeros((m, 4))
    row[N_FIT] = row[N_FIT_USED] = float(fit_pred.sum())
    row[N_USED], row[DEEPEST] = float(use_pred.sum()), -1.0
    if given is not None:
        C, R = [float(given[0]), float(given[1]), float(given[2])], float(given[3])
        with np.errstate(all="ignore"):
            rho = np.where(fit_pred, np.sqrt(dist2(P, C)) - R, 0.0)
        ssr, nfu = _sum(rho * rho, fit_pred), int(fit_pred.sum())
    else:
        f = fit(P, fit_pred, piv_rel, margin)
        if not f["exists"]:
            return row, rad, dec
        nfu = f["count"]
        if reject_k > 0.0 and f["ssr"] > 0.0:
            thr = (reject_k * reject_k) * (f["ssr"] / float(f["count"]))
            rr = f["rho"] * f["rho"]
            keep = fit_pred & (rr <= thr)
            if margin is not None and fit_pred.any():
                margin.append(("reject", float(np.min(np.abs(rr[fit_pred] - thr) / np.maximum(rr[fit_pred], thr)))))
            kc = int(keep.sum())
            if kc < f["count"]:
                f2 = fit(P, keep, piv_rel, margin)
                if f2["exists"]:
                    f, nfu, row[REJECTED] = f2, kc, 1.0
        C, R, ssr = f["C"], f["R"], f["ssr"]
    row[N_FIT_USED] = float(nfu)
    row[CX:CZ + 1], row[RADIUS] = C, R
    row[RMS_FIT] = math.sqrt(ssr / float(nfu)) if nfu > 0 else 0.0
    r2 = dist2(P, C)
    Rc = R - contact_depth
    thr2 = Rc * Rc
    contact = use_pred & (r2 < thr2) if Rc > 0.0 else np.zeros(m, dtype=bool)
    if margin is not None:
        margin.append(("Rc", abs(Rc) / R))
        if Rc > 0.0 and use_pred.any():
            margin.append(("member", float(np.min(np.abs(r2[use_pred] - thr2) / np.maximum(r2[use_pred], thr2)))))
    with np.errstate(all="ignore"):
        rad[:, 0] = use_pred
        rad[:, 1] = np.where(use_pred, np.sqrt(r2) - R, 0.0)
    if Q is not None:
        dec = decompose(P, Q, use_pred & np.asarray(q_ok, dtype=bool), C)
    nc = int(contact.sum())
    row[N_CONTACT] = float(nc)
    row[FLAG] = 1.0
    if nc == 0:
        return row, rad, dec
    with np.errstate(all="ignore"):
        depth = np.where(contact, R - np.sqrt(r2), 0.0)
    pl = plane(P, contact, C, gap_rel, sweeps, margin)
    r2min = float(np.min(r2[contact]))
    row[FLAG] = 2.0
    row[CMX:CMZ + 1] = pl["cm"]
    row[DEPTH_SUM] = _sum(depth, contact)
    row[DEPTH_MEAN] = row[DEPTH_SUM] / float(nc)
    row[DEPTH_MAX] = R - math.sqrt(r2min)
    row[DEEPEST] = float(np.flatnonzero(contact & (r2 == r2min))[0])
    row[GAP] = pl["gap"]
    if not pl["exists"]:
        return row, rad, dec
    n, dd = pl["n"], pl["dist"]
    row[FLAG] = 3.0
    row[NX:NZ + 1], row[DIST], row[OFFSET] = n, dd, R - dd
    h2 = R * R - dd * dd
    row[SPOT_RADIUS] = math.sqrt(h2 if h2 > 0.0 else 0.0)
    row[TILT_DEG] = math.atan2(math.sqrt(n[0] * n[0] + n[1] * n[1]), n[2]) * DEG
    row[AZIMUTH_DEG] = math.atan2(n[1], n[0]) * DEG
    row[SX:SZ + 1] = [C[k] - dd * n[k] for k in range(3)]
    row[PLANE_RMS] = math.sqrt((pl["lmin"] if pl["lmin"] > 0.0 else 0.0) / float(nc))
    return row, rad, dec


def decompose(P, Q, pred, C):
    """decomp [m, 4] = (1, d_n, d_mer, d_az) for the slots of `pred` whose Q is not the centre."""
    m = P.shape[0]
    out = np.zeros((m, 4))
    for r in np.flatnonzero(pred):
        qx, qy, qz = (float(x) for x in Q[r])
        wx, wy, wz = qx - C[0], qy - C[1], qz - C[2]
        wn = math.sqrt((wx * wx + wy * wy) + wz * wz)
        if not wn > 0.0:
            continue
        hx, hy, hz = wx / wn, wy / wn, wz / wn
        h2 = hx * hx + hy * hy
        ax, ay, ex, ey, ez = 0.0, 1.0, 1.0, 0.0, 0.0
        if h2 != 0.0:
            h = math.sqrt(h2)
            ax, ay = -hy / h, hx / h
            ex, ey, ez = ay * hz, -(ax * hz), ax * hy - ay * hx
        Dx, Dy, Dz = float(P[r, 0]) - qx, float(P[r, 1]) - qy, float(P[r, 2]) - qz
        out[r] = (1.0, (Dx * hx + Dy * hy) + Dz * hz, (Dx * ex + Dy * ey) + Dz * ez, Dx * ax + Dy * ay)
    return out


def used_points(table, mask=None, frame_range=None):
    """-> (P [F, m, 3], used [F, m]): the used rule of the entry for one mask."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    fa, fb = (0, n) if frame_range is None else frame_range
    sel = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    xyz = (np.nan_to_num(t[fa:fb, :, 0], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) & 2) != 0
    return t[fa:fb, :, 6:9].astype(np.float64), xyz & sel[None]


def sphere_series(table, given=None, fit_mask=None, slot_mask=None, source=None, contact_depth=0.1, piv_rel=1e-9, gap_rel=1e-3,
                  reject_k=0.0, frame_range=None, sweeps=SWEEPS, margins=None):
    """vbs_sphere_series: -> (sphere [F, 31], radial [F, m, 2], decomp [F, m, 4]); `margins`: a list that receives (kind, relative
    margin) of every decision."""
    P, fit_used = used_points(table, fit_mask, frame_range)
    _, used = used_points(table, slot_mask, frame_range)
    F, m = used.shape
    Q = q_ok = None
    if source is not None:
        src = np.asarray(source, dtype=np.float64)
        Q, q_ok = src[:, 1:4], src[:, 0] != 0
    sph, rad, dec = np.zeros((F, SPHERE_COLS)), np.zeros((F, m, 2)), np.zeros((F, m, 4))
    for f in range(F):
        sph[f], rad[f], dec[f] = frame(P[f], fit_used[f], used[f], given, Q, q_ok, float(contact_depth), float(piv_rel), float(gap_rel),
                                       float(reject_k), sweeps, margins)
    return sph, rad, dec


def assert_margins(margins, what=""):
    """Every decision of a case is far (MIN_MARGIN, relatively) from flipping: 4 ulp of a root moves a compared quantity by 2^-50."""
    bad = [(k, v) for k, v in margins if not v > MIN_MARGIN]
    assert not bad, f"{what}: decisions without a margin: {bad[:5]}"


# ---- the independent side -----------------------------------------------------------------------------------------------------------
def geometric_fit(P, x0=None):
    """The least-squares sphere of points P [k, 3] on the GEOMETRIC residual |P - C| - R by `scipy.optimize.least_squares`, started
    from `x0` = (C, R) or from the centroid: -> (C [3], R)."""
    from scipy.optimize import least_squares
    P = np.asarray(P, dtype=np.float64)
    if x0 is None:
        c0 = P.mean(axis=0)
        x0 = np.concatenate([c0 + np.array([0.0, 0.0, 1.0]), [np.sqrt(((P - c0) ** 2).sum(axis=1)).mean() + 1.0]])
    res = least_squares(lambda x: np.sqrt(((P - x[:3]) ** 2).sum(axis=1)) - x[3], np.asarray(x0, dtype=np.float64), xtol=1e-15, ftol=1e-15,
                        gtol=1e-15, x_scale="jac")
    return res.x[:3], float(res.x[3])


def svd_plane(points, C):
    """The plane of points [k, 3] by `np.linalg.svd` of the centred points: -> (n oriented towards C, dist, centroid, singular values)."""
    pts = np.asarray(points, dtype=np.float64)
    cm = pts.mean(axis=0)
    _, S, Vt = np.linalg.svd(pts - cm)
    n = Vt[2]
    d = float(n @ (np.asarray(C) - cm))
    return (n, d, cm, S) if d >= 0.0 else (-n, -d, cm, S)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def _bits_equal(g, w, what):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    assert g.shape == w.shape and g.dtype == np.float64, (what, g.shape, w.shape, g.dtype)
    diff = g.view(np.uint64) != w.view(np.uint64)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} entries differ in bits, first at {list(at)}: {g[at]!r} != {w[at]!r}")


def check(got, want, what=""):
    """(sphere, radial, decomp) of the device (None = not asked for) against the restatement's: everything bit for bit, +0 and -0
    told apart, but the columns `ULP_COLS` of sphere (4 ulp).  No entry is skipped or masked, and no output may hold a NaN."""
    sph, rad, dec = got
    if sph is not None:
        g = np.asarray(sph)
        assert g.shape == want[0].shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "sphere", g.shape)
        _bits_equal(g[:, EXACT_COLS], want[0][:, EXACT_COLS], f"{what}: sphere (exact columns)")
        for col in ULP_COLS:
            u = PO.ulps(g[:, col], want[0][:, col])
            assert (u <= 4).all(), f"{what}: sphere column {col} off by {int(u.max())} ulp in frame {int(u.argmax())}"
    if rad is not None:
        assert not np.isnan(np.asarray(rad)).any(), (what, "radial")
        _bits_equal(np.asarray(rad), want[1], f"{what}: radial")
    if dec is not None:
        assert not np.isnan(np.asarray(dec)).any(), (what, "decomp")
        _bits_equal(np.asarray(dec), want[2], f"{what}: decomp")
