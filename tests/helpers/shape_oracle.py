"""NumPy / Python float64 restatement of `vbs_shape_series` (include/vbs.h; csrc/k_shape.hip), operand for operand: the side the
GPU tests hold `shape`, `coef` and `residual` to BIT FOR BIT in everything but the five columns that pass through sqrt or atan2
(4 ulp).  The common rule and the end points are `pose_oracle.pose_series`'s (through `posecov_oracle.end_points`), every sum is
`pose_oracle.lane_fold` (lane l adds slots l, l + 64, .. ascending, then the fold 32 .. 1); the factorisation, the substitutions
and the columns are scalar IEEE double operations in the stated order (a Python float is one; nothing here contracts).

The independent side (`lstsq_quadric`, `lstsq_plane`) solves the same least-squares problems by `np.linalg.lstsq` on the design
matrix itself: `tests/test_shape_host.py` holds the restatement to it."""
import math

import numpy as np

import pose_oracle as PO
import posecov_oracle as PCO

SHAPE_COLS, GROUP = 24, 4
DEG = 57.29577951308232
ULP_COLS = (12, 13, 16, 17, 18)                                 # rms_plane, rms, k1, k2, dir_deg
EXACT_COLS = tuple(c for c in range(SHAPE_COLS) if c not in ULP_COLS)


def _sum(v, pred):
    return float(PO.lane_fold(np.asarray(v, dtype=np.float64)[None], np.asarray(pred)[None])[0])


def centred(P, pred, mean, length):
    """u, v, w [m] of the slots of `pred` (0 elsewhere)."""
    with np.errstate(all="ignore"):
        u = np.where(pred, (P[:, 0] - mean[0]) / length, 0.0)
        v = np.where(pred, (P[:, 1] - mean[1]) / length, 0.0)
        w = np.where(pred, P[:, 2] - mean[2], 0.0)
    return u, v, w


def sums(u, v, w, pred):
    """The 20 sums in the entry's order: 14 of the monomials, 6 of the monomials times w."""
    u2, uv, v2 = u * u, u * v, v * v
    u3, u2v, uv2, v3 = u2 * u, u2 * v, u * v2, v2 * v
    u4, u3v, u2v2, uv3, v4 = u2 * u2, u3 * v, u2 * v2, u * v3, v2 * v2
    terms = (u, v, u2, uv, v2, u3, u2v, uv2, v3, u4, u3v, u2v2, uv3, v4, w, u * w, v * w, u2 * w, uv * w, v2 * w)
    return [_sum(t, pred) for t in terms]


def normal_matrix(n, S):
    return [[n, S[0], S[1], S[2], S[3], S[4]], [S[0], S[2], S[3], S[5], S[6], S[7]], [S[1], S[3], S[4], S[6], S[7], S[8]],
            [S[2], S[5], S[6], S[9], S[10], S[11]], [S[3], S[6], S[7], S[10], S[11], S[12]], [S[4], S[7], S[8], S[11], S[12], S[13]]]


def solve(n, S, piv_rel):
    """LDL' in basis order, stopped at the first failing pivot -> (npass, beta [6] or None, gamma [3] or None, d [npass])."""
    N, g = normal_matrix(n, S), S[14:20]
    Lm = [[0.0] * 6 for _ in range(6)]
    c = [[0.0] * 6 for _ in range(6)]
    d = []
    for j in range(6):
        dj = N[j][j]
        for k in range(j):
            dj = dj - Lm[j][k] * c[j][k]
        if not dj > piv_rel * N[j][j]:
            break
        d.append(dj)
        for i in range(j + 1, 6):
            cij = N[i][j]
            for k in range(j):
                cij = cij - Lm[j][k] * c[i][k]
            c[i][j], Lm[i][j] = cij, cij / dj
    npass = len(d)
    z, y = [], []
    for i in range(npass):
        zi = g[i]
        for k in range(i):
            zi = zi - Lm[i][k] * z[k]
        z.append(zi)
        y.append(zi / d[i])
    gam = beta = None
    if npass >= 3:
        g2 = y[2]
        g1 = y[1] - Lm[2][1] * g2
        gam = [(y[0] - Lm[1][0] * g1) - Lm[2][0] * g2, g1, g2]
    if npass == 6:
        beta = [0.0] * 6
        for i in range(5, -1, -1):
            b = y[i]
            for k in range(i + 1, 6):
                b = b - Lm[k][i] * beta[k]
            beta[i] = b
    return npass, beta, gam, d


def resid(u, v, w, degree, beta, gam):
    if degree == 2:
        u2, uv, v2 = u * u, u * v, v * v
        return w - (((((beta[0] + beta[1] * u) + beta[2] * v) + beta[3] * u2) + beta[4] * uv) + beta[5] * v2)
    return w - ((gam[0] + gam[1] * u) + gam[2] * v)


def fit(P, pred, length, min_count, piv_rel):
    """The fit of one set of one frame -> dict(count, mean, degree (what the set reaches), npass, beta, gam, u, v, w) ."""
    c = int(pred.sum())
    out = dict(count=c, mean=[0.0, 0.0, 0.0], degree=0, npass=0, beta=None, gam=None)
    if c == 0:
        return out
    n = float(c)
    out["mean"] = mean = [_sum(P[:, k], pred) / n for k in range(3)]
    if c < 3:
        return out
    u, v, w = centred(P, pred, mean, length)
    npass, beta, gam, _ = solve(n, sums(u, v, w, pred), piv_rel)
    out.update(npass=npass, beta=beta, gam=gam, u=u, v=v, w=w, degree=2 if (c >= min_count and npass == 6) else (1 if npass >= 3 else 0))
    return out


def _ssr(f, degree, pred):
    r = np.where(pred, resid(f["u"], f["v"], f["w"], degree, f["beta"], f["gam"]), 0.0)
    return _sum(r * r, pred), r


def frame(P, common, length, reject_k=0.0, min_count=9, piv_rel=1e-10, apex_rel=1e-6, max_apex=2.0):
    """One frame: P [m, 3] end points, common [m] -> (shape row [24], coef [2, 4], residual [m, 2], used [m])."""
    m = P.shape[0]
    row, coef, res = np.zeros(SHAPE_COLS), np.zeros((2, 4)), np.zeros((m, 2))
    f = fit(P, common, length, min_count, piv_rel)
    used, degree = common, f["degree"]
    row[1] = row[2] = f["count"]
    row[3:6] = f["mean"]
    if degree == 0:
        return row, coef, res, used
    s1, r1 = _ssr(f, 1, used)
    s2, r2 = _ssr(f, 2, used) if degree == 2 else (0.0, None)
    sel, r = (s2, r2) if degree == 2 else (s1, r1)
    if reject_k > 0.0 and sel > 0.0:
        thr = (reject_k * reject_k) * (sel / float(f["count"]))
        keep = common & (r * r <= thr)
        kc = int(keep.sum())
        if kc < f["count"] and kc >= 3:
            f2 = fit(P, keep, length, min_count, piv_rel)
            if f2["degree"] >= degree:
                f, used = f2, keep
                s1, r1 = _ssr(f, 1, used)
                s2, r2 = _ssr(f, 2, used) if degree == 2 else (0.0, None)
                r = r2 if degree == 2 else r1
    nu = float(used.sum())
    mean, gam = f["mean"], f["gam"]
    cf = f["beta"] if degree == 2 else gam
    c0, a, b = mean[2] + cf[0], cf[1] / length, cf[2] / length
    row[0], row[2], row[3:6] = degree, nu, mean
    row[6], row[7], row[8] = c0, a, b
    row[12] = math.sqrt(s1 / nu)
    coef[0] = (degree, c0, a, b)
    res[:, 0], res[:, 1] = used, np.where(used, r, 0.0)
    if degree < 2:
        return row, coef, res, used
    beta = f["beta"]
    p, q, rr = ((2.0 * beta[3]) / length) / length, (beta[4] / length) / length, ((2.0 * beta[5]) / length) / length
    H, K = (p + rr) / 2.0, p * rr - q * q
    hd = (p - rr) / 2.0
    s = math.sqrt(hd * hd + q * q)
    row[9], row[10], row[11], row[13], row[14], row[15] = p, q, rr, math.sqrt(s2 / nu), H, K
    row[16], row[17], row[18] = H + s, H - s, (0.5 * math.atan2(2.0 * q, p - rr)) * DEG
    coef[1] = (1.0, p, q, rr)
    if abs(K) > apex_rel * ((p * p + 2.0 * (q * q)) + rr * rr):
        xi, eta = (q * b - rr * a) / K, (q * a - p * b) / K
        reach = max_apex * length
        if xi * xi + eta * eta <= reach * reach:
            az = c0 + (a * xi + b * eta) / 2.0
            row[19], row[20], row[21], row[22] = 1.0, mean[0] + xi, mean[1] + eta, az
            row[23] = az - (mean[2] + ((gam[0] + (gam[1] * xi) / length) + (gam[2] * eta) / length))
    return row, coef, res, used


def shape_series(table, ref_disp, ref_xyz, start_frame=0, mask=None, shell=False, scale=1.0, length=1.0, reject_k=0.0, min_count=9,
                 piv_rel=1e-10, apex_rel=1e-6, max_apex=2.0, frame_range=None):
    """vbs_shape_series: -> (shape [F, 24], coef [F, 2, 4], residual [F, m, 2])."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    fa, fb = (0, n) if frame_range is None else frame_range
    _, P, common, _ = PCO.end_points(t, ref_disp, ref_xyz, start_frame, mask, shell, scale, 0.0, (fa, fb))
    shape, coef, res = np.zeros((fb - fa, SHAPE_COLS)), np.zeros((fb - fa, 2, 4)), np.zeros((fb - fa, m, 2))
    for f in range(fb - fa):
        shape[f], coef[f], res[f], _ = frame(P[f], common[f], float(length), float(reject_k), int(min_count), float(piv_rel),
                                             float(apex_rel), float(max_apex))
    return shape, coef, res


# ---- the independent side -----------------------------------------------------------------------------------------------------------
def lstsq_quadric(P, mean, length):
    """beta [6] of w ~ phi(u, v) beta over the points P [k, 3], by `np.linalg.lstsq` on the design matrix."""
    u, v, w = (P[:, 0] - mean[0]) / length, (P[:, 1] - mean[1]) / length, P[:, 2] - mean[2]
    A = np.column_stack([np.ones_like(u), u, v, u * u, u * v, v * v])
    return np.linalg.lstsq(A, w, rcond=None)[0]


def lstsq_plane(P, mean, length):
    u, v, w = (P[:, 0] - mean[0]) / length, (P[:, 1] - mean[1]) / length, P[:, 2] - mean[2]
    return np.linalg.lstsq(np.column_stack([np.ones_like(u), u, v]), w, rcond=None)[0]


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def _bits_equal(g, w, what):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    assert g.shape == w.shape and g.dtype == np.float64, (what, g.shape, w.shape, g.dtype)
    diff = g.view(np.uint64) != w.view(np.uint64)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} entries differ in bits, first at {list(at)}: {g[at]!r} != {w[at]!r}")


def check(got, want, what=""):
    """(shape, coef, residual) of the device (None = not asked for) against the restatement's: everything bit for bit but the
    columns `ULP_COLS` of shape (4 ulp).  No entry is skipped or masked, and no output may hold a NaN."""
    shape, coef, res = got
    if shape is not None:
        g = np.asarray(shape)
        assert g.shape == want[0].shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "shape", g.shape)
        _bits_equal(g[:, EXACT_COLS], want[0][:, EXACT_COLS], f"{what}: shape (exact columns {EXACT_COLS})")
        for col in ULP_COLS:
            u = PO.ulps(g[:, col], want[0][:, col])
            assert (u <= 4).all(), f"{what}: shape column {col} off by {int(u.max())} ulp in frame {int(u.argmax())}"
    if coef is not None:
        assert not np.isnan(np.asarray(coef)).any(), (what, "coef")
        _bits_equal(np.asarray(coef), want[1], f"{what}: coef")
    if res is not None:
        assert not np.isnan(np.asarray(res)).any(), (what, "residual")
        _bits_equal(np.asarray(res), want[2], f"{what}: residual")
