"""NumPy float64 restatement of `vbs_pose_cov` (include/vbs.h; csrc/k_posecov.hip), operand for operand: the side the GPU tests
hold all 17 columns of `pcov` to BIT FOR BIT.  It is built on the pieces the two parent entries are already held to:
`uncert_oracle._rows` (usable, J_obs Sigma_o J_obs', G = J_cam L of table rows), `uncert_oracle.lane_sums` (lane l adds slots l,
l + 64, .. ascending, then the fold 32 .. 1) and `pose_oracle.pose_series` (the plane, its flag and the rejection).

The independent side (`lstsq_plane`) fits z = a x + b y + c by `np.linalg.lstsq` on [x, y, 1], uncentred: the host tests hold the
influence matrix to its central differences and Sigma_obs to a Monte-Carlo run through it."""
import numpy as np

import pose_oracle as PO
import uncert_oracle as U

POSECOV_COLS, GROUP = 17, 4
DEG = 57.29577951308232


def influence(a, b, x, y, r, xx, xy, yy, det, n_used, mx, my):
    """K [m, 3, 3] of slots with the centred coordinates x, y [m] and residual r [m]: column k = what the unit perturbation e_k of
    ONE slot does to (a, b, c)."""
    K = np.zeros(x.shape + (3, 3))
    with np.errstate(all="ignore"):
        for k in range(3):
            dx, dy, dz = (1.0 if k == j else 0.0 for j in range(3))
            e = (dz - a * dx) - b * dy
            h1, h2 = x * e + r * dx, y * e + r * dy
            da, db = (h1 * yy - h2 * xy) / det, (h2 * xx - h1 * xy) / det
            K[..., 0, k], K[..., 1, k], K[..., 2, k] = da, db, (e / n_used - da * mx) - db * my
    return K


def used_plane(P, used):
    """What the linearisation needs of the used set of ONE frame (P [m, 3], used [m]): (mean [3], xx, xy, yy, det, n_used, x, y,
    z [m]) in the stated order of every sum."""
    n = float(used.sum())
    with np.errstate(all="ignore"):
        mean = [U.lane_sums(P[:, k], used) / n for k in range(3)]
        x, y, z = (np.where(used, P[:, k] - mean[k], 0.0) for k in range(3))
        xx, xy, yy = U.lane_sums(x * x, used), U.lane_sums(x * y, used), U.lane_sums(y * y, used)
    return mean, xx, xy, yy, xx * yy - xy * xy, n, x, y, z


def end_points(table, ref_disp, ref_xyz, start_frame, mask, shell, scale, reject_k, frame_range):
    """-> (pose [F, 8], P [F, m, 3] (zeros where not common), common [F, m], used [F, m]) of `pose_oracle.pose_series`."""
    dev, _, pose, _ = PO.pose_series(table, ref_disp, ref_xyz, start_frame, mask, shell, scale, reject_k, frame_range)
    rx = np.asarray(ref_xyz, dtype=np.float64).copy()
    if not shell:
        rx[:, 2] = 0.0
    ok = dev[..., 0] != 0
    with np.errstate(all="ignore"):
        P = np.where(ok[..., None], rx[None] + float(scale) * dev[..., 1:4], 0.0)
        used = ok.copy()
        if float(reject_k) > 0.0:
            cnt = ok.sum(axis=1)
            exists, _, _, _, ssr, r = PO._plane(P, ok, cnt)
            thr = (float(reject_k) * float(reject_k)) * (ssr / cnt.astype(np.float64))
            keep = ok & (r * r <= thr[:, None])
            used = np.where((pose[:, 0] == 2.0)[:, None], keep, ok)
    return pose, P, ok, used


def fixed_rows(c, start_row, ref_rows, min_size, obs, L):
    """The pre-pass: -> (fixed_usable [m], S_fix [m, 6], g_fix [m, q, 3])."""
    ok, part, G = U._rows(c, start_row, min_size, obs, L)
    if ref_rows is not None:
        ok2, part2, G2 = U._rows(c, ref_rows[0], min_size, obs, L)       # ref_start
        ok1, part1, G1 = U._rows(c, ref_rows[1], min_size, obs, L)       # ref_end
        ok = ok & ok1 & ok2
        part = (part + part1) + part2
        G = (G + G1) - G2
    return ok, np.where(ok[:, None], part, 0.0), np.where(ok[:, None, None], G, 0.0)


def pose_cov(table, ref_disp, ref_xyz, c, obs, L=None, ref_rows=None, start_frame=0, mask=None, shell=False, scale=1.0, reject_k=0.0,
             min_size=5.0, piv_rel=1e-12, frame_range=None, detail=None):
    """vbs_pose_cov: -> (pose [F, 8], pcov [F, 17]).  `detail`: a list that receives, per frame with flag bit 1, a dict of what the
    sums were made of (used, P, C [m, 6], K [m, 3, 3], sigma_obs [6])."""
    t = np.asarray(table)
    n, m = t.shape[:2]
    fa, fb = (0, n) if frame_range is None else frame_range
    L, obs = U._factor(L), U._obs(obs, m)
    q = L.shape[1]
    scale = float(scale)
    pose, P, _, used = end_points(t, ref_disp, ref_xyz, start_frame, mask, shell, scale, reject_k, (fa, fb))
    fix_ok, s_fix, g_fix = fixed_rows(c, t[start_frame], None if ref_rows is None else np.asarray(ref_rows), min_size, obs, L)
    ss = scale * scale
    k2 = DEG * DEG
    out = np.zeros((fb - fa, POSECOV_COLS))
    for f in range(fb - fa):
        okf, partf, Gf = U._rows(c, t[fa + f], min_size, obs, L)
        u = used[f]
        bad = int((u & ~(fix_ok & okf)).sum())
        o = out[f]
        o[1] = bad
        if pose[f, 0] == 0.0 or bad:
            continue
        a, b = pose[f, 1], pose[f, 2]
        mean, xx, xy, yy, det, n_used, x, y, z = used_plane(P[f], u)
        with np.errstate(all="ignore"):
            r = np.where(u, z - (a * x + b * y), 0.0)
            K = influence(a, b, x, y, r, xx, xy, yy, det, n_used, mean[0], mean[1])
            C = ss * (partf + s_fix)
            ko = U.obs_product(K, C)
            so = [U.lane_sums(ko[:, e], u) for e in range(6)]
            sc = [0.0] * 6
            for col in range(q):
                d = [scale * (Gf[:, col, k] - g_fix[:, col, k]) for k in range(3)]
                v = [U.lane_sums((K[:, i, 0] * d[0] + K[:, i, 1] * d[1]) + K[:, i, 2] * d[2], u) for i in range(3)]
                e = 0
                for i in range(3):
                    for j in range(i, 3):
                        sc[e] = sc[e] + v[i] * v[j]
                        e += 1
            S = [so[e] + sc[e] for e in range(6)]
            aa, bb, ab2 = a * a, b * b, (2.0 * a) * b
            rho2 = aa + bb
            flag = 1.0
            if rho2 > 0.0:
                w = 1.0 + rho2
                o[14] = (k2 * ((aa * S[0] + ab2 * S[1]) + bb * S[3])) / (rho2 * (w * w))
                o[15] = (k2 * ((bb * S[0] - ab2 * S[1]) + aa * S[3])) / (rho2 * rho2)
            piv = piv_rel * (S[0] + S[3])
            d1 = S[0]
            valid = False
            if d1 > piv:
                l = S[1] / d1
                d2 = S[3] - l * S[1]
                if d2 > piv:
                    z1, z2 = a, b - l * a
                    o[16] = z1 * z1 / d1 + z2 * z2 / d2
                    valid = True
            o[0] = (flag + (2.0 if valid else 0.0)) + (4.0 if rho2 > 0.0 else 0.0)
            o[2:8], o[8:14] = S, sc
        if detail is not None:
            detail.append(dict(frame=fa + f, used=u, P=P[f], C=C, K=K, sigma_obs=np.array(so), a=a, b=b, c=pose[f, 3]))
    return pose, out


def lstsq_plane(P):
    """The independent fit: (a, b, c) of z = a x + b y + c over the points P [k, 3]."""
    A = np.column_stack([P[:, 0], P[:, 1], np.ones(P.shape[0])])
    return np.linalg.lstsq(A, P[:, 2], rcond=None)[0]


def check_pcov(got, want, what=""):
    """All 17 columns of the device's pcov against the restatement's, bit for bit; no entry is skipped or masked."""
    g = np.ascontiguousarray(np.asarray(got))
    assert g.shape == want.shape and g.dtype == np.float64, (what, g.shape, want.shape)
    diff = g.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)
    assert not diff.any(), (f"{what}: pcov: {int(diff.sum())} entries differ in bits, first at {np.argwhere(diff)[0].tolist()}: "
                            f"{g[tuple(np.argwhere(diff)[0])]!r} != {want[tuple(np.argwhere(diff)[0])]!r}")
