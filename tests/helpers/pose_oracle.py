"""NumPy restatement of the pose-misalignment series (`include/vbs.h`: vbs_pose_series), the side that shares none of its
order (`np.linalg.lstsq` on the end points, `math.fsum` means), the synthetic recordings both test files use, and the bounds.

The restatement is the SAME IEEE operations in the SAME order as the device, vectorised over frames: per sum the 64 lane sums
(lane l adds slots l, l + 64, ... ascending; select, never multiply by zero) and the fold a[i] + a[i + 32], + 16, ... + 1, as
`filter_oracle.axis_total`; NumPy's ufuncs do not contract a product into a sum.  The device is held to it BIT FOR BIT in
everything but the three columns that pass through sqrt / atan / atan2 last (4 ulp, the precedent of the dwell `std`).

The independent side solves the same least-squares problem by another algorithm (an SVD on [x, y, 1], uncentred) and takes its
means exactly rounded.  The restatement solves the centred normal equations, so the two differ by the conditioning of those:
with kappa = cond of the centred [x, y] columns, the forward error of (a, b) is of the order m u kappa^2 (|a| + |b| + |r| / |x|),
far below anything a fit of float32 table entries means.  The project's convention for such a bound is the measured worst
ratio with a margin of 10: `PLANE_TOL` below is 10 x the worst |restatement - lstsq| seen by `tests/test_pose_host.py` over its
cases (3.9e-15 at 60 degrees, m = 3, relative to max(1, |a|, |b|, |c|)), NOT anything a device gave; where only a few slots
are common the points can lie close to a line, so the bound carries the factor max(1, kappa^2) the argument above gives it.  The means are held to the
summation bound m 2^-52 sum|v| / count of `filter_oracle`."""
import math

import numpy as np

U2 = 2.0 ** -52
DEG = 57.29577951308232
PLANE_TOL = 4e-14            # |a, b, c - lstsq| <= PLANE_TOL max(1, |a|, |b|, |c|): 10 x the measured 3.9e-15 (see above)
TREND_TOL_DEG = 0.15         # |trend tilt - ramp| on the synthetic ramp: 10 x the 0.013 deg the restatement meets on the CPU


def lane_fold(v, pred):
    """[F, m] values, [F, m] predicate -> [F]: the stated order of every sum."""
    v, pred = np.asarray(v, dtype=np.float64), np.asarray(pred, dtype=bool)
    f, m = v.shape
    rows = (m + 63) // 64
    vp, pp = np.zeros((f, rows * 64)), np.zeros((f, rows * 64), dtype=bool)
    vp[:, :m], pp[:, :m] = np.where(pred, v, 0.0), pred
    vp, pp = vp.reshape(f, rows, 64), pp.reshape(f, rows, 64)
    lane = np.zeros((f, 64))
    for r in range(rows):
        lane = np.where(pp[:, r], lane + vp[:, r], lane)
    off = 32
    while off >= 1:
        lane = lane[:, :off] + lane[:, off:2 * off]
        off //= 2
    return lane[:, 0]


def _plane(P, pred, cnt):
    """Means, centred sums, plane and SSR over the slots of `pred` ([F, m]); cnt = pred.sum(1).  -> exists, a, b, c, ssr, r."""
    n = cnt.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = [np.where(cnt > 0, lane_fold(P[..., k], pred) / n, 0.0) for k in range(3)]
        x, y, z = (np.where(pred, P[..., k] - mean[k][:, None], 0.0) for k in range(3))
        xx, xy, yy = lane_fold(x * x, pred), lane_fold(x * y, pred), lane_fold(y * y, pred)
        xz, yz = lane_fold(x * z, pred), lane_fold(y * z, pred)
        det = xx * yy - xy * xy
        exists = (cnt >= 3) & (np.abs(det) > 1e-300)
        a = np.where(exists, (xz * yy - yz * xy) / det, 0.0)
        b = np.where(exists, (yz * xx - xz * xy) / det, 0.0)
        c = np.where(exists, mean[2] - a * mean[0] - b * mean[1], 0.0)
        r = np.where(pred, z - (a[:, None] * x + b[:, None] * y), 0.0)
        ssr = np.where(exists, lane_fold(r * r, pred), 0.0)
    return exists, a, b, c, ssr, r


def pose_series(table, ref_disp, ref_xyz, start_frame=0, mask=None, shell=False, scale=1.0, reject_k=0.0, frame_range=None):
    """-> (deviation [b-a, m, 4], field [b-a, 6], pose [b-a, 8], rms2 [b-a]) exactly as vbs_pose_series states them; rms2 =
    SSR / n_used, the quotient `pose[:, 6]` is the square root of (0 where there is no plane)."""
    t = np.asarray(table)
    rd, rx = np.asarray(ref_disp, dtype=np.float64), np.asarray(ref_xyz, dtype=np.float64)
    n, m, _ = t.shape
    fa, fb = (0, n) if frame_range is None else frame_range
    sel = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    xyz = (t[..., 0].astype(np.int64) & 2) != 0
    sel = sel & (rd[:, 0] != 0) & xyz[start_frame]
    ok = xyz[fa:fb] & sel[None, :]
    okc = ok[..., None]
    scale, reject_k = float(scale), float(reject_k)
    with np.errstate(all="ignore"):
        d = (t[fa:fb, :, 6:9].astype(np.float64) - t[start_frame, :, 6:9].astype(np.float64)[None]) - rd[None, :, 1:4]
        d = np.where(okc, d, 0.0)
        sd = scale * d
        base = np.where(sel[:, None], rx, 0.0)
        if not shell:
            base[:, 2] = 0.0
        P = np.where(okc, base[None] + sd, 0.0)
        mag = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        cnt = ok.sum(axis=1)
        want = int(sel.sum())
        n0 = cnt.astype(np.float64)
        field = np.zeros((fb - fa, 6))
        field[:, 0] = (cnt == want) & (want >= 1)
        field[:, 1] = n0
        for k in range(3):
            field[:, 2 + k] = np.where(cnt > 0, lane_fold(sd[..., k], ok) / n0, 0.0)
        field[:, 5] = np.where(cnt > 0, lane_fold(mag, ok) / n0, 0.0)
        deviation = np.concatenate([ok.astype(np.float64)[..., None], d], axis=2)

        exists, a, b, c, ssr, r = _plane(P, ok, cnt)
        flag = exists.astype(np.float64)
        n_used = n0.copy()
        if reject_k > 0.0:
            rej = exists & (ssr > 0.0)
            thr = (reject_k * reject_k) * (ssr / n0)
            keep = ok & (r * r <= thr[:, None]) & rej[:, None]
            kc = keep.sum(axis=1)
            redo = rej & (kc < cnt) & (kc >= 3)
            e2, a2, b2, c2, ssr2, _ = _plane(P, keep & redo[:, None], np.where(redo, kc, 0))
            a, b, c, ssr = np.where(e2, a2, a), np.where(e2, b2, b), np.where(e2, c2, c), np.where(e2, ssr2, ssr)
            n_used = np.where(e2, kc.astype(np.float64), n_used)
            flag = np.where(e2, 2.0, flag)
        any_ = flag != 0
        rms2 = np.where(any_, ssr / n_used, 0.0)
        pose = np.zeros((fb - fa, 8))
        pose[:, 0], pose[:, 1], pose[:, 2], pose[:, 3] = flag, a, b, c
        pose[:, 4] = np.where(any_, np.arctan(np.sqrt(a * a + b * b)) * DEG, 0.0)
        pose[:, 5] = np.where(any_, np.arctan2(b, a) * DEG, 0.0)
        pose[:, 6] = np.where(any_, np.sqrt(rms2), 0.0)
        pose[:, 7] = n_used
    return deviation, field, pose, rms2


def end_points(deviation, ref_xyz, shell=False, scale=1.0):
    """[F, m, 3] end points from a deviation output, as the independent side builds them (junk where the flag is 0)."""
    base = np.asarray(ref_xyz, dtype=np.float64).copy()
    if not shell:
        base[:, 2] = 0.0
    return base[None] + float(scale) * np.asarray(deviation)[..., 1:4]


def independent(deviation, ref_xyz, shell=False, scale=1.0, use=None):
    """The side that shares no order: per frame (count, a, b, c, rms, mean scaled d [3], mean |d|, kappa, span) from
    `np.linalg.lstsq` on [x, y, 1] over the slots with flag 1 (or over `use` [F, m]) and `math.fsum`; NaN plane where count < 3.
    kappa = the condition number of the centred [x, y] columns, span = 1 + max|x| + max|y| + max|z| of the points used."""
    dev = np.asarray(deviation)
    P = end_points(dev, ref_xyz, shell, scale)
    out = []
    for f in range(dev.shape[0]):
        ok = dev[f, :, 0] != 0 if use is None else np.asarray(use)[f]
        cnt = int(ok.sum())
        plane, kappa = (math.nan,) * 4, 1.0
        span = 1.0
        if cnt >= 3:
            A = np.column_stack([P[f, ok, 0], P[f, ok, 1], np.ones(cnt)])
            co = np.linalg.lstsq(A, P[f, ok, 2], rcond=None)[0]
            res = P[f, ok, 2] - A @ co
            plane = (float(co[0]), float(co[1]), float(co[2]), math.sqrt(math.fsum((res * res).tolist()) / cnt))
            sv = np.linalg.svd(A[:, :2] - A[:, :2].mean(axis=0), compute_uv=False)
            kappa = float(sv[0] / sv[1]) if sv[1] > 0 else math.inf
            span = float(np.abs(P[f, ok]).max(axis=0).sum()) + 1.0
        okd = dev[f, :, 0] != 0
        c0 = int(okd.sum())
        mean_d = [math.fsum((float(scale) * dev[f, okd, 1 + k]).tolist()) / c0 if c0 else 0.0 for k in range(3)]
        mags = np.sqrt((dev[f, okd, 1:4] ** 2).sum(axis=1))
        out.append((cnt,) + plane + tuple(mean_d) + (math.fsum(mags.tolist()) / c0 if c0 else 0.0, kappa, span))
    return np.array(out, dtype=np.float64)


def check_against_independent(deviation, field, pose, ref_xyz, shell=False, scale=1.0, what=""):
    """Plane (where flag 1: the first plane, over all common slots) and means against `independent`.  Returns the worst plane
    difference relative to max(1, |a|, |b|, |c|) and to kappa^2, so that a caller can print it."""
    ind = independent(deviation, ref_xyz, shell, scale)
    m = np.asarray(deviation).shape[1]
    worst = 0.0
    for f in range(ind.shape[0]):
        assert field[f, 1] == ind[f, 0], (what, f)
        dsel = np.asarray(deviation)[f, np.asarray(deviation)[f, :, 0] != 0, 1:4]
        for k in range(3):
            bound = m * U2 * float(np.abs(float(scale) * dsel[:, k]).sum()) / max(ind[f, 0], 1.0) + 2 * U2 * abs(ind[f, 5 + k])
            assert abs(field[f, 2 + k] - ind[f, 5 + k]) <= bound, (what, f, k)
        bound = (m + 4) * U2 * ind[f, 8] + 2 * U2 * ind[f, 8]
        assert abs(field[f, 5] - ind[f, 8]) <= bound, (what, f, "mean |d|")
        if pose[f, 0] == 1.0 and np.isfinite(ind[f, 1]) and np.isfinite(ind[f, 9]):
            ref = max(1.0, *np.abs(ind[f, 1:4]))
            tol = PLANE_TOL * max(1.0, ind[f, 9] ** 2)       # the normal equations square the conditioning (1 - 2 on a full grid)
            err = float(np.abs(pose[f, 1:4] - ind[f, 1:4]).max()) / ref
            worst = max(worst, err / max(1.0, ind[f, 9] ** 2))
            assert err <= tol, f"{what}: frame {f} plane off lstsq by {err:.3e} (relative; kappa {ind[f, 9]:.1f})"
            # the residuals move by at most the plane's difference times the points' extent, over a floor of m roundings
            assert abs(pose[f, 6] - ind[f, 4]) <= (tol * ref + m * U2) * ind[f, 10], (what, f, "rms")
    return worst


def ulps(a, b):
    """Distance in units of the last place between float64 arrays (same shape); equal zeros of either sign are 0 apart."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return np.abs(ia - ib)


def check_pose(got, want, what=""):
    """(deviation, field, pose) of the device against the restatement's (deviation, field, pose, rms2): everything bit for bit
    but tilt_deg, azimuth_deg and rms (4 ulp).  rms^2 is no column of its own: SSR / n_used is held through rms, within 4 ulp of
    the square root of the restated quotient.  No entry is skipped or masked."""
    for name, g, w in (("deviation", got[0], want[0]), ("field", got[1], want[1])):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == w.shape and g.dtype == np.float64, (what, name, g.shape, w.shape)
        diff = g.view(np.uint64) != w.view(np.uint64)
        assert not diff.any(), f"{what}: {name}: {int(diff.sum())} entries differ in bits, first at {np.argwhere(diff)[0].tolist()}"
    if got[2] is None:
        return
    g, w = np.asarray(got[2]), want[2]
    assert g.shape == w.shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "pose", g.shape)
    exact = [0, 1, 2, 3, 7]
    diff = g[:, exact].view(np.uint64) != np.ascontiguousarray(w[:, exact]).view(np.uint64)
    assert not diff.any(), f"{what}: pose flag / a / b / c / n_used: {int(diff.sum())} differ in bits, first at {np.argwhere(diff)[0].tolist()}"
    for col, name in ((4, "tilt_deg"), (5, "azimuth_deg"), (6, "rms")):
        u = ulps(g[:, col], w[:, col])
        assert (u <= 4).all(), f"{what}: {name} off by {int(u.max())} ulp in frame {int(u.argmax())}"
    u = ulps(g[:, 6], np.sqrt(want[3]))
    assert (u <= 4).all(), f"{what}: rms is not the root of the restated SSR / n_used ({int(u.max())} ulp)"


# ---- synthetic recordings ------------------------------------------------------------------------------------------------------
def grid_ref(m, pitch=2.0):
    """m reference positions on a square grid of `pitch` mm around the origin, a shallow dome in Z; exactly representable."""
    side = int(math.ceil(math.sqrt(m)))
    i = np.arange(m)
    x, y = (i % side - (side - 1) // 2) * pitch, (i // side - (side - 1) // 2) * pitch
    return np.stack([x, y, 0.015625 * (x * x + y * y)], axis=1).astype(np.float64)


def tilted_table(ref, tilt_deg, azimuth_deg, seed=0, noise=0.0, drop=0.0, offset=-0.5):
    """float32 table [n, m, 10] of a recording whose frame f is tilted by tilt_deg[f] towards azimuth_deg (scalars or [n]):
    slot j rests at ref[j] and moves by dZ = a x + b y + offset, a = tan(tilt) cos(az), b = tan(tilt) sin(az), plus `noise`
    (sigma, mm) on all axes; a fraction `drop` of the entries loses its 3-D point and holds NaN / 1e30 there.  Frame 0 is the
    undisturbed start (no tilt, no offset, no noise, every slot seen)."""
    rng = np.random.default_rng(seed)
    tilt = np.atleast_1d(np.asarray(tilt_deg, dtype=np.float64))
    az = np.broadcast_to(np.asarray(azimuth_deg, dtype=np.float64), tilt.shape)
    n, m = tilt.size, ref.shape[0]
    a, b = np.tan(np.radians(tilt)) * np.cos(np.radians(az)), np.tan(np.radians(tilt)) * np.sin(np.radians(az))
    xyz = np.broadcast_to(ref[None], (n, m, 3)).copy()
    xyz[..., 2] += a[:, None] * ref[None, :, 0] + b[:, None] * ref[None, :, 1] + offset
    xyz += rng.normal(0.0, 1.0, (n, m, 3)) * noise
    xyz[0] = ref
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    t[..., 6:9] = xyz.astype(np.float32)
    dead = rng.random((n, m)) < drop
    dead[0] = False
    poison(t, dead, rng)
    return t


def poison(t, dead, rng):
    """Clear VBS_FLAG_XYZ on the entries of `dead` [n, m] and fill their X, Y, Z with NaN / 1e30: they must never be read."""
    t[..., 0][dead] = rng.choice([0.0, 1.0], int(dead.sum())).astype(np.float32)
    junk = np.where(rng.random((int(dead.sum()), 3)) < 0.5, np.nan, 1e30).astype(np.float32)
    t[..., 6:9][dead] = junk
    return t
