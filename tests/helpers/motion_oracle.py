"""NumPy restatement of the strain entries (`include/vbs.h`: vbs_motion_series_f64, vbs_local_strain_f64), the side that shares
none of their order (`np.linalg.lstsq` on [x, y, 1], uncentred, three right-hand sides), the synthetic fields both test files use,
and the bounds.

The restatement is the SAME IEEE operations in the SAME order as the device, vectorised over frames: for the global fit per sum
the 64 lane sums and the fold of `pose_oracle.lane_fold`; for the local fit one chain over the member list i, nbr[i][0], ..
from 0.0.  NumPy's ufuncs do not contract a product into a sum.  The device is held to it BIT FOR BIT in everything but the
columns that pass through sqrt / atan / atan2 last (4 ulp, the precedent of the pose's tilt, azimuth and rms).

The bounds.  Each is 10 x the worst value MEASURED ON THE CPU, restatement against the independent side, by
`tests/test_motion_host.py` over its own cases (which prints the figures it meets); none is taken from anything a device gave.
That file also holds every figure recorded here to what it meets now (within 0.5 .. 1.25 of the record), so that a bound cannot
go stale unnoticed.  The 65 markers of these cases are `ring_layout`, a SYNTHETIC layout - not the sensor's own list.
  FIT_TOL        |t, g - lstsq| relative to max(1, |t|, |g|) and to max(1, kappa^2), kappa = the condition number of the centred
                 [x, y] columns (the normal equations square it, as for `pose_oracle.PLANE_TOL`).  Measured 4.4e-16 over the global
                 fits with m in {3, 4, 65, 441} and 4.2e-15 over the local fits of the same cases (K = 6; the worst at m = 441, where
                 dropouts thin a neighbourhood out): the bound is 10 x the larger.
  CLOSED_TOL     the closed forms d = (R(theta) S - I) p + t: |rot_deg - theta| (degrees), |lambda - eig S|, |omega, dilation, e1,
                 e2 - their definitions on R S - I|, |t - t|, rms and max |residual| (mm, positions within +-16.3 mm): measured 7.1e-15
                 (at -170 degrees, where |d| is about 2 |p| and the residual is what rounding d to float64 leaves).
  (rejection)    the gradient of the 62 undisturbed ring markers recovered with reject_k = 3: the refit IS the fit of the 62 (bit
                 for bit against the restatement run on those 62 alone under a mask), and is held against lstsq within FIT_TOL.
  TREND_TOL      `pipeline.motion_analysis` on the drag-and-twist recording (48 frames, 65 markers, 0.02 mm noise, 10 % dropouts,
                 a 15-tap low-pass at 0.2 of Nyquist): over ALL frames that have a trend - the first and last seven included,
                 where the normalised one-sided window lags a ramp - |trend rot_deg - ramp| measured 0.080 degrees and
                 |filtered t_X - ramp| 0.0116 mm on the CPU (`motion_analysis_cpu`: the restatements of the axis displacement, of
                 the fit and of the FIR); away from the edges 0.014 degrees and 0.0017 mm."""
import math

import numpy as np

from pose_oracle import lane_fold, ulps
from vbs_amd.synth import _RINGS

DEG = 57.29577951308232
FIT_TOL = 4.2e-14
CLOSED_TOL = 7.1e-14
TREND_TOL_DEG = 0.80
TREND_TOL_MM = 0.116
STRAIN_COLS, LSTRAIN_COLS = 16, 8


def invariants(gxx, gxy, gyx, gyy, gzx, gzy):
    """The columns 3 .. 12 of `strain` from the six gradients ([F] each), by the stated expressions in their order."""
    with np.errstate(all="ignore"):
        dilation = gxx + gyy
        omega = 0.5 * (gyx - gxy)
        e1, e2 = 0.5 * (gxx - gyy), 0.5 * (gxy + gyx)
        max_shear = np.sqrt(e1 * e1 + e2 * e2)
        shear_deg = 0.5 * np.arctan2(e2, e1) * DEG
        f11, f12, f21, f22 = 1.0 + gxx, gxy, gyx, 1.0 + gyy
        p, q = f11 + f22, f21 - f12
        a, b = f11 - f22, f12 + f21
        h, w = np.sqrt(p * p + q * q), np.sqrt(a * a + b * b)
        rot_deg = np.arctan2(q, p) * DEG
        tilt_deg = np.arctan(np.sqrt(gzx * gzx + gzy * gzy)) * DEG
    return np.stack([dilation, omega, e1, e2, max_shear, shear_deg, rot_deg, 0.5 * (h + w), 0.5 * (h - w), tilt_deg], axis=1)


def _fit(px, py, d, pred, below=None):
    """Means, centred sums and gradient over the slots of `pred` [F, m] -> exists, cnt, (mx, my, md [3]), gx [3], gy [3]."""
    cnt = pred.sum(axis=1)
    n = cnt.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = lambda v: np.where(cnt > 0, lane_fold(v, pred) / n, 0.0)      # noqa: E731
        mx, my = mean(px), mean(py)
        md = [mean(d[..., k]) for k in range(3)]
        enough = cnt >= 3 if below is None else (cnt >= 3) & (cnt < below)
        pe = pred & enough[:, None]
        x, y = np.where(pe, px - mx[:, None], 0.0), np.where(pe, py - my[:, None], 0.0)
        e = [np.where(pe, d[..., k] - md[k][:, None], 0.0) for k in range(3)]
        xx, xy, yy = lane_fold(x * x, pe), lane_fold(x * y, pe), lane_fold(y * y, pe)
        xe, ye = [lane_fold(x * e[k], pe) for k in range(3)], [lane_fold(y * e[k], pe) for k in range(3)]
        det = xx * yy - xy * xy
        exists = enough & (np.abs(det) > 1e-300)
        gx = [np.where(exists, (xe[k] * yy - ye[k] * xy) / det, 0.0) for k in range(3)]
        gy = [np.where(exists, (ye[k] * xx - xe[k] * xy) / det, 0.0) for k in range(3)]
    return exists, cnt, (mx, my, md), gx, gy


def _resid(px, py, d, used, mean, gx, gy):
    """r [F, m, 3] and q [F, m] of the slots of `used` against a fit (zeros elsewhere)."""
    mx, my, md = mean
    with np.errstate(all="ignore"):
        x, y = px - mx[:, None], py - my[:, None]
        r = [np.where(used, (d[..., k] - md[k][:, None]) - (gx[k][:, None] * x + gy[k][:, None] * y), 0.0) for k in range(3)]
        q = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    return np.stack(r, axis=2), q


def _worst(q, pred):
    """The slot with the largest q among `pred` [F, m], the smallest index among equals, a NaN never; -1 where there is none."""
    cand = pred & ~np.isnan(q)
    idx = np.where(cand, q, -np.inf).argmax(axis=1)                           # (q >= 0; the first of equal maxima)
    return np.where(cand.any(axis=1), idx, -1).astype(np.float64)


def used_slots(rec, mask=None, frame_range=None):
    rec = np.asarray(rec)
    fa, fb = (0, rec.shape[0]) if frame_range is None else frame_range
    sel = np.ones(rec.shape[1], dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    return (rec[fa:fb, :, 0] != 0) & sel[None, :]


def motion_series(rec, pos, mask=None, reject_k=0.0, frame_range=None):
    """-> (grad [b-a, 3, 4], strain [b-a, 16], residual [b-a, s, 4], rms2 [b-a, 2]) exactly as vbs_motion_series_f64 states
    them; rms2 = the two quotients the rms columns are the square roots of (0 where there is no fit)."""
    rec, pos = np.asarray(rec, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    fa, fb = (0, rec.shape[0]) if frame_range is None else frame_range
    used = used_slots(rec, mask, frame_range)
    F, m = used.shape
    sel = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    with np.errstate(all="ignore"):
        px = np.broadcast_to(np.where(sel, pos[:, 0], 0.0)[None], (F, m))
        py = np.broadcast_to(np.where(sel, pos[:, 1], 0.0)[None], (F, m))
        d = np.where(used[..., None], rec[fa:fb, :, 1:4], 0.0)
        ex, cnt, mean, gx, gy = _fit(px, py, d, used)
        u1 = used & ex[:, None]
        r, q = _resid(px, py, d, u1, mean, gx, gy)
        ss = [lane_fold(r[..., k] * r[..., k], u1) for k in range(3)]
        worst = _worst(q, u1)
        n0 = cnt.astype(np.float64)
        n_used, flag = n0.copy(), ex.astype(np.float64)
        rflag = u1.astype(np.float64)
        reject_k = float(reject_k)
        if reject_k > 0.0:
            ssr = (ss[0] + ss[1]) + ss[2]
            rej = ex & (ssr > 0.0)
            thr = (reject_k * reject_k) * (ssr / n0)
            keep = used & (q <= thr[:, None]) & rej[:, None]
            ex2, kc, mean2, gx2, gy2 = _fit(px, py, d, keep, below=cnt)
            u2 = used & ex2[:, None]
            k2 = keep & ex2[:, None]
            r2, q2 = _resid(px, py, d, u2, mean2, gx2, gy2)
            ss2 = [lane_fold(r2[..., k] * r2[..., k], k2) for k in range(3)]
            pick = lambda new, old: np.where(ex2, new, old)                   # noqa: E731
            mean = (pick(mean2[0], mean[0]), pick(mean2[1], mean[1]), [pick(mean2[2][k], mean[2][k]) for k in range(3)])
            gx, gy = [pick(gx2[k], gx[k]) for k in range(3)], [pick(gy2[k], gy[k]) for k in range(3)]
            ss = [pick(ss2[k], ss[k]) for k in range(3)]
            worst = pick(_worst(q2, k2), worst)
            n_used, flag = pick(kc.astype(np.float64), n_used), pick(2.0, flag)
            r = np.where(ex2[:, None, None], r2, r)
            rflag = np.where(ex2[:, None], np.where(keep, 1.0, 2.0) * u2, rflag)
        any_ = flag != 0
        grad = np.zeros((F, 3, 4))
        for k in range(3):
            grad[:, k, 0] = flag
            grad[:, k, 1] = np.where(any_, mean[2][k] - gx[k] * mean[0] - gy[k] * mean[1], 0.0)
            grad[:, k, 2], grad[:, k, 3] = gx[k], gy[k]
        rms2 = np.stack([np.where(any_, (ss[0] + ss[1]) / n_used, 0.0), np.where(any_, ss[2] / n_used, 0.0)], axis=1)
        strain = np.zeros((F, STRAIN_COLS))
        strain[:, 0], strain[:, 1], strain[:, 2] = flag, n0, n_used
        strain[:, 3:13] = np.where(any_[:, None], invariants(gx[0], gy[0], gx[1], gy[1], gx[2], gy[2]), 0.0)
        strain[:, 13:15] = np.sqrt(rms2)
        strain[:, 15] = np.where(any_, worst, -1.0)
        residual = np.concatenate([rflag[..., None], r], axis=2)
    return grad, strain, residual, rms2


def local_strain(rec, pos, nbr, min_count=4, det_rel=0.01, frame_range=None):
    """-> out [b-a, s, 8] exactly as vbs_local_strain_f64 states it: one chain over the member list of every slot."""
    rec, pos, nbr = np.asarray(rec, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(nbr).astype(np.int64)
    fa, fb = (0, rec.shape[0]) if frame_range is None else frame_range
    used = rec[fa:fb, :, 0] != 0
    F, s = used.shape
    members = np.concatenate([np.arange(s)[:, None], nbr], axis=1)
    inr = (members >= 0) & (members < s)
    members = np.where(inr, members, 0)
    with np.errstate(all="ignore"):
        d = np.where(used[..., None], rec[fa:fb, :, 1:4], 0.0)
        vals = [np.broadcast_to(pos[None, :, 0], (F, s)), np.broadcast_to(pos[None, :, 1], (F, s))] + [d[..., k] for k in range(3)]
        self_ = used.copy()
        u = [inr[None, :, j] & used[:, members[:, j]] & self_ for j in range(members.shape[1])]
        cnt = np.zeros((F, s), dtype=np.int64)
        sm = [np.zeros((F, s)) for _ in range(5)]
        for j in range(members.shape[1]):
            cnt += u[j]
            for c in range(5):
                sm[c] = np.where(u[j], sm[c] + vals[c][:, members[:, j]], sm[c])
        enough = self_ & (cnt >= int(min_count))
        n = cnt.astype(np.float64)
        mean = [np.where(enough, sm[c] / n, 0.0) for c in range(5)]
        cs = [np.zeros((F, s)) for _ in range(9)]
        for j in range(members.shape[1]):
            uj = u[j] & enough
            mj = members[:, j]
            x, y = vals[0][:, mj] - mean[0], vals[1][:, mj] - mean[1]
            terms = [x * x, x * y, y * y]
            for k in range(3):
                e = vals[2 + k][:, mj] - mean[2 + k]
                terms += [x * e, y * e]
            for c in range(9):
                cs[c] = np.where(uj, cs[c] + terms[c], cs[c])
        det = cs[0] * cs[2] - cs[1] * cs[1]
        ok = enough & (det > float(det_rel) * (cs[0] * cs[2]))
        gx = [(cs[3 + 2 * k] * cs[2] - cs[4 + 2 * k] * cs[1]) / det for k in range(3)]
        gy = [(cs[4 + 2 * k] * cs[0] - cs[3 + 2 * k] * cs[1]) / det for k in range(3)]
        dilation = gx[0] + gy[1]
        omega = 0.5 * (gx[1] - gy[0])
        e1, e2 = 0.5 * (gx[0] - gy[1]), 0.5 * (gy[0] + gx[1])
        max_shear = np.sqrt(e1 * e1 + e2 * e2)
        out = np.stack([n, dilation, omega, max_shear, e1, e2, gx[2], gy[2]], axis=2)
    return np.where(ok[..., None], out, 0.0)


# ---- the independent side --------------------------------------------------------------------------------------------------------
def lstsq_fit(pos, d, use):
    """[x, y, 1] against the three right-hand sides over the slots of `use` [m] -> (coef [3, 3] = rows k: (t_k, g_kx, g_ky),
    kappa of the centred [x, y]) or (None, inf) below three slots."""
    use = np.asarray(use, dtype=bool)
    if int(use.sum()) < 3:
        return None, math.inf
    A = np.column_stack([pos[use, 0], pos[use, 1], np.ones(int(use.sum()))])
    co = np.linalg.lstsq(A, d[use], rcond=None)[0]                            # [3 (gx, gy, t), 3 (k)]
    sv = np.linalg.svd(A[:, :2] - A[:, :2].mean(axis=0), compute_uv=False)
    kappa = float(sv[0] / sv[1]) if sv[1] > 0 else math.inf
    return np.stack([co[2], co[0], co[1]], axis=1), kappa


def fit_error(coef, got_t, got_gx, got_gy, kappa):
    """The worst |got - lstsq| relative to max(1, |t|, |g|), divided by max(1, kappa^2)."""
    got = np.stack([got_t, got_gx, got_gy], axis=1)
    ref = max(1.0, float(np.abs(coef).max()))
    return float(np.abs(got - coef).max()) / ref / max(1.0, kappa ** 2)


def check_global_against_independent(rec, pos, grad, residual, what=""):
    """Every frame with a fit: its gradient against lstsq over the slots the final fit used (residual flag 1).  -> the worst
    scaled error, for a caller to print; asserts FIT_TOL."""
    rec, pos = np.asarray(rec, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    worst = 0.0
    for f in range(grad.shape[0]):
        if grad[f, 0, 0] == 0:
            continue
        use = residual[f, :, 0] == 1.0
        coef, kappa = lstsq_fit(pos, rec[f, :, 1:4], use)
        if coef is None or not np.isfinite(kappa):
            continue
        err = fit_error(coef, grad[f, :, 1], grad[f, :, 2], grad[f, :, 3], kappa)
        worst = max(worst, err)
        assert err <= FIT_TOL, f"{what}: frame {f} off lstsq by {err:.3e} (scaled; kappa {kappa:.1f})"
    return worst


def check_local_against_independent(rec, pos, nbr, out, what=""):
    """Every slot with a result: g_Zx, g_Zy and the in-plane invariants against lstsq over its used members."""
    rec, pos, nbr = np.asarray(rec, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(nbr)
    s = pos.shape[0]
    worst = 0.0
    for f in range(out.shape[0]):
        for i in np.flatnonzero(out[f, :, 0] != 0):
            mem = [i] + [int(j) for j in nbr[i] if 0 <= j < s]
            mem = [j for j in mem if rec[f, j, 0] != 0]
            if len(set(mem)) != len(mem):
                continue                                                      # (duplicates weight a member: not lstsq's problem)
            use = np.zeros(s, dtype=bool)
            use[mem] = True
            coef, kappa = lstsq_fit(pos, rec[f, :, 1:4], use)
            if coef is None or not np.isfinite(kappa):
                continue
            gxx, gxy, gyx, gyy = coef[0, 1], coef[0, 2], coef[1, 1], coef[1, 2]
            want = np.array([gxx + gyy, 0.5 * (gyx - gxy), 0.5 * (gxx - gyy), 0.5 * (gxy + gyx), coef[2, 1], coef[2, 2]])
            got = out[f, i, [1, 2, 4, 5, 6, 7]]
            err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(coef).max())) / max(1.0, kappa ** 2)
            worst = max(worst, err)
            assert err <= FIT_TOL, f"{what}: frame {f} slot {i} off lstsq by {err:.3e} (scaled; kappa {kappa:.1f})"
    return worst


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def assert_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == np.float64, (what, g.shape, w.shape, g.dtype)
    diff = g.view(np.uint64) != w.view(np.uint64)
    assert not diff.any(), f"{what}: {int(diff.sum())} entries differ in bits, first at {np.argwhere(diff)[0].tolist()}: " \
                           f"{g[tuple(np.argwhere(diff)[0])]!r} != {w[tuple(np.argwhere(diff)[0])]!r}"


STRAIN_EXACT = [0, 1, 2, 3, 4, 5, 6, 15]
STRAIN_NAMES = ("flag", "count", "n_used", "dilation", "omega", "e1", "e2", "max_shear", "shear_deg", "rot_deg", "lambda1", "lambda2",
                "tilt_deg", "rms_inplane", "rms_z", "worst")


def check_motion(got, want, what=""):
    """A dict with `grad`, `strain`, `residual` (any subset) against `motion_series`'s tuple: grad, residual and strain columns
    0 - 6 and 15 bit for bit, columns 7 - 14 to 4 ulp, the two rms columns also within 4 ulp of the root of the restated quotient.
    No entry is skipped or masked."""
    if "grad" in got:
        assert_bits(got["grad"], want[0], what + ": grad")
    if "residual" in got:
        assert_bits(got["residual"], want[2], what + ": residual")
    if "strain" in got:
        g, w = np.asarray(got["strain"]), want[1]
        assert g.shape == w.shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, "strain", g.shape)
        assert_bits(g[:, STRAIN_EXACT], w[:, STRAIN_EXACT], what + ": strain flag .. e2, worst")
        for col in range(7, 15):
            u = ulps(g[:, col], w[:, col])
            assert (u <= 4).all(), f"{what}: {STRAIN_NAMES[col]} off by {int(u.max())} ulp in frame {int(u.argmax())}"
        u = ulps(g[:, 13:15], np.sqrt(want[3]))
        assert (u <= 4).all(), f"{what}: rms is not the root of the restated quotient ({int(u.max())} ulp)"


def check_local(got, want, what=""):
    """`local_strain_f64` against `local_strain`: everything bit for bit but max_shear (4 ulp).  Nothing is skipped."""
    g = np.asarray(got)
    assert g.shape == want.shape and g.dtype == np.float64 and not np.isnan(g).any(), (what, g.shape, want.shape)
    exact = [0, 1, 2, 4, 5, 6, 7]
    assert_bits(g[..., exact], want[..., exact], what + ": local strain")
    u = ulps(g[..., 3], want[..., 3])
    assert (u <= 4).all(), f"{what}: max_shear off by {int(u.max())} ulp"


# ---- synthetic fields ------------------------------------------------------------------------------------------------------------
def ring_layout():
    """A SYNTHETIC 65-marker ring layout for the fields of these tests, generated from `vbs_amd.synth._RINGS` (radius, count,
    first angle) to 0.01 mm: a centre, rings of 6, 12, 18 and 24 markers and four markers on the axes.  It is NOT the sensor's
    own list of positions (coordinates ending in 5 round differently there and the slot order differs), so nothing measured on
    it is a statement about the sensor's layout; the conditioning of the sensor's neighbourhoods is not checked here.  [65, 2]."""
    pts = []
    for radius, count, a0 in _RINGS:
        for j in range(count):
            a = math.radians(a0 + 360.0 * j / count)
            pts.append((round(radius * math.cos(a) * 100) / 100, round(radius * math.sin(a) * 100) / 100))
    return np.array(pts, dtype=np.float64)


def grid_pos(m, pitch=2.0):
    """m positions on a square grid of `pitch` mm around the origin (`pose_oracle.grid_ref` without the dome)."""
    side = int(math.ceil(math.sqrt(m)))
    i = np.arange(m)
    return np.stack([(i % side - (side - 1) // 2) * pitch, (i // side - (side - 1) // 2) * pitch], axis=1).astype(np.float64)


def affine_field(pos, theta_deg, stretch, t, gz=(0.0, 0.0)):
    """d = (R(theta) S - I) p + t in float64 (in-plane), dZ = gz . p + t_Z.  -> d [m, 3], the 2 x 2 matrix G = R S - I."""
    th = math.radians(theta_deg)
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    G = R @ np.asarray(stretch, dtype=np.float64) - np.eye(2)
    d = np.zeros((pos.shape[0], 3))
    d[:, :2] = pos @ G.T + np.asarray(t[:2])
    d[:, 2] = pos @ np.asarray(gz, dtype=np.float64) + t[2]
    return d, G


def record(d, cols=4, flag=1.0):
    """[n, m, 3] displacements -> rec [n, m, cols] with every slot valid; columns >= 4 hold NaN."""
    n, m, _ = d.shape
    rec = np.full((n, m, cols), np.nan)
    rec[..., 0] = flag
    rec[..., 1:4] = d
    return rec


def poison(rec, dead, rng):
    """Clear the flag on the entries of `dead` [n, m] and fill their values with NaN / 1e30: they must never be read."""
    k = int(dead.sum())
    rec[..., 0][dead] = 0.0
    rec[..., 1:4][dead] = np.where(rng.random((k, 3)) < 0.5, np.nan, 1e30)
    return rec


def random_case(n, m, cols, seed, drop=0.2, thin=True):
    """A recording of n frames over m grid slots: a random affine field per frame plus 0.02 mm noise, any nonzero flag, `drop`
    dropouts, and (thin) the last four frames keeping only 3, 2, 1, 0 slots.  -> rec, pos."""
    rng = np.random.default_rng(seed)
    pos = grid_pos(m) + rng.integers(-64, 65, (m, 2)) / 256.0                 # (off the lattice: det is not a round number)
    d = np.zeros((n, m, 3))
    for f in range(n):
        S = np.array([[1.0 + rng.normal(0, 0.02), rng.normal(0, 0.01)], [0.0, 1.0 + rng.normal(0, 0.02)]])
        S[1, 0] = S[0, 1]
        d[f] = affine_field(pos, rng.uniform(-5, 5), S, rng.normal(0, 0.3, 3), rng.normal(0, 0.02, 2))[0]
    d += rng.normal(0.0, 0.02, d.shape)
    rec = record(d, cols)
    rec[..., 0] = rng.choice([1.0, 2.0, -1.0, 1e-300], (n, m))                # any nonzero flag is valid
    dead = rng.random((n, m)) < drop
    if thin:
        for k in range(4):
            f = n - 4 + k
            if f < 0:
                continue
            keep = np.flatnonzero(~dead[f])[:3 - k]
            dead[f] = True
            dead[f, keep] = False
    return poison(rec, dead, rng), pos


def drag_twist_table(n=48, seed=0, noise=0.02, drop=0.1):
    """float32 table [n, 65, 10] on the ring layout: the tool drags (t_X ramps 0 -> 0.5 mm) and twists (theta ramps 0 -> 3
    degrees) over the recording; `noise` mm on all axes, `drop` of the entries lose their 3-D point (NaN / 1e30 there).  Frame 0
    is the undisturbed start.  -> table, pos [65, 2] (float32-rounded, as the table holds them), t_X ramp [n], theta ramp [n]."""
    rng = np.random.default_rng(seed)
    pos = ring_layout().astype(np.float32).astype(np.float64)
    tx, th = np.linspace(0.0, 0.5, n), np.linspace(0.0, 3.0, n)
    xyz = np.zeros((n, 65, 3))
    for f in range(n):
        d, _ = affine_field(pos, th[f], np.eye(2), (tx[f], 0.0, 0.0))
        xyz[f, :, :2] = pos + d[:, :2]
    xyz += rng.normal(0.0, 1.0, xyz.shape) * noise
    xyz[0, :, :2], xyz[0, :, 2] = pos, 0.0
    t = np.zeros((n, 65, 10), dtype=np.float32)
    t[..., 0] = 3.0
    t[..., 6:9] = xyz.astype(np.float32)
    dead = rng.random((n, 65)) < drop
    dead[0] = False
    t[..., 0][dead] = 1.0
    t[..., 6:9][dead] = np.where(rng.random((int(dead.sum()), 3)) < 0.5, np.nan, 1e30).astype(np.float32)
    return t, pos, tx, th


def motion_analysis_cpu(table, taps, reject_k=0.0, min_coverage=0.5):
    """`pipeline.motion_analysis`'s grad, strain and trend on the CPU for a table all of whose slots are valid in frame 0: the
    restatements of the axis displacement, of the fit and of the FIR (`filter_oracle`), and `strain.invariants`' expressions."""
    import filter_oracle as FO
    from vbs_amd.filters import half_taps
    axis = FO.axis_total(table, 0)[0]
    pos = table[0, :, 6:8].astype(np.float64)
    grad, strain, _, _ = motion_series(axis, pos, None, reject_k)
    gf = FO.fir(grad, half_taps(taps), 3, min_coverage)
    ok = (gf[..., 0] == 3.0).all(axis=1)
    inv = invariants(gf[:, 0, 2], gf[:, 0, 3], gf[:, 1, 2], gf[:, 1, 3], gf[:, 2, 2], gf[:, 2, 3])
    trend = np.concatenate([ok[:, None].astype(np.float64), np.where(ok[:, None], inv, 0.0)], axis=1)
    return grad, strain, gf, trend


def rotated_disc(side=13, pitch=1.5, centre=(1.5, -1.5), radius=5.0, angle_deg=5.0, n=3):
    """A side x side grid of markers of which those within `radius` of `centre` are rotated about it by `angle_deg` and the
    rest is still, the same in each of n frames.  -> rec [n, side^2, 4], pos [side^2, 2], inside [side^2] bool."""
    i = np.arange(side * side)
    pos = np.stack([(i % side - side // 2) * pitch, (i // side - side // 2) * pitch], axis=1).astype(np.float64)
    c = np.asarray(centre, dtype=np.float64)
    inside = ((pos - c) ** 2).sum(axis=1) <= radius * radius
    d = np.zeros((side * side, 3))
    d[inside] = affine_field(pos[inside] - c, angle_deg, np.eye(2), (0.0, 0.0, 0.0))[0]
    return record(np.broadcast_to(d[None], (n,) + d.shape).copy()), pos, inside
