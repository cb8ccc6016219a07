"""Oracle of the device PnP RANSAC (csrc/k_pnp.hip, csrc/pnp_math.h): NumPy float64, no torch.

The hypotheses are computed for all hypotheses of a problem at once (arrays of shape [H]), but every arithmetic operation is the
device's, in the device's order, on IEEE float64 - so counts, masks and the winner can be compared for equality.  (sin / cos of
the Gauss-Newton steps come from another maths library than the device's and may differ in the last place: the case generator
below keeps every decision 1e-6 px away from its threshold.)  The final fit is NOT the device's Levenberg-Marquardt but
scipy.optimize.least_squares on the same pixel residuals with every tolerance at its minimum: the independent optimum.

Also the case generator: 65-dot shell and 169 / 441-marker grids under random poses, with and without distortion, pixel noise,
gross outliers, untracked IDs, and the degenerate problems (3 valid points, collinear points)."""
import numpy as np

SAMPLE, GN_STEPS, POLAR_STEPS = 6, 10, 8
FEW_POINTS, NO_HYPOTHESIS = 1, 2
WELL_CONDITIONED = 1e-3        # smallest pivot of the 8 x 8 elimination / largest entry: above this a hypothesis counts as well-conditioned


def samples(n, iterations, seed):
    """The draw `engine.pnp_samples` makes: per hypothesis 6 distinct indices out of n (fewer than 6 points: all -1 = void)."""
    out = np.full((int(iterations), SAMPLE), -1, dtype=np.int32)
    if n >= SAMPLE:
        rng = np.random.default_rng(seed)
        for h in range(int(iterations)):
            out[h] = rng.choice(n, size=SAMPLE, replace=False)
    return out


def camera(K, dist):
    """(fx, fy, cx, cy, k1, k2, p1, p2, k3) as the device holds them: float32 values widened."""
    K = np.asarray(K, dtype=np.float32).reshape(3, 3).astype(np.float64)
    d = np.zeros(5)
    dd = np.asarray(dist, dtype=np.float32).ravel()[:5].astype(np.float64)
    d[:dd.size] = dd
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[2], d[3], d[4])


def normalise(u, v, cam):
    """track_common.h undistort_point (5 fixed-point iterations, back to pixels), then to normalised coordinates."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    if any(c != 0.0 for c in (k1, k2, p1, p2, k3)):
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dxx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dyy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dxx) * icd, (y0 - dyy) * icd
    uu, vu = x * fx + cx, y * fy + cy
    return (uu - cx) / fx, (vu - cy) / fy


def to_camera(R, t, X, Y, Z):
    return [((R[3 * i] * X + R[3 * i + 1] * Y) + R[3 * i + 2] * Z) + t[i] for i in range(3)]


def project(cam, R, t, X, Y, Z):
    """pnp_project: pixels and the in-front flag.  R = 9 arrays / scalars, t = 3."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    Pc = to_camera(R, t, X, Y, Z)
    front = Pc[2] > 0.0
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * rad + 2.0 * p1 * xy) + p2 * (r2 + 2.0 * x2)
    yd = (y * rad + p1 * (r2 + 2.0 * y2)) + 2.0 * p2 * xy
    return fx * xd + cx, fy * yd + cy, front


def err2(cam, R, t, X, Y, Z, uo, vo):
    with np.errstate(all="ignore"):
        u, v, front = project(cam, R, t, X, Y, Z)
        du, dv = u - uo, v - vo
        return np.where(front, du * du + dv * dv, np.inf)


def chain(Pc, ax, ay, az, bx, by, bz):
    Ju = [ay * -Pc[2] + az * Pc[1], ax * Pc[2] + az * -Pc[0], ax * -Pc[1] + ay * Pc[0], ax, ay, az]
    Jv = [by * -Pc[2] + bz * Pc[1], bx * Pc[2] + bz * -Pc[0], bx * -Pc[1] + by * Pc[0], bx, by, bz]
    return Ju, Jv


def accumulate(Ju, Jv, ru, rv, A, g):
    q = 0
    for i in range(6):
        for j in range(i, 6):
            A[q] = A[q] + (Ju[i] * Ju[j] + Jv[i] * Jv[j])
            q += 1
        g[i] = g[i] + (Ju[i] * ru + Jv[i] * rv)


def solve6(A, g, lam):
    """pnp_solve6: (d[6], ok)."""
    M = [[None] * 6 for _ in range(6)]
    L = [[None] * 6 for _ in range(6)]
    q = 0
    for i in range(6):
        for j in range(i, 6):
            M[i][j] = M[j][i] = A[q]
            q += 1
    for i in range(6):
        M[i][i] = M[i][i] + lam * M[i][i]
    ok = np.ones(np.shape(A[0]), dtype=bool)
    for j in range(6):
        s = M[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        bad = ~(s > 0.0)
        ok = ok & ~bad
        s = np.where(bad, 1.0, s)
        ljj = np.sqrt(s)
        L[j][j] = ljj
        for i in range(j + 1, 6):
            v = M[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / ljj
    y = [None] * 6
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    d = [None] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * d[k]
        d[i] = v / L[i][i]
    return d, ok


def apply_step(d, R, t):
    wx, wy, wz = d[0], d[1], d[2]
    th2 = wx * wx + wy * wy + wz * wz
    th = np.sqrt(th2)
    big = th > 1e-12
    ths, th2s = np.where(big, th, 1.0), np.where(big, th2, 1.0)
    a = np.where(big, np.sin(ths) / ths, 1.0)
    b = np.where(big, (1.0 - np.cos(ths)) / th2s, 0.5)
    E = [1.0 + b * (wx * wx - th2), b * (wx * wy) - a * wz, b * (wx * wz) + a * wy,
         b * (wx * wy) + a * wz, 1.0 + b * (wy * wy - th2), b * (wy * wz) - a * wx,
         b * (wx * wz) - a * wy, b * (wy * wz) + a * wx, 1.0 + b * (wz * wz - th2)]
    Rn = [None] * 9
    tn = [None] * 3
    for i in range(3):
        for j in range(3):
            Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j]
        tn[i] = ((E[3 * i] * t[0] + E[3 * i + 1] * t[1]) + E[3 * i + 2] * t[2]) + d[3 + i]
    return Rn, tn


def minimal(world, xn, yn, smp):
    """pnp_minimal for every hypothesis: (R [H,9], t [H,3], live [H], cond [H]).  smp [H,6] holds usable indices (void ones are
    filtered by the caller through `live`)."""
    H = smp.shape[0]
    idx = np.arange(H)
    with np.errstate(all="ignore"):
        A = np.zeros((H, 8, 9))
        for p in range(4):
            X, Y, x, y = world[smp[:, p], 0], world[smp[:, p], 1], xn[smp[:, p]], yn[smp[:, p]]
            A[:, 2 * p, 0], A[:, 2 * p, 1], A[:, 2 * p, 2] = X, Y, 1.0
            A[:, 2 * p, 6], A[:, 2 * p, 7], A[:, 2 * p, 8] = -(x * X), -(x * Y), x
            A[:, 2 * p + 1, 3], A[:, 2 * p + 1, 4], A[:, 2 * p + 1, 5] = X, Y, 1.0
            A[:, 2 * p + 1, 6], A[:, 2 * p + 1, 7], A[:, 2 * p + 1, 8] = -(y * X), -(y * Y), y
        amax = np.abs(A[:, :, :8]).reshape(H, -1).max(axis=1)
        pmin = np.full(H, np.inf)
        for k in range(8):
            sub = np.abs(A[:, k:, k])
            piv = sub.argmax(axis=1) + k                 # the first maximum, as the device's strict >
            best = sub.max(axis=1)
            rk, rp = A[idx, k, :].copy(), A[idx, piv, :].copy()
            A[idx, k, :], A[idx, piv, :] = rp, rk
            pmin = np.where(best < pmin, best, pmin)
            pv = np.where(best > 0.0, A[:, k, k], 1.0)
            for r in range(k + 1, 8):
                f = A[:, r, k] / pv
                A[:, r, k + 1:] = A[:, r, k + 1:] - f[:, None] * A[:, k, k + 1:]
        cond = pmin / amax
        live = pmin > 1e-9 * amax
        h = [None] * 8
        for i in range(7, -1, -1):
            v = A[:, i, 8]
            for j in range(i + 1, 8):
                v = v - A[:, i, j] * h[j]
            h[i] = v / A[:, i, i]
        n1 = np.sqrt((h[0] * h[0] + h[3] * h[3]) + h[6] * h[6])
        n2 = np.sqrt((h[1] * h[1] + h[4] * h[4]) + h[7] * h[7])
        sc = 0.5 * (n1 + n2)
        live &= sc > 0.0
        sc = 1.0 / sc
        M = [None] * 9
        M[0], M[3], M[6] = h[0] * sc, h[3] * sc, h[6] * sc
        M[1], M[4], M[7] = h[1] * sc, h[4] * sc, h[7] * sc
        t = [h[2] * sc, h[5] * sc, sc]
        M[2] = M[3] * M[7] - M[6] * M[4]
        M[5] = M[6] * M[1] - M[0] * M[7]
        M[8] = M[0] * M[4] - M[3] * M[1]
        for _ in range(POLAR_STEPS):
            C = [M[4] * M[8] - M[5] * M[7], M[5] * M[6] - M[3] * M[8], M[3] * M[7] - M[4] * M[6],
                 M[2] * M[7] - M[1] * M[8], M[0] * M[8] - M[2] * M[6], M[1] * M[6] - M[0] * M[7],
                 M[1] * M[5] - M[2] * M[4], M[2] * M[3] - M[0] * M[5], M[0] * M[4] - M[1] * M[3]]
            det = (M[0] * C[0] + M[1] * C[1]) + M[2] * C[2]
            live &= det > 1e-12
            M = [0.5 * (M[i] + C[i] / det) for i in range(9)]
        R = M
        for _ in range(GN_STEPS):
            N = [np.zeros(H) for _ in range(21)]
            g = [np.zeros(H) for _ in range(6)]
            for p in range(SAMPLE):
                P = world[smp[:, p]]
                Pc = to_camera(R, t, P[:, 0], P[:, 1], P[:, 2])
                live &= Pc[2] > 0.0
                iz = 1.0 / Pc[2]
                x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
                zero = np.zeros(H)
                Ju, Jv = chain(Pc, iz, zero, -(x * iz), zero, iz, -(y * iz))
                accumulate(Ju, Jv, x - xn[smp[:, p]], y - yn[smp[:, p]], N, g)
            d, ok = solve6(N, g, 0.0)
            live &= ok
            R, t = apply_step(d, R, t)
        R, t = np.stack(R, axis=1), np.stack(t, axis=1)
        live &= np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1)
    return R, t, live, cond


def solve(world, image, valid, K, dist, smp, reproj_px=8.0):
    """One problem as the two kernels solve it, up to the winner.  world [N,3], image [N,2], valid [N] bool, smp [H,6]."""
    world = np.asarray(world, dtype=np.float64)
    image = np.asarray(image, dtype=np.float64)
    n = len(world)
    cam = camera(K, dist)
    valid = np.asarray(valid, dtype=bool) & np.isfinite(image).all(axis=1)
    img = np.where(valid[:, None], image, 0.0)
    xn, yn = normalise(img[:, 0], img[:, 1], cam)
    smp = np.asarray(smp, dtype=np.int64)
    H = len(smp)
    live = ((smp >= 0) & (smp < n)).all(axis=1)
    s = np.where(live[:, None], smp, 0)
    live &= valid[s].all(axis=1)
    for k in range(SAMPLE):
        for j in range(k):
            live &= s[:, j] != s[:, k]
    R, t, ok, cond = minimal(world, xn, yn, s)
    live &= ok
    reproj2 = reproj_px * reproj_px
    e2 = err2(cam, [R[:, i:i + 1] for i in range(9)], [t[:, i:i + 1] for i in range(3)],
              world[None, :, 0], world[None, :, 1], world[None, :, 2], img[None, :, 0], img[None, :, 1])      # [H,N]
    inl = (e2 <= reproj2) & valid[None, :]
    count = np.where(live, inl.sum(axis=1), -1).astype(np.int32)
    out = {"count": count, "R": R, "t": t, "cond": cond, "valid": valid, "cam": cam, "n_valid": int(valid.sum())}
    if out["n_valid"] < 4:
        out.update(status=FEW_POINTS, winner=-1)
        return out
    if count.max() < 0:
        out.update(status=NO_HYPOTHESIS, winner=-1)
        return out
    w = int(np.argmax(count))                              # first maximum = a sequential "strictly better" scan
    out.update(status=0, winner=w, mask=inl[w], Rw=R[w].reshape(3, 3), tw=t[w], err_w=np.sqrt(e2[w]))
    return out


def rodrigues(w):
    th = float(np.linalg.norm(w))
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def pixel_errors(cam, R, t, world, image):
    """|projection - observation| in pixels per point (inf behind the camera)."""
    R = np.asarray(R, dtype=np.float64).reshape(9)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    return np.sqrt(err2(cam, R, t, world[:, 0], world[:, 1], world[:, 2], image[:, 0], image[:, 1]))


def residuals(cam, R, t, world, image):
    R = np.asarray(R, dtype=np.float64).reshape(9)
    u, v, _ = project(cam, R, np.asarray(t).reshape(3), world[:, 0], world[:, 1], world[:, 2])
    return np.concatenate([u - image[:, 0], v - image[:, 1]])


def cost(cam, R, t, world, image, mask):
    r = residuals(cam, R, t, world[mask], image[mask])
    return float(r @ r)


def refine(sol, world, image):
    """The independent optimum on the winner's inliers: scipy least_squares, every tolerance at its minimum."""
    from scipy.optimize import least_squares
    world, image = np.asarray(world, dtype=np.float64), np.asarray(image, dtype=np.float64)
    m = sol["mask"]
    R0, t0, cam = sol["Rw"], sol["tw"], sol["cam"]

    def fun(p):
        return residuals(cam, rodrigues(p[:3]) @ R0, p[3:], world[m], image[m])

    # central differences: with forward ones the fit stalls some 1e-8 of the cost short of the optimum.  The rotation is
    # re-centred on each pass so that its parameters stay where the differences are taken, at zero
    eps = np.finfo(np.float64).eps
    x = np.concatenate([np.zeros(3), t0])
    for _ in range(3):
        best = least_squares(fun, x, method="trf", jac="3-point", x_scale="jac", xtol=eps, ftol=eps, gtol=eps, max_nfev=2000)
        R0 = rodrigues(best.x[:3]) @ R0
        x = np.concatenate([np.zeros(3), best.x[3:]])
    best.x = x
    R, t = rodrigues(best.x[:3]) @ R0, best.x[3:]
    e = pixel_errors(cam, R, t, world, image)
    return {"R": R, "t": t, "cost": float(best.fun @ best.fun), "mean_error": float(e[sol["valid"]].mean()),
            "inlier_rms": float(np.sqrt((e[m] ** 2).mean()))}


def rotation_angle_deg(Ra, Rb):
    D = np.asarray(Ra, dtype=np.float64).reshape(3, 3) @ np.asarray(Rb, dtype=np.float64).reshape(3, 3).T
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])      # sin: exact near zero, unlike arccos
    return float(np.degrees(np.arctan2(s, (np.trace(D) - 1.0) / 2.0)))


# ---- cases -------------------------------------------------------------------------------------------------------------------
RING_COUNTS = (1, 6, 12, 18, 24, 4)


def shell_layout():
    """65 dots: rings of 1 + 6 + 12 + 18 + 24 + 4, ring k at radius 3.3 k mm, every ring starting on the +X axis (so that 11 dots
    lie on the X axis: the collinear case), Z rising with r^2 (a shallow shell)."""
    pts = []
    for k, cnt in enumerate(RING_COUNTS):
        for j in range(cnt):
            a = 2.0 * np.pi * j / cnt
            pts.append((3.3 * k * np.cos(a), 3.3 * k * np.sin(a)))
    xy = np.round(np.asarray(pts), 6) + 0.0
    return np.column_stack([xy, np.round(0.012 * (xy ** 2).sum(axis=1), 6)])


def grid_layout(n, pitch):
    c = (np.arange(n) - (n - 1) / 2.0) * pitch
    X, Y = np.meshgrid(c, c)
    xy = np.column_stack([X.ravel(), Y.ravel()])
    return np.column_stack([xy, np.round(0.008 * (xy ** 2).sum(axis=1), 6)])


LAYOUTS = {"shell65": shell_layout, "grid169": lambda: grid_layout(13, 2.4), "grid441": lambda: grid_layout(21, 1.4)}
K_CASES = np.array([[1200.0, 0, 640.0], [0, 1195.0, 512.0], [0, 0, 1]], dtype=np.float32)
DIST_ON = np.array([-0.12, 0.06, 0.0011, -0.0008, 0.01], dtype=np.float32)
DIST_OFF = np.zeros(5, dtype=np.float32)


def collinear_indices(world):
    return np.nonzero(world[:, 1] == 0.0)[0]


def random_pose(rng):
    """Within +-15 degrees about a random axis and +-3 mm around a camera 40 mm away."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R = rodrigues(axis * np.radians(rng.uniform(-15.0, 15.0)))
    return R, np.array([0.0, 0.0, 40.0]) + rng.uniform(-3.0, 3.0, size=3)


def make_problem(world, dist, rng, noise, outliers, untracked, kind="regular"):
    n = len(world)
    cam = camera(K_CASES, dist)
    R, t = random_pose(rng)
    u, v, front = project(cam, R.reshape(9), t, world[:, 0], world[:, 1], world[:, 2])
    assert front.all()
    uv = np.column_stack([u, v])
    if noise:
        uv = uv + rng.normal(scale=noise, size=uv.shape)
    out = np.zeros(n, dtype=bool)
    if outliers:
        out[rng.choice(n, size=int(round(outliers * n)), replace=False)] = True
        a = rng.uniform(0, 2 * np.pi, size=n)
        r = rng.uniform(15.0, 40.0, size=n)
        uv = uv + np.where(out[:, None], np.column_stack([r * np.cos(a), r * np.sin(a)]), 0.0)
    valid = np.ones(n, dtype=bool)
    if untracked:
        valid[rng.choice(n, size=max(3, n // 12), replace=False)] = False
    if kind == "three":
        valid[:] = False
        valid[rng.choice(n, size=3, replace=False)] = True
    elif kind == "collinear":
        valid[:] = False
        valid[collinear_indices(world)] = True
    uv = uv.astype(np.float32).astype(np.float64)          # what a tracker table can hold: both input forms carry the same values
    return {"R": R, "t": t, "image": uv, "valid": valid, "outlier": out, "noise": noise, "kind": kind,
            "true_inliers": valid & ~out, "exact": kind == "regular" and not noise and not outliers}


def make_batch(layout, dist_on, iterations=1000, seed=0, reproj_px=8.0):
    """One call's worth of problems (they share world points, camera and samples): noise x outliers x untracked, with the two
    degenerate problems in the middle.  Every regular problem satisfies the preconditions the equality tests rest on - under
    the helper's winning pose no valid point's error lies within 1e-6 px of reproj_px, and the winner's inliers are exactly the
    true inliers - or is generated again from the next seed.  Returns the problems with the helper's solution attached."""
    world = LAYOUTS[layout]()
    dist = DIST_ON if dist_on else DIST_OFF
    smp = samples(len(world), iterations, seed)
    kinds = []
    for noise in (0.0, 0.3):
        for outliers in (0.0, 0.2):
            for untracked in (False, True):
                kinds.append((noise, outliers, untracked, "regular"))
    kinds.insert(3, (0.3, 0.0, False, "three"))
    kinds.insert(6, (0.3, 0.0, False, "collinear"))
    problems = []
    for k, (noise, outliers, untracked, kind) in enumerate(kinds):
        for attempt in range(50):
            rng = np.random.default_rng([seed, k, attempt, len(world), int(dist_on)])
            p = make_problem(world, dist, rng, noise, outliers, untracked, kind)
            sol = solve(world, p["image"], p["valid"], K_CASES, dist, smp, reproj_px)
            if kind == "regular":
                if sol["status"] != 0:
                    continue
                e = sol["err_w"][sol["valid"]]
                if np.abs(e - reproj_px).min() <= 1e-6 or not np.array_equal(sol["mask"], p["true_inliers"]):
                    continue
            p["sol"] = sol
            break
        else:
            raise AssertionError(f"no case for {layout} {kinds[k]} within 50 seeds")
        problems.append(p)
    return {"world": world, "K": K_CASES, "dist": dist, "samples": smp, "problems": problems, "layout": layout,
            "reproj_px": reproj_px}


def all_batches(iterations=1000, seed=0):
    return [make_batch(layout, d, iterations, seed) for layout in LAYOUTS for d in (False, True)]
