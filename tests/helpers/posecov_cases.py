"""Recordings the tests of `vbs_pose_cov` share (`tests/test_posecov_host.py`, `tests/test_gpu_posecov.py`): tables whose pixel
columns and 3-D columns belong together (X, Y, Z = the solve of Cx, Cy, major, as `uncert_cases.table` builds them), with what
the entry has to step around planted where a test can name it."""
import numpy as np

import pose_oracle as PO
import posecov_oracle as O
import uncert_cases as UC
import uncert_oracle as U

FLAG_TRACKED, FLAG_XYZ = 1, 2


def obs_cov(form, m, seed=0):
    """One covariance of (Cx, Cy, major) for all slots ("one") or one per slot."""
    if form == "one":
        return np.array([0.0025, 0.0004, -0.0003, 0.0036, 0.0002, 0.0064])
    rng = np.random.default_rng(50 + seed)
    A = rng.normal(size=(m, 3, 3)) * 0.05
    S = A @ A.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def _junk(rng, shape):
    return np.where(rng.random(shape) < 0.5, np.float32(np.nan), np.float32(1e30)).astype(np.float32)


def drop_rows(t, dead, rng):
    """The rows of `dead` [n, m] lose their 3-D point: half of them keep VBS_FLAG_TRACKED (despiked), the others lose the whole row;
    every cell that must then not be read holds NaN / 1e30."""
    k = int(dead.sum())
    tracked = rng.random(k) < 0.5
    t[..., 0][dead] = tracked.astype(np.float32) * FLAG_TRACKED
    t[..., 6:9][dead] = _junk(rng, (k, 3))
    pix = t[..., 1:4][dead]
    t[..., 1:4][dead] = np.where(tracked[:, None], pix, _junk(rng, (k, 3)))
    return t


def recording(cam, n, m, size=(640, 480), seed=0, drop=0.08, outliers=0, sparse=(), small=(), flat=()):
    """-> dict(table float32 [n, m, 10], ref_disp [m, 4], ref_xyz [m, 3], ref_rows float32 [2, m, 10], start).  ref_disp is the
    displacement between the two reference rows where both have a 3-D point; elsewhere its flag is 0 and its values and the
    slot's ref_xyz hold NaN / 1e30.
    drop      the fraction of rows without a 3-D point (the start frame and the reference rows included)
    outliers  slots per frame (from frame 2 on) whose diameter is off by a quarter: planted for the rejection
    sparse    (frame, k): only the first k common slots of that frame keep their point
    small     (frame, slot): the row carries VBS_FLAG_XYZ but a major of 4 px, below the entry's gate
    flat      frames whose X, Y, Z columns are the start frame's (with ref_disp = 0 the deviation is exactly zero)"""
    rng = np.random.default_rng(700 + seed)
    move = np.cumsum(rng.normal(size=(n, m, 3)) * np.array([0.2, 0.2, 0.05]), axis=0)
    for f in range(2, n):
        for s in rng.choice(m, size=min(outliers, m), replace=False):
            move[f, s, 2] += 3.5
    t = UC.table(cam, n, m, size, seed=seed, move=move, gaps=False, poison=False)
    start = n // 3
    for f in flat:
        t[f, :, 6:9] = t[start, :, 6:9]
    for col in (4, 5, 9):
        t[..., col] = _junk(rng, (n, m))
    dead = rng.random((n, m)) < drop
    for f, k in sparse:
        alive = np.flatnonzero(~dead[f] & ~dead[start])
        dead[f] = True
        dead[f, alive[:k]] = False
    for f, s in small:
        dead[f, s] = dead[start, s] = False
    drop_rows(t, dead, rng)
    for f, s in small:
        t[f, s, 3] = 4.0
    rr = UC.table(cam, 2, m, size, seed=seed + 31, move=np.cumsum(rng.normal(size=(2, m, 3)) * 0.3, axis=0), gaps=False, poison=False)
    for col in (4, 5, 9):
        rr[..., col] = _junk(rng, (2, m))
    drop_rows(rr, rng.random((2, m)) < drop / 2, rng)
    both = ((rr[..., 0].astype(np.int64) & FLAG_XYZ) != 0).all(axis=0)
    ref_disp = np.zeros((m, 4))
    ref_disp[:, 0] = both
    with np.errstate(all="ignore"):
        ref_disp[:, 1:] = np.where(both[:, None], rr[1, :, 6:9].astype(np.float64) - rr[0, :, 6:9].astype(np.float64), np.nan)
    if len(flat):
        ref_disp[:, 1:] = np.where(both[:, None], 0.0, np.nan)
    ref_xyz = np.where(both[:, None], PO.grid_ref(m), np.where(rng.random((m, 3)) < 0.5, np.nan, 1e30))
    return dict(table=t, ref_disp=ref_disp, ref_xyz=ref_xyz, ref_rows=rr, start=start)


# ---- a recording whose 3-D points are prescribed: the inverse of the solve ----------------------------------------------------------
def observe(c, X):
    """(Cx, Cy, major) [N, 3] of world points X [N, 3] under the camera c (`uncert_oracle.Cam`): the solve run backwards, the
    distortion applied forwards (the solve's five iterations undo it to their own accuracy)."""
    pc = np.stack([c.R[i, 0] * X[:, 0] + c.R[i, 1] * X[:, 1] + c.R[i, 2] * X[:, 2] for i in range(3)], axis=1) + c.T[None]
    h = pc[:, 2]
    du, dv = pc[:, 0] * c.fx / h, pc[:, 1] * c.fy / h
    S = np.sqrt(du * du + dv * dv + np.float64(c.f2_32))
    d = np.float64(c.f_avg32) * np.float64(c.k32) * S / h
    x, y = du / c.fx, dv / c.fy
    if c.has_dist:
        k = c.k
        r2 = x * x + y * y
        cd = 1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
        x, y = (x * cd + 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x), y * cd + k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y)
    return np.stack([x * c.fx + c.cx, y * c.fy + c.cy, d], axis=1)


def tilted_recording(cam, ref, tilt_deg, azimuth_deg=30.0, pixel_sigma=(0.05, 0.05), seed=0):
    """A float32 table [n, m, 10] of markers resting at `ref` [m, 3] (world, mm) whose frame f is tilted by tilt_deg[f]: dZ = a x +
    b y; the pixel columns carry Gaussian noise of `pixel_sigma` = (centre, diameter) px and X, Y, Z are their solve.  Frame 0 is
    the start.  -> (table, obs_cov [6])."""
    rng = np.random.default_rng(900 + seed)
    c = U.Cam(*cam)
    tilt = np.asarray(tilt_deg, dtype=np.float64)
    n, m = tilt.size, ref.shape[0]
    a = np.tan(np.radians(tilt)) * np.cos(np.radians(azimuth_deg))
    b = np.tan(np.radians(tilt)) * np.sin(np.radians(azimuth_deg))
    t = np.zeros((n, m, 10), dtype=np.float32)
    for f in range(n):
        X = ref.copy()
        X[:, 2] += a[f] * ref[:, 0] + b[f] * ref[:, 1]
        o = observe(c, X) + rng.normal(size=(m, 3)) * np.array([pixel_sigma[0], pixel_sigma[0], pixel_sigma[1]])
        t[f, :, 1:4] = o
    _, Xs, ok = U.primal(c, t[..., 1].ravel().astype(np.float64), t[..., 2].ravel().astype(np.float64),
                         t[..., 3].ravel().astype(np.float64))
    assert ok.all()
    t[..., 6:9] = Xs.reshape(n, m, 3)
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    s0, s1 = pixel_sigma[0] ** 2, pixel_sigma[1] ** 2
    return t, np.array([s0, 0.0, 0.0, s0, 0.0, s1])


# ---- a recording that reaches every exit of the rejection round ---------------------------------------------------------------------
# what frame f of `exit_recording` does after its first plane, in frame order
EXIT_FRAMES = ("no round", "refitted", "nothing rejected", "fewer than 3 kept", "kept set degenerate")
EXIT_RK = 1.0                # a slot is kept where r * r <= SSR / count


def second_round_exits(k, reject_k=EXIT_RK):
    """Which way every frame of the recording k leaves the rejection round, from the restatement alone (`pose_oracle._plane` on
    the end points of `posecov_oracle.end_points`): one of EXIT_FRAMES per frame."""
    sel = None if k.get("slots") is None else np.isin(np.arange(k["table"].shape[1]), k["slots"])
    pose, P, ok, used = O.end_points(k["table"], k["ref_disp"], k["ref_xyz"], k["start"], sel, False, 1.0, reject_k, (0, k["table"].shape[0]))
    cnt = ok.sum(axis=1)
    with np.errstate(all="ignore"):
        exists, _, _, _, ssr, r = PO._plane(P, ok, cnt)
        keep = ok & (r * r <= ((reject_k * reject_k) * (ssr / cnt.astype(np.float64)))[:, None])
    kc = keep.sum(axis=1)
    out = []
    for f in range(cnt.size):
        if not (reject_k > 0.0 and exists[f] and ssr[f] > 0.0):
            name = "no round"
        elif kc[f] >= cnt[f]:
            name = "nothing rejected"
        elif kc[f] < 3:
            name = "fewer than 3 kept"
        else:
            refit = bool(PO._plane(P[f:f + 1], keep[f:f + 1], kc[f:f + 1])[0][0])
            name = "refitted" if refit else "kept set degenerate"
        # the restatement's own outputs say the same: only a refit changes flag, n_used and the used set
        assert (pose[f, 0] == 2.0) == (name == "refitted") and pose[f, 7] == (kc[f] if name == "refitted" else cnt[f]), (f, name)
        assert np.array_equal(used[f], keep[f] if name == "refitted" else ok[f]) and (pose[f, 0] != 0.0) == bool(exists[f]), (f, name)
        out.append(name)
    return out


def exit_recording(cam, masked=False, seed=0):
    """VBS_POSECOV_GROUP + 1 = 5 frames of 7 slots (8 with `masked`: one more slot that a slot mask hides and that would tilt every
    plane), frame f leaving the rejection round by EXIT_FRAMES[f] at reject_k = EXIT_RK; asserted here from the restatement.
    The pixel columns are a recording's; X and Y never move, the reference positions are five on the line y = 0 and one on
    either side of it, and Z is set so that every sum of a frame is exact:
      0  the start frame: no deviation, SSR = 0, no round
      1  one slot lifted at the end of the line: it and two more go, four stay and are refitted
      2  the cross (+-1, 0), (0, +-1) alone at Z = +d, +d, -d, -d: the plane is flat, every r * r equals SSR / 4, all are kept
      3  that cross and the centre at Z = 0: only the centre is kept
      4  both slots off the line lifted: they go, and the five that stay lie on the line
    -> the dict of `recording`, with `slots` (None, or the seven under the mask)."""
    m, n, d = 8 if masked else 7, len(EXIT_FRAMES), 0.5
    k = recording(cam, n, m, seed=40 + seed, drop=0.0)
    pos = np.array([[-2.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    z = np.zeros((n, 7))
    z[1, 4] = 8.0
    z[2, [1, 3]], z[2, [5, 6]] = d, -d
    z[3] = z[2]
    z[4, [5, 6]] = 7.0
    t = k["table"]
    t[..., 0] = FLAG_TRACKED + FLAG_XYZ
    t[..., 6:8] = 0.0
    t[:, :7, 8] = z
    dead = np.zeros((n, m), dtype=bool)
    dead[2, [0, 2, 4]] = True
    dead[3, [0, 4]] = True
    drop_rows(t, dead, np.random.default_rng(41 + seed))
    k["ref_disp"] = np.concatenate([np.ones((m, 1)), np.zeros((m, 3))], axis=1)
    k["ref_xyz"] = np.concatenate([pos, np.full((7, 1), 0.5)], axis=1)
    k["slots"], k["start"] = None, 0
    if masked:
        t[1:, 7, 8] = 40.0
        k["ref_xyz"] = np.concatenate([k["ref_xyz"], [[3.0, 2.0, 0.5]]], axis=0)
        k["slots"] = np.arange(7)
    got = second_round_exits(k)
    assert got == list(EXIT_FRAMES), got
    return k
