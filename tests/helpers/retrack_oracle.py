"""The re-tracking rule of include/vbs.h (vbs_retrack) as loops in NumPy float64: the same operations in the same order, so a
device result is compared bit for bit.  `match_sorted` is the definition (one walk over the candidate pairs sorted by
(d2, j, i)), `match_rounds` the parallel form the kernel runs (mutual best pairs, round after round); `legacy_track` restates the
per-frame rule of vbs_track for comparison; `scenario` builds the drag-plus-torsion recording both are judged on."""
import numpy as np

STATE_COLS, INFO_COLS, TABLE_COLS = 6, 4, 10
DEFAULTS = dict(gate=10.0, max_travel=np.inf, vel_gain=0.5, max_coast=5)


def initial_state(ref_xy):
    ref = np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    st = np.zeros((ref.shape[0], STATE_COLS), dtype=np.float64)
    st[:, 0:2] = ref
    return st


def candidates(q, ref, xy, gate, max_travel):
    """d2 [m, cnt] of the candidate pairs, -1 elsewhere.  q [m, 2] predictions, xy [cnt, 2] the frame's detections."""
    m, cnt = q.shape[0], xy.shape[0]
    d2 = np.full((m, cnt), -1.0)
    g2 = np.float64(gate) * np.float64(gate)
    travel = np.isfinite(max_travel)
    t2 = np.float64(max_travel) * np.float64(max_travel)
    with np.errstate(all="ignore"):
        for i in range(cnt):
            x, y = xy[i]
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            dx = q[:, 0] - x
            dy = q[:, 1] - y
            d = dx * dx + dy * dy
            ok = d <= g2
            if travel:
                tx = x - ref[:, 0]
                ty = y - ref[:, 1]
                ok &= tx * tx + ty * ty <= t2
            d2[ok, i] = d[ok]
    return d2


def match_sorted(d2):
    """The definition: the candidate pairs by (d2, j, i) ascending, a pair taken iff its slot and its detection are free."""
    m, cnt = d2.shape
    jj, ii = np.nonzero(d2 >= 0)
    order = np.lexsort((ii, jj, d2[jj, ii]))
    assign = np.full(m, -1, dtype=np.int32)
    taken = np.zeros(cnt, dtype=bool)
    for k in order:
        j, i = jj[k], ii[k]
        if assign[j] < 0 and not taken[i]:
            assign[j] = i
            taken[i] = True
    return assign


def match_rounds(d2, only_namers=False):
    """The parallel form: every free slot names its best free candidate by (d2, i), every free detection its best free slot by
    (d2, j) among ALL free slots that hold it as a candidate, mutual pairs are fixed.  Returns (assign, rounds).
    `only_namers`: the detection chooses among the slots that named it only - NOT equivalent, kept to show that it differs."""
    m, cnt = d2.shape
    assign = np.full(m, -1, dtype=np.int32)
    taken = np.zeros(cnt, dtype=bool)
    rounds = 0
    while True:
        free = np.nonzero(assign < 0)[0]
        named = {}
        for j in free:
            c = [(d2[j, i], i) for i in range(cnt) if d2[j, i] >= 0 and not taken[i]]
            if c:
                named[j] = min(c)[1]
        if not named:
            return assign, rounds
        rounds += 1
        fixed = []
        for i in set(named.values()):
            pool = [j for j in named if named[j] == i] if only_namers else [j for j in named if d2[j, i] >= 0]
            best = min((d2[j, i], j) for j in pool)[1]
            if named[best] == i:
                fixed.append((best, i))
        assert fixed, "the smallest remaining pair is mutual"
        for j, i in fixed:
            assign[j] = i
            taken[i] = True


def retrack(det, counts, ref_xy, gate=10.0, max_travel=np.inf, vel_gain=0.5, max_coast=5, state=None, match=match_sorted):
    """-> dict(assign int32 [n, m], table float32 [n, m, 10], dist2 float64 [n, m], info int32 [n, 4], state float64 [m, 6])."""
    det = np.asarray(det, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int32)
    ref = np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    n, max_det = det.shape[0], det.shape[1]
    m = ref.shape[0]
    st = initial_state(ref) if state is None else np.array(state, dtype=np.float64).reshape(m, STATE_COLS)
    px, py, vx, vy, age, seen = (st[:, c].copy() for c in range(STATE_COLS))
    assign = np.full((n, m), -1, dtype=np.int32)
    dist2 = np.full((n, m), -1.0)
    info = np.zeros((n, INFO_COLS), dtype=np.int32)
    table = np.zeros((n, m, TABLE_COLS), dtype=np.float32)
    vel_gain = np.float64(vel_gain)
    for f in range(n):
        k = age + 1.0
        with np.errstate(all="ignore"):
            q = np.stack([px + vx * k, py + vy * k], axis=1)
        used = counts[f] >= 0
        cnt = min(int(counts[f]), max_det) if used else 0
        d2 = candidates(q, ref, det[f, :cnt, 0:2], gate, max_travel)
        a = match(d2)
        a = a[0] if isinstance(a, tuple) else a
        for j in range(m):
            i = a[j]
            if i >= 0:
                x, y = det[f, i, 0], det[f, i, 1]
                if seen[j] == 1.0:
                    ux = (x - px[j]) / k[j]
                    uy = (y - py[j]) / k[j]
                    vx[j] = vx[j] + vel_gain * (ux - vx[j])
                    vy[j] = vy[j] + vel_gain * (uy - vy[j])
                px[j], py[j], age[j], seen[j] = x, y, 0.0, 1.0
                dist2[f, j] = d2[j, i]
                table[f, j, 0] = 1.0
                table[f, j, 1:6] = det[f, i, 0:5].astype(np.float32)
                table[f, j, 9] = np.float32(i)
            else:
                age[j] = age[j] + 1.0
                if age[j] > max_coast:
                    vx[j] = vy[j] = 0.0
        assign[f] = a
        has = (d2 >= 0).any(axis=1)
        best = np.full(m, -1, dtype=np.int64)                      # a slot's own best candidate by (d2, i): the first minimum
        if cnt:
            best[has] = np.where(d2 >= 0, d2, np.inf).argmin(axis=1)[has]
        info[f] = (int(used), int((a >= 0).sum()), int(has.sum()), int((has & (a != best)).sum()))
    return dict(assign=assign, table=table, dist2=dist2, info=info, state=np.stack([px, py, vx, vy, age, seen], axis=1))


def legacy_track(det, counts, ref_xy, min_dist=20.0):
    """vbs_track's rule: every ID takes the detection nearest to its FIRST-FRAME position, dropped beyond min_dist; frames alone,
    and nothing keeps two IDs from one detection.  -> assign int32 [n, m]."""
    det = np.asarray(det, dtype=np.float64)
    ref = np.asarray(ref_xy, dtype=np.float64).reshape(-1, 2)
    n, m = det.shape[0], ref.shape[0]
    assign = np.full((n, m), -1, dtype=np.int32)
    for f in range(n):
        cnt = max(min(int(counts[f]), det.shape[1]), 0)
        if cnt == 0:
            continue
        d = np.sqrt(((ref[:, None, :] - det[f, None, :cnt, 0:2]) ** 2).sum(axis=2))
        i = d.argmin(axis=1)
        keep = ~(d[np.arange(m), i] > min_dist)
        assign[f, keep] = i[keep]
    return assign


def ring_layout(pitch=40.0, rings=(6, 12, 18, 24), centre=(320.0, 240.0)):
    """1 + 6 + 12 + 18 + 24 markers on rings `pitch` apart around `centre`."""
    pts = [(0.0, 0.0)]
    for r, k in enumerate(rings, start=1):
        for t in range(k):
            a = 2.0 * np.pi * t / k
            pts.append((r * pitch * np.cos(a), r * pitch * np.sin(a)))
    return np.asarray(pts, dtype=np.float64) + np.asarray(centre, dtype=np.float64)


def trajectory(n=120, ramp=60, drag=45.0, torsion_deg=8.0, pitch=40.0, centre=(320.0, 240.0), rings=(6, 12, 18, 24)):
    """The ring layout dragged by `drag` px along x and turned by `torsion_deg` about its centre over the first `ramp` frames,
    then held: float64 [n, m, 2]."""
    ref0 = ring_layout(pitch, rings, centre)
    c = np.asarray(centre, dtype=np.float64)
    pos = np.zeros((n,) + ref0.shape)
    for f in range(n):
        s = min(f, ramp) / float(ramp)
        a = np.deg2rad(torsion_deg) * s
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        pos[f] = (ref0 - c) @ R.T + c + np.array([drag * s, 0.0])
    return pos


def scenario(n=120, ramp=60, drag=45.0, torsion_deg=8.0, noise=0.05, dropout=0.03, seed=0, pitch=40.0, centre=(320.0, 240.0),
             max_det=None, rings=(6, 12, 18, 24)):
    """The recording both rules are judged on: `trajectory` with noise on every detection, a share `dropout` of the detections
    after frame 0 removed, the order of the detections permuted in every frame.  -> (det [n, max_det, 6], counts [n], ref_xy
    [m, 2] = the detections of frame 0 in marker order, truth [n, m] = the detection index of marker j in frame f, or -1 where it
    dropped out)."""
    rng = np.random.default_rng(seed)
    pos = trajectory(n, ramp, drag, torsion_deg, pitch, centre, rings)
    m = pos.shape[1]
    max_det = m if max_det is None else max_det
    det = np.zeros((n, max_det, 6))
    counts = np.zeros(n, dtype=np.int32)
    truth = np.full((n, m), -1, dtype=np.int32)
    ref_xy = None
    for f in range(n):
        p = pos[f] + rng.normal(0.0, noise, size=(m, 2))
        keep = np.ones(m, dtype=bool) if f == 0 else rng.random(m) >= dropout
        ids = np.nonzero(keep)[0]
        ids = ids[rng.permutation(ids.size)]
        counts[f] = ids.size
        det[f, :ids.size, 0:2] = p[ids]
        det[f, :ids.size, 2] = 12.0
        det[f, :ids.size, 3] = 11.0
        det[f, :ids.size, 4] = 30.0
        det[f, :ids.size, 5] = np.arange(1, ids.size + 1)
        truth[f, ids] = np.arange(ids.size)
        if f == 0:
            ref_xy = p.copy()
    return det, counts, ref_xy, truth


def score(assign, truth):
    """-> (wrong, missed): rows that name another detection than the marker's own (or one where it dropped out), and rows left
    empty although the marker was detected."""
    wrong = int(((assign >= 0) & (assign != truth)).sum())
    missed = int(((assign < 0) & (truth >= 0)).sum())
    return wrong, missed
