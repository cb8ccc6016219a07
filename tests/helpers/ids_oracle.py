"""Exact reference of the first-frame identity assignment (`_process_first_frame`, marker_detection.py:275-347, as
`vbs_amd/ids.py` and `oracle/stages.py::process_first_frame` state it) for markers whose coordinates are integer multiples of
1/16 px.  Python `int`, `fractions` and `decimal` at 60 digits only: no float, no `atan2`.

Input everywhere: `pts`, a sequence of (X, Y) integer 16ths of a pixel in detection order.

 * centre: argmin of |n p - sum p|^2 (n^2 * 256 times the squared distance to the mean), lowest index on exact ties;
 * rest = every other marker in detection order, v = p - centre, r2 = vx^2 + vy^2 (256 times the squared radius);
 * radius order: stable sort by r2;  angle order: numpy's range (-pi, pi] decided by the half-plane and the sign of the integer
   cross product - vy < 0 | angle 0 (vy == 0, vx >= 0, the point ON the centre included) | vy > 0 | +pi (vy == 0, vx < 0);
   |angle| order: the same after vy -> |vy|;
 * clustering: the DP over contiguous partitions of the sorted radii sqrt(r2) / 16 (Decimal), k = max(1, min(layers, n - 1))
   non-empty clusters, first minimum (smallest split point) on ties closer than 1e-40 relative - which at 60 digits means exact;
 * table: (0,0), then layer-major; `full`: members by angle (stable), index 0 at the first member of smallest |angle|;
   `as_written`: one slot per non-empty layer holding its last member in detection order.
Every exact tie the statement's float restatements could trip over is reported by `analyse`."""
from decimal import Decimal, localcontext
from fractions import Fraction
from functools import cmp_to_key

PREC = 60
_TIE = Decimal("1e-40")


# ---------------------------------------------------------------------------------------------------------------------
def centre(pts):
    """(index of the centre marker, indices tied for it, the integer n^2 * 256 * d^2 of every marker)."""
    n = len(pts)
    sx = sum(int(p[0]) for p in pts)
    sy = sum(int(p[1]) for p in pts)
    d2 = [(n * int(x) - sx) ** 2 + (n * int(y) - sy) ** 2 for x, y in pts]
    m = min(d2)
    ties = [i for i, d in enumerate(d2) if d == m]
    return ties[0], ties, d2


def centre_margin(d2):
    """The margin condition on the centre: the two smallest distances to the mean are equal or differ by more than 1e-9
    relative.  (A single marker has no second distance.)"""
    if len(d2) < 2:
        return True
    a, b = sorted(d2)[:2]
    if a == b:
        return True
    with localcontext() as c:
        c.prec = PREC
        return 1 - (Decimal(a) / Decimal(b)).sqrt() > Decimal("1e-9")


def _cls(vx, vy):
    if vy < 0:
        return 0
    if vy > 0:
        return 2
    return 1 if vx >= 0 else 3


def cmp_angle(a, b):
    """-1 / 0 / +1 as atan2(a) is below / equal to / above atan2(b) in (-pi, pi]; a, b integer vectors (vx, vy)."""
    ca, cb = _cls(*a), _cls(*b)
    if ca != cb:
        return -1 if ca < cb else 1
    if ca in (1, 3):
        return 0
    cross = a[0] * b[1] - a[1] * b[0]          # > 0: b lies counter-clockwise of a within the open half-plane
    return -1 if cross > 0 else (1 if cross < 0 else 0)


def cmp_abs_angle(a, b):
    return cmp_angle((a[0], abs(a[1])), (b[0], abs(b[1])))


def _groups(idx, same):
    """Maximal runs of `idx` (already sorted so that equal items are adjacent) whose neighbours satisfy same(a, b)."""
    out, run = [], []
    for i in idx:
        if run and same(run[-1], i):
            run.append(i)
        else:
            if len(run) > 1:
                out.append(run)
            run = [i]
    if len(run) > 1:
        out.append(run)
    return out


# ---------------------------------------------------------------------------------------------------------------------
def radii(r2s):
    """Decimal radii in px of integer r2 (256 * radius^2)."""
    with localcontext() as c:
        c.prec = PREC
        return [Decimal(int(r)).sqrt() / 16 for r in r2s]


def sse_of_groups(groups):
    """Exact (60-digit) k-means objective of a partition given as lists of integer r2: sum over groups of
    sum r^2 - (sum r)^2 / m, with sum r^2 = sum r2 / 256 exact."""
    with localcontext() as c:
        c.prec = PREC
        tot = Decimal(0)
        for g in groups:
            if not g:
                continue
            s1 = sum(radii(g), Decimal(0))
            tot += Decimal(sum(int(r) for r in g)) / 256 - s1 * s1 / len(g)
        return tot


def kmeans_exact(r2_sorted, k):
    """The DP over contiguous partitions of ascending integer r2 into exactly k non-empty clusters (k <= len).
    Returns (cuts [0 = b_0 < b_1 < .. < b_k = n], optimal SSE as Decimal, number of optimal cut vectors)."""
    n = len(r2_sorted)
    assert 1 <= k <= n and all(r2_sorted[i] <= r2_sorted[i + 1] for i in range(n - 1))
    with localcontext() as c:
        c.prec = PREC
        r = radii(r2_sorted)
        s1, s2 = [Decimal(0)], [0]
        for i in range(n):
            s1.append(s1[-1] + r[i])
            s2.append(s2[-1] + int(r2_sorted[i]))
        inv = [None] + [Decimal(1) / m for m in range(1, n + 1)]
        s2d = [Decimal(v) / 256 for v in s2]

        def tol(v):
            return _TIE * (abs(v) + 1)

        prev = [Decimal(0)] + [None] * n                    # None = infeasible
        ways = [1] + [0] * n
        back = [[0] * (n + 1) for _ in range(k + 1)]
        for cl in range(1, k + 1):
            cur, cw = [None] * (n + 1), [0] * (n + 1)
            for j in range(cl, n - (k - cl) + 1):            # (later clusters need k - cl more values)
                best, bi, bw = None, 0, 0
                for i in range(cl - 1, j):
                    if prev[i] is None:
                        continue
                    d1 = s1[j] - s1[i]
                    cand = prev[i] + (s2d[j] - s2d[i]) - d1 * d1 * inv[j - i]
                    if best is None or cand < best - tol(best):
                        best, bi, bw = cand, i, ways[i]
                    elif abs(cand - best) <= tol(best):       # an exact tie: the first (smallest i) stays
                        bw += ways[i]
                cur[j], cw[j], back[cl][j] = best, bw, bi
            prev, ways = cur, cw
        cuts = [n]
        for cl in range(k, 0, -1):
            cuts.append(back[cl][cuts[-1]])
        cuts.reverse()
        return cuts, prev[n], ways[n]


def sse_of_cuts(r2_sorted, cuts):
    return sse_of_groups([r2_sorted[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


# ---------------------------------------------------------------------------------------------------------------------
def analyse(pts, num_layers, cluster=True):
    """Everything but the table: a dict with
      n, ci, centre_ties, centre_d2, rest (original indices, detection order), vec, r2 (per rest position),
      k, order (rest positions by ascending radius, stable), r2_sorted, cuts, sse, n_optimal, layer (per rest position, 1..k),
      radius_ties (groups of rest positions of equal r2), angle_ties {layer: groups of rest positions on one ray, each in
      detection order}, absmin {layer: rest positions sharing the layer's smallest |angle|, in angle order}.
    cluster=False stops before the DP (sizes where 60-digit arithmetic takes too long): no cuts / layer / per-layer reports."""
    pts = [(int(x), int(y)) for x, y in pts]
    n = len(pts)
    if n == 0:
        raise ValueError("No markers detected in first frame!")
    ci, cties, d2 = centre(pts)
    rest = [i for i in range(n) if i != ci]
    vec = [(pts[i][0] - pts[ci][0], pts[i][1] - pts[ci][1]) for i in rest]
    r2 = [vx * vx + vy * vy for vx, vy in vec]
    nr = len(rest)
    k = max(1, min(int(num_layers), nr))
    order = sorted(range(nr), key=lambda i: (r2[i], i))
    rep = {"n": n, "ci": ci, "centre_ties": cties, "centre_d2": d2, "rest": rest, "vec": vec, "r2": r2, "k": k,
           "num_layers": int(num_layers), "order": order, "r2_sorted": [r2[i] for i in order],
           "radius_ties": _groups(order, lambda a, b: r2[a] == r2[b])}
    if not cluster or nr == 0:
        rep.update({"cuts": [0, 0] if nr == 0 else None, "sse": Decimal(0) if nr == 0 else None, "n_optimal": 1 if nr == 0 else None,
                    "layer": [] if nr == 0 else None, "angle_ties": {}, "absmin": {}})
        return rep
    cuts, sse, nopt = kmeans_exact(rep["r2_sorted"], k)
    layer = [0] * nr
    for cl in range(k):
        for q in range(cuts[cl], cuts[cl + 1]):
            layer[order[q]] = cl + 1
    ang, absmin = {}, {}
    for lay in range(1, k + 1):
        mem = _sorted_members(vec, layer, lay)
        g = _groups(mem, lambda a, b: cmp_angle(vec[a], vec[b]) == 0)
        if g:
            ang[lay] = g
        if mem:
            lo = min(mem, key=cmp_to_key(lambda a, b: cmp_abs_angle(vec[a], vec[b])))
            absmin[lay] = [i for i in mem if cmp_abs_angle(vec[i], vec[lo]) == 0]
    rep.update({"cuts": cuts, "sse": sse, "n_optimal": nopt, "layer": layer, "angle_ties": ang, "absmin": absmin})
    return rep


def _sorted_members(vec, layer, lay):
    mem = [i for i in range(len(vec)) if layer[i] == lay]                  # detection order
    mem.sort(key=cmp_to_key(lambda a, b: cmp_angle(vec[a], vec[b])))      # stable: equal angles keep detection order
    return mem


def table(rep, id_mode):
    """The ID table in dict order: (keys [(layer, idx)], the ORIGINAL marker index each slot holds)."""
    if id_mode not in ("as_written", "full"):
        raise ValueError(id_mode)
    keys, slots = [(0, 0)], [rep["ci"]]
    rest, layer, vec = rep["rest"], rep["layer"], rep["vec"]
    for lay in range(1, rep["k"] + 1):
        mem = _sorted_members(vec, layer, lay)
        if not mem:
            continue
        if id_mode == "as_written":
            keys.append((lay, 0))
            slots.append(rest[max(mem)])                                   # last member in detection order
            continue
        start = 0                                                          # first member, in sorted order, of smallest |angle|
        for p in range(1, len(mem)):
            if cmp_abs_angle(vec[mem[p]], vec[mem[start]]) < 0:
                start = p
        for pos, i in enumerate(mem):                                      # dict order is the sorted order, not the index order
            keys.append((lay, (pos - start) % len(mem)))
            slots.append(rest[i])
    return keys, slots


def margin(rep, host_cuts=None):
    """The two margin conditions: (centre ok, the exact-optimal cuts are unique [and are `host_cuts`])."""
    uniq = rep["n_optimal"] == 1 and (host_cuts is None or list(host_cuts) == list(rep["cuts"]))
    return centre_margin(rep["centre_d2"]), uniq


def mean_is_exact(pts):
    """True when sum / n is a multiple of 2^-20 px in both coordinates: the float64 mean of the restatements is then exact, and
    exact centre ties are bit-equal distances on their side too."""
    n = len(pts)
    return all((Fraction(sum(int(p[a]) for p in pts), 16 * n) * (1 << 20)).denominator == 1 for a in (0, 1))
