"""Cases for the first-frame identity assignment (`k_assign_ids`, csrc/k_ids.hip; `ids.assign_ids`; `oracle.process_first_frame`).

Every coordinate is an integer multiple of 1/16 px in [0, 4096): the case holds the integer 16ths (`pts`, int64 [n, 2], in
detection order) and `xy(case)` divides by 16.0.  Differences, squares (< 2^33) and the coordinate sums of up to 1024 points
are then exact in float64, square roots and the mean's division are correctly rounded on every side, equal integers give
bit-equal radii, two distinct directions differ by at least 1 / (2 * 65536^2) = 1.2e-10 rad (five orders above an ulp of an
angle), and collinear points on one ray have the same real vy / vx.  So every expected value is decided by integer arithmetic
(`ids_oracle.py`) and no comparison hangs on the last bit of an `atan2`, a `sqrt` or a sum.

kind:
  "margin"  the two smallest distances to the mean are equal or differ by more than 1e-9 relative, and the exact-optimal cuts
            are unique and those of the float64 DP (both asserted in tests/test_ids_host.py): every side must give the exact
            oracle's table, detection order within an exact angle tie included;
  "tie"     regular lattices and rings of equal radii, where the DP has exactly tied optima and "first minimum = smallest
            split point" decides among float64 sums: the expected value is the host restatement bit for bit, the centre is the
            oracle's, and the cuts must be exactly optimal;
  "host"    IDS_MAXN-sized clouds, where the 60-digit DP takes too long: the host restatements only.
Fixed seeds; CASES is a list of dicts {name, group, kind, pts, layers}, BY_NAME the same by name."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ids_oracle as X                                        # noqa: E402

LIM = 4096 * 16
MODES = ("as_written", "full")
CASES = []


def _add(name, group, kind, pts, layers):
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    assert pts.size and pts.min() >= 0 and pts.max() < LIM, name
    CASES.append({"name": name, "group": group, "kind": kind, "pts": pts, "layers": int(layers)})


def _q(a):
    """float px -> integer 16ths"""
    return np.rint(np.asarray(a, dtype=np.float64) * 16.0).astype(np.int64)


def _cloud(rng, n, lo=0, hi=LIM):
    return rng.integers(lo, hi, (n, 2))


def _rings(rng, n_rings, jitter_px, short=False):
    """A centre and rings of 6k markers (6k - 0..2 when `short`) at 38 k px, as the sensor's pattern, with Gaussian jitter."""
    pts = [[320.0 + rng.normal(0, 1), 240.0 + rng.normal(0, 1)]]
    for k in range(1, n_rings + 1):
        cnt = 6 * k - (int(rng.integers(0, 3)) if short else 0)
        a0 = rng.uniform(0, 2 * np.pi)
        for j in range(cnt):
            a = a0 + 2 * np.pi * j / cnt
            pts.append([320 + 38 * k * np.cos(a) + rng.normal(0, jitter_px), 240 + 38 * k * np.sin(a) + rng.normal(0, jitter_px)])
    return _q(pts)


def _lattice(nx, ny, pitch=(40 * 16, 30 * 16), origin=(30 * 16, 20 * 16)):
    gx, gy = np.meshgrid(np.arange(nx) * pitch[0] + origin[0], np.arange(ny) * pitch[1] + origin[1])
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.int64)


def _circle_points(r):
    """Integer points on the circle a^2 + b^2 = r^2, by ascending angle in [0, pi) (the other half are their negatives)."""
    half = [(a, b) for a in range(-r, r + 1) for b in range(0, r + 1) if a * a + b * b == r * r and (b > 0 or a > 0)]
    half.sort(key=functools.cmp_to_key(X.cmp_angle))
    return half


def _exact_rings(rng):
    """1 + 6 + 12 + 18 + 24 markers on circles of EXACTLY equal radii 32.5 j px (integer points of a^2 + b^2 = 65^2 scaled by
    8 j sixteenths), centrally symmetric, so the mean is the centre marker exactly."""
    c = np.array([320 * 16, 240 * 16])
    half = _circle_points(65)
    assert len(half) == 18
    pts = [c]
    for j in range(1, 5):
        for i in range(3 * j):
            a, b = half[(i * 18) // (3 * j)]
            pts += [c + 8 * j * np.array([a, b]), c - 8 * j * np.array([a, b])]
    pts = np.array(pts)
    return pts[rng.permutation(len(pts))]


def _build():
    # tiny: no rest or one rest, k clamps to n - 1, M = 1, 2, 3
    rng = np.random.default_rng(101)
    for n in (1, 2, 3):
        p = _cloud(rng, n)
        for lay in (1, 5, 16):
            _add(f"tiny_n{n}_L{lay}", "tiny", "margin", p, lay)
    # fewer markers than layers: every marker its own layer
    rng = np.random.default_rng(102)
    for n in (4, 6, 17):
        p = _cloud(rng, n)
        for lay in (5, 16):
            _add(f"fewer_n{n}_L{lay}", "fewer", "margin", p, lay)
    # the 256-thread stride: nr = n - 1 on either side of 256
    rng = np.random.default_rng(103)
    for n in (255, 256, 257, 258):
        _add(f"stride_n{n}_L5", "stride", "margin", _cloud(rng, n), 5)
    # IDS_MAXN
    rng = np.random.default_rng(104)
    for n in (1023, 1024):
        p = _cloud(rng, n)
        for lay in (1, 16):
            _add(f"capacity_n{n}_L{lay}", "capacity", "host", p, lay)
    # layers sweep on 61 markers (1 + 6 + 12 + 18 + 24): jittered rings (margin) and rings of exactly equal radii (tie)
    jit = _rings(np.random.default_rng(105), 4, 1.5)
    exact = _exact_rings(np.random.default_rng(106))
    assert len(jit) == len(exact) == 61
    for lay in (1, 2, 3, 5, 6, 15, 16):
        _add(f"sweep_jitter_L{lay}", "sweep", "margin", jit, lay)
        _add(f"sweep_exact_L{lay}", "sweep", "margin" if lay == 1 else "tie", exact, lay)
    # centre ties: the four middle markers of an even lattice are exactly equidistant from the mean; 4 detection orders
    rng = np.random.default_rng(107)
    for side in (2, 4, 6):
        base = _lattice(side, side)
        orders = [np.arange(len(base)), np.arange(len(base))[::-1], rng.permutation(len(base)), rng.permutation(len(base))]
        for lay in (1, 3):
            for o, perm in enumerate(orders):
                _add(f"lattice{side}x{side}_L{lay}_o{o}", "centre_ties", "margin" if lay == 1 else "tie", base[perm], lay)
    # angle ties: 8 rays of exactly equal radii 40 j px, three markers on each; +-theta pairs; a marker at +pi
    rng = np.random.default_rng(108)
    c = np.array([300 * 16, 260 * 16])
    rays = [(5, 0), (3, 4), (0, 5), (-3, 4), (-5, 0), (-3, -4), (0, -5), (3, -4)]
    p = np.array([c] + [c + 128 * j * np.array(d) for d in rays for j in (1, 2, 3)])
    p = p[rng.permutation(len(p))]
    _add("rays8_L1", "angle_ties", "margin", p, 1)
    _add("rays8_L2", "angle_ties", "tie", p, 2)
    # three markers on one ray (and on its opposite), the pair (2, -1), (2, 1) sharing the smallest |angle| (no marker at angle
    # 0), one marker at +pi; the ray's members out of radius order in detection order
    off = [(0, 0)] + [(64 * t, 64 * t) for t in (3, 1, 2)] + [(-64 * t, -64 * t) for t in (2, 3, 1)] + \
          [(800, 400), (800, -400), (-800, -400), (-800, 400), (-500, 0)]
    p = c + np.array(off)
    for lay in (1, 2):
        _add(f"pm_theta_L{lay}", "angle_ties", "margin", p, lay)
        _add(f"pm_theta_rev_L{lay}", "angle_ties", "margin", p[::-1], lay)
    # on the centre: a second marker AT the centre marker (radius 0, atan2(0, 0) = 0), two coincident non-centre markers
    rng = np.random.default_rng(109)
    half = rng.integers(-2000, 2001, (6, 2))
    half = half[(half != 0).any(axis=1)]
    sym = np.concatenate([c + half, c - half])
    variants = {"dup_centre": np.concatenate([sym, [c, c]]),
                "dup_rest": np.concatenate([sym, [c], sym[:1], sym[len(half):len(half) + 1]]),
                "dup_both": np.concatenate([sym, [c, c], sym[1:2], sym[len(half) + 1:len(half) + 2]])}
    for tag, q in variants.items():
        q = q[rng.permutation(len(q))]
        for lay in (2, 5):
            _add(f"{tag}_L{lay}", "on_centre", "margin", q, lay)
    # detection order: one 40-marker cloud under 6 permutations
    rng = np.random.default_rng(110)
    p = _cloud(rng, 40, 0, 640 * 16)
    for o in range(6):
        _add(f"order_p{o}", "order", "margin", p if o == 0 else p[rng.permutation(40)], 5)
    # the bounded soak: clouds, jittered ring sets, jittered lattices; layers uniform in 1..16
    rng = np.random.default_rng(111)
    for i in range(40):
        _add(f"random_cloud{i:02d}", "random", "margin", _cloud(rng, int(rng.integers(1, 121)), 0, 640 * 16), int(rng.integers(1, 17)))
    for i in range(20):
        _add(f"random_rings{i:02d}", "random", "margin", _rings(rng, int(rng.integers(1, 6)), 2.0, short=True), int(rng.integers(1, 17)))
    for i in range(20):
        n = int(rng.integers(2, 12))
        lat = _lattice(n, n).astype(np.float64) / 16.0 + rng.normal(0, 0.5, (n * n, 2))
        _add(f"random_lattice{i:02d}", "random", "margin", _q(lat), int(rng.integers(1, 17)))


_build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(kind=None, group=None):
    return [c["name"] for c in CASES if (kind is None or c["kind"] == kind) and (group is None or c["group"] == group)]


def xy(case):
    """float64 [n, 2] px, exact"""
    return case["pts"].astype(np.float64) / 16.0


def markers(case):
    """The marker dicts the host restatements take."""
    return [{"center": (float(x), float(y)), "major_axis": 20.0, "minor_axis": 19.0, "angle": 0.0} for x, y in xy(case)]


def det_rows(case, max_markers, seed=0):
    """float64 [max_markers, 6] as `det`: columns 0, 1 of the first n rows are the markers, everything else is junk that must
    not be read (NaN and +-1e300)."""
    n = len(case["pts"])
    assert max_markers > n
    rng = np.random.default_rng(seed)
    det = rng.choice(np.array([np.nan, 1e300, -1e300]), size=(max_markers, 6))
    det[:n, :2] = xy(case)
    return det


@functools.lru_cache(maxsize=None)
def report(name):
    """The exact oracle's analysis of a case, computed once per process and never changed."""
    case = BY_NAME[name]
    return X.analyse(case["pts"].tolist(), case["layers"], cluster=case["kind"] != "host")


@functools.lru_cache(maxsize=None)
def exact_table(name, id_mode):
    """(ids int64 [M, 2] in dict order, xy float64 [M, 2]) of the exact oracle."""
    keys, slots = X.table(report(name), id_mode)
    ids = np.array(keys, dtype=np.int64).reshape(-1, 2)
    out = xy(BY_NAME[name])[np.array(slots, dtype=np.int64)]
    ids.setflags(write=False)
    out.setflags(write=False)
    return ids, out


def arrays(table):
    """(ids int64 [M, 2], xy float64 [M, 2]) of a restatement's dict, in dict order."""
    ids = np.array(list(table.keys()), dtype=np.int64).reshape(-1, 2)
    out = np.array([[v["Ox"], v["Oy"]] for v in table.values()], dtype=np.float64).reshape(-1, 2)
    return ids, out


def layer_r2(case, ids, out_xy):
    """Integer r2 (256 * radius^2 about slot 0) of the markers of a `full` table, grouped by layer: what `ids_oracle.sse_of_groups`
    takes to price the cuts a table implies.  The coordinates are exact sixteenths, so the way back to integers is too."""
    p = np.rint(np.asarray(out_xy) * 16.0).astype(np.int64)
    assert np.array_equal(p / 16.0, out_xy)
    groups = {}
    for (lay, _), q in zip(np.asarray(ids).tolist()[1:], p[1:].tolist()):
        groups.setdefault(lay, []).append((q[0] - int(p[0, 0])) ** 2 + (q[1] - int(p[0, 1])) ** 2)
    return [groups[k] for k in sorted(groups)]
