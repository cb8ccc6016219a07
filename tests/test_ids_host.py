"""CPU tests of the first-frame identity assignment's references (no GPU): the exact integer oracle
(`tests/helpers/ids_oracle.py`) against brute force, the cases (`tests/helpers/ids_cases.py`) against the conditions their labels
claim, and the two float64 restatements - `ids.assign_ids` (the product's checker) and `oracle.process_first_frame` - against the
exact oracle wherever it decides, against each other wherever exactly tied optima leave the choice to float64 sums.
`tests/test_gpu_ids.py` holds `k_assign_ids` to the same expected values."""
import itertools
import os
import re
import sys
from decimal import Decimal

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import ids as I
from oracle import stages as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ids_cases as K                                         # noqa: E402
import ids_oracle as X                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, TIE, HOST = K.names("margin"), K.names("tie"), K.names("host")


def host_cuts(case, rep):
    """The cuts of the float64 DP `ids.kmeans_1d` on the radii as `ids.assign_ids` forms them about the oracle's centre."""
    if not rep["rest"]:
        return [0, 0]
    p = K.xy(case)
    rad = np.linalg.norm(p[rep["rest"]] - p[rep["ci"]], axis=1)
    lab = I.kmeans_1d(rad, case["layers"])
    srt = lab[np.argsort(rad, kind="stable")]
    assert (np.diff(srt) >= 0).all()
    return [0] + np.cumsum(np.bincount(srt, minlength=rep["k"])).tolist()


def both(case, mode):
    ms = K.markers(case)
    return K.arrays(I.assign_ids(ms, case["layers"], mode, "optimal")), K.arrays(O.process_first_frame(ms, case["layers"], mode, "optimal"))


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
def test_limits_are_in_the_header_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.IDS_MAX_MARKERS, L.IDS_MAX_LAYERS) == (defs["VBS_IDS_MAX_MARKERS"], defs["VBS_IDS_MAX_LAYERS"]) == (1024, 16)
    src = open(os.path.join(os.path.dirname(L.__file__), "csrc", "k_ids.hip")).read()
    assert re.search(r"#define\s+IDS_MAXN\s+VBS_IDS_MAX_MARKERS\b", src) and re.search(r"#define\s+IDS_MAXK\s+VBS_IDS_MAX_LAYERS\b", src)
    assert L.lib().vbs_assign_ids(None, None, None, 5, 0, None, None, 1, None, None) == L.VBS_EINVAL


def test_case_table_is_complete():
    """The groups and sizes the cases are there for."""
    def sizes(group):
        return sorted({(len(K.BY_NAME[n]["pts"]), K.BY_NAME[n]["layers"]) for n in K.names(group=group)})
    assert sizes("tiny") == [(n, lay) for n in (1, 2, 3) for lay in (1, 5, 16)]
    assert sizes("fewer") == [(n, lay) for n in (4, 6, 17) for lay in (5, 16)]
    assert sizes("stride") == [(n, 5) for n in (255, 256, 257, 258)]
    assert sizes("capacity") == [(n, lay) for n in (1023, L.IDS_MAX_MARKERS) for lay in (1, L.IDS_MAX_LAYERS)]
    assert {lay for _, lay in sizes("sweep")} == {1, 2, 3, 5, 6, 15, 16} and {n for n, _ in sizes("sweep")} == {61}
    assert sizes("centre_ties") == [(n, lay) for n in (4, 16, 36) for lay in (1, 3)] and len(K.names(group="centre_ties")) == 24
    assert len(K.names(group="order")) == 6 and len(K.names(group="random")) == 80
    rnd = [K.BY_NAME[n] for n in K.names(group="random")]
    assert {c["layers"] for c in rnd} == set(range(1, 17)) and all(1 <= len(c["pts"]) <= 127 for c in rnd)
    for c in K.CASES:
        assert c["pts"].dtype == np.int64 and c["pts"].min() >= 0 and c["pts"].max() < 4096 * 16
        det = K.det_rows(c, len(c["pts"]) + 3)
        assert np.array_equal(det[:len(c["pts"]), :2] * 16.0, c["pts"]) and not np.isfinite(det[len(c["pts"]):]).all()
        assert (~np.isfinite(det[:, 2:]) | (np.abs(det[:, 2:]) == 1e300)).all()


# ---------------------------------------------------------------------------------------------------------------------
def _partitions(n, k):
    """Every partition of range(n) into exactly k non-empty blocks (restricted growth strings)."""
    def rec(i, used, lab):
        if i == n:
            if used == k:
                yield lab
            return
        if used + (n - i) < k:
            return
        for b in range(min(used + 1, k)):
            yield from rec(i + 1, max(used, b + 1), lab + [b])
    return rec(0, 0, [])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 9])
def test_exact_dp_against_brute_force_over_all_partitions(n):
    """The DP searches contiguous partitions only; every partition of n <= 9 values (contiguous or not) confirms its optimum,
    and that it counts the optimal cut vectors right - on distinct values, on values with duplicates, on all-equal values."""
    rng = np.random.default_rng(n)
    sets = [sorted(int(v) for v in rng.integers(1, 10 ** 9, n)), sorted(int(v) for v in rng.integers(1, 4, n) ** 2 * 4096),
            [4225 * 64] * n]
    for r2 in sets:
        for k in range(1, n + 1):
            cuts, sse, nopt = X.kmeans_exact(r2, k)
            assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts[:-1], cuts[1:])) and len(cuts) == k + 1
            assert abs(X.sse_of_cuts(r2, cuts) - sse) <= Decimal("1e-40") * (sse + 1)
            best = min(X.sse_of_groups([[r2[i] for i in range(n) if lab[i] == b] for b in range(k)]) for lab in _partitions(n, k))
            assert abs(best - sse) <= Decimal("1e-40") * (sse + 1), (r2, k)
            tied = [c for c in itertools.combinations(range(1, n), k - 1)
                    if abs(X.sse_of_cuts(r2, [0, *c, n]) - sse) <= Decimal("1e-40") * (sse + 1)]
            # first minimum = smallest split point, decided from the last cluster backwards
            assert nopt == len(tied) and list(min(tied, key=lambda c: c[::-1])) == cuts[1:-1]


def test_exact_angle_order_on_the_axes_and_around_pi():
    v = [(-5, -1), (-1, -5), (0, -3), (4, -1), (7, 0), (0, 0), (4, 1), (0, 2), (-1, 5), (-9, 1), (-2, 0), (-6, 0)]
    for a, b in itertools.combinations(range(len(v)), 2):
        want = 0 if {a, b} in ({4, 5}, {10, 11}) else -1
        assert X.cmp_angle(v[a], v[b]) == want and X.cmp_angle(v[b], v[a]) == -want, (v[a], v[b])
    assert X.cmp_abs_angle((3, -4), (3, 4)) == 0 and X.cmp_abs_angle((3, -4), (3, 5)) == -1
    assert X.cmp_angle((65535, 1), (65534, 1)) == -1 and X.cmp_angle((2, 1), (4, 2)) == 0 and X.cmp_angle((2, 1), (-4, -2)) == 1


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MARGIN)
def test_margin_conditions_hold(name):
    case, rep = K.BY_NAME[name], K.report(name)
    centre_ok, unique = X.margin(rep, host_cuts(case, rep))
    assert centre_ok, "the two smallest distances to the mean are closer than 1e-9 relative without being equal"
    assert unique, (rep["n_optimal"], rep["cuts"], host_cuts(case, rep))
    assert rep["k"] == max(1, min(case["layers"], rep["n"] - 1))
    if len(rep["centre_ties"]) > 1:                           # an exact tie is only bit-equal on the float side with an exact mean
        assert X.mean_is_exact(case["pts"].tolist())


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", MARGIN)
def test_restatements_equal_the_exact_oracle_on_margin_cases(name, mode):
    """Keys in dict order and float64 coordinates bit for bit - detection order within every exact angle tie included, which
    is np.arctan2 returning equal bits for collinear points under a stable sort."""
    want = K.exact_table(name, mode)
    host, orc = both(K.BY_NAME[name], mode)
    assert same(host, want), "ids.assign_ids"
    assert same(orc, want), "oracle.process_first_frame"


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", TIE + [n for n in HOST if n.endswith("_L1")] + K.names(group="stride"))
def test_restatements_equal_each_other(name, mode):
    """Where exactly tied optima leave the cuts to the float64 sums (and at the sizes the exact DP is too slow for) the two
    restatements - one vectorised, one a scalar loop - must still agree bit for bit; the centre is the exact oracle's, and on
    tie cases the cuts they chose are exactly optimal.  (`oracle.process_first_frame`'s scalar DP takes 12 s at 1024 markers
    and 16 layers, so that size is left to `ids.assign_ids` alone.)"""
    case, rep = K.BY_NAME[name], K.report(name)
    host, orc = both(case, mode)
    assert same(host, orc)
    assert host[1][0].tobytes() == K.xy(case)[rep["ci"]].tobytes()
    if case["kind"] == "tie" and mode == "full":
        assert rep["n_optimal"] >= 1 and X.centre_margin(rep["centre_d2"])
        got = X.sse_of_groups(K.layer_r2(case, *host))
        assert abs(got - rep["sse"]) <= Decimal("1e-12") * rep["sse"]
        assert sum(len(g) for g in K.layer_r2(case, *host)) == rep["n"] - 1


def test_every_group_holds_the_property_it_is_named_for():
    reps = {g: [(K.BY_NAME[n], K.report(n)) for n in K.names(group=g)] for g in {c["group"] for c in K.CASES}}
    # an exact centre tie (four markers, the first in detection order wins - and it is another marker in another order)
    lat = reps["centre_ties"]
    assert all(len(r["centre_ties"]) == 4 and r["ci"] == min(r["centre_ties"]) for _, r in lat)
    for side in (4, 16, 36):
        assert len({tuple(c["pts"][r["ci"]]) for c, r in lat if r["n"] == side}) >= 2
    assert any(len(r["centre_ties"]) == 2 for _, r in reps["tiny"]) and any(len(r["centre_ties"]) == 2 for _, r in reps["on_centre"])
    # an angle-tie group of three inside one layer whose detection order is not its radius order
    ang = reps["angle_ties"]
    assert any(len(g) >= 3 and [r["r2"][i] for i in g] != sorted(r["r2"][i] for i in g)
               for _, r in ang for gs in r["angle_ties"].values() for g in gs)
    # a +-theta pair sharing the smallest |angle| of a layer, the negative one first; and a marker at +pi
    def pm(r, mem):
        return len(mem) == 2 and r["vec"][mem[0]][1] == -r["vec"][mem[1]][1] < 0 and r["vec"][mem[0]][0] == r["vec"][mem[1]][0]
    assert any(pm(r, mem) for _, r in ang for mem in r["absmin"].values())
    assert all(any(vy == 0 and vx < 0 for vx, vy in r["vec"]) for _, r in ang)
    # on the centre: a rest marker of radius 0; two coincident rest markers (equal radius AND equal angle)
    assert any(0 in r["r2"] for _, r in reps["on_centre"])
    assert any(r["vec"][g[0]] == r["vec"][g[1]] != (0, 0) for _, r in reps["on_centre"] for gs in r["angle_ties"].values() for g in gs)
    # k < num_layers; every marker its own layer
    assert any(r["k"] < c["layers"] for c, r in reps["tiny"]) and any(r["k"] == r["n"] - 1 < c["layers"] for c, r in reps["fewer"])
    assert any(r["k"] == r["n"] - 1 > 1 for _, r in reps["fewer"])
    for c, r in reps["fewer"]:
        if r["k"] == r["n"] - 1:
            assert np.array_equal(K.exact_table(c["name"], "full")[0], K.exact_table(c["name"], "as_written")[0])
    # rings of exactly equal radii: more layers than rings has exactly tied optima, fewer merges rings
    ex = {c["layers"]: r for c, r in reps["sweep"] if "exact" in c["name"]}
    assert len(set(ex[1]["r2"])) == 4 and all(ex[lay]["n_optimal"] > 1 for lay in (5, 6, 15, 16)) and ex[2]["n_optimal"] == 1
    assert any(r["n_optimal"] > 1 for c, r in ang if c["kind"] == "tie")
    # the stride and capacity groups sit on either side of the block size and at the limit
    assert sorted(r["n"] - 1 for _, r in reps["stride"]) == [254, 255, 256, 257]
    assert max(r["n"] for _, r in reps["capacity"]) == L.IDS_MAX_MARKERS


def test_detection_order_moves_only_the_as_written_slot():
    """One cloud under six detection orders: `full` is the same id -> coordinates map every time; `as_written` holds, per layer,
    the member that comes last in THAT order - and it is not always the same marker."""
    tabs = {n: {m: K.exact_table(n, m) for m in K.MODES} for n in K.names(group="order")}
    maps = [{tuple(k): tuple(v) for k, v in zip(t["full"][0].tolist(), t["full"][1].tolist())} for t in tabs.values()]
    assert all(m == maps[0] for m in maps) and len(maps[0]) == 40
    slots = {n: tuple(map(tuple, t["as_written"][1].tolist())) for n, t in tabs.items()}
    assert len(set(slots.values())) > 1 and all(len(s) == 6 for s in slots.values())
    for n in tabs:
        case, rep = K.BY_NAME[n], K.report(n)
        for lay in range(1, 6):
            last = max(i for i in range(39) if rep["layer"][i] == lay)
            assert tabs[n]["as_written"][1][lay].tobytes() == K.xy(case)[rep["rest"][last]].tobytes()
