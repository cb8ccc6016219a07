"""The references of tests/test_gpu_ellipse.py against each other, on the CPU: `oracle.stages.fit_ellipse` against the exact
rational fit (tests/helpers/ellipse_oracle.py), the vertex moments against a second summation, and the caps that the GPU
tests rely on, established on the oracle alone:
  * at most 1 % of the compared cx, cy, w, h differ from the exact value rounded to float32, none by more than 1 ulp;
  * under 10 % of the fitted contours are too round ((h - w) / h < 1e-3) for their angle to be held;
  * at most 2 % of the tiles lie on a decision boundary (minor axis within 1 float32 ulp of 5, a squared distance within
    1e-9 relative of the threshold or of a competing distance - the exactly equidistant pairs placed on purpose
    included), none in `minor5`;
  * every branch of `inside_polygon`, accepting and rejecting, is reached by a placed centroid on an interior tile and on a
    tile at the frame's border; in rows and columns 0 to 1 only whole, on-row and on-column cells can be reached
    (ellipse_cases._notch_frames says why), and a centre claimed by two contours cannot be built at all;
  * the int64 moments: the tall frame that must overflow does, the one below it does not (range of the moments).
Each test prints what it measured (pytest -s)."""
import collections
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from oracle import stages as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ellipse_cases as EC                                    # noqa: E402
import ellipse_oracle as E                                    # noqa: E402
import label_cases as LC                                      # noqa: E402

SMALL = [g for g in EC.GEOMETRIES if g not in ((130, 4096), (1200, 1920))]

# every (branch, decision) of inside_polygon (k_finalize.hip); "two_side": two pixels of the cell that share an edge
BRANCHES = [("vertex", True), ("vertex", False), ("on_row", True), ("on_row", False), ("on_col", True), ("on_col", False),
            ("four", True), ("three_no11", True), ("three_no11", False), ("three_no00", True), ("three_no00", False),
            ("three_no10", True), ("three_no10", False), ("three_no01", True), ("three_no01", False),
            ("diag_main", True), ("diag_main", False), ("diag_anti", True), ("diag_anti", False),
            ("two_side", False), ("one", False), ("zero", False)]


def _fitted():
    for g in EC.GEOMETRIES:
        for f in EC.frames(*g):
            if f.kind != "self":
                continue                                      # (the pieces twins have the same area mask)
            info = EC.analyse(f)
            for c, p in zip(info["contours"], info["per"]):
                yield g, f, c, p


def test_oracle_fit_against_exact_fit():
    worst = collections.defaultdict(lambda: [0, 0, 0, 0, 0.0])
    compared = differ = fitted = round_ones = 0
    for g, f, c, p in _fitted():
        if p["n"] < 5:
            assert p["exact"] is None and p["oracle"] is None
            continue
        ex = p["exact"]
        assert ex is not None, (f.name, p["first"])           # no singular system among the cases: ok = 0 only below 5 vertices
        assert not ex["branch_differs"], (f.name, p["first"])
        fitted += 1
        u, dev, tol = E.fit_deviation(p["oracle"], ex)
        compared += 4
        differ += sum(v != 0 for v in u)
        assert max(u) <= 1, (f.name, p["first"], u, p["oracle"], ex)
        w = worst[f.family]
        for i in range(4):
            w[i] = max(w[i], u[i])
        if dev is None:
            round_ones += 1
        else:
            assert dev <= tol, (f.name, p["first"], dev, tol, p["oracle"], ex["angle_exact"])
            w[4] = max(w[4], dev)
        # the kernel's mean (exact sum, one rounding) is cv2's (running float32 sum) wherever the sums stay below 2^24
        if f.family != "large":
            assert E.mean32(c, True) == E.mean32(c, False)
    print(f"\noracle against exact: {fitted} fitted contours, {differ} of {compared} values differ "
          f"({100.0 * differ / compared:.3f} %), {round_ones} ({100.0 * round_ones / fitted:.2f} %) excluded from the angle")
    for fam, w in sorted(worst.items()):
        print(f"  {fam:9s} max ulps cx {w[0]} cy {w[1]} w {w[2]} h {w[3]}   max angle deviation {w[4]:.2e} deg")
    assert differ <= 0.01 * compared
    assert round_ones < 0.10 * fitted


def test_large_cases_mean_and_moment_size():
    """what the `large` frames are there for: coordinate sums at or beyond 2^24 (where cv2's running float32 mean and the
    kernel's one rounding can part) and fourth moments at the edge of float64's 53 bits."""
    top = 0
    for g, f, c, p in _fitted():
        if f.family != "large":
            continue
        big = max(abs(v) for v in p["moments"])
        top = max(top, big)
        a, b = E.mean32(c, True), E.mean32(c, False)
        print(f"\n{f.name}: {p['n']} vertices, largest |moment| {big:.3e} = 2^{np.log2(float(big)):.1f}, "
              f"sum x {int(np.asarray(c)[..., 0].sum())}, running mean {a}, one rounding {b}")
    assert 2 ** 52 < top < 2 ** 63


def test_tall_frames_straddle_the_int64_range():
    """the frame the range derivation says overflows does, the one below it does not, and the kernel's guard
    (an upper bound from sum x^2 and sum y^2, which cannot overflow) separates them."""
    for which, rows in EC.TALL.items():
        f = EC.tall_frame(which)
        info = EC.analyse(f, fits=False)
        assert len(info["per"]) == 1
        m = info["per"][0]["moments"]
        assert LC.runs(info["opened"]) == rows <= LC.RUN_CAP   # inside the run capacity: nothing else refuses the frame
        top, guard = max(abs(v) for v in m), EC.moment_guard(m, *f.area.shape)
        print(f"\ntall_{which}: {rows} rows, {m[0]} vertices, largest |moment| 2^{np.log2(float(top)):.2f}, guard {guard:.3e}")
        assert top <= guard
        assert max(abs(v) for v in m[:6]) < 2 ** 50             # n, the first and the second moments: far inside
        if which == "over":
            assert top >= 2 ** 63 and guard >= 9.0e18
        else:
            assert guard < 9.0e18
    # and no other case comes near the guard
    for g, f, c, p in _fitted():
        assert EC.moment_guard(p["moments"], *g) < 9.0e18 / 8, f.name


def test_vertex_moments_against_a_second_summation():
    """raw power sums about the frame's origin in Python ints, moved to the first pixel by the binomial theorem."""
    from math import comb
    n = 0
    for g, f, c, p in _fitted():
        pts = [(int(x), int(y)) for x, y in np.asarray(c).reshape(-1, 2)]
        ax, ay = min((y, x) for x, y in pts)[::-1]
        assert (ax, ay) == p["first"]
        # the first pixel is where the raster scan meets the component: nothing of the opened mask before it on its row
        info = EC.analyse(f)
        assert info["opened"][ay, ax] and (ax == 0 or not info["opened"][ay, ax - 1])
        raw = {(a, b): sum(x ** a * y ** b for x, y in pts) for a in range(5) for b in range(5 - a)}
        want = [len(pts)]
        for a, b in E.ORDER:
            want.append(sum(comb(a, i) * comb(b, j) * (-ax) ** (a - i) * (-ay) ** (b - j) * raw[i, j]
                            for i in range(a + 1) for j in range(b + 1)))
        assert want == p["moments"], (f.name, p["first"])
        n += 1
    assert n > 1500


def test_fit_depends_on_the_origin_but_not_on_the_scale():
    """why exact_fit takes cv2's float32 mean as its origin: the first fit is not translation-invariant."""
    worst = {}
    for fam, shape in (("squares", EC.squares([(5, 5)])), ("squares", EC.squares([(3, 4)])),
                       ("ellipse", EC.digitised_ellipse(12.5, 4.5, 0.4, 0.3, 0.6))):
        c = O.find_contours_external(O.morph_open5(np.pad(shape, 8)))[0]
        base = E.exact_fit(c)
        m = E.mean32(c)
        t = Fraction(1, 10 ** 6)
        moved = E.exact_fit(c, origin=(Fraction(m[0]) + t, Fraction(m[1])))
        worst[fam] = max(worst.get(fam, 0.0), abs(float((moved["cx_exact"] - base["cx_exact"]) / t)))
    print(f"\ncentre moved per unit of origin shift: {worst}")
    assert worst["squares"] > 0.1 and worst["ellipse"] < 0.05


def _placed(border: bool):
    geos = [(64, 128)] if border else [g for g in SMALL if g != (64, 128)]
    for g in geos:
        for f in EC.frames(*g):
            if f.kind == "pieces":
                yield from ((f, p) for p in f.placed)


@pytest.mark.parametrize("where", ["interior", "border"])
def test_every_branch_of_inside_polygon_is_reached(where):
    seen = collections.Counter()
    low = collections.Counter()
    for f, p in _placed(where == "border"):
        seen[(p["branch"], p["decision"])] += 1
        x, y = p["centroid"]
        if where == "border" and (x < 2 or y < 2):
            low[(p["branch"], p["decision"])] += 1
    print(f"\n{where}: " + ", ".join(f"{b}/{'in' if d else 'out'} {seen[(b, d)]}" for b, d in BRANCHES))
    if where == "border":
        print("  of these with the cell in columns or rows 0 to 1: " + ", ".join(f"{b}/{'in' if d else 'out'} {n}"
                                                                                  for (b, d), n in sorted(low.items())))
        assert sum(low.values()) >= 10
    missing = [b for b in BRANCHES if not seen[b]]
    assert not missing, missing


def test_placed_branches_are_what_the_polygon_test_says():
    """the cell's decision (a restatement of inside_polygon in NumPy float32) equals pointPolygonTest >= 0 of the traced
    contour for every placed centroid: the kernel's cell rule is the reference's polygon rule, also in rows and columns 0 to
    1, where the float32 sum fx + fy can round."""
    n = 0
    for border in (False, True):
        for f, p in _placed(border):
            if p["branch"] == "no_fit":
                continue
            c = EC.analyse(f)["contours"][p["contour"]]
            assert (O.point_polygon_test(c, p["centroid"]) >= 0) == p["decision"], (f.name, p)
            n += 1
    assert n > 1000


def test_share_of_tiles_on_a_decision_boundary():
    tiles = on = equal = 0
    minor5 = 0
    for g in SMALL:
        for f in EC.frames(*g):
            info = EC.analyse(f)
            centres = EC.band_centres(f)
            bad = EC.boundary_contours(info, centres)
            tiles += len(info["per"])
            on += len(bad)
            equal += sum(why == "equal" for why in bad.values())
            if f.family == "minor5":
                minor5 += len(bad)
            if any(why != "equal" for why in bad.values()):
                print(f"\n{f.name}: contours on a decision boundary {sorted(bad.items())}")
    print(f"\n{on} of {tiles} tiles on a decision boundary ({100.0 * on / tiles:.3f} %), {minor5} in minor5; {equal} of them "
          f"hold two exactly equidistant centres on purpose (first index wins)")
    assert on <= 0.02 * tiles and minor5 == 0
