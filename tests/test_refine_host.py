"""CPU tests of the grey-level refinement (`vbs_refine_markers`): the restatement of the rule (tests/helpers/refine_oracle.py,
written from include/vbs.h) against a second, brute-force form; the int64 bound at R = 63; the geometry for every diameter the
window admits; the accuracy of the RULE on a seeded set of rendered markers - the restatement is the reference there, never the
kernel; the entry's refusals and the host-side pieces of `vbs_amd.refine`."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import refine as RF

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import refine_cases as RC                                      # noqa: E402
import refine_oracle as O                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED_MAX, BOUND = RC.MEASURED_MAX, RC.BOUND


@pytest.fixture(scope="module")
def accuracy():
    cases = RC.accuracy_set()
    return cases, [O.refine_row(c["gray"], c["row"]) for c in cases]


def test_symbol_and_defines_are_in_the_header_and_in_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    assert "vbs_refine_markers" in L.SYMBOLS and re.search(r"\bvbs_refine_markers\s*\(", hdr)
    assert hasattr(L.lib(), "vbs_refine_markers")
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_REFINE_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert len(defs) == 11
    for k, v in defs.items():
        assert getattr(L, k[4:]) == v, k
    assert (O.COLS, O.SUM_COLS, O.MAX_R) == (L.REFINE_COLS, L.REFINE_SUM_COLS, L.REFINE_MAX_R)
    assert set(RF.STATUS_NAMES) == set(range(8)) and len(RF.REC_COLUMNS) == L.REFINE_COLS and len(RF.SUM_COLUMNS) == L.REFINE_SUM_COLS
    assert RF.DEFAULTS == O.DEFAULTS


def test_entry_refuses_bad_arguments_before_it_selects_a_device():
    one = (C.c_uint8 * 64)()
    p = C.cast(one, C.c_void_p)

    def call(gray=p, n=1, h=8, w=8, sn=64, sr=8, table=p, m=1, core=0.5, disc=1.5, ring=2.0, mc=16.0, ms=1.0, pol=0, keep=0, rec=p,
             sums=None, out=None):
        return L.lib().vbs_refine_markers(0, gray, n, h, w, sn, sr, table, m, core, disc, ring, mc, ms, pol, keep, rec, sums, out, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(gray=None), dict(table=None), dict(rec=None), dict(n=-1), dict(m=0), dict(n=1 << 15, m=1 << 15), dict(h=0), dict(w=0),
           dict(h=16385), dict(w=16385, sr=16385), dict(sr=7), dict(core=0.0), dict(core=nan), dict(core=1.6), dict(disc=2.5),
           dict(ring=65.0), dict(ring=inf), dict(mc=0.1), dict(mc=256.0), dict(mc=nan), dict(ms=-1.0), dict(ms=inf), dict(pol=2),
           dict(pol=-1), dict(keep=2)]
    for kw in bad:
        assert call(**kw) == L.VBS_EINVAL, kw


def test_params_window_and_report_on_the_host():
    assert RF.params(None) is None and RF.params(False) is None and RF.params(True) == RF.DEFAULTS
    assert RF.params({"polarity": 1})["polarity"] == 1 and RF.params(True, ring_f=2.5)["ring_f"] == 2.5
    assert RF.params({"passes": 3})["passes"] == 3 and "passes" not in RF.params(True)
    for bad in ({"nope": 1}, {"core_f": 2.0}, {"min_contrast": 0.0}, {"max_shift_f": -1}, {"polarity": 2}, {"ring_f": float("nan")}, 7,
                {"passes": 0}, {"passes": RF.MAX_PASSES + 1}, {"passes": 1.5}):
        with pytest.raises(ValueError):
            RF.params(bad)
    win = RF.window(16.0)
    assert (win["R"], win["c2"], win["g2"], win["R2"], win["fits"]) == (17, 16, 144, 289, True)
    assert RF.max_major() == 62.0 and RF.window(62.0)["fits"] and not RF.window(62.5)["fits"]
    rec = np.zeros((3, 2, L.REFINE_COLS))
    rec[:, 0, 0] = (0, 0, 5)
    rec[:, 1, 0] = (4, 4, 1)
    rec[:2, 0, 3], rec[:2, 0, 11], rec[:2, 0, 10] = (15.0, 16.0), (0.25, 0.75), (1.0, 3.0)
    tab = np.zeros((3, 2, L.TABLE_COLS), np.float32)
    tab[..., 3] = 16.0
    rep = RF.report(rec, tab)
    assert rep["status_per_frame"].tolist() == [[1, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 1, 0, 0]]
    assert rep["status_per_slot"].tolist() == [[2, 0, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 2, 0, 0, 0]]
    assert rep["dmajor_mean"][0] == -0.5 and rep["dmajor_std"][0] == 0.5 and rep["shift_mean"][0] == 0.5 and rep["shift_std"][0] == 0.25
    assert np.isnan(rep["dmajor_mean"][1]) and rep["never_refined"].tolist() == [1] and rep["edge_var_median"] == 2.0
    # a refined row is `uncovered` where the disc of its start (1.5 x 8 = 12 px) does not reach a pixel beyond major' / 2
    assert not rep["uncovered"].any() and rep["uncovered_per_slot"].tolist() == [0, 0]
    rec[0, 0, 3], rec[1, 0, 3] = 22.0, 22.5
    rep = RF.report(rec, tab)
    assert rep["uncovered"].tolist() == [[False, False], [True, False], [False, False]] and rep["uncovered_per_slot"].tolist() == [1, 0]
    assert RF.report(rec, tab, disc_f=2.0)["uncovered"].sum() == 0


def test_the_largest_products_stay_inside_int64_at_the_largest_window():
    """The all-saturated window at R = VBS_REFINE_MAX_R - every pixel of the 127 x 127 square at the largest weight 8 x 255,
    which over-counts the disc - with Python integers: the products the tail forms in int64 stay below 2^63, also for the
    one-sided half window that maximises |Sx|."""
    R, wmax = L.REFINE_MAX_R, 8 * 255
    d = range(-R, R + 1)
    S0 = sum(wmax for _ in d for _ in d)
    Sxx = sum(wmax * dx * dx for dx in d for _ in d)
    Sx_half = sum(wmax * dx for dx in d if dx > 0 for _ in d)
    Sxy_quadrants = sum(wmax * dx * dy for dx in d for dy in d if dx * dy > 0)
    assert S0 == 2040 * 16129 and S0 < 2 ** 25 and Sx_half <= 63 * S0 < 2 ** 31 and Sxx <= 3969 * S0 < 2 ** 37
    for prod in (Sxx * S0, Sx_half * Sx_half, Sxy_quadrants * S0, Sxx * S0 + Sx_half * Sx_half):
        assert prod < 2 ** 63
    # and a lane's int32 column sums (k_refine adds sum w, sum w dy, sum w dy dy per column before it multiplies by dx)
    assert wmax * sum(dy * dy for dy in d) < 2 ** 29


def test_geometry_for_every_diameter_from_2_to_62():
    """R, c2, g2 against exact rationals for major = 2, 2.25, .. 62 (exact in float32); core and ring are never empty, the disc
    lies inside the window, and 62 is the last diameter whose window fits."""
    for q in range(8, 62 * 4 + 1):
        major = q / 4.0
        st, x0, y0, R, c2, g2 = O.geometry(100.0, 100.0, major, 400, 400)
        r = Fraction(q, 8)
        assert st == 0 and (x0, y0) == (100, 100)
        assert R == math.ceil(2 * r) + 1 and c2 == math.floor((r / 2) ** 2) and g2 == math.floor((3 * r / 2) ** 2), major
        assert 2 <= R <= L.REFINE_MAX_R and 0 <= c2 <= g2 < (R - 1) ** 2 + 1 and g2 < R * R
        win = RF.window(major)
        assert (win["R"], win["c2"], win["g2"]) == (R, c2, g2) and win["core"] >= 1 and win["ring"] >= 4 and win["fits"]
    assert O.geometry(100.0, 100.0, 62.0, 400, 400)[3] == 63
    assert O.geometry(100.0, 100.0, np.nextafter(np.float32(62.0), np.float32(63.0)), 400, 400)[0] == 3
    assert O.geometry(100.0, 100.0, 1e30, 400, 400)[0] == 3 and O.geometry(100.0, 100.0, np.float32(np.inf), 400, 400)[0] == 2
    assert O.geometry(100.0, 100.0, 1.999, 400, 400)[0] == 2 and O.geometry(np.nan, 100.0, 16.0, 400, 400)[0] == 2
    assert O.geometry(2.0 ** 30, 100.0, 16.0, 400, 400)[0] == 2 and O.geometry(-2.0 ** 31, 100.0, 16.0, 400, 400)[0] == 2
    # half-way centres round up (floor(C + 0.5)), also below zero
    assert O.geometry(99.5, 100.5, 16.0, 400, 400)[1:3] == (100, 101) and O.geometry(-0.5, -1.5, 16.0, 400, 400)[1:3] == (0, -1)
    # flush with each border: status 0; one pixel over: status 4
    for cx, cy, ok in ((17, 50, True), (16, 50, False), (50, 17, True), (50, 16, False), (82, 50, True), (83, 50, False),
                       (50, 72, True), (50, 73, False)):
        assert (O.geometry(cx, cy, 16.0, 90, 100)[0] == 0) == ok, (cx, cy)


def test_restatement_equals_the_brute_force_form(accuracy):
    cases, res = accuracy
    seen = set()
    rng = np.random.default_rng(5)
    extra = []
    for pol in (0, 1):
        noise = rng.integers(0, 256, (48, 48)).astype(np.uint8)                       # pure noise: every level, ties in the quartiles
        extra.append((noise, RC.row(24.2, 23.7, 9.0), {"polarity": pol, "min_contrast": 0.125}))
        flat = np.full((48, 48), 97, np.uint8)
        extra.append((flat, RC.row(24, 24, 12.0), {"polarity": pol}))
        g = RC.render(64, 64, [(31.6, 32.3, 9.0, 6.3, 30.0)], 60.0, 200.0, 1.0, noise=1.5, seed=3) if pol else \
            RC.render(64, 64, [(31.6, 32.3, 9.0, 6.3, 30.0)], 200.0, 60.0, 1.0, noise=1.5, seed=3)
        extra.append((g, RC.row(31.0, 33.0, 17.0), {"polarity": pol}))
        extra.append((g, RC.row(31.0 + 16.0, 33.0, 16.0), {"polarity": pol}))        # started two radii off
        extra.append((g, RC.row(31.0, 33.0, 17.0), {"polarity": pol, "max_shift_f": 0.01}))
    for gray, row, kw in [(c["gray"], c["row"], {}) for c in cases[::4]] + extra:
        rec, sums, _ = O.refine_row(gray, row, **kw)
        st, bsums = O.refine_row_brute(gray, row, **kw)
        assert int(rec[0]) == st and [int(v) for v in sums] == bsums, (row.tolist(), kw)
        seen.add(st)
    assert {0, 5, 7} <= seen


def test_the_rule_is_accurate_on_the_seeded_set_of_rendered_markers(accuracy):
    cases, res = accuracy
    assert len(cases) >= 64
    assert {(c["bg"], c["fg"], c["sigma"]) for c in cases} == {(200.0, 60.0, 0.0), (200.0, 60.0, 1.0), (120.0, 90.0, 0.0), (120.0, 90.0, 1.0)}
    assert all(0.85 <= c["b"] / c["a"] <= 1.0 for c in cases)
    assert all(int(rec[0]) == 0 for rec, _, _ in res), "every marker of the set must be refined: nothing is left out"
    err = {"major": [], "d_area": [], "centre": []}
    for c, (rec, _, out) in zip(cases, res):
        err["major"].append(abs(rec[3] - 2 * c["a"]))
        err["d_area"].append(abs(rec[6] - 2 * math.sqrt(c["a"] * c["b"])))
        err["centre"].append(math.hypot(rec[1] - c["cx"], rec[2] - c["cy"]))
        assert rec[3] >= rec[4] > 0 and 90.0 < rec[5] <= 270.0 and out[0] == 1.0
    for k in err:
        print(f"{k}: max {max(err[k]):.4f} px, mean {np.mean(err[k]):.4f} px, bound {BOUND[k]:.4f} px")
        assert max(err[k]) <= BOUND[k], k
        # the recorded maxima are what this set gave when the bounds were set; another NumPy or SciPy may render it a little
        # differently, so they are held loosely: a bound several times what the set needs would no longer be a measured one
        assert 0.5 * MEASURED_MAX[k] <= max(err[k]), f"the recorded maximum of {k} is far above what the restatement gives"


def test_area_diameter_is_insensitive_to_blur_gain_and_offset_where_the_binary_contour_is_not():
    """The property the estimator is there for: one ellipse under blur sigma 0 .. 2, gain 0.5 .. 1 and an offset - d_area moves by
    less than the d_area bound, the centre by less than the centre bound."""
    a, b = 8.0, 7.2
    ref = None
    for sigma, gain, offset in ((0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.5, 60.0), (0.0, 0.6, 30.0)):
        g = RC.render(72, 72, [(36.3, 35.8, a, b, 20.0)], 200.0, 60.0, sigma, gain, offset, noise=0.0)
        rec, _, _ = O.refine_row(g, RC.row(36.0, 36.0, 16.0))
        assert rec[0] == 0
        ref = rec if ref is None else ref
        assert abs(rec[6] - ref[6]) <= BOUND["d_area"] and math.hypot(rec[1] - ref[1], rec[2] - ref[2]) <= BOUND["centre"]
        assert abs(rec[6] - 2 * math.sqrt(a * b)) <= BOUND["d_area"]


def test_angle_is_the_direction_of_the_major_axis_in_column_5s_convention():
    """An ellipse whose major axis points along theta (from +x towards +y, y down) gives theta modulo 180, in (90, 270]: what the
    binary path writes - cv2.fitEllipse's angle (`oracle.stages.fit_ellipse`) plus 90 where its first axis is the shorter, as
    `oracle.stages.marker_center` restates marker_detection.py:217."""
    from oracle import stages as OS
    for theta in (0.0, 30.0, 75.0, 90.0, 140.0):
        g = RC.render(72, 72, [(36.0, 36.0, 10.0, 7.0, theta)], 200.0, 60.0, 0.5)
        rec, _, _ = O.refine_row(g, RC.row(36.0, 36.0, 18.0))
        assert rec[0] == 0
        want = theta % 180.0
        assert 90.0 < rec[5] <= 270.0
        assert abs((rec[5] - want + 90.0) % 180.0 - 90.0) < 1.0, (theta, rec[5])
        if theta % 90.0 == 0.0:          # (an exactly axis-aligned, symmetric contour: fitEllipse's own angle is ambiguous there - its
            continue                     # cross term is +-0 - and the restated fit returns 90 for both directions)
        cnt = max(OS.find_contours_external(g < 130), key=len)
        (_, _), (w_, h_), ang = OS.fit_ellipse(cnt.reshape(-1, 2).astype(np.float64))
        binary = ang if w_ > h_ else ang + 90.0              # the direction of the longer axis
        assert abs((rec[5] - binary + 90.0) % 180.0 - 90.0) < 3.0, (theta, rec[5], binary)
