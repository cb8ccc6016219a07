"""CPU tests of the bonnet contact geometry (`vbs_sphere_series`), all on the NumPy restatement
`tests/helpers/sphere_oracle.py` the device is held to bit for bit (`tests/test_gpu_sphere.py`): the algebraic sphere against
`scipy.optimize.least_squares` on the geometric residual, the contact plane against `np.linalg.svd`, exact dyadic cases, the sweep
count, every degeneracy, the decomposition in the shell's frame, the host module `vbs_amd.sphere`, the argument checks of the
Python shim, and a synthetic press of the 65-marker cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import rigid_cases as RC                                       # noqa: E402
import sphere_cases as SC                                      # noqa: E402
import sphere_oracle as O                                      # noqa: E402

# max(|C - C_geo|, |R - R_geo|, |C - C_true|, |R - R_true|) / R over the NOISE-FREE caps of `_caps` (both fits return the sphere the
# points lie on; the worst is the cap 40 m from the origin, where an ulp of a coordinate is 7e-12 mm): 10 x the MEASURED_EXACT this
# file measures on the CPU
MEASURED_EXACT = 3.37e-13
SPHERE_TOL = 10 * MEASURED_EXACT
# max(|C - C_geo|, |R - R_geo|) with 0.02 mm of noise, in mm: the algebraic fit minimises sum (|P - C|^2 - R^2)^2, not the geometric
# residual, so the two differ in second order; both lie 0.05 mm from the true sphere, which a cap only 5.5 mm deep determines no
# better (the sagitta carries R with a lever of R / depth = 5).  10 x the MEASURED_NOISY this file measures
MEASURED_NOISY = 9.66e-3
NOISY_TOL = 10 * MEASURED_NOISY
# max(|n - n_svd|, |dist - dist_svd| / R, |cm - cm_svd| / R) over the contact planes of the synthetic press: 10 x the MEASURED_PLANE
# this file measures on the CPU
MEASURED_PLANE = 3.25e-15
PLANE_TOL = 10 * MEASURED_PLANE
NOISE = 0.02                                                    # mm, every coordinate of the synthetic press
DEPTH = 0.1                                                     # contact_depth
HELD = (0.0, 0.0, 27.0, 27.0)


def _caps(noise):
    """(name, P [k, 3], C, R): the layout on R = 27, at the origin and 40 m from it, the full cap and the rim only."""
    rng = np.random.default_rng(31)
    lay = RC.layout65()[:, :2]
    rim = (lay ** 2).sum(axis=1) > 10.0 ** 2                   # the rings at 10.23, 13.37 and 16.29 mm
    for off in (0.0, 40000.0):
        c = SC.C0 + np.array([off, -0.5 * off, 0.25 * off])
        for name, sel in (("full", np.ones(65, dtype=bool)), ("rim", rim)):
            P = SC.cap(lay[sel], c)
            yield f"{name} off={off}", P + rng.normal(size=P.shape) * noise, c, SC.R0


def _dev(f, C, R):
    return max(float(np.abs(np.asarray(f["C"]) - C).max()), abs(f["R"] - R))


def test_the_algebraic_sphere_agrees_with_a_geometric_least_squares_fit():
    worst_exact = worst_noisy = 0.0
    for name, P, c, r in _caps(0.0):
        f = O.fit(P, np.ones(len(P), dtype=bool))
        assert f["exists"], name
        Cg, Rg = O.geometric_fit(P, np.concatenate([f["C"], [f["R"]]]) + 0.01)
        worst_exact = max(worst_exact, _dev(f, Cg, Rg) / r, _dev(f, c, r) / r)
    for name, P, c, r in _caps(NOISE):
        f = O.fit(P, np.ones(len(P), dtype=bool))
        assert f["exists"], name
        Cg, Rg = O.geometric_fit(P, np.concatenate([c, [r]]))
        worst_noisy = max(worst_noisy, _dev(f, Cg, Rg))
    print(f"sphere vs least_squares: noise-free {worst_exact:.3e} of R (bound {SPHERE_TOL:.1e}), "
          f"with noise {worst_noisy:.3e} mm (bound {NOISY_TOL:.1e})")
    assert worst_exact <= SPHERE_TOL and worst_noisy <= NOISY_TOL


def test_the_published_layout_lies_on_its_sphere():
    """`rigid_cases.layout65()` rises 5.47 mm over a radius of 16.29 mm: a sphere of R = (16.29^2 + 5.47^2) / (2 x 5.47) = 26.99 mm
    whose centre lies R below the apex."""
    big = (RC.SHELL_RADIUS ** 2 + RC.SHELL_RISE ** 2) / (2.0 * RC.SHELL_RISE)
    f = O.fit(RC.layout65(), np.ones(65, dtype=bool))
    assert f["exists"] and abs(f["R"] - big) < 1e-12 and np.abs(np.asarray(f["C"]) - (0.0, 0.0, RC.SHELL_RISE - big)).max() < 1e-12
    assert np.sqrt(f["ssr"] / 65.0) < 1e-13


def _dyadic():
    """Dyadic points on the dyadic sphere about (8, -16, 32) of radius 15 = |(10, 11, 2)| = |(5, 10, 10)| = .. and four inside it."""
    c = np.array([8.0, -16.0, 32.0])
    on = [(2, 10, 11), (2, 11, 10), (10, 2, 11), (5, 10, 10), (10, 10, 5), (14, 5, 2), (2, 5, 14), (9, 12, 0), (12, 9, 0), (0, 15, 0)]
    pts = []
    for v in on:
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            pts.append((sx * v[0], sy * v[1], -v[2]))
    inner = [(0.0, 0.0, -14.5), (3.0, 0.0, -14.0), (0.0, 3.0, -14.0), (-3.0, -3.0, -13.5)]       # r2 = 210.25, 205, 205, 200.25
    return c, np.asarray(pts + inner, dtype=np.float64) + c


def test_dyadic_points_on_a_dyadic_sphere_are_exact():
    c, P = _dyadic()
    m = len(P)
    allm = np.ones(m, dtype=bool)
    row, rad, _ = O.frame(P, allm, allm, given=(c[0], c[1], c[2], 15.0), contact_depth=0.5)
    assert (rad[:40, 1] == 0.0).all() and (rad[:, 0] == 1.0).all()
    assert rad[40:, 1].tolist() == [-0.5, np.sqrt(205.0) - 15.0, np.sqrt(205.0) - 15.0, np.sqrt(200.25) - 15.0]
    # (R - 0.5)^2 = 210.25: the slot AT the threshold is not a contact slot (strictly inside); the other three are
    assert row[O.N_CONTACT] == 3.0 and row[O.DEEPEST] == 43.0 and row[O.DEPTH_MAX] == 15.0 - np.sqrt(200.25)
    assert row[O.FLAG] == 3.0 and row[O.N_USED] == m and row[O.N_FIT] == m
    row2, _, _ = O.frame(P, allm, allm, given=(c[0], c[1], c[2], 15.0), contact_depth=0.25)
    assert row2[O.N_CONTACT] == 4.0
    # equal depths: the smaller slot
    rowe, _, _ = O.frame(P[[41, 42, 40]], np.ones(3, dtype=bool), np.ones(3, dtype=bool), given=(c[0], c[1], c[2], 15.0))
    assert rowe[O.DEEPEST] == 0.0 and rowe[O.N_CONTACT] == 3.0
    # the fit of the 40 points on the sphere returns it to rounding, and rho is then of the order of an ulp of R
    f = O.fit(P, np.arange(m) < 40)
    assert f["exists"] and _dev(f, c, 15.0) < 1e-13 and np.abs(f["rho"]).max() < 1e-13


def _press(seed=0):
    k = SC.press_recording(40, still=0, seed=seed)
    margins = []
    k["want"] = O.sphere_series(k["table"], HELD, contact_depth=DEPTH, margins=margins)
    O.assert_margins(margins, "the synthetic press")
    return k


@pytest.fixture(scope="module")
def press():
    return _press()


def _contact_points(k, f):
    P, used = O.used_points(k["table"])
    sel = used[f] & (k["want"][1][f, :, 1] < -DEPTH)
    return P[f][sel]


def test_the_contact_plane_agrees_with_an_svd(press):
    rows = press["want"][0]
    worst, seen = 0.0, 0
    for f in np.flatnonzero(rows[:, O.FLAG] == 3.0):
        pts = _contact_points(press, f)
        assert len(pts) == rows[f, O.N_CONTACT]
        n, d, cm, S = O.svd_plane(pts, HELD[:3])
        worst = max(worst, float(np.abs(rows[f, O.NX:O.NZ + 1] - n).max()), abs(rows[f, O.DIST] - d) / HELD[3],
                    float(np.abs(rows[f, O.CMX:O.CMZ + 1] - cm).max()) / HELD[3])
        assert abs(rows[f, O.PLANE_RMS] - S[2] / np.sqrt(len(pts))) <= 1e-9
        seen += 1
    print(f"plane vs SVD over {seen} frames: worst deviation {worst:.3e} (bound {PLANE_TOL:.1e})")
    assert seen >= 30 and worst <= PLANE_TOL


def test_one_more_sweep_changes_no_bit_of_the_normal(press):
    """`SWEEPS` is one more than the number after which every host case is diagonal in bits: SWEEPS - 1 sweeps diagonalise every case,
    SWEEPS - 2 do not, and sweep SWEEPS + 1 changes nothing."""
    cases = []
    P, used = O.used_points(press["table"])
    for f in np.flatnonzero(press["want"][0][:, O.FLAG] == 3.0):
        cases.append((P[f], used[f] & (press["want"][1][f, :, 1] < -DEPTH)))
    tab, _, _ = SC.special_contacts()
    Ps, us = O.used_points(tab)
    for f in (3, 6):
        _, rad, _ = O.frame(Ps[f], us[f], us[f], given=HELD)
        cases.append((Ps[f], us[f] & (rad[:, 1] < -DEPTH)))
    rng = np.random.default_rng(77)
    for _ in range(40):                                           # random clouds of every shape: needles, discs, balls
        k = int(rng.integers(3, 40))
        cases.append((rng.normal(size=(k, 3)) * 10.0 ** rng.uniform(-3, 1, size=3) + rng.normal(size=3) * 5.0, np.ones(k, dtype=bool)))
    diagonal = lambda T: all(T[i][j] == 0.0 for i in range(3) for j in range(3) if i != j)        # noqa: E731
    needed = 0
    for pts, sel in cases:
        a = O.plane(pts, sel, HELD[:3], gap_rel=0.0, sweeps=O.SWEEPS)
        b = O.plane(pts, sel, HELD[:3], gap_rel=0.0, sweeps=O.SWEEPS + 1)
        assert a["exists"] and a["n"] == b["n"] and a["dist"] == b["dist"] and a["gap"] == b["gap"] and diagonal(a["T"])
        assert diagonal(O.plane(pts, sel, HELD[:3], gap_rel=0.0, sweeps=O.SWEEPS - 1)["T"])
        s = 0
        while not diagonal(O.plane(pts, sel, HELD[:3], gap_rel=0.0, sweeps=s)["T"]):
            s += 1
        needed = max(needed, s)
    print(f"sweeps needed over {len(cases)} cases: {needed}")
    assert needed == O.SWEEPS - 1


def test_contact_sets_that_fix_no_plane_and_fits_that_do_not_exist():
    tab, n_contact, flag = SC.special_contacts()
    margins = []
    rows, rad, _ = O.sphere_series(tab, HELD, margins=margins)
    O.assert_margins(margins, "the special contact sets")
    assert rows[:, O.N_CONTACT].tolist() == n_contact.tolist() and rows[:, O.FLAG].tolist() == flag.tolist()
    assert (rows[[1, 2, 4, 5], O.NX:O.PLANE_RMS + 1] == 0.0).all() and (rows[[1, 2, 4, 5], O.DEPTH_MAX] > 0.4).all()
    assert rows[4, O.GAP] == 0.0 and rows[5, O.GAP] == 0.0 and rows[0, O.DEEPEST] == -1.0 and rows[1, O.DEEPEST] == 0.0
    assert (rows[0, O.N_CONTACT:O.GAP + 1] == [0.0] * 7 + [-1.0] + [0.0] * 13).all()
    # the fit: fewer than four slots, coincident points, points in a plane -> no sphere, a row of zeros but the counts
    lay = SC.cap65()
    for P, pred in ((lay, np.arange(65) < 3), (np.ones((65, 3)), np.ones(65, dtype=bool)),
                    (np.column_stack([lay[:, :2], np.full(65, 2.0)]), np.ones(65, dtype=bool))):
        row, rad, dec = O.frame(P, pred, np.ones(65, dtype=bool))
        assert row[O.FLAG] == 0.0 and row[O.N_FIT] == pred.sum() and row[O.N_USED] == 65.0 and row[O.DEEPEST] == -1.0
        assert (np.delete(row, [O.N_FIT, O.N_FIT_USED, O.N_USED, O.DEEPEST]) == 0.0).all() and (rad == 0.0).all() and (dec == 0.0).all()
    # contact_depth >= R: no slot can be that deep
    row, _, _ = O.frame(lay * 0.5, np.ones(65, dtype=bool), np.ones(65, dtype=bool), given=HELD, contact_depth=27.0)
    assert row[O.FLAG] == 1.0 and row[O.N_CONTACT] == 0.0


def test_the_rejection_removes_a_planted_slot_and_leaves_a_clean_frame_alone():
    rng = np.random.default_rng(5)
    lay = SC.cap65()
    clean = lay + rng.normal(size=lay.shape) * NOISE
    planted = clean.copy()
    planted[60] += 1.5 * (planted[60] - SC.C0) / SC.R0
    allm = np.ones(65, dtype=bool)
    a, _, _ = O.frame(planted, allm, allm, reject_k=3.0)
    b, _, _ = O.frame(planted, allm, allm, reject_k=0.0)
    assert a[O.REJECTED] == 1.0 and a[O.N_FIT_USED] == 64.0 and a[O.N_FIT] == 65.0 and b[O.REJECTED] == 0.0
    # (R of ONE noisy frame: the cap is 5.5 mm deep, so R = a^2 / (2 sagitta) carries the sagitta's noise with a lever of about 5;
    # 0.02 mm over 65 slots leaves R to some 0.05 mm - `test_the_algebraic_sphere_..` measures it -, the bound is 5 times that)
    assert abs(a[O.RADIUS] - 27.0) < 0.25 and a[O.RMS_FIT] < 1.5 * NOISE and b[O.RMS_FIT] > 5 * NOISE
    c, _, _ = O.frame(clean, allm, allm, reject_k=4.5)
    assert c[O.REJECTED] == 0.0 and c[O.N_FIT_USED] == 65.0 and abs(c[O.RADIUS] - 27.0) < 0.25


def _sigmas(pts, dist):
    """What NOISE allows a plane through the contact points `pts`: S the singular values of the centred points (S[1]^2 the smaller
    in-plane spread), l the lateral distance of the centroid from the foot of the centre on the plane.  The normal turns by
    sigma_angle = NOISE / S[1] about the weaker axis; the distance n . (C - cm) moves by the centroid's noise along n,
    NOISE / sqrt(k), and by the turn times l.  -> (sigma_offset mm, sigma_angle rad)."""
    n, d, cm, S = O.svd_plane(pts, HELD[:3])
    lever = (np.asarray(HELD[:3]) - cm) - d * n
    s_angle = NOISE / S[1]
    return float(np.sqrt(NOISE ** 2 / len(pts) + (s_angle ** 2) * float(lever @ lever))), float(s_angle)


def test_the_synthetic_press_is_recovered_within_what_its_noise_allows(press):
    """The cap cut at 0 -> 2.8 mm while leaning 0 -> 15 degrees towards 35, noise 0.02 mm, 3 % gaps, against the HELD sphere: offset,
    tilt, azimuth (where the tilt is >= 1 degree) and spot radius within 5 sigma of `_sigmas`; the spot radius sqrt(R^2 - dist^2)
    carries d a = (dist / a) d dist."""
    rows, delta, tilt = press["want"][0], press["delta"], press["tilt"]
    R = HELD[3]
    worst = dict(offset=0.0, tilt=0.0, azimuth=0.0, spot=0.0)
    worst_abs = dict(worst)
    flat = np.flatnonzero(rows[:, O.FLAG] == 3.0)
    for f in flat:
        s_off, s_ang = _sigmas(_contact_points(press, f), rows[f, O.DIST])
        a_true = np.sqrt(R * R - (R - delta[f]) ** 2)
        errs = dict(offset=(abs(rows[f, O.OFFSET] - delta[f]), s_off),
                    tilt=(abs(rows[f, O.TILT_DEG] - tilt[f]), np.rad2deg(s_ang)),
                    spot=(abs(rows[f, O.SPOT_RADIUS] - a_true), s_off * rows[f, O.DIST] / rows[f, O.SPOT_RADIUS]))
        if tilt[f] >= 1.0:
            errs["azimuth"] = (abs(rows[f, O.AZIMUTH_DEG] - press["azimuth"]), np.rad2deg(s_ang) / np.sin(np.deg2rad(tilt[f])))
        for name, (e, s) in errs.items():
            worst[name], worst_abs[name] = max(worst[name], e / s), max(worst_abs[name], e)
            assert e <= 5.0 * s, (f, name, e, s)
    print("synthetic press, worst errors: " + ", ".join(f"{k} {worst_abs[k]:.4f} ({worst[k]:.2f} sigma)" for k in worst)
          + f" over {len(flat)} frames with a plane")
    assert len(flat) >= 30
    # the first frame of contact is found while fewer than three slots are deeper than contact_depth, and not before the cut is that deep
    deep = np.array([(SC.true_depth(press["P"][f])[~press["dead"][f]] > DEPTH).sum() for f in range(len(delta))])
    first = int(np.argmax(rows[:, O.FLAG] >= 2.0))
    assert rows[first, O.FLAG] >= 2.0 and deep[first] < 3 and delta[first] > DEPTH - 5.0 * NOISE
    assert first <= int(np.argmax(deep >= 1)), "a slot deeper than contact_depth was not seen"


def test_a_sphere_fitted_per_frame_over_a_pressed_cap_is_wrong(press):
    """Why `bonnet_analysis` holds the sphere: at delta = 1.5 mm the all-marker fit of the pressed frame is off by more than 1 mm
    in R, with and without rejection; over the rim slots alone it is not."""
    lay = SC.cap65()
    P, _ = SC.press(lay, 1.5, 5.0, 35.0)
    P = P + np.random.default_rng(9).normal(size=P.shape) * NOISE
    allm = np.ones(65, dtype=bool)
    for rk in (0.0, 3.0):
        row, _, _ = O.frame(P, allm, allm, reject_k=rk)
        assert row[O.FLAG] >= 1.0 and abs(row[O.RADIUS] - 27.0) > 1.0, (rk, row[O.RADIUS])
    rim = (lay[:, :2] ** 2).sum(axis=1) > 10.0 ** 2
    row, _, _ = O.frame(P, rim, allm)
    # (the rim's 46 slots span 3.6 mm of sagitta only: R of one frame to some 0.1 mm, five times that allowed; the offset carries it)
    assert abs(row[O.RADIUS] - 27.0) < 0.5 and row[O.FLAG] == 3.0 and abs(row[O.OFFSET] - 1.5) < 0.5


def test_decomp_splits_a_push_and_a_turn_in_the_shells_own_frame():
    lay = SC.cap65()
    C = SC.C0
    allm = np.ones(65, dtype=bool)
    h = (lay - C) / SC.R0
    push = O.decompose(lay - 0.3 * h, lay, allm, list(C))        # a pure radial push of 0.3 mm towards the centre
    assert (push[:, 0] == 1.0).all() and np.abs(push[:, 1] + 0.3).max() < 1e-14 and np.abs(push[:, 2:]).max() < 1e-14
    t = np.deg2rad(0.1)
    turn = O.decompose(lay @ np.array([[np.cos(t), np.sin(t), 0.0], [-np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]]), lay, allm, list(C))
    r = np.sqrt((lay[:, :2] ** 2).sum(axis=1))
    assert np.abs(turn[1:, 3] - r[1:] * t).max() < 1e-6 * r.max()            # the azimuthal part is r theta to first order
    assert np.abs(turn[:, 1:3]).max() < r.max() * t * t                      # the rest is of second order
    # the apex rule: Q below the centre exactly -> e_mer = (1, 0, 0), e_az = (0, 1, 0)
    D = np.array([0.25, -0.5, 0.125])
    apex = O.decompose((lay[0] + D)[None], lay[:1], np.ones(1, dtype=bool), list(C))
    assert lay[0, 0] == 0.0 and lay[0, 1] == 0.0 and apex[0].tolist() == [1.0, -0.125, 0.25, -0.5]
    # Q at the centre has no normal: flag 0
    assert (O.decompose(lay[:1], C[None], np.ones(1, dtype=bool), list(C)) == 0.0).all()
    # the three directions are orthonormal: |D|^2 = d_n^2 + d_mer^2 + d_az^2
    rng = np.random.default_rng(3)
    Dm = rng.normal(size=lay.shape)
    dec = O.decompose(lay + Dm, lay, allm, list(C))
    assert np.abs((dec[:, 1:] ** 2).sum(axis=1) - (Dm ** 2).sum(axis=1)).max() < 1e-13


def test_the_host_module_agrees_with_the_columns(press):
    from vbs_amd import sphere as SP
    rows = press["want"][0]
    assert SP.SPHERE_COLS == O.SPHERE_COLS == len(SP.SPHERE_COLUMNS) and SP.SPHERE_SWEEPS == O.SWEEPS
    for name in ("FLAG", "RADIUS", "N_CONTACT", "DEEPEST", "OFFSET", "SPOT_RADIUS", "TILT_DEG", "AZIMUTH_DEG", "PLANE_RMS", "GAP"):
        assert getattr(SP, name) == getattr(O, name), name
    s = SP.summary(rows)
    flat = rows[:, O.FLAG] == 3.0
    assert np.array_equal(s["kind"], rows[:, O.FLAG].astype(np.int64)) and s["first_contact"] == int(np.argmax(rows[:, O.FLAG] >= 2.0))
    assert np.array_equal(s["offset"][flat], rows[flat, O.OFFSET]) and np.isnan(s["offset"][~flat]).all()
    assert s["max_offset_frame"] == len(rows) - 1 and s["max_tilt_frame"] >= len(rows) - 3
    assert abs(sum(s["share"].values()) - 1.0) < 1e-12 and s["share"]["flat"] == flat.mean()
    assert np.abs(SP.spot(27.0, rows[flat, O.OFFSET]) - rows[flat, O.SPOT_RADIUS]).max() < 1e-12
    assert SP.spot(27.0, -1.0) == 0.0 and SP.spot(27.0, 30.0) == 27.0 and abs(SP.spot(27.0, 0.7) - 6.11) < 0.01
    tilt, az = SP.normal_angles(rows[flat, O.NX:O.NZ + 1])
    assert np.abs(tilt - rows[flat, O.TILT_DEG]).max() < 1e-12 and np.abs(az - rows[flat, O.AZIMUTH_DEG]).max() < 1e-12
    rec = SP.trend_record(rows)
    assert rec.shape == (len(rows), 1, 8) and np.array_equal(rec[:, 0, 0], flat.astype(np.float64)) and (rec[~flat] == 0.0).all()
    # a filter that passes its input: the trend is the rows' own, the normal renormalised
    f = np.concatenate([np.where(flat, 3.0, 0.0)[:, None, None], rec[:, :, 1:], np.zeros((len(rows), 1, 7))], axis=2)
    tr = SP.trend(f)
    assert tr.shape == (len(rows), 10) and np.array_equal(tr[:, 0], flat.astype(np.float64)) and (tr[~flat] == 0.0).all()
    assert np.abs(tr[flat, 8] - rows[flat, O.TILT_DEG]).max() < 1e-9 and np.abs(tr[flat, 1] - rows[flat, O.OFFSET]).max() == 0.0
    # combine: the median sphere of per-frame fits over unloaded frames, and its scatter
    still = SC.press_recording(1, still=7, delta_end=0.0, seed=4)
    fits, _, _ = O.sphere_series(still["table"], reject_k=3.0)
    held = SP.combine(fits)
    assert held["frames"] == 8 and np.abs(held["sphere"] - HELD).max() < 0.05 and (held["scatter"] < 0.1).all() and held["rms"] < 2 * NOISE
    with pytest.raises(ValueError):
        SP.combine(np.zeros((3, O.SPHERE_COLS)))
    # rim_slots: the outer share of the valid source slots
    src = RC.source_of(SC.cap65(), np.arange(65) == 64)
    rim = SP.rim_slots(src, 0.4)
    rr = (SC.cap65()[:, :2] ** 2).sum(axis=1)
    assert len(rim) == 26 and 64 not in rim and rr[rim].min() >= np.sort(rr[:64])[-26] and (np.diff(rim) > 0).all()
    with pytest.raises(ValueError):
        SP.rim_slots(src, 0.0)
    # offset_steps: the mean offset of the frames with a plane per dwell
    st = SP.offset_steps(rows, [0, 20, 30], [10, 30, 40])
    assert st["count"].tolist() == [int(flat[:10].sum()), 10, 10] and abs(st["offset"][2] - rows[30:40, O.OFFSET].mean()) < 1e-12
    assert st["delta"].shape == (2,) and abs(st["delta"][1] - (st["offset"][2] - st["offset"][1])) < 1e-15
    with pytest.raises(ValueError):
        SP.offset_steps(rows, [0], [len(rows) + 1])


def test_the_shim_refuses_what_the_header_refuses_without_a_device():
    from vbs_amd import engine as E
    n, m = 4, 12
    good = dict(n=n, m=m, sphere=None, source_shape=(m, 4), fit_slots=None, slots=None, contact_depth=0.1, piv_rel=1e-9, gap_rel=1e-3,
                reject_k=0.0, frame_range=None, want=None)
    assert E._sphere_args(**good) == (0, n, None, ("sphere", "radial", "decomp"))
    assert E._sphere_args(**dict(good, source_shape=None)) == (0, n, None, ("sphere", "radial"))
    a, b, sph, want = E._sphere_args(**dict(good, sphere=HELD, frame_range=(1, 3), want="radial", slots=[0, m - 1], fit_slots=[3]))
    assert (a, b, want) == (1, 3, ("radial",)) and sph.tolist() == list(HELD) and sph.dtype == np.float64
    bad = [dict(n=0), dict(m=0), dict(source_shape=(m, 3)), dict(source_shape=(m + 1, 4)), dict(contact_depth=0.0),
           dict(contact_depth=-0.1), dict(contact_depth=np.nan), dict(contact_depth=np.inf), dict(piv_rel=-1e-9), dict(piv_rel=np.nan),
           dict(gap_rel=-1e-9), dict(gap_rel=np.inf), dict(reject_k=-1.0), dict(reject_k=np.nan), dict(frame_range=(2, 1)),
           dict(frame_range=(0, n + 1)), dict(frame_range=(-1, 2)), dict(slots=[m]), dict(fit_slots=[-1]), dict(want=()),
           dict(want=("pose",)), dict(sphere=(0.0, 0.0, 27.0, 0.0)), dict(sphere=(0.0, 0.0, 27.0, -1.0)),
           dict(sphere=(0.0, np.nan, 27.0, 27.0)), dict(sphere=(0.0, 0.0, 27.0, np.inf)), dict(sphere=(0.0, 0.0, 27.0)),
           dict(source_shape=None, want=("decomp",))]
    for change in bad:
        with pytest.raises(ValueError):
            E._sphere_args(**dict(good, **change))


def test_radial_and_decomp_are_records_of_the_filter_and_of_the_field_map():
    from vbs_amd import analysis as A
    k = SC.recording(4, 12, seed=2, drop=0.0, bad_src=0.0)
    _, rad, dec = O.sphere_series(k["table"], source=k["source"])
    for rec, nv in ((rad, 1), (dec, 3)):
        F, s, cols = rec.shape
        assert A._n_values(cols, nv, None) == nv and cols == nv + 1
