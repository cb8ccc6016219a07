"""CPU tests of the rigid motion (`vbs_rigid_series`), all on the NumPy restatement `tests/helpers/rigid_oracle.py` the
device is held to bit for bit (`tests/test_gpu_rigid.py`): Horn's form against an SVD Kabsch fit with the determinant fix and
Umeyama's scale, the exact cases, the sweep count, every degeneracy, the rejection, the host module `vbs_amd.rigid`, the argument
checks of the Python shim, and two synthetic recordings of the 65-marker shell."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pose_oracle as PO                                       # noqa: E402
import rigid_cases as RC                                       # noqa: E402
import rigid_oracle as O                                       # noqa: E402

# max(|R - R_svd|, |s - s_svd|, |t - t_svd| / max(1, |qm|, |pm|)) over the cases of `_svd_cases`: 10 x the MEASURED_DEV this file
# measures on the CPU (the translation carries the lever of the centroid: an error of R of 1e-15 moves t by 1e-15 |qm|)
MEASURED_DEV = 6.442e-15
RIGID_TOL = 10 * MEASURED_DEV
ANGLES = (0.01, 0.5, 2.0, 30.0, 90.0, 179.9, 180.0)
NOISE = 0.02                                                    # mm, every coordinate of the synthetic recordings
ALL65 = np.ones(65, dtype=bool)


def _svd_cases():
    """(name, Q, P, with_scale): a curved and a flat cloud, at the origin and 40 m from it, seven angles, with and without scale."""
    rng = np.random.default_rng(2024)
    for shell in (True, False):
        lay = RC.layout65(shell)
        for off in (0.0, 40000.0):
            for ang in ANGLES:
                for ws in (False, True):
                    R, t, s = RC.rotation(rng.normal(size=3), ang), rng.normal(size=3) * 3.0, 1.07 if ws else 1.0
                    Q = lay + np.array([off, -0.5 * off, 0.25 * off])
                    yield f"shell={shell} off={off} angle={ang} scale={ws}", Q, RC.moved(Q, R, t, s) + rng.normal(size=lay.shape) * 0.01, ws


def test_horn_agrees_with_an_svd_kabsch_fit():
    worst = 0.0
    for name, Q, P, ws in _svd_cases():
        f = O.fit(Q, P, ALL65, ws)
        assert f["exists"], (name, f["gap"])
        R, t, s = O.svd_fit(Q, P, ws)
        lever = max(1.0, float(np.abs(f["qm"]).max()), float(np.abs(f["pm"]).max()))
        dev = max(float(np.abs(np.asarray(f["R"]) - R).max()), abs(f["s"] - s), float(np.abs(np.asarray(f["t"]) - t).max()) / lever)
        worst = max(worst, dev)
        assert abs(np.linalg.det(np.asarray(f["R"])) - 1.0) <= RIGID_TOL
    print(f"Horn vs SVD: worst deviation {worst:.3e} (bound {RIGID_TOL:.1e})")
    assert worst <= RIGID_TOL


def test_the_same_points_give_the_identity_exactly():
    for shell in (True, False):
        lay = RC.layout65(shell).astype(np.float32).astype(np.float64) + np.array([1024.0, -512.0, 40.0])
        row, coef, res, _ = O.frame(lay, lay, ALL65, with_scale=False)
        assert row[0] == 1.0 and row[1] == 65.0 and row[9:13].tolist() == [1.0, 0.0, 0.0, 0.0]
        assert row[13:22].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and row[22:26].tolist() == [0.0, 0.0, 0.0, 1.0]
        assert (row[26:32] == 0.0).all() and (res[:, 1:] == 0.0).all() and (res[:, 0] == 1.0).all()
        assert coef.tolist() == [[1.0, 1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0]]


def test_a_dyadic_translation_of_dyadic_points_is_exact():
    k = (np.arange(6) * 2 - 5) / 2.0
    gx, gy = np.meshgrid(k, k)
    Q = np.column_stack([gx.ravel(), gy.ravel(), 0.25 * (gx.ravel() ** 2 + gy.ravel() ** 2)]) + np.array([64.0, -32.0, 8.0])
    t = np.array([3.5, -1.25, 0.75])
    row, _, res, _ = O.frame(Q, Q + t, np.ones(36, dtype=bool), with_scale=True)
    assert row[0] == 1.0 and row[13:22].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert row[22:25].tolist() == t.tolist() and row[25] == 1.0 and row[26] == 0.0 and (res[:, 1:] == 0.0).all()
    assert row[27] == float(np.sqrt(t @ t))


def _recordings():
    plain = RC.tilt_twist_recording(12, seed=3)
    dimple = RC.tilt_twist_recording(12, seed=3, dimple=(4.0, -3.0, 0.3, 2.5))
    return plain, dimple


def test_a_ninth_sweep_changes_no_bit_of_the_rotation():
    cases = [(Q, P, ALL65, ws) for _, Q, P, ws in _svd_cases()]
    for k in _recordings():
        Q, P, common = O.common_points(k["table"], k["source"])
        cases += [(Q, P[f], common[f], False) for f in range(P.shape[0])]
    lay = RC.layout65()
    cases.append((lay, lay * np.array([-1.0, 1.0, 1.0]), ALL65, False))
    for Q, P, pred, ws in cases:
        a, b = O.fit(Q, P, pred, ws, sweeps=O.SWEEPS), O.fit(Q, P, pred, ws, sweeps=O.SWEEPS + 1)
        assert a["exists"] and a["R"] == b["R"] and a["quat"] == b["quat"] and a["t"] == b["t"] and a["s"] == b["s"]
        T = a["T"]
        assert all(T[i][j] == 0.0 for i in range(4) for j in range(4) if i != j)


def test_a_mirrored_cloud_gives_a_proper_rotation_with_a_large_rms():
    lay = RC.layout65()
    row, _, _, _ = O.frame(lay, lay * np.array([-1.0, 1.0, 1.0]), ALL65)
    R = row[13:22].reshape(3, 3)
    assert row[0] == 1.0 and abs(np.linalg.det(R) - 1.0) <= RIGID_TOL and np.abs(R @ R.T - np.eye(3)).max() <= RIGID_TOL
    assert row[26] > 1.0                                          # mm: the shell's heights cannot be mirrored by a rotation


def test_sets_that_fix_no_rotation_give_flag_zero():
    lay = RC.layout65()
    R = RC.rotation((0.2, 0.3, 0.9), 20.0)
    P = RC.moved(lay, R, (1.0, 2.0, 3.0))
    t = np.linspace(-5.0, 5.0, 65)
    line = np.column_stack([1.0 + 0.6 * t, -2.0 + 0.8 * t, 0.5 * t])
    sets = {"collinear": (line, RC.moved(line, R, (0.5, 0.0, 0.0)), ALL65),
            "coincident frame": (lay, np.broadcast_to(np.array([1.0, 2.0, 3.0]), (65, 3)).copy(), ALL65),
            "coincident source": (np.zeros((65, 3)), P, ALL65), "all coincident": (np.ones((65, 3)), np.ones((65, 3)), ALL65)}
    for c in (0, 1, 2):
        sets[f"count {c}"] = (lay, P, np.arange(65) < c)
    for name, (Q, Pf, pred) in sets.items():
        row, coef, res, _ = O.frame(Q, Pf, pred, reject_k=3.0)
        c = float(pred.sum())
        assert row[0] == 0.0 and row[1] == c and row[2] == c, name
        assert (row[9:32] == 0.0).all() and (coef == 0.0).all() and (res == 0.0).all(), name
        if c >= 1:
            assert np.allclose(row[3:6], Q[pred].mean(axis=0)) and np.allclose(row[6:9], Pf[pred].mean(axis=0)), name
        else:
            assert (row[3:9] == 0.0).all()
        assert 0.0 <= row[32] <= 1e-6, (name, row[32])
    three = np.arange(65) < 3
    assert O.frame(lay, P, three)[0][0] == 1.0                     # three points off a line do fix it


def test_nearest_rotation_returns_a_rotation():
    from vbs_amd import rigid as RG
    rng = np.random.default_rng(5)
    Rs = np.stack([RC.rotation(rng.normal(size=3), a) for a in ANGLES + (0.0,)])
    back = RG.nearest_rotation(Rs)
    assert back.shape == Rs.shape and np.abs(back - Rs).max() <= RIGID_TOL
    noisy = Rs + rng.normal(size=Rs.shape) * 0.05
    near = RG.nearest_rotation(noisy)
    for A, M in zip(near, noisy):
        assert np.abs(A @ A.T - np.eye(3)).max() <= RIGID_TOL and abs(np.linalg.det(A) - 1.0) <= RIGID_TOL
        U, _, Vt = np.linalg.svd(M)                               # the Frobenius-nearest rotation by the other algorithm
        d = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        assert np.abs(A - U @ d @ Vt).max() <= RIGID_TOL
    assert np.isnan(RG.nearest_rotation(np.full((3, 3), np.nan))).all()
    ang = RG.angles(RC.swing_twist(2.0, 35.0, 3.0))
    assert np.allclose(ang[1:], (2.0, 35.0, 3.0), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        RG.nearest_rotation(np.zeros((3, 2)))


def test_the_host_module_agrees_with_the_columns():
    from vbs_amd import rigid as RG
    k = RC.recording(5, 30, seed=1, drop=0.1, bad_src=0.1)
    rigid, _, _ = O.rigid_series(k["table"], k["source"])
    assert (rigid[:, 0] == 1.0).all()
    ang = RG.angles(rigid[:, 13:22].reshape(-1, 3, 3))
    assert np.allclose(ang, rigid[:, 28:32], rtol=0, atol=1e-10)
    share = RG.rigid_share(rigid[:, 26], rigid[:, 27])
    assert share[0] != share[0] or share[0] <= 1.0               # frame 0 barely moves: the share means little there
    assert (share[2:] > 0.99).all() and np.isnan(RG.rigid_share(0.0, 0.0))
    src = RG.source_from_table(k["table"], 0)
    xyz = (k["table"][0, :, 0].astype(np.int64) & 2) != 0
    assert src.shape == (30, 4) and np.array_equal(src[:, 0], xyz.astype(np.float64)) and np.isfinite(src).all()
    assert np.array_equal(src[xyz, 1:], k["table"][0, xyz, 6:9].astype(np.float64))
    lay = k["layout"].copy()
    lay[3, 1] = np.nan
    sl = RG.source_from_layout(lay, valid=np.arange(30) != 7)
    assert sl[3].tolist() == [0.0] * 4 and sl[7].tolist() == [0.0] * 4 and sl[:, 0].sum() == 28.0 and np.array_equal(sl[0, 1:], lay[0])
    rows = np.zeros((6, 33))
    rows[1:, 0] = 1.0
    rows[2, 6] = 1.0                                              # a shift of the centroid of 1 mm
    rows[3, 29] = 2.0
    rows[4, 31] = -3.0
    rows[5, 29], rows[5, 31] = 2.0, 3.0
    assert [RG.KIND_NAMES[i] for i in RG.kind(rows)] == ["none", "still", "shift", "tilt", "twist", "mixed"]
    assert RG.kind(rows[3], tilt_deg=5.0).tolist() == [RG.KIND_STILL]


def test_one_gross_outlier_is_dropped_and_the_fit_becomes_the_clean_one():
    rng = np.random.default_rng(11)
    Q = RC.flat_grid(30, 2.0, seed=4)
    Q[:, 2] = 0.02 * (Q[:, 0] ** 2)
    P = RC.moved(Q, RC.rotation((0.4, 0.1, 0.9), 7.0), (0.5, -0.25, 1.0)) + rng.normal(size=Q.shape) * 0.01
    P[11] += np.array([1.5, -1.0, 2.0])
    pred = np.ones(30, dtype=bool)
    first = O.frame(Q, P, pred)
    again = O.frame(Q, P, pred, reject_k=3.0)
    clean = O.frame(Q, P, np.arange(30) != 11)
    assert first[0][0] == 1.0 and first[0][2] == 30.0 and again[0][0] == 2.0 and again[0][1] == 30.0 and again[0][2] == 29.0
    assert np.array_equal(again[0][3:], clean[0][3:]) and np.array_equal(again[1][:, 1:], clean[1][:, 1:])
    assert np.array_equal(again[2], clean[2]) and again[2][11].tolist() == [0.0] * 4
    assert again[0][26] < 0.03 < 0.3 < first[0][26]


def test_the_first_fit_stands_where_the_kept_set_fixes_no_rotation():
    """Four points: three nearly on a line and one off it, which alone carries the error.  Rejection drops it; the kept three are
    collinear to the gap rule, so the first fit stands with flag 1."""
    Q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0, 0.0]])
    P = Q.copy()
    P[3] += np.array([0.0, 0.0, 0.4])
    P[:3] += np.array([[0.0, 0.0, 1e-3], [0.0, 0.0, -2e-3], [0.0, 0.0, 1e-3]])
    pred = np.ones(4, dtype=bool)
    first, again = O.frame(Q, P, pred), O.frame(Q, P, pred, reject_k=1.0)
    e = first[2][:, 1:]
    assert ((e * e).sum(axis=1) > (first[0][26] ** 2)).any(), "the case rejects nothing"
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(a, b)
    assert again[0][0] == 1.0 and again[0][2] == 4.0


def test_the_shim_refuses_what_the_header_refuses_without_a_device():
    from vbs_amd import engine as E
    n, m = 4, 12
    good = dict(n=n, m=m, source_shape=(m, 4), slots=None, with_scale=False, reject_k=0.0, gap_rel=1e-6, frame_range=None,
                want=("rigid", "coef", "residual"))
    assert E._rigid_args(**good) == (0, n, 0, ("rigid", "coef", "residual"))
    assert E._rigid_args(**dict(good, with_scale=True, frame_range=(1, 3), want="coef", slots=[0, m - 1])) == (1, 3, 1, ("coef",))
    bad = [dict(n=0), dict(m=0), dict(source_shape=(m, 3)), dict(source_shape=(m + 1, 4)), dict(source_shape=(m * 4,)),
           dict(with_scale=2), dict(with_scale=0.5), dict(reject_k=-1.0), dict(reject_k=np.inf), dict(reject_k=np.nan),
           dict(gap_rel=-1e-9), dict(gap_rel=np.inf), dict(gap_rel=np.nan), dict(frame_range=(2, 1)), dict(frame_range=(0, n + 1)),
           dict(frame_range=(-1, 2)), dict(slots=[m]), dict(slots=[-1]), dict(want=()), dict(want=("pose",))]
    for change in bad:
        with pytest.raises(ValueError):
            E._rigid_args(**dict(good, **change))


def test_coef_and_residual_are_records_of_the_filter_and_of_the_field_map():
    from vbs_amd import analysis as A
    k = RC.recording(4, 12, seed=2, drop=0.0, bad_src=0.0)
    _, coef, res = O.rigid_series(k["table"], k["source"])
    F, s, cols = coef.shape
    A._record_shape(F, s, cols)
    assert (F, s, cols) == (4, 4, 4) and A._n_values(cols, 3, None) == 3 and (coef[..., 0] == 1.0).all()
    Fr, m, rc = res.shape
    assert A._field_args(Fr, m, rc, 5, (5, m), (5,), 0.5, None, None) == (0, Fr, 3)
    assert set(np.unique(res[..., 0]).tolist()) <= {0.0, 1.0}


# ---- synthetic recordings ---------------------------------------------------------------------------------------------------------------
def _sigmas(k):
    """The standard deviations of tilt and twist (degrees) the noise allows, per frame - NOT from what the fit gave.  A rotation by a
    small angle about an axis through the centroid moves marker i by (its distance r_i from the axis) x angle, so the least-squares
    angle of isotropic noise sigma on the frame's points alone (the source is the exact layout) has the variance sigma^2 / sum r_i^2,
    the sum over the frame's common markers: the moment of the cloud about that axis.  Tilt: the in-plane axis with the SMALLER
    moment bounds both in-plane axes; twist: the z axis.  For the full layout: sum (x^2 + z^2) = 3990 mm^2 and sum (x^2 + y^2) = 7883
    mm^2, so sigma_tilt = 0.02 / 63.2 rad = 0.018 deg and sigma_twist = 0.02 / 88.8 rad = 0.013 deg."""
    _, _, common = O.common_points(k["table"], k["source"])
    lay = k["layout"]
    st, sw = [], []
    for c in common:
        d = lay[c] - lay[c].mean(axis=0)
        ix, iy, iz = (d[:, 1] ** 2 + d[:, 2] ** 2).sum(), (d[:, 0] ** 2 + d[:, 2] ** 2).sum(), (d[:, 0] ** 2 + d[:, 1] ** 2).sum()
        st.append(np.degrees(NOISE / np.sqrt(min(ix, iy))))
        sw.append(np.degrees(NOISE / np.sqrt(iz)))
    return np.array(st), np.array(sw)


def test_a_tilting_and_twisting_shell_gives_its_tilt_azimuth_and_twist():
    """0 -> 2 degrees of tilt towards 35 degrees and 0 -> 3 degrees of twist, 0.02 mm noise, 3 % gaps.  Bounds: 5 sigma of `_sigmas`;
    the azimuth is the direction of a lean of size tilt, so its sigma is sigma_tilt / sin(tilt): it is held where the true tilt is
    at least 1 degree (5 sigma = 5.2 degrees there, 2.6 degrees at the end)."""
    k, _ = _recordings()
    rigid, _, res = O.rigid_series(k["table"], k["source"])
    assert (rigid[:, 0] == 1.0).all() and (rigid[:, 1] >= 55.0).all() and (rigid[:, 1] < 65.0).any()
    st, sw = _sigmas(k)
    assert (st < 0.021).all() and (sw < 0.015).all()
    d_tilt, d_twist = np.abs(rigid[:, 29] - k["tilt"]), np.abs(rigid[:, 31] - k["twist"])
    lean = k["tilt"] >= 1.0
    d_az = np.abs(rigid[lean, 30] - k["azimuth"])
    az_bound = 5.0 * st[lean] / np.sin(np.radians(k["tilt"][lean]))
    # the plane of pose_series on the same recording, reported next to them: a plane fitted to the heights of a curved shell
    rd = np.zeros((65, 4))
    rd[:, 0] = 1.0
    pose = PO.pose_series(k["table"], rd, k["layout"], 0, shell=True)[2]
    for f in range(rigid.shape[0]):
        print(f"frame {f:2d}: tilt {k['tilt'][f]:.3f} -> rigid {rigid[f, 29]:.3f}, plane {pose[f, 4]:.3f} deg; twist {k['twist'][f]:.3f} -> "
              f"{rigid[f, 31]:.3f} deg; azimuth -> {rigid[f, 30]:.2f} (plane {pose[f, 5]:.2f}); rms {rigid[f, 26]:.4f} mm")
    print(f"worst |tilt error| {d_tilt.max():.4f} deg (5 sigma {5 * st.max():.4f}), |twist error| {d_twist.max():.4f} ({5 * sw.max():.4f}), "
          f"|azimuth error| {d_az.max():.3f} ({az_bound.max():.3f})")
    assert (d_tilt <= 5.0 * st).all() and (d_twist <= 5.0 * sw).all() and (d_az <= az_bound).all()
    # what is left is the noise: three coordinates per marker, less the six of the motion
    assert (np.abs(rigid[:, 26] / (NOISE * np.sqrt(3.0)) - 1.0) < 0.25).all()


def test_a_dimple_shows_in_the_residual_map_and_hardly_moves_the_rigid_columns():
    """The same recording with a Gaussian dimple of 0.3 mm (width 2.5 mm) pressed in at (4, -3) mm.  The dimple is a field d_i along
    the layout's -Z; a least-squares fit projects it onto the six rigid modes, and the projection onto a unit mode is at most |d| =
    sqrt(sum d_i^2).  So the angles move by at most |d| / sqrt(sum r_i^2) (`_sigmas`'s moments: |d| / NOISE x sigma) and the centroid
    by at most |d| / sqrt(n); both recordings carry the same noise, so nothing else differs to first order."""
    from vbs_amd import fields
    plain, dimple = _recordings()
    a, _, _ = O.rigid_series(plain["table"], plain["source"])
    b, _, res = O.rigid_series(dimple["table"], dimple["source"])
    lay = plain["layout"]
    x, y, depth, width = 4.0, -3.0, 0.3, 2.5
    d = depth * np.exp(-((lay[:, 0] - x) ** 2 + (lay[:, 1] - y) ** 2) / (2.0 * width * width))
    dn = float(np.sqrt((d * d).sum()))
    st, sw = _sigmas(dimple)
    f = a.shape[0] - 1
    moved = (abs(b[f, 29] - a[f, 29]), abs(b[f, 31] - a[f, 31]), float(np.abs((b[f, 6:9] - b[f, 3:6]) - (a[f, 6:9] - a[f, 3:6])).max()))
    bounds = (dn / NOISE * st[f], dn / NOISE * sw[f], dn / np.sqrt(a[f, 1]))
    print(f"dimple |d| = {dn:.3f} mm: tilt moved {moved[0]:.4f} deg (bound {bounds[0]:.4f}), twist {moved[1]:.4f} ({bounds[1]:.4f}), "
          f"centroid {moved[2]:.4f} mm ({bounds[2]:.4f})")
    assert all(m <= bd for m, bd in zip(moved, bounds))
    # the map of |e| on a grid of 2 mm: its peak lies within one cell of the dimple
    pitch = 2.0
    g = np.arange(-14.0, 14.0 + pitch / 2, pitch)
    grid_xy = np.stack([c.ravel() for c in np.meshgrid(g, g)], axis=1)
    W = fields.gaussian_weights(lay[:, :2], grid_xy, 2.0)
    used = res[f, :, 0] == 1.0
    mag = np.sqrt((res[f, :, 1:] ** 2).sum(axis=1))
    den = (W * used[None]).sum(axis=1)
    covered = den >= 0.5 * fields.row_sums(W)
    mp = np.where(covered, (W * (used * mag)[None]).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0)
    peak = grid_xy[int(np.argmax(mp))]
    print(f"residual map: peak {mp.max():.3f} mm at {peak.tolist()}")
    assert abs(peak[0] - x) <= pitch and abs(peak[1] - y) <= pitch and mp.max() > 5.0 * NOISE
