"""CPU tests of the indentation shape (`vbs_shape_series`), all on the NumPy restatement
`tests/helpers/shape_oracle.py` the device is held to bit for bit (`tests/test_gpu_shape.py`): the factorisation against
`np.linalg.lstsq` of the design matrix, the degree-1 prefix against `pose_oracle`'s plane, exact inputs, a rendered spherical cap,
every degeneracy and both outcomes of the rejection, and the argument checks of the Python shim."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pose_oracle as PO                                       # noqa: E402
import shape_cases as SC                                       # noqa: E402
import shape_oracle as O                                       # noqa: E402
import uncert_cases as UC                                      # noqa: E402

# max|beta - lstsq| / max(1, max|beta|) over the exact quadrics below: 10 x the 1.081e-15 this file measures on the CPU
BETA_TOL = 1.1e-14
# the degree-1 prefix against pose_oracle's closed form, (a, b, the plane at the mean) relative to max(1, |a|, |b|, |value|):
# 10 x the measured 2.527e-14 (the case 40000 mm from the origin: pose_oracle's c = mz - a mx - b my cancels there)
PLANE_TOL = 2.6e-13
# The rendered cap (R = 60 mm, field radius A = 13.4 mm, n = 61 markers, 0.05 px noise on a 30 px diameter at h = 40 mm: sigma_z = h
# 0.05 / 30 = 0.067 mm).  NOT from what the fit gave: on a disc Var(x^2) = A^4 / 16, so sigma_p = 8 sigma_z / (sqrt(n) A^2) = 3.8e-4
# per mm = 2.3 % of 1 / R, up to 1.5 x that for an eigenvalue of the noisy Hessian (3.5 %); a quadric through a sphere is biased by
# about (3 / 8) (A / R)^2 = 2 %.  Bound: bias + 5 sigma = 0.20.  The gradient has sigma_a = 2 sigma_z / (sqrt(n) A) = 1.3e-3, the
# apex moves by sigma_a R = 0.077 mm per axis: 5 sqrt(2) sigma = 0.55 mm.  Measured over seeds 0 .. 3: 0.069 and 0.187 mm.
CAP_K_TOL, CAP_APEX_TOL = 0.20, 0.55
CAP_R, CAP_CENTRE, CAP_DEPTH = 60.0, (1.5, -1.0), 1.0

QUADRICS = [  # m, seed, angle, offset, (c0, a, b, p, q, r)
    (9, 0, 0.0, (0.0, 0.0), (0.2, 0.01, -0.02, 0.05, 0.01, 0.03)),
    (30, 1, 33.0, (1234.5, -987.25), (-3.0, 0.05, 0.02, 0.08, -0.02, 0.04)),
    (65, 2, 71.0, (-40000.0, 25000.0), (12.0, -0.03, 0.04, -0.06, 0.03, 0.02)),
    (129, 3, 12.5, (300.125, 800.5), (0.0, 0.2, -0.1, 0.01, 0.0, -0.015)),
]


def _points(m, seed, angle, offset, coeffs, noise=0.0):
    xy = SC.irregular_xy(m, seed, angle, offset)
    centre = xy.mean(axis=0)
    z = SC.quadric_z(xy, centre, coeffs)
    if noise:
        z = z + np.random.default_rng(seed).normal(size=m) * noise
    return np.column_stack([xy, z])


def test_the_factorisation_agrees_with_lstsq_on_exact_quadrics():
    worst = 0.0
    for m, seed, angle, offset, coeffs in QUADRICS:
        P = _points(m, seed, angle, offset, coeffs)
        pred = np.ones(m, dtype=bool)
        length = SC.rms_length(P[:, :2])
        f = O.fit(P, pred, length, 9, 1e-10)
        assert f["degree"] == 2 and f["npass"] == 6, (m, f["npass"])
        want = O.lstsq_quadric(P, f["mean"], length)
        err = float(np.abs(np.asarray(f["beta"]) - want).max()) / max(1.0, float(np.abs(want).max()))
        worst = max(worst, err)
        # and the columns say what was put in: gradient and Hessian of the quadric at the mean
        row = O.frame(P, pred, length)[0]
        c0, a, b, p, q, r = coeffs
        assert np.allclose(row[9:12], (p, q, r), rtol=0, atol=1e-9) and row[0] == 2.0 and row[13] < 1e-9
    print(f"beta vs lstsq: worst relative deviation {worst:.3e} (bound {BETA_TOL:.1e})")
    assert worst <= BETA_TOL


def test_the_degree_one_prefix_agrees_with_the_plane_of_pose_series():
    worst = 0.0
    for m, seed, angle, offset, coeffs in QUADRICS:
        P = _points(m, seed, angle, offset, coeffs, noise=0.02)
        pred = np.ones(m, dtype=bool)
        length = SC.rms_length(P[:, :2])
        f = O.fit(P, pred, length, 9, 1e-10)
        exists, a, b, c, _, _ = PO._plane(P[None], pred[None], np.array([m]))
        assert exists[0]
        mean, g = f["mean"], f["gam"]
        ours = np.array([g[1] / length, g[2] / length, mean[2] + g[0]])
        theirs = np.array([a[0], b[0], (c[0] + a[0] * mean[0]) + b[0] * mean[1]])
        worst = max(worst, float(np.abs(ours - theirs).max()) / max(1.0, float(np.abs(theirs).max())))
    print(f"degree-1 prefix vs pose_oracle: worst relative deviation {worst:.3e} (bound {PLANE_TOL:.1e})")
    assert worst <= PLANE_TOL


def test_exact_inputs_give_exact_coefficients():
    """An 8 x 8 grid of half-odd integers moved by whole numbers, length 4, dyadic coefficients: the means, every monomial and
    every sum are exact, the normal matrix of a product grid has only dyadic or zero multipliers, so every coefficient is exact."""
    k = (np.arange(8) * 2 - 7) / 2.0
    gx, gy = np.meshgrid(k, k)
    centre = np.array([1024.0, -512.0])
    xy = np.column_stack([gx.ravel(), gy.ravel()]) + centre
    c0, a, b, p, q, r = 3.0, 0.25, -0.125, 0.5, 0.0625, -0.25
    P = np.column_stack([xy, SC.quadric_z(xy, centre, (c0, a, b, p, q, r))])
    row, coef, res, _ = O.frame(P, np.ones(64, dtype=bool), 4.0)
    assert row[0] == 2.0 and row[1] == 64.0 and row[3:6].tolist() == [1024.0, -512.0, c0 + (p + r) * 5.25 / 2.0]
    assert row[6:12].tolist() == [c0, a, b, p, q, r]
    assert row[13] == 0.0 and (res[:, 1] == 0.0).all() and (res[:, 0] == 1.0).all()
    assert row[14] == (p + r) / 2.0 and row[15] == p * r - q * q
    assert coef.tolist() == [[2.0, c0, a, b], [1.0, p, q, r]]


def _cap_table(seed, centre):
    cam = UC.camera((640, 480), distorted=True)
    ref = SC.ring61()
    return ref, SC.cap_recording(cam, ref, CAP_R, [centre], [CAP_DEPTH], seed=seed)


def _flat_ref_disp(m):
    rd = np.zeros((m, 4))
    rd[:, 0] = 1.0
    return rd


def test_a_rendered_spherical_cap_gives_its_curvature_and_its_centre():
    from vbs_amd import shapes
    worst_k = worst_apex = 0.0
    for seed in range(4):
        ref, tab = _cap_table(seed, CAP_CENTRE)
        length = shapes.default_length(ref)
        assert abs(length - SC.rms_length(ref[:, :2])) <= 1e-12 * length
        shape, _, _ = O.shape_series(tab, _flat_ref_disp(61), ref, 0, length=length, frame_range=(1, 2))
        row = shape[0]
        assert row[0] == 2.0 and row[19] == 1.0, row
        assert shapes.kind(shape).tolist() == [shapes.KIND_BOWL]
        worst_k = max(worst_k, abs(row[16] * CAP_R - 1.0), abs(row[17] * CAP_R - 1.0))
        worst_apex = max(worst_apex, float(np.hypot(row[20] - CAP_CENTRE[0], row[21] - CAP_CENTRE[1])))
        rad, valid = shapes.radius(shape)
        assert valid.all() and np.array_equal(rad[0], 1.0 / row[16:18])
        assert row[23] < 0.0 and row[12] > row[13] > 0.0          # the apex lies below the plane; the quadric explains more than it
    print(f"cap: worst |k R - 1| {worst_k:.3e} (bound {CAP_K_TOL:.1e}), worst apex error {worst_apex:.3e} mm (bound {CAP_APEX_TOL:.1e})")
    assert worst_k <= CAP_K_TOL and worst_apex <= CAP_APEX_TOL


def test_a_cap_centred_outside_the_reach_has_no_apex():
    from vbs_amd import shapes
    ref, tab = _cap_table(0, (35.0, 0.0))
    length = shapes.default_length(ref)
    assert 35.0 > 2.0 * length + 10.0
    shape, _, _ = O.shape_series(tab, _flat_ref_disp(61), ref, 0, length=length, max_apex=2.0, frame_range=(1, 2))
    assert shape[0, 0] == 2.0 and shape[0, 19] == 0.0 and (shape[0, 20:24] == 0.0).all()
    far, _, _ = O.shape_series(tab, _flat_ref_disp(61), ref, 0, length=length, max_apex=10.0, frame_range=(1, 2))
    assert far[0, 19] == 1.0 and far[0, 20] > 2.0 * length


@pytest.mark.parametrize("name", list(SC.degeneracies()))
def test_degeneracies(name):
    xy, dz, missing, min_count, want = SC.degeneracies()[name]
    k = SC.table_of_heights(xy, dz[None], missing[None])
    length = SC.rms_length(xy)
    shape, coef, res = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=length, min_count=min_count, frame_range=(1, 2))
    row = shape[0]
    assert row[1] == float((~missing).sum()) and row[2] == row[1]
    if isinstance(want, tuple):
        assert row[0] <= want[1]
    else:
        assert row[0] == want, row
    assert coef[0, 0, 0] == row[0] and coef[0, 1, 0] == (1.0 if row[0] == 2.0 else 0.0)
    if row[0] == 0.0:
        assert (row[6:] == 0.0).all() and (res == 0.0).all() and (coef[0, :, 1:] == 0.0).all()
    if row[0] == 1.0:
        assert (row[9:12] == 0.0).all() and (row[13:] == 0.0).all() and row[12] >= 0.0
        assert res[0, :, 0].sum() == row[2]


def test_one_gross_outlier_is_dropped_and_the_fit_becomes_the_clean_one():
    xy, dz, min_count, rk = SC.rejection_sets()["outlier"]
    k = SC.table_of_heights(xy, dz[None])
    length = SC.rms_length(xy)
    args = dict(start_frame=0, length=length, min_count=min_count, frame_range=(1, 2))
    first, _, _ = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], reject_k=0.0, **args)
    shape, coef, res = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], reject_k=rk, **args)
    clean_mask = np.arange(30) != 11
    clean, ccoef, cres = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], mask=clean_mask, reject_k=0.0, **args)
    assert first[0, 2] == 30.0 and shape[0, 1] == 30.0 and shape[0, 2] == 29.0 and shape[0, 0] == 2.0
    assert res[0, 11].tolist() == [0.0, 0.0] and res[0, :, 0].sum() == 29.0
    assert np.array_equal(shape[0, 3:], clean[0, 3:]) and np.array_equal(coef, ccoef) and np.array_equal(res, cres)
    assert shape[0, 13] < 0.02 < 0.2 < first[0, 13]


def test_the_first_fit_stands_where_the_kept_set_cannot_hold_the_degree():
    xy, dz, min_count, rk = SC.rejection_sets()["too few kept"]
    k = SC.table_of_heights(xy, dz[None])
    args = dict(start_frame=0, length=SC.rms_length(xy), min_count=min_count, frame_range=(1, 2))
    first = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], reject_k=0.0, **args)
    again = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], reject_k=rk, **args)
    assert first[0][0, 0] == 2.0 and first[0][0, 13] > 0.0
    r = first[2][0, :, 1]
    assert ((r * r) > (rk * rk) * (r @ r) / 9.0).any(), "the case rejects nothing"
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    assert again[0][0, 2] == 9.0


def test_the_shim_refuses_what_the_header_refuses_without_a_device():
    from vbs_amd import engine as E
    n, m = 4, 12
    good = dict(n=n, m=m, start_frame=1, mode="plane", scale=1.0, length=3.0, slots=None, reject_k=0.0, min_count=9, piv_rel=1e-10,
                apex_rel=1e-6, max_apex=2.0, frame_range=None, ref_disp_shape=(m, 4), ref_xyz_shape=(m, 3),
                want=("shape", "coef", "residual"))
    assert E._shape_args(**good) == (0, n, 0, 9, ("shape", "coef", "residual"))
    assert E._shape_args(**dict(good, mode="shell", frame_range=(1, 3), want="coef", min_count=6)) == (1, 3, 1, 6, ("coef",))
    bad = [dict(n=0), dict(m=0), dict(mode="sphere"), dict(start_frame=-1), dict(start_frame=n), dict(start_frame=0.5),
           dict(scale=np.inf), dict(scale=np.nan), dict(reject_k=-1.0), dict(reject_k=np.inf), dict(reject_k=np.nan),
           dict(ref_disp_shape=(m, 3)), dict(ref_xyz_shape=(m + 1, 3)), dict(length=0.0), dict(length=-1.0), dict(length=np.inf),
           dict(length=np.nan), dict(min_count=5), dict(min_count=9.5), dict(piv_rel=-1e-3), dict(piv_rel=np.inf), dict(piv_rel=np.nan),
           dict(apex_rel=-1.0), dict(apex_rel=np.inf), dict(apex_rel=np.nan), dict(max_apex=-1.0), dict(max_apex=np.inf),
           dict(max_apex=np.nan), dict(frame_range=(2, 1)), dict(frame_range=(0, n + 1)), dict(frame_range=(-1, 2)), dict(slots=[m]),
           dict(want=()), dict(want=("pose",))]
    for change in bad:
        with pytest.raises(ValueError):
            E._shape_args(**dict(good, **change))


def test_coef_and_residual_are_records_of_the_filter_and_of_the_field_map():
    """`coef` [F, 2, 4] read with n_values 3 and `residual` [F, m, 2] read with n_values 1 pass those entries' own argument checks."""
    from vbs_amd import analysis as A
    from vbs_amd.filters import half_taps
    xy, dz, _, _, _ = SC.degeneracies()["count 16"]
    k = SC.table_of_heights(xy, np.stack([dz, 2.0 * dz, 3.0 * dz]))
    shape, coef, res = O.shape_series(k["table"], k["ref_disp"], k["ref_xyz"], 0, length=SC.rms_length(xy))
    F, s, cols = coef.shape
    A._record_shape(F, s, cols)
    assert (F, s, cols) == (4, 2, 4) and A._n_values(cols, 3, None) == 3 and half_taps(np.ones(3) / 3.0).size == 2
    assert (coef[..., 0] != 0.0).all()                            # (frame 0 is the start: flat, a quadric of zeros)
    Fr, m, rc = res.shape
    assert A._field_args(Fr, m, rc, 5, (5, m), (5,), 0.5, None, None) == (0, Fr, 1)
    assert set(np.unique(res[..., 0]).tolist()) <= {0.0, 1.0}
