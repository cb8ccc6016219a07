"""Host tests (no GPU) of the uncertainty of the 3-D solve: the header, the symbols and what the entries refuse; the
NumPy restatement the GPU tests hold the device to (`tests/helpers/uncert_oracle.py`) - its primal against the back end's own
oracle, its forward mode against the complex step, against central differences and against closed forms; the factor helpers of
`vbs_amd/uncertainty.py`; and three statements of physics on the restatement's covariances."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import _build, uncertainty as UN

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import backend_oracle as BO                                    # noqa: E402
import uncert_cases as UC                                      # noqa: E402
import uncert_oracle as U                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((640, 480), (1920, 1200))
EPS = 2.0 ** -52

# The largest discrepancy between the forward mode and the complex step, relative to the norm of the Jacobian's row, over
# `_all_cases()`; both are float64 evaluations of the same analytic function, and 16 x covers other libm builds.
#   cameras whose float32 constants are exact (the solve is the smooth function): measured 4.3e-16
#   every other camera (f_avg, dmm / f_avg, f_avg^2 rounded to float32): measured 7.2e-8
MEASURED_EXACT, MEASURED_F32 = 4.3e-16, 7.2e-8
TOL_EXACT, TOL_F32 = 16 * MEASURED_EXACT, 16 * MEASURED_F32


def _all_cases():
    for size in SIZES:
        for distorted in (False, True):
            for exact in (False, True):
                yield size, distorted, exact, UC.camera(size, distorted, exact)


def _ids(v):
    return f"{v[0][0]}x{v[0][1]}-{'dist' if v[1] else 'plain'}-{'exact' if v[2] else 'f32'}"


CASES = list(_all_cases())


def test_header_symbols_constants_and_source_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("vbs_uncert_points", "vbs_uncert_cov", "vbs_uncert_total", "vbs_pixel_noise"):
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    for name in ("UNCERT_CAM", "UNCERT_COV_COLS", "UNCERT_DCOV_COLS", "UNCERT_TOTAL_COLS", "UNCERT_GROUP", "UNCERT_REF_COLS",
                 "UNCERT_WORK_COLS", "NOISE_COLS"):
        assert getattr(L, name) == defs["VBS_" + name], name
    assert (L.UNCERT_CAM, L.UNCERT_COV_COLS, L.UNCERT_DCOV_COLS, L.UNCERT_TOTAL_COLS, L.NOISE_COLS, L.UNCERT_GROUP) == (
        U.NCAM, U.COV_COLS, U.DCOV_COLS, U.TOTAL_COLS, U.NOISE_COLS, U.GROUP)
    assert L.UNCERT_REF_COLS == 7 + 3 * L.UNCERT_CAM and L.UNCERT_WORK_COLS == L.UNCERT_REF_COLS + 6
    assert UN.N_THETA == L.UNCERT_CAM and UN.THETA == U.THETA
    assert "k_uncert.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "k_uncert.hip"))


def test_refusals_without_a_gpu():
    """Every refusal is decided before a device is selected (device -1, device pointers nothing follows); obs_cov and cam_factor
    live on the host and are read."""
    lib = L.lib()
    p = C.c_void_p(8)
    cam = L.make_camera(*UC.camera()[:4], 2.0)
    obs = np.array([[0.01, 0.0, 0.0, 0.01, 0.0, 0.02]])
    fac = UC.factor(5)

    def hp(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def cov(table=p, n=4, m=3, obs=obs, rows=1, fac=fac, q=5, ref=0, mins=5.0, piv=1e-12, fb=0, fe=4, work=p, cv=p, dc=p):
        return lib.vbs_uncert_cov(-1, table, n, m, C.byref(cam), hp(obs), rows, hp(fac), q, ref, mins, piv, fb, fe, work, cv, dc, None)

    def tot(table=p, n=4, m=3, obs=obs, rows=1, fac=fac, q=5, ref=0, mask=None, mins=5.0, fb=0, fe=4, work=p, out=p):
        return lib.vbs_uncert_total(-1, table, n, m, C.byref(cam), hp(obs), rows, hp(fac), q, ref, mask, mins, fb, fe, work, out, None)

    assert cov() == L.VBS_EHIP and tot() == L.VBS_EHIP           # valid arguments get as far as the device that is not there
    bad_obs, bad_fac = obs.copy(), fac.copy()
    bad_obs[0, 4] = np.inf
    bad_fac[3, 2] = np.nan
    for kw in (dict(q=17), dict(q=-1), dict(ref=4), dict(ref=-1), dict(obs=bad_obs), dict(fac=bad_fac), dict(rows=2), dict(table=None),
               dict(obs=None), dict(work=None), dict(n=0), dict(m=0), dict(fb=3, fe=2), dict(fe=5), dict(mins=float("nan")),
               dict(fac=None)):
        assert cov(**kw) == L.VBS_EINVAL, kw
        assert tot(**kw) == L.VBS_EINVAL, kw
    assert cov(piv=-1.0) == L.VBS_EINVAL and cov(piv=float("inf")) == L.VBS_EINVAL and cov(cv=None, dc=None) == L.VBS_EINVAL
    assert cov(dc=None, ref=0) == L.VBS_EINVAL and cov(dc=None, ref=-1) == L.VBS_EHIP and cov(q=0, fac=None) == L.VBS_EHIP
    assert tot(out=None) == L.VBS_EINVAL
    assert lib.vbs_uncert_points(-1, None, 3, C.byref(cam), p, p, p, p, None) == L.VBS_EINVAL
    assert lib.vbs_uncert_points(-1, p, -1, C.byref(cam), p, p, p, p, None) == L.VBS_EINVAL
    assert lib.vbs_uncert_points(-1, p, 3, C.byref(cam), p, None, p, p, None) == L.VBS_EINVAL
    assert lib.vbs_pixel_noise(-1, p, 4, 3, 0, 5, p, None) == L.VBS_EINVAL
    assert lib.vbs_pixel_noise(-1, p, 4, 3, 0, 4, None, None) == L.VBS_EINVAL
    assert lib.vbs_pixel_noise(-1, p, 4, 3, 0, 4, p, None) == L.VBS_EHIP


def test_wrapper_argument_checks():
    from vbs_amd.engine import _uncert_args
    good = dict(n=4, m=3, obs_cov=UN.obs_cov(0.1, 0.1), cam_factor=UC.factor(5), ref_frame=0, slots=None, min_marker_size_px=5.0,
                piv_rel=1e-12, frame_range=None)
    obs, Lf, rf, a, b = _uncert_args(**good)
    assert obs.shape == (1, 6) and Lf.shape == (16, 5) and (rf, a, b) == (0, 0, 4)
    assert _uncert_args(**dict(good, obs_cov=np.diag([1.0, 2.0, 3.0])))[0].tolist() == [[1.0, 0.0, 0.0, 2.0, 0.0, 3.0]]
    none = _uncert_args(**dict(good, cam_factor=None, ref_frame=None))
    assert none[1].shape == (16, 0) and none[2] == -1
    asym = np.diag([1.0, 2.0, 3.0])
    asym[0, 1] = 0.5
    for kw in (dict(obs_cov=np.zeros(5)), dict(obs_cov=np.zeros((2, 6))), dict(obs_cov=asym), dict(obs_cov=[np.nan] * 6),
               dict(cam_factor=np.zeros((16, 17))), dict(cam_factor=np.zeros((15, 2))), dict(cam_factor=np.full((16, 1), np.inf)),
               dict(ref_frame=4), dict(ref_frame=-1), dict(slots=[3]), dict(piv_rel=-1.0), dict(frame_range=(2, 5)),
               dict(min_marker_size_px=float("nan"))):
        with pytest.raises(ValueError):
            _uncert_args(**dict(good, **kw))


# ---- 1. the primal ---------------------------------------------------------------------------------------------------------------------
SIGNED_PERMUTATIONS = (np.eye(3), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
                       np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("distorted", (False, True))
def test_primal_is_the_back_end_oracle_bit_for_bit(size, distorted):
    """`uncert_oracle.primal` against `backend_oracle.solve_table` (the reference's own function bodies).  The reference rotates
    with `R.T @ p`, a BLAS product whose order of summation and fused multiply-adds are the library's, not the kernel's
    left-to-right sum: the two agree bit for bit where every sum of the rotation has one non-zero term (R a signed permutation),
    and for a general R within the bound of a sum of three products, gamma_3 sum_k |R_ki| |pc_k| on either side."""
    for R in SIGNED_PERMUTATIONS + (None,):
        cam = UC.camera(size, distorted, R=R)
        c = U.Cam(*cam)
        uvd = UC.points(cam, size)
        tab = np.zeros((uvd.shape[0] + 1, 10))
        tab[:, 0], tab[:-1, 1:4] = 1.0, uvd
        tab[-1, 1:4] = c.cx32, c.cy32, 12.0                       # the principal point: no solve
        flags, xyz = BO.solve_table(tab, *cam[:4], cam[4], 5.0)
        P, X, ok = U.primal(c, tab[:, 1], tab[:, 2], tab[:, 3])
        assert np.array_equal(ok, (flags & 2) != 0) and ok[:-1].all() and not ok[-1]
        if R is not None:
            assert np.array_equal(np.where(ok[:, None], X, 0.0), xyz)
        else:
            bound = 2 * 3 * 2.0 ** -53 / (1 - 3 * 2.0 ** -53) * (np.abs(c.R).T @ np.abs(np.array(P["pc"])))
            assert (np.abs(X - xyz)[ok] <= bound.T[ok]).all()


# ---- 2. forward mode against the complex step -----------------------------------------------------------------------------------------
def _discrepancy(size, distorted, cam):
    c = U.Cam(*cam)
    uvd = UC.points(cam, size)
    X, Jo, Jc, ok = U.jacobians(c, uvd)
    assert ok.all()
    worst = 0.0
    for i, o in enumerate(uvd):
        jo, jc = U.jacobian_complex_step(c, o)
        if not distorted:
            jc[:, 4:9] = 0.0                                      # the iterations are skipped: as executed, no dependence on k
        J1, J2 = np.concatenate([Jc[i], Jo[i]], axis=1), np.concatenate([jc, jo], axis=1)
        worst = max(worst, float((np.abs(J1 - J2) / np.linalg.norm(J2, axis=1, keepdims=True)).max()))
    return worst


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_mode_against_the_complex_step(case):
    size, distorted, exact, cam = case
    worst = _discrepancy(size, distorted, cam)
    print(f"forward mode against complex step, {_ids(case)}: {worst:.3e}")
    assert worst <= (TOL_EXACT if exact else TOL_F32)


# ---- 3. central differences ------------------------------------------------------------------------------------------------------------
H_OBS = (1e-4, 1e-4, 1e-5)
H_CAM = (1e-3, 1e-3, 1e-4, 1e-4, 1e-6, 1e-6, 1e-6, 1e-6, 1e-6, 1e-7, 1e-7, 1e-7, 1e-4, 1e-4, 1e-4, 1e-6)
PRIMAL_ROUNDING = 2.0 ** -45                                     # ~ 128 roundings of 2^-53 in each of the two evaluations


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("distorted", (False, True))
def test_central_differences_of_the_primal(size, distorted):
    """By the mean value theorem a central difference IS the derivative somewhere in [p - h, p + h], so it differs from the
    Jacobian at p by at most the Jacobian's own change over that interval, |J(p + h) - J(p - h)| - h times the second derivative's
    scale, taken from the Jacobian itself at the two ends - plus the rounding of the two primal values over 2h.  The observation
    directions difference the product's restatement itself; the camera directions need a camera that is not float32 and
    difference the float64 model on a camera whose float32 constants are exact, where it is the same function."""
    cam = UC.camera(size, distorted, exact=True)
    c = U.Cam(*cam)
    uvd = UC.points(cam, size)
    X, Jo, Jc, ok = U.jacobians(c, uvd)
    scale = np.linalg.norm(X, axis=1)
    for k, h in enumerate(H_OBS):
        e = np.zeros(3)
        e[k] = h
        Xp, Jp, _, _ = U.jacobians(c, uvd + e)
        Xm, Jm, _, _ = U.jacobians(c, uvd - e)
        fd = (Xp - Xm) / (2 * h)
        bound = np.abs(Jp[:, :, k] - Jm[:, :, k]) + PRIMAL_ROUNDING * scale[:, None] / h
        assert (np.abs(fd - Jo[:, :, k]) <= bound).all(), (k, float((np.abs(fd - Jo[:, :, k]) / bound).max()))
    th = c.theta()
    for i, o in enumerate(uvd):
        assert np.abs(U.model_complex(th, o, c.R, c.has_dist) - X[i]).max() <= 64 * EPS * scale[i]
        for k, h in enumerate(H_CAM):
            if not distorted and 4 <= k <= 8:
                continue
            tp, tm = th.copy(), th.copy()
            tp[k] += h
            tm[k] -= h
            fd = (U.model_complex(tp, o, c.R, c.has_dist) - U.model_complex(tm, o, c.R, c.has_dist)) / (2 * h)
            Jp = U.jacobian_complex_step_theta(tp, o, c.R, c.has_dist)[:, k]
            Jm = U.jacobian_complex_step_theta(tm, o, c.R, c.has_dist)[:, k]
            bound = np.abs(Jp - Jm) + PRIMAL_ROUNDING * scale[i] / h + TOL_EXACT * np.linalg.norm(Jc[i], axis=1)
            assert (np.abs(fd - Jc[i][:, k]) <= bound).all(), (i, k, fd, Jc[i][:, k], bound)


# ---- 4. closed forms ---------------------------------------------------------------------------------------------------------------------
def test_closed_forms_without_distortion_rotation_and_translation():
    """No distortion, R = I, T = 0, and float32 constants that are exact (f_avg = 512, dmm = 2: otherwise dX/ddmm = X / k32 / f_avg
    differs from X / dmm by k32's float32 rounding, the deviation DESIGN 7 states): dZ/dd = -h / d, dX/dT = -I, dX/ddmm = X / dmm,
    each within 4 ulp."""
    for size in SIZES:
        cam = UC.camera(size, distorted=False, exact=True, R=np.eye(3), T=(0.0, 0.0, 0.0))
        uvd = UC.points(cam, size)
        X, Jo, Jc, ok = U.jacobians(U.Cam(*cam), uvd)
        assert ok.all()

        def ulps(got, want):
            return np.abs(got - want) / np.spacing(np.abs(want))
        assert (ulps(Jo[:, 2, 2], -X[:, 2] / uvd[:, 2]) <= 4).all()
        assert np.array_equal(Jc[:, :, 12:15], np.broadcast_to(-np.eye(3), (uvd.shape[0], 3, 3)))
        assert (ulps(Jc[:, :, 15], X / 2.0) <= 4).all()


# ---- 5. the factor helpers --------------------------------------------------------------------------------------------------------------
def test_camera_factor_reproduces_a_covariance_and_drops_what_is_zero():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(16, 16)) * UC.factor(16)[np.arange(16), np.arange(16)][:, None]
    S = A @ A.T
    S = (S + S.T) / 2
    Lf = UN.camera_factor(cov=S)
    assert Lf.shape == (16, 16)
    assert np.abs(Lf @ Lf.T - S).max() <= UN.CHOL_EPS * np.trace(S)
    S0 = S.copy()
    S0[7, :] = 0.0
    S0[:, 7] = 0.0                                                # p2 is exact: a zero direction
    L0 = UN.camera_factor(cov=S0)
    assert L0.shape == (16, 15) and not L0[7].any()
    assert np.abs(L0 @ L0.T - S0).max() <= UN.CHOL_EPS * np.trace(S0)
    v = rng.normal(size=16)
    L1 = UN.camera_factor(cov=np.outer(v, v))                     # rank one: what is left after the first pivot is rounding
    assert 1 <= L1.shape[1] <= 16 and np.abs(L1 @ L1.T - np.outer(v, v)).max() <= UN.CHOL_EPS * (v @ v) * 16
    bad = S.copy()
    bad[2, 5] += 1e-9
    with pytest.raises(ValueError):
        UN.camera_factor(cov=bad)
    with pytest.raises(ValueError):
        UN.camera_factor(cov=S[:15, :15])
    with pytest.raises(ValueError):
        UN.camera_factor(cov=S, diameter_std=0.1)


def test_camera_factor_from_standard_deviations():
    Lf = UN.camera_factor(std_intrinsics=[1.0, 2.0, 0.0, 0.5, 0, 0, 0, 0, 0], t_std=[0.0, 0.0, 0.3], diameter_std=0.01)
    assert Lf.shape == (16, 5)
    want = np.zeros(16)
    want[[0, 1, 3, 14, 15]] = [1.0, 4.0, 0.25, 0.09, 1e-4]
    assert np.array_equal(Lf @ Lf.T, np.diag(want))
    assert UN.camera_factor().shape == (16, 0)
    for kw in (dict(std_intrinsics=[1.0] * 8), dict(omega_std=[1.0, -1.0, 0.0]), dict(t_std=[np.nan, 0, 0])):
        with pytest.raises(ValueError):
            UN.camera_factor(**kw)
    assert UN.obs_cov(0.1, 0.2).tolist() == [0.1 * 0.1, 0.0, 0.0, 0.1 * 0.1, 0.0, 0.2 * 0.2]


def test_pose_scatter_recovers_the_covariance_of_small_rotations():
    """Poses R_k = exp(w_k) R_0, T_k = T_0 + t_k with zero-mean w_k: the chordal mean is exp(delta) R_0 with |delta| of third order
    (the second-order term of the mean of exp(w_k) is symmetric), log(R_k R_mean') = w_k - delta + O(|w| |delta|), so the
    recovered covariance differs from the sample covariance of (w_k, t_k) by at most 2 |x|max (|delta| + ..) K / (K - 1)
    <= 4 wmax^3 |x|max: second order in |w| relative to the covariance itself."""
    rng = np.random.default_rng(9)
    K, wmax = 40, 2e-3
    w = rng.uniform(-1, 1, size=(K, 3)) * wmax / np.sqrt(3)
    w -= w.mean(axis=0)
    t = rng.normal(size=(K, 3)) * 0.01
    R0 = UC._rot(0.4, -0.3)
    Rs = [UN._exp_so3(wk) @ R0 for wk in w]
    Ts = np.array([1.0, 2.0, 30.0]) + t
    got = UN.pose_scatter(Rs, Ts)
    x = np.concatenate([w, t - t.mean(axis=0)], axis=1)
    want = x.T @ x / (K - 1)
    assert got.shape == (6, 6) and np.array_equal(got, got.T)
    xmax = np.abs(x).max()
    assert np.abs(got - want).max() <= 4 * wmax ** 3 * xmax + 64 * EPS * np.abs(want).max()
    assert np.abs(got - want).max() < 1e-3 * np.abs(want[:3, :3]).max()
    Rm, Tm = UN.mean_pose(Rs, Ts)
    assert np.abs(Rm - R0).max() <= wmax ** 2 and np.abs(Tm - Ts.mean(axis=0)).max() == 0.0
    S = UN.embed_pose_cov(got)
    assert S.shape == (16, 16) and np.array_equal(S[9:15, 9:15], got) and not S[:9].any() and not S[15].any()
    with pytest.raises(ValueError):
        UN.pose_scatter(Rs[:1], Ts[:1])


# ---- 6. statements of physics ----------------------------------------------------------------------------------------------------------
def test_a_shift_of_the_camera_cancels_in_every_displacement():
    """Sigma_o = 0 and a camera factor that holds only T: dX/dT = -R' for every row, so G_f - G_0 is exactly zero - Sigma_D is
    exactly 0 for every row and the camera share of the total is 0, while Sigma_X is not."""
    cam = UC.camera()
    c = U.Cam(*cam)
    move = np.zeros((5, 30, 3))
    move[3:, :, 2] = -0.8
    tab = UC.table(cam, 5, 30, move=move, seed=3)
    Lf = UN.camera_factor(t_std=[0.05, 0.02, 0.1])
    cov, dcov = U.solve3d_cov(tab, c, np.zeros(6), Lf, ref_frame=1)
    assert (dcov[..., 0] >= 1).sum() > 30 and not dcov[..., 1:].any() and (dcov[..., 0] != 3).all()
    assert (cov[cov[..., 0] == 1][:, [1, 4, 6]] > 0).all()
    tot = U.solve3d_total(tab, c, np.zeros(6), Lf, ref_frame=1)
    assert tot[:, 0].max() > 10 and not tot[:, 2:].any()


def test_the_diameter_error_adds_coherently_over_the_markers():
    """Only dmm is uncertain: dD/ddmm = D / dmm for every marker.  Markers on a circle around the principal point, all of one
    diameter and all coming closer by the same amount, have the same D_z up to rounding, so over `count` of them the camera share
    of var_z is (count g)^2 - it grows as count^2 - while the pixel-noise part grows as count."""
    cam = UC.camera(distorted=False, exact=True, R=np.eye(3), T=(0.0, 0.0, 0.0))
    c = U.Cam(*cam)
    m = 128
    ang = 2 * np.pi * np.arange(m) / m
    tab = np.zeros((2, m, 10), dtype=np.float32)
    for f, d in enumerate((16.0, 17.0)):
        tab[f, :, 1], tab[f, :, 2], tab[f, :, 3] = c.cx + 100 * np.cos(ang), c.cy + 100 * np.sin(ang), d
        P, X, ok = U.primal(c, *(tab[f, :, k].astype(np.float64) for k in (1, 2, 3)))
        tab[f, :, 6:9], tab[f, :, 0] = X, 3.0
    Lf, obs = UN.camera_factor(diameter_std=0.01), UN.obs_cov(0.05, 0.05)
    one = U.solve3d_total(tab, c, obs, Lf, ref_frame=0, slots=np.arange(m) == 0)[1]
    assert one[0] == 1 and one[7] > 0 and one[4] > one[7]
    for count in (2, 16, 64, 128):
        got = U.solve3d_total(tab, c, obs, Lf, ref_frame=0, slots=np.arange(m) < count)[1]
        assert got[0] == count and got[1] == 1
        # the markers' Rr differ by the float32 rounding of their centres (2^-24 relative), and so do their shares
        assert abs(got[7] / (count ** 2 * one[7]) - 1) <= 8 * 2.0 ** -24
        assert abs((got[4] - got[7]) / (count * (one[4] - one[7])) - 1) <= 8 * 2.0 ** -24
    # per marker: the camera's part of Sigma_D's zz is (D_z sigma / dmm)^2, D_z from the table's float32 X Y Z (2^-24 of |Z| each)
    with_cam = U.solve3d_cov(tab, c, obs, Lf, ref_frame=0)[1][1]
    without = U.solve3d_cov(tab, c, obs, None, ref_frame=0)[1][1]
    Z = tab[:, :, 8].astype(np.float64)
    D = Z[1] - Z[0]
    rel = 2 * (2 * 2.0 ** -24 * np.abs(Z).max() / np.abs(D).min()) + 64 * EPS * with_cam[:, 6].max() / (with_cam[:, 6] - without[:, 6]).min()
    assert (np.abs((with_cam[:, 6] - without[:, 6]) / (D * 0.01 / 2.0) ** 2 - 1) <= rel).all()


def test_restated_fold_and_ldl():
    """The fold is the tree of wave_fold.h; t2 of the restatement is D' Sigma_D^-1 D."""
    x = np.arange(64, dtype=np.float64) + 0.1
    tree = x.copy()
    for off in (32, 16, 8, 4, 2, 1):
        tree = tree[:off] + tree[off:2 * off]
    assert U.fold_down(x) == tree[0]
    cam = UC.camera()
    tab = UC.table(cam, 4, 20, seed=1, move=np.cumsum(np.full((4, 20, 3), 0.3), axis=0))
    cov, dcov = U.solve3d_cov(tab, U.Cam(*cam), UN.obs_cov(0.05, 0.08), UC.factor(16), ref_frame=0)
    v = dcov[..., 0] == 3
    assert v.sum() > 20
    for f, s in zip(*np.nonzero(v)):
        xx, xy, xz, yy, yz, zz = dcov[f, s, 1:7]
        S = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        D = tab[f, s, 6:9].astype(np.float64) - tab[0, s, 6:9].astype(np.float64)
        want = D @ np.linalg.solve(S, D)
        assert abs(dcov[f, s, 7] - want) <= 64 * np.linalg.cond(S) * EPS * want
        assert np.linalg.eigvalsh(S).min() >= -64 * EPS * np.trace(S)
