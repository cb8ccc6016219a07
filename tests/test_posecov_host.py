"""CPU tests of the uncertainty of the pose misalignment (`vbs_pose_cov`), all on the NumPy restatement
`tests/helpers/posecov_oracle.py` the device is held to bit for bit (`tests/test_gpu_posecov.py`): the linearisation against an
independent fit, the covariance against a Monte-Carlo run, the two cancellations the model promises, and the argument checks of
the Python shim."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pose_oracle as PO                                       # noqa: E402
import posecov_cases as PC                                     # noqa: E402
import posecov_oracle as O                                     # noqa: E402
import uncert_cases as UC                                      # noqa: E402
import uncert_oracle as U                                      # noqa: E402

# |K - central differences of the lstsq fit| / max|K| at h = 1e-6 over every used slot of the frame below: 10 x the 5.7e-10 measured
# on the CPU (the differences' own rounding, u / h = 1e-10 per unit of the fit's sensitivity, and their h^2 term)
K_TOL = 5.7e-9
MC_DRAWS = 20000


@pytest.fixture(scope="module")
def frame():
    """One frame of a 65-marker recording, tilted by a degree, with everything the restatement made of it."""
    cam = UC.camera((640, 480), distorted=True)
    ref = PO.grid_ref(65)
    tab, obs = PC.tilted_recording(cam, ref, [0.0, 1.0], pixel_sigma=(0.05, 0.05), seed=1)
    rd = np.zeros((65, 4))
    rd[:, 0] = 1.0
    detail = []
    pose, pcov = O.pose_cov(tab, rd, ref, U.Cam(*cam), obs, None, None, 0, frame_range=(1, 2), detail=detail)
    assert pcov[0, 0] == 7.0 and len(detail) == 1
    return dict(pose=pose[0], pcov=pcov[0], **detail[0])


def test_influence_matrix_equals_central_differences_of_an_independent_fit(frame):
    P, K = frame["P"], frame["K"]
    h = 1e-6
    worst = 0.0
    for r in range(P.shape[0]):
        for k in range(3):
            Pp, Pm = P.copy(), P.copy()
            Pp[r, k] += h
            Pm[r, k] -= h
            fd = (O.lstsq_plane(Pp) - O.lstsq_plane(Pm)) / (2.0 * h)
            worst = max(worst, float(np.abs(K[r, :, k] - fd).max()))
    rel = worst / float(np.abs(K).max())
    print(f"K against central differences: {rel:.3e} relative")
    assert rel <= K_TOL
    assert np.abs(O.lstsq_plane(P)[:2] - frame["pose"][1:3]).max() <= PO.PLANE_TOL


def test_sigma_obs_equals_a_monte_carlo_run_through_the_independent_fit(frame):
    """N draws of end-point noise with each slot's own covariance C, refitted by lstsq: the sample variances of a, b, c over the
    restatement's must lie within five standard deviations of a variance's sampling error of 1."""
    P, C, so = frame["P"], frame["C"], frame["sigma_obs"]
    m = P.shape[0]
    rng = np.random.default_rng(11)
    chol = np.zeros((m, 3, 3))
    for r in range(m):
        S = np.array([[C[r, 0], C[r, 1], C[r, 2]], [C[r, 1], C[r, 3], C[r, 4]], [C[r, 2], C[r, 4], C[r, 5]]])
        chol[r] = np.linalg.cholesky(S)
    fits = np.empty((MC_DRAWS, 3))
    for i in range(MC_DRAWS):
        fits[i] = O.lstsq_plane(P + np.einsum("rij,rj->ri", chol, rng.normal(size=(m, 3))))
    ratio = fits.var(axis=0, ddof=1) / so[[0, 3, 5]]
    bound = 5.0 * np.sqrt(2.0 / (MC_DRAWS - 1))
    print(f"variance ratios a, b, c: {ratio}, bound {bound:.4f}")
    assert (np.abs(ratio - 1.0) <= bound).all()
    cov_ab = np.cov(fits[:, 0], fits[:, 1])[0, 1]
    assert abs(cov_ab - so[1]) <= 5.0 * np.sqrt((so[0] * so[3] + so[1] * so[1]) / (MC_DRAWS - 1))


@pytest.fixture(scope="module")
def rec():
    cam = UC.camera((640, 480), distorted=True)
    k = PC.recording(cam, 5, 65, seed=3, drop=0.0)
    k["cam"], k["obs"] = cam, PC.obs_cov("slot", 65, 3)
    return k


def test_a_shift_of_T_cancels_to_exactly_zero(rec):
    """A camera factor that only shifts T moves every one of the four solves of a deviation alike: Sigma_cam is exactly zero, with
    and without the reference rows; a factor on dmm does not cancel."""
    c = U.Cam(*rec["cam"])
    L = np.zeros((16, 3))
    L[12, 0], L[13, 1], L[14, 2], L[12, 2] = 0.02, 0.03, 0.05, 0.01
    for rows in (None, rec["ref_rows"]):
        _, pcov = O.pose_cov(rec["table"], rec["ref_disp"], rec["ref_xyz"], c, rec["obs"], L, rows, rec["start"])
        _, none = O.pose_cov(rec["table"], rec["ref_disp"], rec["ref_xyz"], c, rec["obs"], None, rows, rec["start"])
        assert (pcov[:, 0] >= 1.0).sum() >= 3
        assert (pcov[:, 8:14] == 0.0).all()
        assert np.array_equal(pcov, none)
    _, pcov = O.pose_cov(rec["table"], rec["ref_disp"], rec["ref_xyz"], c, rec["obs"], UC.factor(1), rec["ref_rows"], rec["start"])
    ok = pcov[:, 0] >= 1.0
    moving = ok & (np.arange(5) != rec["start"])
    assert (pcov[moving][:, [8, 11, 13]] > 0.0).all()


def test_doubling_scale_at_reference_positions_zero_scales_sigma_as_the_algebra_says(rec):
    """With ref_xyz = 0 the end points are scale d: doubling scale doubles them exactly, so a and b stay, c doubles, and Sigma
    becomes D Sigma D with D = diag(1, 1, 2) - in bits, every factor being a power of two.  The angles and t2 do not move."""
    c = U.Cam(*rec["cam"])
    zero = np.zeros((65, 3))
    p1, s1 = O.pose_cov(rec["table"], rec["ref_disp"], zero, c, rec["obs"], UC.factor(5), rec["ref_rows"], rec["start"], scale=1.0)
    p2, s2 = O.pose_cov(rec["table"], rec["ref_disp"], zero, c, rec["obs"], UC.factor(5), rec["ref_rows"], rec["start"], scale=2.0)
    ok = s1[:, 0] >= 1.0
    assert ok.sum() >= 3 and np.array_equal(s1[:, :2], s2[:, :2])
    assert np.array_equal(p1[:, 1:3], p2[:, 1:3]) and np.array_equal(2.0 * p1[:, 3], p2[:, 3])
    D = np.array([1.0, 1.0, 2.0, 1.0, 2.0, 4.0])                 # aa, ab, ac, bb, bc, cc
    assert np.array_equal(s1[:, 2:8] * D, s2[:, 2:8]) and np.array_equal(s1[:, 8:14] * D, s2[:, 8:14])
    assert np.array_equal(s1[:, 14:], s2[:, 14:])
    assert (s1[ok][:, [2, 5, 7]] > 0.0).all()


@pytest.mark.parametrize("masked", [False, True])
def test_the_exit_recording_reaches_every_exit_of_the_rejection_round(masked):
    """`posecov_cases.exit_recording` asserts, from the restatement alone, that its frame f leaves the round by EXIT_FRAMES[f]: no
    frame is unnamed and each of the four exits of the second round has its frame (what `tests/test_gpu_posecov.py` then holds the
    device to).  Every frame has a plane and a covariance, so that a wrong exit shows in `pose` and in `pcov`."""
    cam = UC.camera((640, 480), distorted=True)
    k = PC.exit_recording(cam, masked)
    assert PC.second_round_exits(k) == list(PC.EXIT_FRAMES) and len(set(PC.EXIT_FRAMES)) == k["table"].shape[0] == O.GROUP + 1
    sel = None if k["slots"] is None else np.isin(np.arange(k["table"].shape[1]), k["slots"])
    pose, pcov = O.pose_cov(k["table"], k["ref_disp"], k["ref_xyz"], U.Cam(*cam), PC.obs_cov("one", 7), UC.factor(5, 2), k["ref_rows"],
                            k["start"], sel, False, 1.0, PC.EXIT_RK)
    assert pose[:, 0].tolist() == [1.0, 2.0, 1.0, 1.0, 1.0] and pose[:, 7].tolist() == [7.0, 4.0, 4.0, 5.0, 7.0]
    assert ((pcov[:, 0].astype(np.int64) & 1) != 0).all() and (pcov[:, 1] == 0.0).all()


def test_the_shim_refuses_what_the_header_refuses_without_a_device():
    from vbs_amd import engine as E, pipeline as PL
    obs, m, n = np.eye(3) * 0.01, 7, 4
    good = dict(n=n, m=m, obs_cov=obs, cam_factor=np.zeros((16, 2)), start_frame=1, mode="plane", scale=1.0, slots=None, reject_k=0.0,
                min_marker_size_px=5.0, piv_rel=1e-12, frame_range=None, ref_disp_shape=(m, 4), ref_xyz_shape=(m, 3),
                ref_rows_shape=(2, m, 10), want=("pose", "pcov"))
    o, Lf, a, b, shell, want = E._posecov_args(**good)
    assert o.shape == (1, 6) and Lf.shape == (16, 2) and (a, b, shell) == (0, n, 0) and want == ("pose", "pcov")
    assert E._posecov_args(**dict(good, mode="shell", frame_range=(1, 3), cam_factor=None, ref_rows_shape=None))[2:5] == (1, 3, 1)
    bad = [dict(mode="sphere"), dict(start_frame=-1), dict(start_frame=n), dict(start_frame=0.5), dict(scale=np.inf), dict(scale=np.nan),
           dict(reject_k=-1.0), dict(reject_k=np.inf), dict(ref_disp_shape=(m, 3)), dict(ref_xyz_shape=(m + 1, 3)),
           dict(ref_rows_shape=(1, m, 10)), dict(ref_rows_shape=(2, m, 9)), dict(obs_cov=np.zeros((2, 6))),
           dict(obs_cov=np.full(6, np.nan)), dict(cam_factor=np.zeros((16, 17))), dict(cam_factor=np.zeros((15, 2))),
           dict(cam_factor=np.full((16, 1), np.inf)), dict(min_marker_size_px=np.nan), dict(piv_rel=-1.0), dict(piv_rel=np.inf),
           dict(frame_range=(2, 1)), dict(frame_range=(0, n + 1)), dict(slots=[m]), dict(want=()), dict(want=("field",)), dict(n=0)]
    for change in bad:
        with pytest.raises(ValueError):
            E._posecov_args(**dict(good, **change))
    assert PL._misalignment_uncertainty_args(5, 0, -1, 3.0) == (0, 4, 3.0)
    for args in ((5, 0, 5, 3.0), (5, 5, -1, 3.0), (5, 0, -6, 3.0), (5, 0, -1, 0.0), (5, 0, -1, np.nan)):
        with pytest.raises(ValueError):
            PL._misalignment_uncertainty_args(*args)
