"""GPU tests of the extrinsic calibration (k_pnp.hip; `pytest -m gpu` on an MI355X): the device against the sequential helper
`tests/helpers/pnp_oracle.py` over every generated case - three layouts x distortion on / off, each batch one call.

Equal: status, winning hypothesis, inlier count and mask (the generator keeps every decision of the winner 1e-6 px from its
threshold), and the count of every well-conditioned all-inlier hypothesis.  The refined pose is held to the independent scipy
optimum on the same inliers; the bounds are 10 x the largest gap measured on an MI355X over these cases (the device result is
deterministic: the margin is for other seeds), see DESIGN.md 4.8."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pnp_oracle as P                                        # noqa: E402

# Measured on an MI355X over the 48 regular cases (device LM against scipy's optimum on the same inliers):
#   relative cost gap 5.2e-08 (the device's cost is the LOWER one there; where it is the higher one: 1.6e-09),
#   rotation 2.568e-05 degrees, translation 9.789e-07 mm.
# Those figures were taken while the helper's scipy fit used forward differences and stopped short of the optimum; it now
# uses central differences, against which the same arithmetic on the host differs by 2.5e-08 degrees and 1.1e-09 mm.  The
# device has not been measured against it yet, so the bounds stay at 10 x the device measurements above.
COST_REL_BOUND = 5.2e-7       # (a bound above 1e-6 would mean the LM has not converged: a defect, not a tolerance)
ROT_DEG_BOUND = 2.568e-4
T_MM_BOUND = 9.789e-6
# Noise-free, outlier-free cases against the generated truth.  Measured scipy-vs-truth gap (the float32 rounding of the image
# points): 3.435e-06 degrees, 5.156e-07 mm; the bound is 10 x that, for the device as for scipy
TRUTH_ROT_DEG_BOUND = 3.435e-5
TRUTH_T_MM_BOUND = 5.156e-6


def camera(b):
    return L.make_camera(b["K"], b["dist"], np.eye(3), np.zeros(3))


def table_of(b):
    """The problems of a batch as a tracker table: Cx, Cy in columns 1, 2, FLAG_TRACKED where valid."""
    t = np.zeros((len(b["problems"]), len(b["world"]), L.TABLE_COLS), dtype=np.float32)
    for k, p in enumerate(b["problems"]):
        t[k, :, 0] = np.where(p["valid"], L.FLAG_TRACKED, 0)
        t[k, :, 1:3] = p["image"].astype(np.float32)
    return t


def run(b, form="image", only=None):
    from vbs_amd.engine import pnp_ransac
    probs = b["problems"] if only is None else [b["problems"][k] for k in only]
    if form == "table":
        t = table_of(b)
        return pnp_ransac(b["world"], torch.from_numpy(t if only is None else t[list(only)]).cuda(), camera(b),
                          reproj_px=b["reproj_px"], samples=b["samples"])
    image = np.stack([p["image"] for p in probs])
    valid = np.stack([p["valid"] for p in probs])
    return pnp_ransac(b["world"], image, camera(b), reproj_px=b["reproj_px"], samples=b["samples"], valid=valid)


KEYS = ("status", "R", "T", "inlier_count", "inlier_mask", "mean_error", "inlier_rms", "winner", "hyp_count", "hyp_pose")


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in KEYS:
        x, y = a[k][rows_a].cpu().numpy(), b[k][rows_b].cpu().numpy()
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def batches():
    return P.all_batches()


@pytest.fixture(scope="module")
def results(batches):
    out = [run(b) for b in batches]
    torch.cuda.synchronize()
    return out


def test_default_samples_are_the_helpers(batches):
    from vbs_amd.engine import pnp_ransac
    b = batches[0]
    r = pnp_ransac(b["world"], b["problems"][0]["image"], camera(b), iterations=len(b["samples"]), seed=0)
    assert np.array_equal(r["samples"], b["samples"])


def test_winner_status_count_mask_equal(batches, results):
    for b, r in zip(batches, results):
        st, win = r["status"].cpu().numpy(), r["winner"].cpu().numpy()
        cnt, mask = r["inlier_count"].cpu().numpy(), r["inlier_mask"].cpu().numpy()
        for k, p in enumerate(b["problems"]):
            sol = p["sol"]
            assert st[k] == sol["status"], (b["layout"], k)
            assert win[k] == sol["winner"], (b["layout"], k)
            if sol["status"] == 0:
                assert cnt[k] == int(sol["mask"].sum()) and np.array_equal(mask[k].astype(bool), sol["mask"])
            else:
                assert cnt[k] == 0 and not mask[k].any()


def test_hypothesis_counts_equal(batches, results):
    total_all, total_well = 0, 0
    for b, r in zip(batches, results):
        hc = r["hyp_count"].cpu().numpy()
        for k, p in enumerate(b["problems"]):
            sol = p["sol"]
            if sol["status"] != 0:                          # which hypotheses are void is decided before any arithmetic rounds
                assert np.array_equal(hc[k] == -1, sol["count"] == -1), (b["layout"], k)
                continue
            allin = p["true_inliers"][b["samples"]].all(axis=1)
            well = allin & (sol["cond"] > P.WELL_CONDITIONED)
            total_all += int(allin.sum())
            total_well += int(well.sum())
            bad = np.nonzero(well & (hc[k] != sol["count"]))[0]
            assert bad.size == 0, (b["layout"], k, bad[:5], hc[k][bad[:5]], sol["count"][bad[:5]])
    print(f"well-conditioned all-inlier hypotheses: {total_well} of {total_all} all-inlier ones")
    assert 2 * total_well >= total_all, "the conditioning criterion rejects too much: fix the criterion"


def test_refined_pose_against_scipy(batches, results):
    worst = {"cost": 0.0, "rot": 0.0, "t": 0.0, "mean": 0.0, "rms": 0.0}
    for b, r in zip(batches, results):
        R, T = r["R"].cpu().numpy(), r["T"].cpu().numpy()
        me, rms = r["mean_error"].cpu().numpy(), r["inlier_rms"].cpu().numpy()
        for k, p in enumerate(b["problems"]):
            sol = p["sol"]
            if sol["status"] != 0:
                assert np.isnan(R[k]).all() and np.isnan(T[k]).all() and np.isnan(me[k]) and np.isnan(rms[k])
                continue
            ref = P.refine(sol, b["world"], p["image"])
            c = P.cost(sol["cam"], R[k], T[k], b["world"], p["image"], sol["mask"])
            worst["cost"] = max(worst["cost"], abs(c - ref["cost"]) / ref["cost"])
            worst["rot"] = max(worst["rot"], P.rotation_angle_deg(R[k], ref["R"]))
            worst["t"] = max(worst["t"], float(np.abs(T[k] - ref["t"]).max()))
            # the two reported errors are those of the RETURNED pose (helper's projection, 1e-9 px)
            e = P.pixel_errors(sol["cam"], R[k], T[k], b["world"], p["image"])
            worst["mean"] = max(worst["mean"], abs(me[k] - e[sol["valid"]].mean()))
            worst["rms"] = max(worst["rms"], abs(rms[k] - np.sqrt((e[sol["mask"]] ** 2).mean())))
            assert abs(np.linalg.det(R[k]) - 1.0) < 1e-12 and np.abs(R[k] @ R[k].T - np.eye(3)).max() < 1e-12
    print(f"device vs scipy: cost rel {worst['cost']:.3e}, rotation {worst['rot']:.3e} deg, T {worst['t']:.3e} mm; "
          f"reported mean error off by {worst['mean']:.3e} px, inlier RMS by {worst['rms']:.3e} px")
    assert worst["cost"] <= COST_REL_BOUND
    assert worst["rot"] <= ROT_DEG_BOUND and worst["t"] <= T_MM_BOUND
    assert worst["mean"] <= 1e-9 and worst["rms"] <= 1e-9


def test_exact_cases_against_truth(batches, results):
    dev, ref_gap, n = [0.0, 0.0], [0.0, 0.0], 0
    for b, r in zip(batches, results):
        R, T = r["R"].cpu().numpy(), r["T"].cpu().numpy()
        for k, p in enumerate(b["problems"]):
            if not p["exact"]:
                continue
            ref = P.refine(p["sol"], b["world"], p["image"])
            ref_gap = [max(ref_gap[0], P.rotation_angle_deg(ref["R"], p["R"])), max(ref_gap[1], float(np.abs(ref["t"] - p["t"]).max()))]
            dev = [max(dev[0], P.rotation_angle_deg(R[k], p["R"])), max(dev[1], float(np.abs(T[k] - p["t"]).max()))]
            n += 1
    print(f"{n} exact cases: scipy vs truth {ref_gap[0]:.3e} deg {ref_gap[1]:.3e} mm; device vs truth {dev[0]:.3e} deg {dev[1]:.3e} mm")
    assert n == 12
    assert dev[0] <= TRUTH_ROT_DEG_BOUND and dev[1] <= TRUTH_T_MM_BOUND


def test_table_form_is_bit_identical(batches, results):
    for b, r in zip(batches, results):
        same_bits(run(b, "table"), r)


def test_two_runs_are_bit_identical(batches, results):
    for b, r in zip(batches[:2], results[:2]):
        same_bits(run(b), r)


def test_result_does_not_depend_on_the_batch(batches, results):
    """B = 1 against the same problem inside a batch of 64 (the batch's problems repeated), failed neighbours included."""
    from vbs_amd.engine import pnp_ransac
    for b, r in zip(batches[:2], results[:2]):
        nb = len(b["problems"])
        order = [k % nb for k in range(64)]
        image = np.stack([b["problems"][k]["image"] for k in order])
        valid = np.stack([b["problems"][k]["valid"] for k in order])
        big = pnp_ransac(b["world"], image, camera(b), reproj_px=b["reproj_px"], samples=b["samples"], valid=valid)
        for k in (0, 2, 4, 9):
            one = run(b, only=[k])
            same_bits(one, r, slice(0, 1), slice(k, k + 1))
            for at in (k, k + nb, k + 5 * nb):
                same_bits(one, big, slice(0, 1), slice(at, at + 1))


def test_failed_problem_leaves_neighbours_intact(batches, results):
    """The degenerate problems sit at 3 and 6: their neighbours equal what they give alone, and the failures carry their status."""
    b, r = batches[0], results[0]
    st = r["status"].cpu().numpy()
    assert st[3] == L.PNP_FEW_POINTS and st[6] == L.PNP_NO_HYPOTHESIS
    assert (r["winner"].cpu().numpy()[[3, 6]] == -1).all()
    for k in (2, 4, 5, 7):
        assert st[k] == 0
        same_bits(run(b, only=[k]), r, slice(0, 1), slice(k, k + 1))


def test_calibrate_camera_extrinsics(batches, capsys):
    from vbs_amd.extrinsic_calibration import calibrate_camera_extrinsics
    b = batches[1]                                             # the shell, distortion on
    p = b["problems"][8]                                       # noise and outliers, every ID tracked
    assert p["valid"].all() and p["outlier"].any()
    R, T, error = calibrate_camera_extrinsics(b["world"], p["image"], b["K"], b["dist"])
    assert R.shape == (3, 3) and T.shape == (3, 1)
    w32 = b["world"].astype(np.float32).astype(np.float64)     # the reference's casts (:93-94)
    want = np.mean(np.linalg.norm(np.stack(P.project(P.camera(b["K"], b["dist"]), R.reshape(9), T.reshape(3), w32[:, 0], w32[:, 1],
                                                     w32[:, 2])[:2], axis=1) - p["image"], axis=1))
    print(f"error {error!r}, helper's projection of all points {want!r}")
    assert abs(error - want) <= 1e-9
    assert "PnP solved with" in capsys.readouterr().out
    assert calibrate_camera_extrinsics(b["world"][:3], p["image"][:3], b["K"], b["dist"]) == (None, None, None)
    line = P.collinear_indices(b["world"])
    assert calibrate_camera_extrinsics(b["world"][line], p["image"][line], b["K"], b["dist"]) == (None, None, None)


def test_calibrate_recording_on_a_tracked_still():
    """A still synthetic recording of the shell under a known pose, tracked by Engine.track_to_3d: one pose per frame; their mean
    reproduces the pose the frames were rendered with as well as the helper's own per-frame solution of the same table does."""
    import vbs_amd.synth as S
    from vbs_amd.engine import Engine
    from vbs_amd.extrinsic_calibration import calibrate_recording
    world = P.shell_layout()
    K = np.array([[480.0, 0, 320.0], [0, 480.0, 240.0], [0, 0, 1]], dtype=np.float32)
    dist = np.zeros(5, dtype=np.float32)
    Rt = P.rodrigues(np.radians([2.0, -3.0, 4.0]))
    Tt = np.array([0.4, -0.3, 40.0])
    cam = P.camera(K, dist)
    u, v, _ = P.project(cam, Rt.reshape(9), Tt, world[:, 0], world[:, 1], world[:, 2])
    c16 = np.round(np.column_stack([u, v]) * 16).astype(np.int64)
    spec = S.FrameSpec(640, 480, c16, 20 * 16, jitter16=0, djitter16=0, name="shell_still")
    n = 12
    frames = S.make_frames(spec, list(range(n)), seed=3, channels=1)
    eng = Engine(spec.height, spec.width, max_markers=256, max_batch=n, device=0)
    table, _, _ = eng.track_to_3d(torch.from_numpy(frames).cuda(), c16 / 16.0, 20.0, L.make_camera(K, dist, np.eye(3), np.zeros(3)), 5.0)
    tab = table.cpu().numpy()
    assert ((tab[..., 0].astype(int) & L.FLAG_TRACKED) != 0).all(), "the tracker lost markers of the synthetic still"
    res = calibrate_recording(table, world, K, dist, frames=slice(2, n))
    assert res["n_ok"] == n - 2 and (res["status"] == 0).all() and list(res["frames"]) == list(range(2, n))
    assert res["R"].shape == (n - 2, 3, 3) and res["T_std"].shape == (3,) and res["R_std"].shape == (3, 3)
    smp = P.samples(len(world), 1000, 0)
    hR, hT = [], []
    for f in range(2, n):
        img = tab[f, :, 1:3].astype(np.float64)
        sol = P.solve(world, img, np.ones(len(world), dtype=bool), K, dist, smp)
        assert sol["status"] == 0 and sol["mask"].all()
        ref = P.refine(sol, world, img)
        hR.append(ref["R"])
        hT.append(ref["t"])
        k = f - 2
        gap = (P.rotation_angle_deg(res["R"][k], ref["R"]), float(np.abs(res["T"][k] - ref["t"]).max()))
        print(f"frame {f}: device vs scipy {gap[0]:.3e} deg {gap[1]:.3e} mm")
        assert gap[0] <= ROT_DEG_BOUND and gap[1] <= T_MM_BOUND
    uu, _, vt = np.linalg.svd(np.mean(hR, axis=0))
    hRm, hTm = uu @ vt, np.mean(hT, axis=0)
    h_rot, h_t = P.rotation_angle_deg(hRm, Rt), float(np.abs(hTm - Tt).max())
    d_rot, d_t = P.rotation_angle_deg(res["R_mean"], Rt), float(np.abs(res["T_mean"] - Tt).max())
    print(f"mean pose vs rendered: helper {h_rot:.3e} deg {h_t:.3e} mm, device {d_rot:.3e} deg {d_t:.3e} mm; "
          f"T std {res['T_std']}")
    assert d_rot <= h_rot + ROT_DEG_BOUND and d_t <= h_t + T_MM_BOUND
    eng.close()
