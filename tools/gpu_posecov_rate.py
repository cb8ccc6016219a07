"""Time of `vbs_pose_cov` (k_posecov.hip) on a resident table, next to `vbs_pose_series` on the same table.

For 4096 frames x 169 and x 441 markers (a tilt ramp plus pixel noise, 3 % of the rows untracked), a distorted camera and camera
factors of q = 5 and q = 16 columns, with and without one round of rejection (reject_k = 0 and 3): HIP-event time per call of
`vbs_pose_cov` emitting `pose` and `pcov`, with the reference rows given, and of `vbs_pose_series` emitting `pose` alone, after
warm-up calls, median and minimum over `--reps` calls.  `vbs_pose_cov` recomputes the solve of every used row once for Sigma_obs
and once per camera column, so its time grows with 1 + q; `vbs_pose_series` reads 40-byte rows and nothing else.
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under
its own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape;
`--out FILE` also appends them there.

    python tools/gpu_posecov_rate.py [--reps 10] [--limit 240] [--out profiles/posecov_rate.log]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = tuple((s, q, k) for s in (169, 441) for q in (5, 16) for k in (0.0, 3.0))
DIST = (-0.28, 0.09, 1e-3, -5e-4, -0.01)


def recording(n, m, cam, seed, ramp_px):
    """-> float32 table [n, m, 10] with X, Y, Z from `engine.calculate_3d(undistort_points(..))`: the diameters of the markers grow
    along x by up to `ramp_px` over the recording (a tilt), plus pixel noise; 3 % of the rows are untracked."""
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import calculate_3d, undistort_points
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    gx, gy = np.meshgrid(np.linspace(200, 1720, side), np.linspace(150, 1050, side))
    gx, gy = gx.ravel()[:m], gy.ravel()[:m]
    f = np.linspace(0.0, 1.0, n)
    o = np.stack([np.broadcast_to(gx, (n, m)), np.broadcast_to(gy, (n, m)),
                  16.0 + ramp_px * f[:, None] * ((gx - 960.0) / 760.0)[None, :]], axis=2) + r.normal(0.0, 0.05, (n, m, 3))
    t = np.zeros((n, m, L.TABLE_COLS), dtype=np.float32)
    t[..., 1:4] = o
    uvd = t[..., 1:4].reshape(-1, 3).astype(np.float64)
    und = undistort_points(uvd[:, :2].copy(), cam)
    xyz, ok = calculate_3d(torch.cat([und, torch.as_tensor(uvd[:, 2:3], device=und.device)], dim=1), cam)
    t[..., 6:9] = xyz.cpu().numpy().reshape(n, m, 3)
    tracked = r.random((n, m)) >= 0.03
    tracked[0] = True
    t[..., 0] = tracked * (1 + 2 * ok.cpu().numpy().reshape(n, m))
    return t


def one_shape(m, q, reject_k, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import uncertainty as UN
    from vbs_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    K = np.array([[1500.0 * 1.01, 0, 963.3], [0, 1500.0 * 0.99, 597.9], [0, 0, 1]])
    a, b = 0.3, 0.2
    R = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @
         np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    cam = L.make_camera(K, DIST, R, np.array([3.0, -2.0, 40.0]), 2.0)
    tab = torch.from_numpy(recording(n, m, cam, m, 0.4)).cuda()
    rows = torch.from_numpy(recording(2, m, cam, m + 1, 0.0)).cuda()
    obs = np.ascontiguousarray(UN.obs_cov(0.05, 0.05).reshape(1, 6))
    if q == 5:
        fac = UN.camera_factor(omega_std=[1e-4] * 3, t_std=[0.02, 0.02, 0.0])
    else:
        r = np.random.default_rng(1)
        sd = np.array([0.5, 0.5, 0.3, 0.3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-3, 1e-4, 1e-4, 1e-4, 0.02, 0.02, 0.05, 0.01])
        fac = np.tril(r.normal(size=(16, 16))) * sd[:, None]
    fac = np.ascontiguousarray(fac)
    assert fac.shape == (16, q)
    dev = torch.device("cuda", 0)
    eng = Engine(1200, 1920, max_markers=512, max_batch=2)
    ref_disp = eng.axis_displacement(rows, 0, None, frame_range=(1, 2))[0][0].contiguous()
    ref_xyz = tab[0, :, 6:9].to(torch.float64).contiguous()
    work = torch.empty((m * L.UNCERT_WORK_COLS,), dtype=torch.float64, device=dev)
    pose = torch.empty((n, L.POSE_COLS), dtype=torch.float64, device=dev)
    pose2 = torch.empty((n, L.POSE_COLS), dtype=torch.float64, device=dev)
    pcov = torch.empty((n, L.POSECOV_COLS), dtype=torch.float64, device=dev)
    hp, p = A._host_ptr, A._ptr

    def timed(fn, warm=2):
        for i in range(warm):
            fn(i)
        torch.cuda.synchronize()
        ts = []
        for i in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts))}

    res = {"frames": n, "slots": m, "q": q, "reject_k": reject_k, "device": torch.cuda.get_device_name(0), "reps": reps,
           "posecov_group": L.POSECOV_GROUP}
    res["pose_cov"] = timed(lambda i: A._call("vbs_pose_cov", "", dev, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 0, 1.0, reject_k,
                                              C.byref(cam), hp(obs), 1, hp(fac), q, 5.0, 1e-12, p(rows), 0, n, p(work), p(pose), p(pcov)))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res["pose_series"] = timed(lambda i: eng.lib.vbs_pose_series(eng._h, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 0, 1.0, reject_k,
                                                                 0, n, None, None, p(pose2), stream))
    torch.cuda.synchronize()
    flag = pcov[:, 0].to(torch.int64)
    res["frames_with_covariance"] = int(((flag & 1) != 0).sum())
    res["frames_refitted"] = int((pose[:, 0] == 2).sum())
    res["pose_equal_bits"] = bool(torch.equal(pose[:, [0, 1, 2, 3, 7]], pose2[:, [0, 1, 2, 3, 7]]))
    res["ratio_to_pose_series"] = res["pose_cov"]["median_us"] / res["pose_series"]["median_us"]
    good = (flag & 4) != 0
    res["median_sigma_tilt_deg"] = float(torch.sqrt(pcov[good, 14]).median()) if bool(good.any()) else None
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,q,reject_k of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        m, q, k = a.shape.split(",")
        print(json.dumps(one_shape(int(m), int(q), float(k), a.reps)), flush=True)
        return 0
    for m, q, k in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{m},{q},{k}", "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {m} q {q} reject_k {k}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {m} q {q} reject_k {k}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
