"""Time of `vbs_shape_series` (k_shape.hip) on a resident table, next to `vbs_pose_series` on the same table in the same run.

For 4096 frames x 169 and x 441 markers (a bowl that deepens along the recording plus noise, 3 % of the rows without a 3-D point,
two lifted markers per frame for the rejection to find), with and without one round of rejection (reject_k = 0 and 3): HIP-event
time per call of `vbs_shape_series` emitting `shape`, `coef` and `residual`, and of `vbs_pose_series` emitting `pose` alone, after
warm-up calls, median and minimum over `--reps` calls.  The yardstick is a batched float64 `torch.linalg.lstsq` on the same end
points (the design matrix [1, u, v, u2, uv, v2] of every frame, rows of missing markers zeroed), which gives the six coefficients
and nothing else; it solves matrix after matrix, so it is timed over the first `YARD_FRAMES` frames only, one warm-up and three
calls, and both sides are also given per frame.  No rate is a pass criterion; the figures are single-run numbers on a shared
machine.  Every shape runs in a child process under its own time limit (`--limit` seconds); a child that fails or runs out of time
ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_shape_rate.py [--reps 10] [--limit 240] [--out profiles/shape_rate.log]
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
YARD_FRAMES = 256              # frames the yardstick is timed over (it is a loop over matrices)
SHAPES = tuple((s, k) for s in (169, 441) for k in (0.0, 3.0))


def recording(n, m, seed):
    """-> (float32 table [n, m, 10], ref_xyz float64 [m, 3]): markers on a square grid of 2 mm, frame f pressed by a paraboloid of
    curvature 1 / 60 per mm whose depth grows with f, 0.01 mm noise, 3 % of the rows without a point, two markers lifted by 2 mm."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    i = np.arange(m)
    ref = np.stack([(i % side - (side - 1) / 2) * 2.0, (i // side - (side - 1) / 2) * 2.0, np.zeros(m)], axis=1)
    rho2 = (ref[:, 0] - 1.5) ** 2 + (ref[:, 1] + 1.0) ** 2
    xyz = np.broadcast_to(ref[None], (n, m, 3)).copy()
    xyz[..., 2] += np.linspace(0.0, 1.0, n)[:, None] * (rho2[None, :] / 120.0 - 1.0)
    xyz += r.normal(0.0, 0.01, (n, m, 3))
    lifted = r.integers(0, m, (n, 2))
    xyz[np.arange(n)[:, None], lifted, 2] += 2.0
    xyz[0] = ref
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 6:9] = xyz
    seen = r.random((n, m)) >= 0.03
    seen[0] = True
    t[..., 0] = 1 + 2 * seen
    return t, ref


def one_shape(m, reject_k, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import shapes
    from vbs_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    dev = torch.device("cuda", 0)
    t, ref = recording(n, m, m)
    tab = torch.from_numpy(t).cuda()
    ref_xyz = torch.from_numpy(ref).cuda()
    ref_disp = torch.zeros((m, 4), dtype=torch.float64, device=dev)
    ref_disp[:, 0] = 1.0
    length = shapes.default_length(ref)
    eng = Engine(1200, 1920, max_markers=512, max_batch=2)
    shape = torch.empty((n, L.SHAPE_COLS), dtype=torch.float64, device=dev)
    coef = torch.empty((n, 2, 4), dtype=torch.float64, device=dev)
    resid = torch.empty((n, m, 2), dtype=torch.float64, device=dev)
    pose = torch.empty((n, L.POSE_COLS), dtype=torch.float64, device=dev)
    p = A._ptr

    def timed(fn, warm=2, reps=reps):
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

    res = {"frames": n, "slots": m, "reject_k": reject_k, "device": torch.cuda.get_device_name(0), "reps": reps,
           "shape_group": L.SHAPE_GROUP, "length": length}
    res["shape_series"] = timed(lambda i: A._call("vbs_shape_series", "", dev, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 0, 1.0,
                                                  length, reject_k, 9, 1e-10, 1e-6, 2.0, 0, n, p(shape), p(coef), p(resid)))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res["pose_series"] = timed(lambda i: eng.lib.vbs_pose_series(eng._h, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 0, 1.0, reject_k,
                                                                 0, n, None, None, p(pose), stream))

    print(f"slots {m} reject_k {reject_k}: entries timed, yardstick next", file=sys.stderr, flush=True)
    ny = min(n, YARD_FRAMES)
    seen = ((tab[:ny, :, 0].to(torch.int32) & 2) != 0).to(torch.float64)
    P = torch.cat([ref_xyz[None, :, :2].expand(ny, m, 2), torch.zeros((ny, m, 1), dtype=torch.float64, device=dev)], dim=2) + \
        (tab[:ny, :, 6:9].to(torch.float64) - tab[0:1, :, 6:9].to(torch.float64))

    def yardstick(i):
        cnt = seen.sum(dim=1, keepdim=True)
        mean = (P * seen[..., None]).sum(dim=1, keepdim=True) / cnt[..., None]
        u, v, w = (P[..., 0] - mean[..., 0]) / length, (P[..., 1] - mean[..., 1]) / length, P[..., 2] - mean[..., 2]
        Am = torch.stack([torch.ones_like(u), u, v, u * u, u * v, v * v], dim=2) * seen[..., None]
        return torch.linalg.lstsq(Am, (w * seen)[..., None]).solution[..., 0]

    res["torch_lstsq"] = dict(timed(yardstick, warm=1, reps=3), frames=ny)
    torch.cuda.synchronize()
    beta = yardstick(0)
    deg2 = shape[:, 0] == 2.0
    first = (deg2 & (shape[:, 2] == shape[:, 1]))[:ny]           # the yardstick fits all common slots: compare where nothing was rejected
    res["frames_degree_2"] = int(deg2.sum())
    res["frames_refitted"] = int((shape[:, 2] < shape[:, 1]).sum())
    res["frames_with_apex"] = int((shape[:, 19] == 1.0).sum())
    if bool(first.any()):
        pq = torch.stack([2.0 * beta[:, 3], beta[:, 4], 2.0 * beta[:, 5]], dim=1) / (length * length)
        res["max_hessian_diff_to_lstsq"] = float((pq[first] - shape[:ny][first, 9:12]).abs().max())
    res["ratio_to_pose_series"] = res["shape_series"]["median_us"] / res["pose_series"]["median_us"]
    res["shape_us_per_frame"] = res["shape_series"]["median_us"] / n
    res["lstsq_us_per_frame"] = res["torch_lstsq"]["median_us"] / ny
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,reject_k of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        m, k = a.shape.split(",")
        print(json.dumps(one_shape(int(m), float(k), a.reps)), flush=True)
        return 0
    for m, k in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{m},{k}", "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired as e:
            print(f"slots {m} reject_k {k}: no result within {a.limit} s; stopping\n{(e.stderr or b'')[-500:]}", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {m} reject_k {k}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
