"""Time of `vbs_rigid_series` (k_rigid.hip) on a resident table, next to `vbs_shape_series` and `vbs_pose_series` on the same table
in the same run.

For 4096 frames x 169 and x 441 markers (a shallow dome that tilts, twists and shifts along the recording plus noise, 3 % of the
rows without a 3-D point, two markers moved by 2 mm per frame for the rejection to find), with and without one round of rejection
(reject_k = 0 and 3): HIP-event time per call of `vbs_rigid_series` emitting `rigid`, `coef` and `residual` (with_scale 0), of
`vbs_shape_series` emitting its three outputs and of `vbs_pose_series` emitting `pose` alone, after warm-up calls, median and
minimum over `--reps` calls.  The yardstick is a batched float64 `torch.linalg.svd` Kabsch fit on PRE-SELECTED points (every
marker of every frame, no flags, no gaps, no residual record): means, the 3 x 3 products, the SVD, the determinant fix, R and t.
The rotations of the two are compared where nothing is missing from what the yardstick sees (it reads every row, so only the
size of the difference is reported, not asserted).  No rate is a pass criterion; the figures are single-run numbers on a shared
machine.  Every shape runs in a child process under its own time limit (`--limit` seconds); a child that fails or runs out of time
ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_rigid_rate.py [--reps 10] [--limit 240] [--out profiles/rigid_rate.log]
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
SHAPES = tuple((s, k) for s in (169, 441) for k in (0.0, 3.0))


def recording(n, m, seed):
    """-> (float32 table [n, m, 10], layout float64 [m, 3]): markers on a square grid of 2 mm on a shallow dome; frame f is the
    layout tilted by up to 2 degrees, twisted by up to 3 and shifted by up to 0.5 mm, with 0.01 mm noise, 3 % of the rows without a
    point and two markers moved by 2 mm."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    i = np.arange(m)
    lay = np.stack([(i % side - (side - 1) / 2) * 2.0, (i // side - (side - 1) / 2) * 2.0, np.zeros(m)], axis=1)
    lay[:, 2] = 3.0 - 0.005 * (lay[:, 0] ** 2 + lay[:, 1] ** 2)
    u = np.linspace(0.0, 1.0, n)
    a, b, c = np.radians(2.0) * u, np.radians(-1.0) * u, np.radians(3.0) * u      # about x, about y, about z
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    one, zero = np.ones(n), np.zeros(n)
    Rx = np.stack([one, zero, zero, zero, ca, -sa, zero, sa, ca], axis=1).reshape(n, 3, 3)
    Ry = np.stack([cb, zero, sb, zero, one, zero, -sb, zero, cb], axis=1).reshape(n, 3, 3)
    Rz = np.stack([cc, -sc, zero, sc, cc, zero, zero, zero, one], axis=1).reshape(n, 3, 3)
    R = Rx @ Ry @ Rz
    xyz = np.einsum("fij,mj->fmi", R, lay) + (u[:, None] * np.array([0.5, -0.3, 0.2]))[:, None, :]
    xyz += r.normal(0.0, 0.01, (n, m, 3))
    moved = r.integers(0, m, (n, 2))
    xyz[np.arange(n)[:, None], moved, 2] += 2.0
    xyz[0] = lay
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 6:9] = xyz
    seen = r.random((n, m)) >= 0.03
    seen[0] = True
    t[..., 0] = 1 + 2 * seen
    return t, lay


def one_shape(m, reject_k, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import rigid as RG
    from vbs_amd import shapes
    from vbs_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    dev = torch.device("cuda", 0)
    t, lay = recording(n, m, m)
    tab = torch.from_numpy(t).cuda()
    source = torch.from_numpy(RG.source_from_table(t, 0)).cuda()
    ref_xyz = torch.from_numpy(lay).cuda()
    ref_disp = torch.zeros((m, 4), dtype=torch.float64, device=dev)
    ref_disp[:, 0] = 1.0
    length = shapes.default_length(lay)
    eng = Engine(1200, 1920, max_markers=512, max_batch=2)
    rigid = torch.empty((n, L.RIGID_COLS), dtype=torch.float64, device=dev)
    rcoef = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    rres = torch.empty((n, m, 4), dtype=torch.float64, device=dev)
    shape = torch.empty((n, L.SHAPE_COLS), dtype=torch.float64, device=dev)
    scoef = torch.empty((n, 2, 4), dtype=torch.float64, device=dev)
    sres = torch.empty((n, m, 2), dtype=torch.float64, device=dev)
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
           "rigid_group": L.RIGID_GROUP, "sweeps": L.RIGID_SWEEPS}
    res["rigid_series"] = timed(lambda i: A._call("vbs_rigid_series", "", dev, p(tab), n, m, p(source), None, 0, reject_k, 1e-6, 0, n,
                                                  p(rigid), p(rcoef), p(rres)))
    res["shape_series"] = timed(lambda i: A._call("vbs_shape_series", "", dev, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 1, 1.0,
                                                  length, reject_k, 9, 1e-10, 1e-6, 2.0, 0, n, p(shape), p(scoef), p(sres)))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res["pose_series"] = timed(lambda i: eng.lib.vbs_pose_series(eng._h, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 1, 1.0, reject_k,
                                                                 0, n, None, None, p(pose), stream))

    print(f"slots {m} reject_k {reject_k}: entries timed, yardstick next", file=sys.stderr, flush=True)
    Q = source[None, :, 1:4]
    P = tab[:, :, 6:9].to(torch.float64)

    def yardstick(i):
        qm, pm = Q.mean(dim=1, keepdim=True), P.mean(dim=1, keepdim=True)
        q, pc = Q - qm, P - pm
        M = pc.transpose(1, 2) @ q.expand(n, m, 3)                # sum p q'
        U, S, Vh = torch.linalg.svd(M)
        d = torch.ones((n, 3), dtype=torch.float64, device=dev)
        d[:, 2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))
        R = (U * d[:, None, :]) @ Vh
        return R, pm[:, 0] - (R @ qm[0, 0])

    res["torch_svd_kabsch"] = timed(yardstick, warm=1, reps=3)
    torch.cuda.synchronize()
    R, _ = yardstick(0)
    full = ((tab[:, :, 0].to(torch.int32) & 2) != 0).all(dim=1) & (rigid[:, 0] == 1.0)
    res["frames_with_fit"] = int((rigid[:, 0] >= 1.0).sum())
    res["frames_refitted"] = int((rigid[:, 0] == 2.0).sum())
    res["frames_compared"] = int(full.sum())
    if bool(full.any()):
        res["max_rotation_diff_to_svd"] = float((R[full].reshape(-1, 9) - rigid[full, 13:22]).abs().max())
    res["ratio_to_pose_series"] = res["rigid_series"]["median_us"] / res["pose_series"]["median_us"]
    res["ratio_to_shape_series"] = res["rigid_series"]["median_us"] / res["shape_series"]["median_us"]
    res["rigid_us_per_frame"] = res["rigid_series"]["median_us"] / n
    res["svd_us_per_frame"] = res["torch_svd_kabsch"]["median_us"] / n
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
