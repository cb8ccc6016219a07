"""Time of `vbs_sphere_series` (k_sphere.hip) on a resident table, next to `vbs_rigid_series` and `vbs_pose_series` on the same table
in the same run.

For 4096 frames x 169 and x 441 markers (a grid on a sphere of R = 27 mm cut by a plane whose depth grows to 2.8 mm while it leans
to 15 degrees, plus 0.02 mm of noise, 3 % of the rows without a 3-D point), in BOTH modes - the sphere fitted per frame with one
round of rejection (reject_k = 3), and the sphere given and held -: HIP-event time per call of `vbs_sphere_series` emitting
`sphere`, `radial` and `decomp`, of `vbs_rigid_series` emitting its three outputs (reject_k = 3) and of `vbs_pose_series` emitting
`pose` alone, after warm-up calls, median and minimum over `--reps` calls.  No rate is a pass criterion; the figures are single-run
numbers on a shared machine.  Every shape runs in a child process under its own time limit (`--limit` seconds); a child that fails
or runs out of time ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_sphere_rate.py [--reps 10] [--limit 240] [--out profiles/sphere_rate.log]
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
SHAPES = tuple((s, mode) for s in (169, 441) for mode in ("fit", "given"))
CENTRE, RADIUS = (0.0, 0.0, 27.0), 27.0


def recording(n, m, seed):
    """-> (float32 table [n, m, 10], layout float64 [m, 3]): markers on a square grid inside a radius of 16 mm on the sphere; frame
    f is the cap cut at 2.8 f / (n - 1) mm by a plane leaning 15 f / (n - 1) degrees towards 35, with 0.02 mm noise and 3 % of the
    rows without a point."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    pitch = 22.0 / (side - 1)
    i = np.arange(m)
    xy = np.stack([(i % side - (side - 1) / 2) * pitch, (i // side - (side - 1) / 2) * pitch], axis=1)
    c = np.asarray(CENTRE)
    lay = np.column_stack([xy, c[2] - np.sqrt(RADIUS ** 2 - (xy ** 2).sum(axis=1))])
    u = np.linspace(0.0, 1.0, n)
    tilt, az = np.radians(15.0) * u, np.radians(35.0)
    nrm = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)      # [n, 3]
    over = np.maximum(((c - lay)[None] * nrm[:, None, :]).sum(axis=2) - (RADIUS - 2.8 * u)[:, None], 0.0)
    xyz = lay[None] + over[..., None] * nrm[:, None, :] + r.normal(0.0, 0.02, (n, m, 3))
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 6:9] = xyz
    seen = r.random((n, m)) >= 0.03
    seen[0] = True
    t[..., 0] = 1 + 2 * seen
    return t, lay


def one_shape(m, mode, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import rigid as RG
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
    eng = Engine(1200, 1920, max_markers=512, max_batch=2)
    sph = torch.empty((n, L.SPHERE_COLS), dtype=torch.float64, device=dev)
    rad = torch.empty((n, m, 2), dtype=torch.float64, device=dev)
    dec = torch.empty((n, m, 4), dtype=torch.float64, device=dev)
    rigid = torch.empty((n, L.RIGID_COLS), dtype=torch.float64, device=dev)
    rcoef = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    rres = torch.empty((n, m, 4), dtype=torch.float64, device=dev)
    pose = torch.empty((n, L.POSE_COLS), dtype=torch.float64, device=dev)
    p = A._ptr
    held = np.ascontiguousarray(np.asarray(CENTRE + (RADIUS,), dtype=np.float64))
    given = A._host_ptr(held) if mode == "given" else C.c_void_p(0)
    reject_k = 3.0 if mode == "fit" else 0.0

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

    res = {"frames": n, "slots": m, "mode": mode, "reject_k": reject_k, "device": torch.cuda.get_device_name(0), "reps": reps,
           "sphere_group": L.SPHERE_GROUP, "sweeps": L.SPHERE_SWEEPS}
    res["sphere_series"] = timed(lambda i: A._call("vbs_sphere_series", "", dev, p(tab), n, m, given, None, None, p(source), 0.1, 1e-9,
                                                   1e-3, reject_k, 0, n, p(sph), p(rad), p(dec)))
    res["rigid_series"] = timed(lambda i: A._call("vbs_rigid_series", "", dev, p(tab), n, m, p(source), None, 0, 3.0, 1e-6, 0, n,
                                                  p(rigid), p(rcoef), p(rres)))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    res["pose_series"] = timed(lambda i: eng.lib.vbs_pose_series(eng._h, p(tab), n, m, 0, p(ref_disp), p(ref_xyz), None, 1, 1.0, 3.0,
                                                                 0, n, None, None, p(pose), stream))
    torch.cuda.synchronize()
    rows = sph.cpu().numpy()
    flat = rows[:, 0] == 3.0
    res["frames_with_sphere"] = int((rows[:, 0] >= 1.0).sum())
    res["frames_with_plane"] = int(flat.sum())
    res["frames_refitted"] = int((rows[:, 3] == 1.0).sum())
    if flat.any():
        res["max_offset_error_mm"] = float(np.abs(rows[flat, 22] - 2.8 * np.linspace(0.0, 1.0, n)[flat]).max())
    res["ratio_to_rigid_series"] = res["sphere_series"]["median_us"] / res["rigid_series"]["median_us"]
    res["ratio_to_pose_series"] = res["sphere_series"]["median_us"] / res["pose_series"]["median_us"]
    res["sphere_us_per_frame"] = res["sphere_series"]["median_us"] / n
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,mode of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        m, mode = a.shape.split(",")
        print(json.dumps(one_shape(int(m), mode, a.reps)), flush=True)
        return 0
    for m, mode in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{m},{mode}", "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired as e:
            print(f"slots {m} mode {mode}: no result within {a.limit} s; stopping\n{(e.stderr or b'')[-500:]}", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {m} mode {mode}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
