"""Time of the contact maps (k_field.hip) on a resident recording, with a library product as the yardstick.

For 4096 frames x 169 and x 441 slots (a Gaussian dimple walking over the node grid, 3 % of the entries missing) and grids of
32 x 32 and 64 x 64 points: HIP-event time per call of `engine.field_map_f64` (all frames, one launch) and of
`engine.patch_stats_f64` on its result, after warm-up calls of every shape, median and minimum over `--reps` calls, the record
rotated over `--buffers` copies.  Beside it, on the same device:
  * float64 `torch.matmul` of the same W [P, s] against the same SELECTED columns [s, frames x 4] (values of invalid entries set
    to 0, the flag as 1.0 / 0.0 - prepared once, outside the timed region), plus the division by the flag column's product.
    A YARDSTICK ONLY: no flags in the output, no coverage rule, and its operand was selected for it.
Every shape runs in a child process under its own time limit (`--limit` seconds), so one slow shape cannot take the others with
it; a child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_field_rate.py [--reps 20] [--buffers 2] [--limit 120] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = ((169, 32), (169, 64), (441, 32), (441, 64))


def recording(n, side, seed, drop=0.03):
    """-> (rec float64 [n, side^2, 4] = flag, dX, dY, dZ, nodes [side^2, 2])."""
    import numpy as np
    r = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    nodes = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)
    cx = np.linspace(3.0, side - 4.0, n)
    cy = (side - 1) / 2 + 2.0 * np.sin(np.linspace(0.0, 6.0, n))
    r2 = (nodes[None, :, 0] - cx[:, None]) ** 2 + (nodes[None, :, 1] - cy[:, None]) ** 2
    rec = np.zeros((n, side * side, 4))
    rec[..., 0] = r.random((n, side * side)) >= drop
    rec[..., 3] = 0.8 * np.exp(-r2 / (2 * 1.6 ** 2))
    rec[..., 1:3] = r.normal(0.0, 0.01, (n, side * side, 2))
    rec[..., 1:][rec[..., 0] == 0.0] = np.nan
    return rec, nodes


def one_shape(s, g, reps, buffers):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import fields
    from vbs_amd.engine import field_map_f64, patch_stats_f64
    assert torch.cuda.is_available(), "needs a GPU"
    side = int(round(s ** 0.5))
    rec, nodes = recording(FRAMES, side, s)
    grid, _ = fields.grid_over(nodes, (g, g))
    W = fields.gaussian_weights(nodes, grid, 1.0)
    Wd, ws, gd = torch.from_numpy(W).cuda(), torch.from_numpy(fields.row_sums(W)).cuda(), torch.from_numpy(grid).cuda()
    recs = [torch.from_numpy(rec).cuda() for _ in range(buffers)]

    def timed(fn, warm=3):
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

    P = g * g
    res = {"frames": FRAMES, "slots": s, "grid": [g, g], "device": torch.cuda.get_device_name(0), "reps": reps, "buffers": buffers,
           "field_frames": L.FIELD_FRAMES, "patch_group": L.PATCH_GROUP, "multiply_adds": P * s * 4 * FRAMES}
    res["field_map_f64"] = timed(lambda i: field_map_f64(recs[i % buffers], Wd, ws, 0.5, 3))
    mp = field_map_f64(recs[0], Wd, ws, 0.5, 3)
    res["patch_stats_f64"] = timed(lambda i: patch_stats_f64(mp, gd, 2, 1.0, 0.2))
    res["frames_with_a_patch"] = int((patch_stats_f64(mp, gd, 2, 1.0, 0.2)[:, 0] == 2).sum())
    # the yardstick: the selected operand [s, F * 4] is prepared once, outside the timed region
    sel = []
    for r in recs:
        v = torch.where(r[..., :1] != 0, r[..., 1:4], torch.zeros((), dtype=torch.float64, device="cuda"))
        x = torch.cat([v, (r[..., :1] != 0).to(torch.float64)], dim=2)               # [F, s, 4]: x1, x2, x3, flag
        sel.append(x.permute(1, 0, 2).reshape(s, FRAMES * 4).contiguous())

    def yard(i):
        prod = torch.matmul(Wd, sel[i % buffers]).view(P, FRAMES, 4)
        return prod[..., :3] / prod[..., 3:]
    res["matmul_f64_yardstick"] = timed(yard)
    us = res["field_map_f64"]["median_us"]
    res["gflops_f64"] = 2 * res["multiply_adds"] / us * 1e-3
    res["speedup_over_matmul_yardstick"] = res["matmul_f64_yardstick"]["median_us"] / us
    ok = mp[..., 0] != 0
    ref = yard(0).permute(1, 0, 2)
    res["max_abs_difference_from_yardstick"] = float((mp[..., 1:][ok] - ref[ok]).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,grid of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        s, g = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(s, g, a.reps, a.buffers)), flush=True)
        return 0
    for s, g in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{s},{g}", "--reps", str(a.reps), "--buffers", str(a.buffers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {s} grid {g}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {s} grid {g}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
