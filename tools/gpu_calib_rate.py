#!/usr/bin/env python3
"""Rate of engine.calibrate_camera_points (intrinsic calibration) on 20 synthetic views of a 6 x 6 board, as 1 problem (all
views), 21 (the jackknife) and 1000 (random subsets of 10 views).

    python tools/gpu_calib_rate.py [--views 20] [--reps 10] [--warmup 2]

HIP events around the whole call (output buffers included), median over `reps` after `warmup`.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from vbs_amd.engine import calibrate_camera_points            # noqa: E402
import calib_oracle as O                                      # noqa: E402   (the case generator only)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    c = O.make_case("rate", a.views, (6, 6), O.DIST_A, 0.1, 0)
    obj, img = torch.as_tensor(c["obj"], device="cuda"), torch.as_tensor(c["imgs"], device="cuda")
    rng = np.random.default_rng(0)
    jack = np.ones((a.views + 1, a.views), dtype=np.uint8)
    jack[np.arange(1, a.views + 1), np.arange(a.views)] = 0
    subsets = np.zeros((1000, a.views), dtype=np.uint8)
    for row in subsets:
        row[rng.choice(a.views, size=min(10, a.views), replace=False)] = 1
    out = {"tool": "gpu_calib_rate", "views": a.views, "points": len(c["obj"])}
    for name, mask in (("all_views", None), ("jackknife", jack), ("subsets_1000", subsets)):
        m = None if mask is None else torch.as_tensor(mask, device="cuda")
        times = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = calibrate_camera_points(obj, img, c["size"], view_mask=m)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        nb = 1 if mask is None else len(mask)
        out[name] = {"problems": nb, "median_ms": ms, "problems_per_s": nb / ms * 1e3, "solved": int((res["status"] == 0).sum().item()),
                     "mean_iterations": float(res["iterations"].double().mean().item())}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
