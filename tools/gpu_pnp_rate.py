#!/usr/bin/env python3
"""Rate of engine.pnp_ransac (extrinsic calibration) on a batch of synthetic frames of the 65-dot shell.

    python tools/gpu_pnp_rate.py [--frames 4096] [--hypotheses 1000] [--reps 10] [--warmup 2]

HIP events around the whole call (sample table and buffers included), median over `reps` after `warmup`.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd.engine import pnp_ransac, pnp_samples            # noqa: E402

K = np.array([[1200.0, 0, 640.0], [0, 1195.0, 512.0], [0, 0, 1]], dtype=np.float32)


def shell():
    """65 dots in rings of 1 + 6 + 12 + 18 + 24 + 4 on a shallow shell (mm)."""
    pts = [(3.3 * k * np.cos(2 * np.pi * j / c), 3.3 * k * np.sin(2 * np.pi * j / c)) for k, c in enumerate((1, 6, 12, 18, 24, 4))
           for j in range(c)]
    xy = np.asarray(pts)
    return np.column_stack([xy, 0.012 * (xy ** 2).sum(axis=1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    world = shell()
    rng = np.random.default_rng(0)
    a1, a2 = np.radians(8.0), np.radians(-5.0)                 # a pose tilted about x and y, 40 mm away; no distortion
    Rx = np.array([[1, 0, 0], [0, np.cos(a1), -np.sin(a1)], [0, np.sin(a1), np.cos(a1)]])
    Ry = np.array([[np.cos(a2), 0, np.sin(a2)], [0, 1, 0], [-np.sin(a2), 0, np.cos(a2)]])
    pc = world @ (Rx @ Ry).T + np.array([1.0, -2.0, 40.0])
    uv = pc[:, :2] / pc[:, 2:] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    image = uv[None] + rng.normal(scale=0.3, size=(a.frames, len(world), 2))
    image_d = torch.as_tensor(image, device="cuda")
    smp = pnp_samples(len(world), a.hypotheses, 0)
    c = L.make_camera(K, np.zeros(5), np.eye(3), np.zeros(3))
    times = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = pnp_ransac(world, image_d, c, samples=smp)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    ok = int((res["status"] == 0).sum().item())
    print(json.dumps({"tool": "gpu_pnp_rate", "frames": a.frames, "markers": len(world), "hypotheses": a.hypotheses,
                      "median_ms": ms, "problems_per_s": a.frames / ms * 1e3, "solved": ok,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
