#!/usr/bin/env python3
"""Rate of Engine.measure_markers (marker diameter validation) on batches of synthetic validation shots.

    python tools/gpu_diameter_rate.py [--frames 64] [--reps 20] [--warmup 3]

HIP events around the whole call, median over `reps` after `warmup`; then one profiled call (vbs_profile) for the per-kernel
times.  Prints one JSON line per geometry (640x480 and 1280x1024).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vbs_amd.engine import Engine                             # noqa: E402


def shot(H, W, seed, pitch=56):
    """Dark discs of 15-40 px on a bright noisy background, one per grid cell."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.full((H, W), 200.0, np.float32)
    for gy in range(pitch // 2, H - pitch // 2, pitch):
        for gx in range(pitch // 2, W - pitch // 2, pitch):
            cx, cy, r = gx + rng.uniform(-4, 4), gy + rng.uniform(-4, 4), rng.uniform(7.5, 20.0)
            y0, y1, x0, x1 = int(cy - r - 2), int(cy + r + 3), int(cx - r - 2), int(cx + r + 3)
            d = np.hypot(xx[y0:y1, x0:x1] - cx, yy[y0:y1, x0:x1] - cy) - r
            cov = np.clip(0.5 - d / 0.8, 0, 1)
            img[y0:y1, x0:x1] = img[y0:y1, x0:x1] * (1 - cov) + 40.0 * cov
    img += rng.normal(0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for H, W in ((480, 640), (1024, 1280)):
        base = [shot(H, W, s) for s in range(4)]
        frames = torch.from_numpy(np.stack([base[i % 4] for i in range(a.frames)])).cuda()
        eng = Engine(H, W, max_markers=512, max_batch=a.frames)
        for _ in range(a.warmup):
            rec, counts, stats = eng.measure_markers(frames, 120, 20.0)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rec, counts, stats = eng.measure_markers(frames, 120, 20.0)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        eng.profile(True)
        eng.measure_markers(frames, 120, 20.0)
        kern = eng.profile_read()
        eng.profile(False)
        med = float(np.median(ms))
        print(json.dumps({"tool": "gpu_diameter_rate", "height": H, "width": W, "frames": a.frames, "reps": a.reps,
                          "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                          "frames_per_s": round(a.frames / med * 1e3, 1), "markers_per_frame": float(counts.float().mean()),
                          "mean_diameter_mm": float(stats[0, 1]), "kernels": kern}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
