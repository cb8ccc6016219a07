"""Time of the probe-indentation entries (k_steps.hip) on a resident sequence, with a dense torch restatement as a yardstick.

For 4096 frames x 169 and x 441 slots x 3 axes (the `axis` layout [n, m, 4]; 3 % of the entries missing; a staircase of a step
every 256 frames under noise) at w = 8 and w = 64: HIP-event time per call of `engine.step_response_f64`, `find_steps_f64` and
`dwell_stats_f64` (each series' own steps, guard = w), after warm-up calls of every shape, median and minimum over `--reps` calls,
the input rotated over `--buffers` copies so that a call does not find the previous call's rows in the caches by construction.
Beside it, on the same device, the response as differences of a float64 `cumsum` along time: A YARDSTICK ONLY - it has no gaps, no
populations, a running sum (another summation order, and it drifts) and several passes over the data.
Prints one JSON line per shape and window; `--out FILE` also appends them there.

    python tools/gpu_step_rate.py [--reps 30] [--buffers 4] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import dwell_stats_f64, find_steps_f64, step_response_f64
    assert torch.cuda.is_available(), "needs a GPU"

    def timed(fn, reps):
        for i in range(5):
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

    def cumsum_response(x, w):
        """x [n, s, 3] gap-free: mean of [f, f+w) minus mean of [f-w, f) for f in [w, n-w], from one running sum."""
        c = torch.cumsum(x, dim=0)
        c = torch.cat([torch.zeros_like(c[:1]), c], dim=0)   # c[k] = sum of x[:k]
        n = x.shape[0]
        right = c[2 * w:n + 1] - c[w:n + 1 - w]
        left = c[w:n + 1 - w] - c[0:n + 1 - 2 * w]
        r = (right - left) / w
        return (r * r).sum(dim=2)

    n = 4096
    for m in (169, 441):
        rng = np.random.default_rng(m)
        rec = np.zeros((n, m, 4))
        rec[..., 0] = rng.random((n, m)) >= 0.03
        rec[..., 1:] = (np.arange(n) // 256)[:, None, None] * 0.7 + rng.normal(0.0, 0.02, (n, m, 3))
        recs = [torch.from_numpy(rec).cuda() for _ in range(a.buffers)]
        dense = [r[..., 1:].contiguous() for r in recs]
        base = {"frames": n, "slots": m, "values": 3, "device": torch.cuda.get_device_name(0), "reps": a.reps, "buffers": a.buffers}
        for w in (8, 64):
            res = dict(base, window=w)
            resps = [step_response_f64(r, w, 3) for r in recs]
            steps = find_steps_f64(resps[0], w, 0.35)
            res["steps_found_per_series"] = float(steps[:, 0].double().mean())
            res["step_response_f64"] = timed(lambda i: step_response_f64(recs[i % a.buffers], w, 3), a.reps)
            res["find_steps_f64"] = timed(lambda i: find_steps_f64(resps[i % a.buffers], w, 0.35), a.reps)
            res["dwell_stats_f64"] = timed(lambda i: dwell_stats_f64(recs[i % a.buffers], steps, w, 3), a.reps)
            res["cumsum_f64_yardstick"] = timed(lambda i: cumsum_response(dense[i % a.buffers], w), a.reps)
            us = res["step_response_f64"]["median_us"]
            res["response_gadds_per_s"] = n * m * 3 * 2 * w / us * 1e-3
            res["response_input_gb_per_s"] = n * m * 4 * 8 / us * 1e-3
            res["max_steps"] = L.STEP_MAX_STEPS
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fo:
                    fo.write(line + "\n")


if __name__ == "__main__":
    main()
