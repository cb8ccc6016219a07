"""Time of the gap-aware rolling median / MAD with the Hampel rule (k_robust.hip) on a resident sequence, with a dense sort as a
yardstick.

For 4096 frames x 169 and x 441 slots x 3 values (a record [n, m, 4]) at half windows h = 3, 7 and 31, without gaps and with 3 %
of the entries missing, with the clean record and without (`want_clean=False`): HIP-event time per call of
`engine.hampel_series_f64`, after warm-up calls of every shape, median and minimum over `--reps` calls, the input rotated over
`--buffers` copies so that a call does not find the previous call's rows in the caches by construction.  Beside it, on the same
device, float64 `tensor.unfold(0, 2h + 1, 1)` + `torch.sort` along the window + the middle element over the same values: A
YARDSTICK ONLY - it has no gaps, no MAD, no flags and no ends (n - 2h outputs).  Every shape is warmed up before any is timed.
Prints one JSON line per shape, half window and gap rate; `--out FILE` also appends them there.

    python tools/gpu_robust_rate.py [--reps 20] [--buffers 4] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import hampel_series_f64
    assert torch.cuda.is_available(), "needs a GPU"

    def timed(fn, reps):
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

    def yardstick(x, h):
        return x.unfold(0, 2 * h + 1, 1).sort(dim=-1).values[..., h]

    n, halves = 4096, (3, 7, 31)
    cases = []
    for m in (169, 441):
        for gaps in (0.0, 0.03):
            rng = np.random.default_rng(m)
            rec = np.empty((n, m, 4))
            rec[..., 0] = rng.random((n, m)) >= gaps
            rec[..., 1:] = 20 * rng.standard_normal((n, m, 3))
            recs = [torch.from_numpy(rec).cuda() for _ in range(a.buffers)]
            dense = [r[..., 1:].contiguous() for r in recs]
            cases.append((m, gaps, recs, dense))
    for m, gaps, recs, dense in cases:                           # the warm-up of every shape, before anything is timed
        for h in halves:
            for clean in (True, False):
                hampel_series_f64(recs[0], h, min_scale=0.1, want_clean=clean)
            if gaps == 0.0:
                yardstick(dense[0], h)
    torch.cuda.synchronize()
    for m, gaps, recs, dense in cases:
        for h in halves:
            res = {"frames": n, "slots": m, "values": 3, "half_window": h, "gaps": gaps, "device": torch.cuda.get_device_name(0),
                   "reps": a.reps, "buffers": a.buffers, "tile_frames": L.ROBUST_TILE}
            res["hampel_series_f64"] = timed(lambda i: hampel_series_f64(recs[i % a.buffers], h, min_scale=0.1), a.reps)
            res["hampel_series_f64_no_clean"] = timed(
                lambda i: hampel_series_f64(recs[i % a.buffers], h, min_scale=0.1, want_clean=False), a.reps)
            if gaps == 0.0:
                res["unfold_sort_f64_yardstick"] = timed(lambda i: yardstick(dense[i % a.buffers], h), a.reps)
            res["mwindows_per_s"] = n * m * 3 / res["hampel_series_f64"]["median_us"]
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fo:
                    fo.write(line + "\n")


if __name__ == "__main__":
    main()
