"""Time of the gap-aware zero-phase FIR (k_filter.hip) on a resident sequence, with a dense convolution as a yardstick.

For 4096 frames x 169 and x 441 slots x 3 axes (the `axis` layout [n, m, 4]; 3 % of the entries missing) at K = 31 and K = 255:
HIP-event time per call of `engine.fir_series_f64` and of `Engine.axis_displacement`, after warm-up calls of every shape, median
and minimum over `--reps` calls, the input rotated over `--buffers` copies so that a call does not find the previous call's rows
in the caches by construction.  Beside it, on the same device, `torch.nn.functional.conv1d` in float64 over the same values laid
out [3 m, 1, n]: A YARDSTICK ONLY - it has no gaps, no normalisation and no residual, and its layout is the one it likes best.
Prints one JSON line per shape and filter length; `--out FILE` also appends them there.

    python tools/gpu_filter_rate.py [--reps 30] [--buffers 4] [--out FILE]
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
    from vbs_amd import filters as F
    from vbs_amd.engine import Engine, fir_series_f64
    assert torch.cuda.is_available(), "needs a GPU"
    eng = Engine(480, 640, max_markers=256, max_batch=2, device=0)

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

    n = 4096
    for m in (169, 441):
        rng = np.random.default_rng(m)
        table = np.zeros((n, m, 10), dtype=np.float32)
        table[..., 0] = np.where(rng.random((n, m)) >= 0.03, 3, 0)
        table[0, :, 0] = 3
        table[..., 6:9] = 20 * rng.standard_normal((n, m, 3))
        t = torch.from_numpy(table).cuda()
        axis, _ = eng.axis_displacement(t)
        recs = [axis.clone() for _ in range(a.buffers)]
        dense = [r[..., 1:].permute(1, 2, 0).reshape(3 * m, 1, n).contiguous() for r in recs]
        base = {"frames": n, "slots": m, "values": 3, "device": torch.cuda.get_device_name(0), "reps": a.reps, "buffers": a.buffers,
                "tile_frames": L.FIR_TILE}
        base["axis_displacement"] = timed(lambda i: eng.axis_displacement(t), a.reps)
        for k in (31, 255):
            taps = F.lowpass_taps(k, 2.5 / k)
            w = torch.from_numpy(taps).cuda().reshape(1, 1, k)
            res = dict(base, taps=k)
            res["fir_series_f64"] = timed(lambda i: fir_series_f64(recs[i % a.buffers], taps, 3), a.reps)
            res["conv1d_f64_yardstick"] = timed(lambda i: torch.nn.functional.conv1d(dense[i % a.buffers], w, padding=k // 2), a.reps)
            us = res["fir_series_f64"]["median_us"]
            res["gtaps_per_s"] = n * m * 3 * k / us * 1e-3
            res["input_gb_per_s"] = n * m * 4 * 8 / us * 1e-3
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fo:
                    fo.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
