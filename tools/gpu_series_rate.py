"""Time of the time-axis reductions (k_series.hip) on a resident sequence, beside the host way to the same numbers.

For 4096 x 169 and 1536 x 441 (frames x slots; 3 % of the entries missing): HIP-event time per call of `series_stats` (with and
without the cumulative series), `window_means` (the reference's two windows) and `displacement_from_frame`, after warm-up
calls of every shape, median and minimum over `--reps` calls; per-kernel microseconds from `vbs_profile` in a separate loop
(the event pairs would otherwise sit inside the timed window); and, in the same run on the same rows, what the package did
before: disp -> host -> DataFrame -> `MarkerAnalysis.analyze_displacement` (wall clock, split into copy, DataFrame and
pandas).  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_series_rate.py [--reps 50] [--host-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import Engine
    from vbs_amd.reconstruction3d import Config, MarkerAnalysis
    assert torch.cuda.is_available(), "needs a GPU"
    eng = Engine(480, 640, max_markers=256, max_batch=2, device=0)
    td = tempfile.mkdtemp()
    ma = MarkerAnalysis(Config(data_dir=os.path.join(td, "d"), output_dir=os.path.join(td, "o"), plots_dir=os.path.join(td, "p")))

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts))}

    for n, m in ((4096, 169), (1536, 441)):
        rng = np.random.default_rng(n + m)
        flag = rng.random((n, m)) >= 0.03
        disp = np.zeros((n, m, 5), dtype=np.float32)
        disp[..., 0] = flag
        disp[..., 4] = np.where(flag, np.abs(0.05 + 0.02 * rng.standard_normal((n, m))), 0)
        table = np.zeros((n, m, 10), dtype=np.float32)
        table[..., 0] = np.where(flag, 3, 0)
        table[..., 6:9] = 20 * rng.standard_normal((n, m, 3))
        d, t = torch.from_numpy(disp).cuda(), torch.from_numpy(table).cuda()
        ids = np.stack([np.arange(m) // 24, np.arange(m) % 24], axis=1)
        res = {"frames": n, "slots": m, "rows": int(flag.sum()), "device": torch.cuda.get_device_name(0), "reps": a.reps,
               "chunk": L.SERIES_CHUNK}
        res["series_stats"] = timed(lambda: eng.series_stats(d), a.reps)
        res["series_stats_cumulative"] = timed(lambda: eng.series_stats(d, cumulative=True), a.reps)
        res["window_means_2"] = timed(lambda: eng.window_means(t, [(1, 30), (120, 150)]), a.reps)
        res["displacement_from_frame"] = timed(lambda: eng.displacement_from_frame(t, 0), a.reps)
        eng.profile(True)
        for _ in range(a.reps):
            eng.series_stats(d, cumulative=True)
            eng.window_means(t, [(1, 30), (120, 150)])
            eng.displacement_from_frame(t, 0)
        res["kernel_us"] = {k: round(ms * 1e3 / c, 2) for k, (c, ms) in eng.profile_read().items()}
        eng.profile(False)
        # the host way, on the same rows: device -> host -> DataFrame -> the existing analyze_displacement
        host = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = d.cpu().numpy()
            t1 = time.perf_counter()
            f, s = np.nonzero(h[..., 0] != 0)
            df = pd.DataFrame({"frameno": f, "row": ids[s, 0], "col": ids[s, 1], "displacement": h[f, s, 4].astype(np.float64)})
            t2 = time.perf_counter()
            ma.analyze_displacement(df)
            t3 = time.perf_counter()
            host.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
        best = min(host)
        res["host_path_ms"] = {"total": best[0] * 1e3, "copy": best[1] * 1e3, "dataframe": best[2] * 1e3,
                               "analyze_displacement": best[3] * 1e3}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
