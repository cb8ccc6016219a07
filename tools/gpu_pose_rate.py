"""Time of the pose-misalignment series (k_pose.hip) on a resident recording, with the code it replaces as yardsticks.

For 4096 frames x 169 and x 441 markers (a tilt ramp 0 -> 6 degrees under noise, 3 % of the entries missing) and reject_k = 0
and 3: HIP-event time per call of `Engine.pose_series` (all three outputs), after warm-up calls of every shape, median and minimum
over `--reps` calls, the table rotated over `--buffers` copies so that a call does not find the previous call's rows in the
caches by construction.  Beside it, on the same device and the same end points:
  * `Engine.deviation_plane` called once per frame (4096 calls of the one-wave float32 kernel, one HIP-event pair around all of
    them, `--plane-reps` times): what the series replaces;
  * a batched float64 `torch.linalg.lstsq` on [x, y, 1] over the end points of every frame (dropouts filled with the reference
    position, which a plane fit cannot do: A YARDSTICK ONLY - no flags, no counts, no field, no rejection, another algorithm).
    The solver took 78 s for the 4096 x 169 x 3 batch on an MI355X (19 ms a matrix, measured once), so the yardstick is taken
    on the first `--lstsq-frames` frames, `--lstsq-reps` times after one warm-up call, and reported per frame.
Bytes: what the algorithm must move once - the table's frames, the shared rows, and the three outputs - over the median time.
Prints one JSON line per shape and reject_k; `--out FILE` also appends them there.

    python tools/gpu_pose_rate.py [--reps 30] [--buffers 4] [--plane-reps 3] [--lstsq-frames 256] [--lstsq-reps 2] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--plane-reps", type=int, default=3)
    ap.add_argument("--lstsq-frames", type=int, default=256)
    ap.add_argument("--lstsq-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import pose_oracle as O                                   # (the recording's generator only)
    from vbs_amd import _lib as L
    from vbs_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a GPU"
    eng = Engine(480, 640, max_markers=256, max_batch=2)

    def timed(fn, reps, warm=5):
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

    n = 4096
    for m in (169, 441):
        ref = O.grid_ref(m)
        t = O.tilted_table(ref, np.linspace(0.0, 6.0, n), 30.0, m, 0.02, 0.03)
        tabs = [torch.from_numpy(t).cuda() for _ in range(a.buffers)]
        rd = torch.zeros((m, 4), dtype=torch.float64, device="cuda")
        rd[:, 0] = 1.0
        rx = torch.from_numpy(ref).cuda()
        ref32 = ref.astype(np.float32)
        base = {"frames": n, "slots": m, "device": torch.cuda.get_device_name(0), "reps": a.reps, "buffers": a.buffers,
                "pose_group": L.POSE_GROUP}
        runs = []
        for k in (0.0, 3.0):                                  # the entry itself first: its lines do not wait for the yardsticks
            res = dict(base, reject_k=k)
            flags = eng.pose_series(tabs[0], rd, rx, reject_k=k)[2][:, 0]
            res["frames_refitted"] = int((flags == 2).sum())
            res["pose_series"] = timed(lambda i: eng.pose_series(tabs[i % a.buffers], rd, rx, reject_k=k), a.reps)
            print(f"m {m} reject_k {k}: pose_series {res['pose_series']}", file=sys.stderr, flush=True)
            runs.append(res)
        # the yardsticks, once per shape
        zero_row = torch.zeros((m, L.TABLE_COLS), dtype=torch.float32, device="cuda")
        zero_row[:, 0] = 3.0

        def per_frame(i):
            tab = tabs[i % a.buffers]
            for f in range(n):
                eng.deviation_plane(zero_row, zero_row, tab[0], tab[f], ref32)
        plane = timed(per_frame, a.plane_reps, warm=1)
        print(f"m {m}: {n} deviation_plane calls {plane}", file=sys.stderr, flush=True)
        dev0 = eng.pose_series(tabs[0], rd, rx)[0]
        pts = torch.stack([rx[:, 0] + dev0[..., 1], rx[:, 1] + dev0[..., 2], dev0[..., 3]], dim=2)      # 'plane' mode, scale 1
        A = torch.stack([pts[..., 0], pts[..., 1], torch.ones_like(pts[..., 0])], dim=2).contiguous()
        z = pts[..., 2:3].contiguous()
        nl = min(n, a.lstsq_frames)                           # (the first frames of the ramp: the solver's time does not depend on values)
        lstsq = dict(timed(lambda i: torch.linalg.lstsq(A[:nl], z[:nl]), a.lstsq_reps, warm=1), frames=nl, reps=a.lstsq_reps)
        lstsq["us_per_frame"] = lstsq["median_us"] / nl
        print(f"m {m}: lstsq {lstsq}", file=sys.stderr, flush=True)
        for res in runs:
            res["deviation_plane_per_frame_yardstick"] = plane
            res["lstsq_f64_yardstick"] = lstsq
            us = res["pose_series"]["median_us"]
            moved = n * m * (L.TABLE_COLS * 4 + 4 * 8) + m * (L.TABLE_COLS * 4 + 7 * 8) + n * (L.POSE_COLS + L.POSEFIELD_COLS) * 8
            res["bytes_moved_once"] = moved
            res["gb_per_s_of_bytes_moved_once"] = moved / us * 1e-3
            res["frames_per_s"] = n / us * 1e6
            res["speedup_over_per_frame_calls"] = plane["median_us"] / us
            res["us_per_frame"] = us / n
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fo:
                    fo.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
