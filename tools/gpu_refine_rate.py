"""Time of the grey-level refinement (k_refine.hip) on a resident recording, with `track_to_3d` on the same frames as the
yardstick: what refinement adds to a tracked frame.

For 4096 resident frames of 1280 x 1024 with 13 x 13 = 169 markers and of 1920 x 1200 with 21 x 21 = 441 markers, each with dots of
16 px (windows of R about 17) and of 39 px (R about 40): HIP-event time per call, after warm-up, median and minimum over `--reps`
calls, of `Engine.refine_markers` on a table that holds every marker at its rendered centre and diameter (every output; then
`sums` alone), and of `track_to_3d` on the same frames in the same run.  Reported per shape: microseconds per call and per
frame, nanoseconds per row that loads pixels, the count of every status, and the bytes of window the kernel reads a second - per
row that reaches the level pass the core and the ring, per row that reaches the sum pass also the disc, counted from the rows'
own geometry - against the HBM figure bench.py uses (the second pass is expected to hit the vector L1, so this is what the
kernel asks of the memory pipe, not HBM traffic).
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under its
own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out
FILE` also appends them there.

    python tools/gpu_refine_rate.py [--frames 4096] [--reps 10] [--limit 240] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # the figure bench.py divides by
# (width, height, dots a side, pitch, diameter)
SHAPES = ((1280, 1024, 13, 72, 16), (1280, 1024, 13, 72, 39), (1920, 1200, 21, 56, 16), (1920, 1200, 21, 56, 39))


def window_bytes(rec, table):
    """Bytes of window the kernel loads for these rows: core + ring for a row that reached the level pass (status 0, 5, 6, 7), the
    disc too for one that reached the sum pass (0, 6, 7); from each row's own R, c2, g2."""
    import numpy as np
    st = rec[..., 0].astype(np.int64).ravel()
    r = 0.5 * table[..., 3].astype(np.float64).ravel()
    lev = np.isin(st, (0, 5, 6, 7))
    R = np.ceil(2.0 * r[lev]).astype(np.int64) + 1
    c2, g2 = np.floor((0.5 * r[lev]) ** 2).astype(np.int64), np.floor((1.5 * r[lev]) ** 2).astype(np.int64)
    summed = np.isin(st[lev], (0, 6, 7))
    total = 0
    trip, inv = np.unique(np.stack([R, c2, g2], axis=1), axis=0, return_inverse=True)
    for k, (Rk, ck, gk) in enumerate(trip):
        d = np.arange(-Rk, Rk + 1)
        d2 = d[:, None] ** 2 + d[None, :] ** 2
        core, disc, ring = int((d2 <= ck).sum()), int((d2 <= gk).sum()), int(((d2 > gk) & (d2 <= Rk * Rk)).sum())
        rows = inv.ravel() == k
        total += int(rows.sum()) * (core + ring) + int((rows & summed).sum()) * disc
    return total


def one_shape(width, height, side, pitch, diameter, frames, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import synth as S
    from vbs_amd.engine import Engine
    assert torch.cuda.is_available(), "needs a GPU"
    spec = S.grid_spec(width, height, side, pitch, diameter)
    fr = S.make_frames_torch(spec, range(frames), seed=0)
    ref_xy = S.dot_truth(spec, 0, [0])[0, :, :2].copy()
    cam = L.make_camera(*S.default_camera(spec), 2.0)
    eng = Engine(height, width, max_markers=512, max_batch=64)

    def timed(fn, warm=2):
        for _ in range(warm):
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

    # the start: every marker tracked at its rendered centre and diameter (float32), so the windows are the shape's whatever the
    # detector makes of dots of this size in frames of this size; track_to_3d's own detections are counted beside it
    truth = S.dot_truth(spec, 0, range(frames))
    tab = np.zeros((frames, side * side, L.TABLE_COLS), dtype=np.float32)
    tab[..., 0], tab[..., 1:3], tab[..., 3], tab[..., 4] = 1.0, truth[..., :2], truth[..., 2], truth[..., 2]
    table = torch.from_numpy(tab).cuda()
    _, _, counts = eng.track_to_3d(fr, ref_xy, 20.0, cam, 5.0)
    assert int(counts.min()) >= 0
    rec, _, _ = eng.refine_markers(fr, table)
    rec_h, tab_h = rec.cpu().numpy(), table.cpu().numpy()
    status = np.bincount(rec_h[..., 0].astype(np.int64).ravel(), minlength=8).tolist()
    res = {"width": width, "height": height, "frames": frames, "slots": side * side, "diameter": diameter,
           "R_median": int(np.median(np.ceil(tab_h[..., 3][rec_h[..., 0] == 0]) + 1)) if status[0] else None,
           "device": torch.cuda.get_device_name(0), "reps": reps, "status_counts": status,
           "detections_per_frame_track_to_3d": float(counts.float().mean())}
    res["refine_all_outputs"] = timed(lambda: eng.refine_markers(fr, table))
    res["refine_sums_only"] = timed(lambda: eng.refine_markers(fr, table, want=("sums",)))
    res["track_to_3d"] = timed(lambda: eng.track_to_3d(fr, ref_xy, 20.0, cam, 5.0))
    us = res["refine_all_outputs"]["median_us"]
    nbytes = window_bytes(rec_h, tab_h)
    res["refine_us_per_frame"] = us / frames
    res["refine_ns_per_row_with_pixels"] = us * 1e3 / max(sum(status[k] for k in (0, 5, 6, 7)), 1)
    res["track_to_3d_us_per_frame"] = res["track_to_3d"]["median_us"] / frames
    res["refine_over_track_to_3d"] = us / res["track_to_3d"]["median_us"]
    res["window_bytes"] = nbytes
    res["window_GBps"] = nbytes / (us * 1e-6) / 1e9
    res["window_GBps_over_hbm_peak"] = res["window_GBps"] / HBM_PEAK_GBS
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape is not None:
        print(json.dumps(one_shape(*SHAPES[a.shape], a.frames, a.reps)), flush=True)
        return 0
    for k in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(k), "--frames", str(a.frames), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"shape {SHAPES[k]} ran out of its {a.limit} s: stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"shape {SHAPES[k]} failed ({r.returncode}): stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
