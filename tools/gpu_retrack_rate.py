"""Time of the re-tracker (k_retrack.hip) on a resident recording of detections, with the per-frame rule it replaces and the
host loop as yardsticks.

For 4096 frames x 169 and x 441 markers (a lattice of pitch 40 px dragged by 45 px and turned by 8 degrees over the first half,
0.05 px of noise, 3 % of the detections after frame 0 removed, the order permuted in every frame) at gate 10 and gate 100:
HIP-event time per call, after warm-up, median and minimum over `--reps` calls, of
  whole          `engine.retrack` with every output
  bin            the cell grids alone (k_retrack_bin; the debug library's VBS_RETRACK_STOP=1, parallel over frames)
  walk           = the call that returns `assign` alone - bin: ONE workgroup by construction, frame after frame
  rows           = the grids and the table rows without the walk (VBS_RETRACK_STOP=2) - bin (k_retrack_rows, parallel over
                   frames and slots)
and beside them `Engine.track` on the same detections (the per-frame rule, parallel over frames) and, on `--oracle-frames` frames
only, the loop of tests/helpers/retrack_oracle.py on the host.  The number to read is the walk's microseconds per frame: it does not
fall with more compute units, only with fewer barriers and shorter candidate scans per round.
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under its
own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out
FILE` also appends them there.

    python tools/gpu_retrack_rate.py [--reps 10] [--limit 120] [--oracle-frames 64] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

FRAMES = 4096
SHAPES = tuple((side, gate) for side in (13, 21) for gate in (10.0, 100.0))


def recording(n, side, seed, pitch=40.0, drag=45.0, torsion_deg=8.0, noise=0.05, drop=0.03):
    """-> det float64 [n, m, 6], counts int32 [n], ref_xy [m, 2] for a side x side lattice."""
    import numpy as np
    r = np.random.default_rng(seed)
    k = np.arange(side * side)
    ref0 = np.stack([200.0 + pitch * (k % side), 200.0 + pitch * (k // side)], axis=1)
    c = ref0.mean(axis=0)
    m = ref0.shape[0]
    det = np.zeros((n, m, 6))
    counts = np.zeros(n, dtype=np.int32)
    ref = None
    for f in range(n):
        s = min(f, n // 2) / float(n // 2)
        a = np.deg2rad(torsion_deg) * s
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        p = (ref0 - c) @ R.T + c + np.array([drag * s, 0.0]) + r.normal(0.0, noise, (m, 2))
        ids = np.nonzero(np.ones(m, dtype=bool) if f == 0 else r.random(m) >= drop)[0]
        ids = ids[r.permutation(ids.size)]
        counts[f] = ids.size
        det[f, :ids.size, 0:2] = p[ids]
        det[f, :ids.size, 2:5] = (12.0, 11.0, 30.0)
        if f == 0:
            ref = p.copy()
    return det, counts, ref


def one_shape(side, gate, reps, oracle_frames):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    L.LIB_PATH = L.LIB_PATH.replace("libvbs.so", "libvbs_dbg.so")            # the same code, plus the knob that stops after the grid
    from vbs_amd.engine import Engine, retrack
    import retrack_oracle as O
    assert torch.cuda.is_available(), "needs a GPU"
    n, m = FRAMES, side * side
    det, counts, ref = recording(n, side, side)
    d, c, rf = torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(ref).cuda()

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

    res = {"frames": n, "slots": m, "max_det": m, "gate": gate, "device": torch.cuda.get_device_name(0), "reps": reps}
    out = retrack(d, c, rf, gate=gate)
    info = out["info"].cpu().numpy()
    res["matched"], res["with_candidate"], res["contested"] = (int(info[:, k].sum()) for k in (1, 2, 3))
    res["whole"] = timed(lambda: retrack(d, c, rf, gate=gate))
    assign_only = timed(lambda: retrack(d, c, rf, gate=gate, want=("assign",)))
    os.environ["VBS_RETRACK_STOP"] = "1"
    res["bin"] = timed(lambda: retrack(d, c, rf, gate=gate, want=("assign",)))
    os.environ["VBS_RETRACK_STOP"] = "2"                 # (the rows of an `assign` nobody wrote: no index is followed outside det)
    bin_and_rows = timed(lambda: retrack(d, c, rf, gate=gate, want=("assign", "table")))
    del os.environ["VBS_RETRACK_STOP"]
    res["walk"] = {k: assign_only[k] - res["bin"][k] for k in assign_only}
    res["rows"] = {k: bin_and_rows[k] - res["bin"][k] for k in assign_only}
    res["walk_us_per_frame"] = res["walk"]["median_us"] / n
    eng = Engine(480, 640, max_markers=m, max_batch=2)
    res["per_frame_rule_track"] = timed(lambda: eng.track(d, c, rf, 20.0))
    t0 = time.perf_counter()
    want = O.retrack(det[:oracle_frames], counts[:oracle_frames], ref, gate=gate)
    res["oracle_host_us_per_frame"] = (time.perf_counter() - t0) * 1e6 / oracle_frames
    res["equal_to_oracle_on_those_frames"] = bool(np.array_equal(out["assign"][:oracle_frames].cpu().numpy(), want["assign"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--oracle-frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape is not None:
        side, gate = SHAPES[a.shape]
        print(json.dumps(one_shape(side, gate, a.reps, a.oracle_frames)), flush=True)
        return 0
    for k in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(k), "--reps", str(a.reps), "--oracle-frames", str(a.oracle_frames)]
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
