"""Time of the modal analysis (k_modes.hip) on a resident recording, with a library product and a library eigensolver as yardsticks.

For 4096 frames x 169 and x 441 markers x 3 axes (a press, a drag and a torsion with their own time courses, noise, 3 % of the
entries missing) and r = 6 and 16 modes: HIP-event time per call of `engine.cross_moments_f64`, `engine.covariance_f64`,
`engine.leading_modes_f64` (48 iterations) and `engine.mode_scores_f64`, after warm-up calls of every shape, median and minimum
over `--reps` calls, the record rotated over `--buffers` copies.  Beside them, on the same device:
  * float64 `torch.matmul` of the pre-selected, pre-centred columns [n, s x 4] (values of invalid entries set to 0, the mean taken
    off, the flag as 1.0 / 0.0 - prepared once, outside the timed region) against their transpose.  A YARDSTICK ONLY: its operand
    was selected for it, it computes both triangles, and its output is column-major over (slot, column).
  * `torch.linalg.eigh` of the same covariance: ALL C eigenpairs where the entry finds r - a different quantity.  It is reported,
    not a criterion.
Every shape runs in a child process under its own time limit (`--limit` seconds), so one slow shape cannot take the others with
it; a child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_modes_rate.py [--reps 20] [--buffers 2] [--limit 120] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = ((169, 6), (169, 16), (441, 6), (441, 16))


def recording(n, s, seed, drop=0.03):
    """-> rec float64 [n, s, 4] = flag, dX, dY, dZ on a square grid of s markers."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(round(s ** 0.5))
    g = np.arange(side, dtype=np.float64) - (side - 1) / 2
    gx, gy = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="xy"))
    f = np.arange(n, dtype=np.float64)
    rec = np.zeros((n, s, 4))
    rec[..., 0] = r.random((n, s)) >= drop
    press = -np.exp(-(gx ** 2 + gy ** 2) / (2 * (side / 5.0) ** 2))
    rec[..., 3] = 0.8 * np.sin(2 * np.pi * f / 970.0)[:, None] * press[None, :]
    rec[..., 1] = 0.2 * np.sin(2 * np.pi * f / 410.0)[:, None] - 0.01 * np.cos(2 * np.pi * f / 230.0)[:, None] * gy[None, :]
    rec[..., 2] = 0.01 * np.cos(2 * np.pi * f / 230.0)[:, None] * gx[None, :]
    rec[..., 1:] += r.normal(0.0, 0.002, (n, s, 3))
    rec[..., 1:][rec[..., 0] == 0.0] = np.nan
    return rec


def one_shape(s, r, reps, buffers):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import covariance_f64, cross_moments_f64, leading_modes_f64, mode_scores_f64
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    rec = recording(n, s, s)
    recs = [torch.from_numpy(rec).cuda() for _ in range(buffers)]
    valid = recs[0][..., :1] != 0
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    shift = torch.where(valid, recs[0][..., 1:], zero).sum(dim=0) / valid.sum(dim=0).clamp(min=1)

    def timed(fn, warm=3):
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

    res = {"frames": n, "slots": s, "modes": r, "iters": 48, "device": torch.cuda.get_device_name(0), "reps": reps, "buffers": buffers,
           "mom_chunk": L.MOM_CHUNK, "mom_wg_slots": L.MOM_WG_SLOTS, "multiply_adds_both_triangles": n * (4 * s) ** 2}
    res["cross_moments_f64"] = timed(lambda i: cross_moments_f64(recs[i % buffers], shift, 3))
    mom = cross_moments_f64(recs[0], shift, 3)
    res["covariance_f64"] = timed(lambda i: covariance_f64(mom, 3, "filled", 2, float(n - 1)))
    cov = covariance_f64(mom, 3, "filled", 2, float(n - 1))
    work = torch.empty((2 * 3 * s * L.MODES_MAX,), dtype=torch.float64, device="cuda")
    res["leading_modes_f64"] = timed(lambda i: leading_modes_f64(cov, r, 48, work=work))
    values, modes, resid, info = leading_modes_f64(cov, r, 48, work=work)
    center = shift.reshape(-1)
    res["mode_scores_f64"] = timed(lambda i: mode_scores_f64(recs[i % buffers], center, modes, 3))
    res["values"] = values[:4].cpu().numpy().tolist()
    res["largest_resid_over_value_1"] = float((resid / values[0]).max())
    res["info"] = info.cpu().numpy().tolist()
    # the yardsticks: the selected, centred operand [n, s * 4] is prepared once, outside the timed region
    sel = []
    for rc in recs:
        v = torch.where(rc[..., :1] != 0, rc[..., 1:4] - shift[None], zero)
        sel.append(torch.cat([v, (rc[..., :1] != 0).to(torch.float64)], dim=2).reshape(n, s * 4).contiguous())
    res["matmul_f64_yardstick"] = timed(lambda i: torch.matmul(sel[i % buffers].T, sel[i % buffers]))
    res["eigh_f64_yardstick"] = timed(lambda i: torch.linalg.eigh(cov), warm=1)
    us = res["cross_moments_f64"]["median_us"]
    res["tflops_f64_both_triangles"] = 2 * res["multiply_adds_both_triangles"] / us * 1e-6
    res["moments_rate_over_matmul_yardstick"] = res["matmul_f64_yardstick"]["median_us"] / us
    res["modes_time_over_eigh"] = res["leading_modes_f64"]["median_us"] / res["eigh_f64_yardstick"]["median_us"]
    ref = torch.matmul(sel[0].T, sel[0]).view(s, 4, s, 4).permute(0, 2, 1, 3)
    res["max_abs_difference_from_yardstick"] = float((mom - ref).abs().max())
    w = torch.linalg.eigh(cov)[0].flip(0)[:r]
    res["max_value_difference_from_eigh_over_value_1"] = float(((values - w).abs() / w[0]).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,modes of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        s, r = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(s, r, a.reps, a.buffers)), flush=True)
        return 0
    for s, r in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{s},{r}", "--reps", str(a.reps), "--buffers", str(a.buffers)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {s} modes {r}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"slots {s} modes {r}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
