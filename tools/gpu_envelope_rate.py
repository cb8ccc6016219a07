"""Time of the time-resolved fit (k_envelope.hip) on a resident recording, with the closest composition of older entries and a
library convolution as yardsticks.

For 4096 frames x 169 and x 441 markers x 3 axes (every marker oscillating at a spindle line with a burst envelope, 3 % of the
entries missing) and Hann windows of half width h = 16, 64 and 127: HIP-event time per call of `engine.window_moments_f64` and of
`engine.window_fit_f64` on its result, after warm-up calls of every shape, median and minimum over `--reps` calls, the record
rotated over `--buffers` copies.  Beside them, on the same device:
  * YARDSTICK 1, the closest composition without k_envelope.hip: the modulated columns (x, x c, x s, x x per axis, and the carrier
    c, s, c2, s2 alone: 16 columns) built in torch OUTSIDE the timed region, then `engine.fir_series_f64` on them - three calls of
    7, 7 and 2 values, timed together.  It returns num / den, not the sums, and still lacks W and the fit.
  * YARDSTICK 2: float64 `torch.nn.functional.conv1d` of the same window over the 17 SELECTED columns of every marker (invalid
    entries set to 0, prepared once, outside the timed region).
The kernel multiplies a band inside 16-frame tiles: of the (2h + 16) input frames a tile row meets, 2h + 1 lie inside its window;
`toeplitz_share` = (2h + 1) / (2h + 16) is the useful part of its matrix work.
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under
its own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape;
`--out FILE` also appends them there.

    python tools/gpu_envelope_rate.py [--reps 20] [--buffers 2] [--limit 120] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
NU0 = 0.0837
SHAPES = ((169, 16), (169, 64), (169, 127), (441, 16), (441, 64), (441, 127))


def recording(n, s, seed, drop=0.03):
    """-> rec float64 [n, s, 4] = flag, dX, dY, dZ."""
    import numpy as np
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    phi = r.uniform(-np.pi, np.pi, s)
    z = (f - 0.45 * n) / (0.04 * n)
    env = 0.02 + 0.13 * 0.5 * (1.0 + np.tanh(z)) + 0.4 * np.exp(-0.5 * z * z)
    rec = np.zeros((n, s, 4))
    rec[..., 0] = r.random((n, s)) >= drop
    rec[..., 3] = env[:, None] * np.cos(2 * np.pi * NU0 * f[:, None] - phi[None, :])
    rec[..., 1:3] = r.normal(0.0, 0.01, (n, s, 2))
    rec[..., 1:][rec[..., 0] == 0.0] = np.nan
    return rec


def one_shape(s, h, reps, buffers):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import spectra
    from vbs_amd.engine import fir_series_f64, taps_sum, window_fit_f64, window_moments_f64
    from vbs_amd.filters import half_taps
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    rec = recording(n, s, s)
    w = spectra.window_taps(h)
    sw = taps_sum(half_taps(w))
    car = torch.from_numpy(spectra.carrier(n, NU0)).cuda()
    recs = [torch.from_numpy(rec).cuda() for _ in range(buffers)]

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

    K = 2 * h + 1
    res = {"frames": n, "slots": s, "half_window": h, "taps": K, "device": torch.cuda.get_device_name(0), "reps": reps,
           "buffers": buffers, "env_tile": L.ENV_TILE, "sums": 17, "useful_multiply_adds": n * s * 17 * K,
           "toeplitz_share": K / (2 * h + 16)}
    res["window_moments_f64"] = timed(lambda i: window_moments_f64(recs[i % buffers], car, w, 3))
    mom = window_moments_f64(recs[0], car, w, 3)
    res["window_fit_f64"] = timed(lambda i: window_fit_f64(mom, sw))
    fit = window_fit_f64(mom, sw)
    res["ok_windows"] = float((fit[..., 0] != 0).double().mean())
    # yardstick 1: the modulated columns, built outside the timed region, through the FIR in three calls of 7, 7 and 2 values
    mods = []
    for r in recs:
        x = r[..., 1:4]
        c, sn = car[0][:, None, None], car[1][:, None, None]
        cols = torch.cat([x, x * c, x * sn, x * x, car.t()[:, None, :].expand(n, s, 4)], dim=2)          # [n, s, 16]
        flag = r[..., :1]
        mods.append([torch.cat([flag, cols[..., a:b]], dim=2).contiguous() for a, b in ((0, 7), (7, 14), (14, 16))])

    def composed(i):
        return [fir_series_f64(m, w, m.shape[2] - 1) for m in mods[i % buffers]]
    res["fir_composition_yardstick"] = timed(composed)
    # yardstick 2: a library convolution over the selected columns
    sel = []
    for r, m in zip(recs, mods):
        ok = r[..., :1] != 0
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        cols = torch.cat([ok.to(torch.float64)] + [torch.where(ok, q[..., 1:], zero) for q in m], dim=2)    # [n, s, 17]
        sel.append(cols.reshape(n, s * 17).t().contiguous()[:, None, :])                                    # [s * 17, 1, n]
    wk = torch.from_numpy(np.ascontiguousarray(w)).cuda()[None, None, :]
    res["conv1d_f64_yardstick"] = timed(lambda i: torch.nn.functional.conv1d(sel[i % buffers], wk, padding=h))
    us = res["window_moments_f64"]["median_us"]
    res["useful_tflops_f64"] = 2 * res["useful_multiply_adds"] / us * 1e-6
    res["speedup_over_fir_composition"] = res["fir_composition_yardstick"]["median_us"] / us
    res["speedup_over_conv1d"] = res["conv1d_f64_yardstick"]["median_us"] / us
    ref = torch.nn.functional.conv1d(sel[0], wk, padding=h)[:, 0, :].t().reshape(n, s, 17)
    order = [0, 13, 14, 15, 16] + [1 + v + 3 * k for v in range(3) for k in range(4)]      # W, c, s, c2, s2, then x, xc, xs, xx per axis
    res["max_abs_difference_from_conv1d"] = float((mom - ref[..., order]).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,half_window of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        s, h = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(s, h, a.reps, a.buffers)), flush=True)
        return 0
    for s, h in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{s},{h}", "--reps", str(a.reps), "--buffers", str(a.buffers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {s} h {h}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {s} h {h}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
