"""Time of the local polynomial fit along time (k_kinematics.hip) on a resident recording, with a library convolution and a
batched solve as the yardstick.

For 4096 frames x 169 and x 441 markers x 3 axes (a smooth press plus noise, 3 % of the entries missing), Hann windows of half
width h = 7, 31 and 127 and degrees d = 2 and 3: HIP-event time per call of `engine.poly_moments_f64` and of `engine.poly_fit_f64`
(with the filled record) on its result, after warm-up calls of every shape, median and minimum over `--reps` calls, the record
rotated over `--buffers` copies.  Beside them, on the same device, the YARDSTICK: float64 `torch.nn.functional.conv1d` of the same
tap rows over the SELECTED columns of every marker (rows 0 .. d over valid, x, y, z; rows d + 1 .. 2d over valid; row 0 over the
squares; invalid entries set to 0, prepared once, outside the timed region), then a batched `torch.linalg.solve_ex` of the Hankel
normal equations - no flags, no thresholds, no fallback in degree, no filled record.
The kernel multiplies bands inside 16-frame tiles: of the (2h + 16) input frames a tile row meets, 2h + 1 lie inside its window;
`toeplitz_share` = (2h + 1) / (2h + 16) is the useful part of its matrix work.
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under
its own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape;
`--out FILE` also appends them there.

    python tools/gpu_kinematics_rate.py [--reps 20] [--buffers 2] [--limit 120] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = tuple((s, h, d) for s in (169, 441) for h in (7, 31, 127) for d in (2, 3))


def recording(n, s, seed, drop=0.03):
    """-> rec float64 [n, s, 4] = flag, dX, dY, dZ."""
    import numpy as np
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    z = np.clip((f - 0.3 * n) / (0.25 * n), 0.0, 1.0)
    press = 0.8 * 0.5 * (1.0 - np.cos(np.pi * z))
    gain = r.uniform(0.5, 1.0, s)
    rec = np.zeros((n, s, 4))
    rec[..., 0] = r.random((n, s)) >= drop
    rec[..., 3] = -gain[None, :] * press[:, None]
    rec[..., 1] = 0.25 * gain[None, :] * press[:, None]
    rec[..., 1:] += r.normal(0.0, 0.002, (n, s, 3))
    rec[..., 1:][rec[..., 0] == 0.0] = np.nan
    return rec


def one_shape(s, h, d, reps, buffers):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import n_kin_sums, poly_fit_f64, poly_moments_f64
    from vbs_amd.filters import poly_taps
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    rec = recording(n, s, s)
    recs = [torch.from_numpy(rec).cuda() for _ in range(buffers)]
    taps, _, _ = poly_taps(h, d)

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

    K, M = 2 * h + 1, n_kin_sums(d, 3)
    res = {"frames": n, "slots": s, "half_window": h, "degree": d, "taps": K, "device": torch.cuda.get_device_name(0), "reps": reps,
           "buffers": buffers, "kin_tile": L.KIN_TILE, "sums": M, "useful_multiply_adds": n * s * M * K,
           "toeplitz_share": K / (2 * h + 16)}
    res["poly_moments_f64"] = timed(lambda i: poly_moments_f64(recs[i % buffers], h, d, "hann", 3))
    mom = poly_moments_f64(recs[0], h, d, "hann", 3)
    res["poly_fit_f64"] = timed(lambda i: poly_fit_f64(mom, recs[0], h, d, "hann", 3, want_filled=True))
    fit = poly_fit_f64(mom, recs[0], h, d, "hann", 3)
    res["full_degree_windows"] = float((fit[..., 1] == d).double().mean())
    # the yardstick: a library convolution of the tap rows over the selected columns, then a batched solve
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    sel = []
    for r in recs:
        ok = r[..., :1] != 0
        x = torch.where(ok, r[..., 1:4], zero)
        a = torch.cat([ok.to(torch.float64), x], dim=2).reshape(n, s * 4).t().contiguous()[:, None, :]       # [s * 4, 1, n]
        fl = ok.to(torch.float64).reshape(n, s).t().contiguous()[:, None, :]                                # [s, 1, n]
        sq = (x * x).reshape(n, s * 3).t().contiguous()[:, None, :]                                         # [s * 3, 1, n]
        sel.append((a, fl, sq))
    wt = torch.from_numpy(np.ascontiguousarray(taps)).cuda()[:, None, :]                                    # [2d + 1, 1, K]
    conv = torch.nn.functional.conv1d
    idx = torch.arange(d + 1, device="cuda")
    hank = idx[:, None] + idx[None, :]

    def yard(i):
        a, fl, sq = sel[i % buffers]
        low = conv(a, wt[:d + 1], padding=h).reshape(s, 4, d + 1, n)                                        # S_k, X_k, k <= d
        high = conv(fl, wt[d + 1:], padding=h)                                                              # S_k, k > d: [s, d, n]
        xx = conv(sq, wt[:1], padding=h)
        S = torch.cat([low[:, 0], high], dim=1).permute(2, 0, 1)                                            # [n, s, 2d + 1]
        G = S[..., hank]                                                                                    # [n, s, d + 1, d + 1]
        X = low[:, 1:].permute(3, 0, 2, 1)                                                                  # [n, s, d + 1, 3]
        c = torch.linalg.solve_ex(G, X)[0]
        return S, X, xx, c
    res["conv1d_solve_f64_yardstick"] = timed(yard, warm=1)
    us = res["poly_moments_f64"]["median_us"] + res["poly_fit_f64"]["median_us"]
    res["useful_tflops_f64"] = 2 * res["useful_multiply_adds"] / res["poly_moments_f64"]["median_us"] * 1e-6
    res["speedup_over_conv1d_solve"] = res["conv1d_solve_f64_yardstick"]["median_us"] / us
    S, X, xx, c = yard(0)
    res["max_abs_difference_of_S_from_conv1d"] = float((mom[..., :2 * d + 1] - S).abs().max())
    full = fit[..., 1] == d
    res["max_abs_difference_of_y0_from_solve"] = float((fit[..., 2::d + 2][..., :3] - c[..., 0, :])[full].abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,half_window,degree of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        s, h, d = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(s, h, d, a.reps, a.buffers)), flush=True)
        return 0
    for s, h, d in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{s},{h},{d}", "--reps", str(a.reps), "--buffers", str(a.buffers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {s} h {h} d {d}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {s} h {h} d {d}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
