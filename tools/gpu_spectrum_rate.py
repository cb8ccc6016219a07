"""Time of the displacement spectra (k_spectrum.hip) on a resident recording, with a library product and an FFT as yardsticks.

For 4096 frames x 169 and x 441 markers x 3 axes (every marker oscillating at a spindle line with its own phase, a slow trend, 3 %
of the entries missing) and zoom grids of Q = 32 and 256 frequencies round the line (R = 1 + 4 Q basis rows): HIP-event time per
call of `engine.project_series_f64` and of `engine.harmonic_fit_f64` on its result, after warm-up calls of every shape, median and
minimum over `--reps` calls, the record rotated over `--buffers` copies.  Beside them, on the same device:
  * float64 `torch.matmul` of the same basis [R, n] against the same SELECTED columns [n, s x 4] (values of invalid entries set to
    0, the flag as 1.0 / 0.0 - prepared once, outside the timed region).  A YARDSTICK ONLY: its operand was selected for it, and
    its output is basis-row-major.
  * `torch.fft.rfft` along time of the zero-filled series and of the mask [n, s x 4]: the same sums on the NATURAL grid q / n only,
    all n / 2 + 1 of them - a different quantity (no zoom, no arbitrary frequencies).  It shows where the crossover to the FFT
    lies as Q grows; it is reported, not a criterion.
Every shape runs in a child process under its own time limit (`--limit` seconds), so one slow shape cannot take the others with
it; a child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_spectrum_rate.py [--reps 20] [--buffers 2] [--limit 120] [--out FILE]
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
SHAPES = ((169, 32), (169, 256), (441, 32), (441, 256))


def recording(n, s, seed, drop=0.03):
    """-> rec float64 [n, s, 4] = flag, dX, dY, dZ."""
    import numpy as np
    r = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.float64)
    phi = r.uniform(-np.pi, np.pi, s)
    rec = np.zeros((n, s, 4))
    rec[..., 0] = r.random((n, s)) >= drop
    rec[..., 3] = 0.7 * np.cos(2 * np.pi * NU0 * f[:, None] - phi[None, :]) + 0.2 * (f / n)[:, None]
    rec[..., 1:3] = r.normal(0.0, 0.01, (n, s, 2))
    rec[..., 1:][rec[..., 0] == 0.0] = np.nan
    return rec


def one_shape(s, Q, reps, buffers):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import spectra
    from vbs_amd.engine import harmonic_fit_f64, project_series_f64
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    rec = recording(n, s, s)
    nu = spectra.zoom_grid(NU0, 4.0 / n, Q)
    basis = torch.from_numpy(spectra.harmonic_basis(n, nu)).cuda()
    R = basis.shape[0]
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

    res = {"frames": n, "slots": s, "Q": Q, "basis_rows": R, "device": torch.cuda.get_device_name(0), "reps": reps, "buffers": buffers,
           "proj_chunk": L.PROJ_CHUNK, "proj_rows": L.PROJ_ROWS, "proj_wg_slots": L.PROJ_WG_SLOTS, "fit_group": L.FIT_GROUP,
           "multiply_adds": R * n * s * 4}
    res["project_series_f64"] = timed(lambda i: project_series_f64(recs[i % buffers], basis, 3))
    pj = project_series_f64(recs[0], basis, 3)
    res["harmonic_fit_f64"] = timed(lambda i: harmonic_fit_f64(pj, Q))
    _, peak = harmonic_fit_f64(pj, Q)
    res["series_with_a_peak"] = int((peak[:, 2, 0] == 2).sum())
    res["peak_bins_z"] = sorted(set(peak[:, 2, 3].cpu().numpy().astype(int).tolist()))[:5]
    # the yardsticks: the selected operand [n, s * 4] is prepared once, outside the timed region
    sel = []
    for r in recs:
        v = torch.where(r[..., :1] != 0, r[..., 1:4], torch.zeros((), dtype=torch.float64, device="cuda"))
        sel.append(torch.cat([v, (r[..., :1] != 0).to(torch.float64)], dim=2).reshape(n, s * 4).contiguous())   # x1, x2, x3, flag
    res["matmul_f64_yardstick"] = timed(lambda i: torch.matmul(basis, sel[i % buffers]))
    res["rfft_natural_grid"] = timed(lambda i: torch.fft.rfft(sel[i % buffers], dim=0))
    us = res["project_series_f64"]["median_us"]
    res["tflops_f64"] = 2 * res["multiply_adds"] / us * 1e-6
    res["speedup_over_matmul_yardstick"] = res["matmul_f64_yardstick"]["median_us"] / us
    res["time_over_rfft"] = (us + res["harmonic_fit_f64"]["median_us"]) / res["rfft_natural_grid"]["median_us"]
    ref = torch.matmul(basis, sel[0]).view(R, s, 4).permute(1, 0, 2)                     # [s, R, (num1, num2, num3, den)]
    res["max_abs_difference_from_yardstick"] = float(max((pj[..., 1:] - ref[..., :3]).abs().max(), (pj[..., 0] - ref[..., 3]).abs().max()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,Q of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        s, Q = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(s, Q, a.reps, a.buffers)), flush=True)
        return 0
    for s, Q in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{s},{Q}", "--reps", str(a.reps), "--buffers", str(a.buffers)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {s} Q {Q}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {s} Q {Q}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
