"""Time of the strain entries (k_motion.hip) on a resident record, with a yardstick in the same run.

For 4096 frames x `--slots` markers (169 or 441; a random affine field per frame under noise, 3 % of the entries missing, K = 6
neighbours): HIP-event time per call of `engine.motion_series_f64` (all three outputs; reject_k = 0 and 3) and of
`engine.local_strain_f64`, after warm-up calls, median and minimum over `--reps` calls, the record rotated over `--buffers` copies
so that a call does not find the previous call's rows in the caches by construction.  Beside it, on the same device and the same
record: the same normal equations as masked float64 `torch.einsum` with a batched 2 x 2 solve - A YARDSTICK ONLY: no flags, no
rejection, no residual, no stated order of summation.
The events bracket the PYTHON entry: `as_tensor`, the `torch.empty` of the outputs, the argument checks and the ctypes call lie
inside the interval, so at tens of microseconds a figure may be bounded by launch and host time, not by the kernel.
Bytes: what the algorithm must move once - the record, pos (and the neighbour lists) and the outputs - over the median time:
a floor on what the kernel sustains.
One shape a run, so that a driver can give every step a time limit of its own:

    timeout 300 python tools/gpu_motion_rate.py --slots 169 [--reps 30] [--buffers 4] [--out FILE]
    timeout 300 python tools/gpu_motion_rate.py --slots 441 ...

Prints one JSON line per entry and reject_k; `--out FILE` also appends them there.  No rate is a pass criterion.
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
    ap.add_argument("--slots", type=int, default=169)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import motion_oracle as O                                 # (the record's generator only)
    from vbs_amd import _lib as L
    from vbs_amd import engine as E
    from vbs_amd import strain as ST
    assert torch.cuda.is_available(), "needs a GPU"

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

    n, m, K = a.frames, a.slots, 6
    rec, pos = O.random_case(n, m, 4, m, drop=0.03, thin=False)
    recs = [torch.from_numpy(rec).cuda() for _ in range(a.buffers)]
    pos_d = torch.from_numpy(pos).cuda()
    nbr = torch.from_numpy(ST.neighbour_lists(pos, K)).cuda()
    base = {"frames": n, "slots": m, "device": torch.cuda.get_device_name(0), "reps": a.reps, "buffers": a.buffers}

    def emit(res, us, moved):
        res["bytes_moved_once"] = moved
        res["gb_per_s_of_bytes_moved_once"] = moved / us * 1e-3
        res["frames_per_s"] = n / us * 1e6
        res["us_per_frame"] = us / n
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")

    def einsum_fit(i):                                        # the normal equations of the first fit, nothing else
        r = recs[i % a.buffers]
        w = (r[..., 0] != 0).to(torch.float64)
        d = torch.where(w[..., None] != 0, r[..., 1:4], torch.zeros((), dtype=torch.float64, device=r.device))
        cnt = w.sum(dim=1)
        mp = torch.einsum("fs,sc->fc", w, pos_d) / cnt[:, None]
        md = torch.einsum("fs,fsk->fk", w, d) / cnt[:, None]
        x = (pos_d[None] - mp[:, None]) * w[..., None]
        e = d - md[:, None]
        A = torch.einsum("fsa,fsb->fab", x, x)
        B = torch.einsum("fsa,fsk->fak", x, e)
        return torch.linalg.solve(A, B)

    yard = timed(einsum_fit, a.reps)
    print(f"m {m}: einsum + 2 x 2 solve {yard}", file=sys.stderr, flush=True)
    for k in (0.0, 3.0):
        res = dict(base, entry="motion_series_f64", reject_k=k, motion_group=L.MOTION_GROUP)
        flags = E.motion_series_f64(recs[0], pos_d, reject_k=k, want="strain")["strain"][:, 0]
        res["frames_refitted"] = int((flags == 2).sum())
        res["motion_series"] = timed(lambda i: E.motion_series_f64(recs[i % a.buffers], pos_d, reject_k=k), a.reps)
        res["einsum_solve_f64_yardstick"] = yard
        res["speedup_over_yardstick"] = yard["median_us"] / res["motion_series"]["median_us"]
        print(f"m {m} reject_k {k}: motion_series {res['motion_series']}", file=sys.stderr, flush=True)
        emit(res, res["motion_series"]["median_us"], n * m * (4 * 8 + 4 * 8) + m * 16 + n * (12 + L.STRAIN_COLS) * 8)
    res = dict(base, entry="local_strain_f64", neighbours=K, lstrain_group=L.LSTRAIN_GROUP)
    res["results"] = int((E.local_strain_f64(recs[0], pos_d, nbr)[..., 0] != 0).sum())
    res["local_strain"] = timed(lambda i: E.local_strain_f64(recs[i % a.buffers], pos_d, nbr), a.reps)
    print(f"m {m}: local_strain {res['local_strain']}", file=sys.stderr, flush=True)
    emit(res, res["local_strain"]["median_us"], n * m * (4 * 8 + L.LSTRAIN_COLS * 8) + m * (16 + 4 * K))


if __name__ == "__main__":
    main()
