"""Time of `vbs_rigid_ml_series` (k_rigid_ml.hip) on resident inputs, next to `vbs_rigid_series` on the same table in the same run.

For 4096 frames x 169 and x 441 markers (the recording of tools/gpu_rigid_rate.py: a shallow dome that tilts, twists and shifts plus
noise, 3 % of the rows without a 3-D point, two markers moved by 2 mm per frame), a covariance per point that is a needle along the
ray to a camera centre 60 mm above the dome (0.004 mm across, 0.3 % of the distance along), the start of `vbs_rigid_series` with one
round of rejection (reject_k = 3) and `iters` = 4 and 8: HIP-event time per call of `vbs_rigid_ml_series` emitting `ml`, `pcov`,
`coef` and `mahal`, without and with `source_cov`, and of `vbs_rigid_series` emitting its three outputs - the yardstick: the
closed form the weighted fit starts from -, after warm-up calls, median and minimum over `--reps` calls.  The largest `step_rot`
and `step_c` of the last step are reported with the times: what the step count reached.  No rate is a pass criterion; the figures
are single-run numbers on a shared machine.  Every shape runs in a child process under its own time limit (`--limit` seconds); a
child that fails or runs out of time ends the run.  Prints one JSON line per shape; `--out FILE` also appends them there.

    python tools/gpu_rigid_ml_rate.py [--reps 10] [--limit 240] [--out profiles/rigid_ml_rate.log]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = tuple((s, k) for s in (169, 441) for k in (4, 8))


def recording(n, m, seed):
    """-> (float32 table [n, m, 10], layout float64 [m, 3]): markers on a square grid of 2 mm on a shallow dome; frame f is the
    layout tilted by up to 2 degrees, twisted by up to 3 and shifted by up to 0.5 mm, with 0.01 mm noise, 3 % of the rows without a
    point and two markers moved by 2 mm."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    i = np.arange(m)
    lay = np.stack([(i % side - (side - 1) / 2) * 2.0, (i // side - (side - 1) / 2) * 2.0, np.zeros(m)], axis=1)
    lay[:, 2] = 3.0 - 0.005 * (lay[:, 0] ** 2 + lay[:, 1] ** 2)
    u = np.linspace(0.0, 1.0, n)
    a, b, c = np.radians(2.0) * u, np.radians(-1.0) * u, np.radians(3.0) * u      # about x, about y, about z
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    one, zero = np.ones(n), np.zeros(n)
    Rx = np.stack([one, zero, zero, zero, ca, -sa, zero, sa, ca], axis=1).reshape(n, 3, 3)
    Ry = np.stack([cb, zero, sb, zero, one, zero, -sb, zero, cb], axis=1).reshape(n, 3, 3)
    Rz = np.stack([cc, -sc, zero, sc, cc, zero, zero, zero, one], axis=1).reshape(n, 3, 3)
    R = Rx @ Ry @ Rz
    xyz = np.einsum("fij,mj->fmi", R, lay) + (u[:, None] * np.array([0.5, -0.3, 0.2]))[:, None, :]
    xyz += r.normal(0.0, 0.01, (n, m, 3))
    moved = r.integers(0, m, (n, 2))
    xyz[np.arange(n)[:, None], moved, 2] += 2.0
    xyz[0] = lay
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 6:9] = xyz
    seen = r.random((n, m)) >= 0.03
    seen[0] = True
    t[..., 0] = 1 + 2 * seen
    return t, lay


def one_shape(m, iters, reps):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import rigid as RG
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    dev = torch.device("cuda", 0)
    t, lay = recording(n, m, m)
    tab = torch.from_numpy(t).cuda()
    source = torch.from_numpy(RG.source_from_table(t, 0)).cuda()

    def needles(X):                                               # flag, xx, xy, xz, yy, yz, zz about a camera 60 mm above the dome
        v = X - np.array([0.0, 0.0, 60.0])
        h2 = (v * v).sum(axis=-1)
        u = v / np.sqrt(h2)[..., None]
        lat, lon = 0.004 ** 2, h2 * 0.003 ** 2
        out = np.ones(X.shape[:-1] + (7,))
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            out[..., 1 + k] = (lat if i == j else 0.0) + (lon - lat) * u[..., i] * u[..., j]
        return out

    cov = torch.from_numpy(needles(t[..., 6:9].astype(np.float64))).cuda()
    source_cov = torch.from_numpy(needles(lay)).cuda()
    rigid = torch.empty((n, L.RIGID_COLS), dtype=torch.float64, device=dev)
    rcoef = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    rres = torch.empty((n, m, 4), dtype=torch.float64, device=dev)
    ml = torch.empty((n, L.RIGID_ML_COLS), dtype=torch.float64, device=dev)
    pcov = torch.empty((n, L.RIGID_ML_PCOV_COLS), dtype=torch.float64, device=dev)
    coef = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    mahal = torch.empty((n, m, 3), dtype=torch.float64, device=dev)
    p = A._ptr

    def timed(fn, warm=2, reps=reps):
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

    res = {"frames": n, "slots": m, "iters": iters, "reject_k": 3.0, "device": torch.cuda.get_device_name(0), "reps": reps,
           "rigid_ml_group": L.RIGID_ML_GROUP, "single_run": True}
    res["rigid_series"] = timed(lambda i: A._call("vbs_rigid_series", "", dev, p(tab), n, m, p(source), None, 0, 3.0, 1e-6, 0, n,
                                                  p(rigid), p(rcoef), p(rres)))
    for name, sc in (("rigid_ml_series", None), ("rigid_ml_series_source_cov", source_cov)):
        res[name] = timed(lambda i: A._call("vbs_rigid_ml_series", "", dev, p(tab), n, m, p(source), p(cov), p(rigid), p(rres), p(sc),
                                            iters, 1e-12, 0, n, p(ml), p(pcov), p(coef), p(mahal)))
        torch.cuda.synchronize()
        fit = ml[:, 0] == 2.0
        res[name].update(frames_fitted=int(fit.sum()), max_step_rot=float(ml[fit, 29].max()), max_step_c=float(ml[fit, 30].max()),
                         mean_chi2_per_dof=float((ml[fit, 26] / ml[fit, 27]).mean()))
    res["ratio_to_rigid_series"] = res["rigid_ml_series"]["median_us"] / res["rigid_series"]["median_us"]
    res["rigid_ml_us_per_frame"] = res["rigid_ml_series"]["median_us"] / n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,iters of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        m, k = a.shape.split(",")
        print(json.dumps(one_shape(int(m), int(k), a.reps)), flush=True)
        return 0
    for m, k in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{m},{k}", "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired as e:
            print(f"slots {m} iters {k}: no result within {a.limit} s; stopping\n{(e.stderr or b'')[-500:]}", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {m} iters {k}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
