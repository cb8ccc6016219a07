"""Time of the uncertainty entries (k_uncert.hip) on a resident table, with forward-mode automatic differentiation of a library
as the yardstick.

For 4096 frames x 169 and x 441 markers (a press plus pixel noise, 3 % of the rows untracked), a distorted camera and camera
factors of q = 5 and q = 16 columns: HIP-event time per call of `vbs_uncert_cov` (Sigma_X, Sigma_D and t2 of every row),
`vbs_uncert_total` and `vbs_pixel_noise` through `engine.solve3d_cov` / `engine.pixel_noise`'s entries, after warm-up calls,
median and minimum over `--reps` calls.  Beside them, on the same device, the YARDSTICK: `torch.func.vmap(torch.func.jacfwd(..))`
of the same model written in torch float64 (five iterations, the closed-form solve, the rotation on the camera side), in chunks of
`--chunk` rows, followed by the same products as batched matrix products (J_cam L, G G', J_obs Sigma_o J_obs', their sums over
the slots) - no flags, no gate, no t2.
No rate is a pass criterion; the figures are single-run numbers on a shared machine.  Every shape runs in a child process under
its own time limit (`--limit` seconds); a child that fails or runs out of time ends the run.  Prints one JSON line per shape;
`--out FILE` also appends them there.

    python tools/gpu_uncert_rate.py [--reps 10] [--limit 240] [--chunk 65536] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 4096
SHAPES = tuple((s, q) for s in (169, 441) for q in (5, 16))
DIST = (-0.28, 0.09, 1e-3, -5e-4, -0.01)


def recording(n, m, cam, seed):
    """-> float32 table [n, m, 10] with X, Y, Z from `engine.calculate_3d(undistort_points(..))`."""
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd.engine import calculate_3d, undistort_points
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(m)))
    gx, gy = np.meshgrid(np.linspace(200, 1720, side), np.linspace(150, 1050, side))
    f = np.arange(n, dtype=np.float64)
    press = 0.5 * (1.0 - np.cos(np.pi * np.clip((f - 0.3 * n) / (0.25 * n), 0.0, 1.0)))
    o = np.stack([np.broadcast_to(gx.ravel()[:m], (n, m)), np.broadcast_to(gy.ravel()[:m], (n, m)),
                  16.0 + 1.5 * press[:, None] * r.uniform(0.5, 1.0, m)[None, :]], axis=2) + r.normal(0.0, 0.05, (n, m, 3))
    t = np.zeros((n, m, L.TABLE_COLS), dtype=np.float32)
    t[..., 1:4] = o
    uvd = t[..., 1:4].reshape(-1, 3).astype(np.float64)
    und = undistort_points(uvd[:, :2].copy(), cam)
    xyz, ok = calculate_3d(torch.cat([und, torch.as_tensor(uvd[:, 2:3], device=und.device)], dim=1), cam)
    t[..., 6:9] = xyz.cpu().numpy().reshape(n, m, 3)
    tracked = r.random((n, m)) >= 0.03
    t[..., 0] = tracked * (1 + 2 * ok.cpu().numpy().reshape(n, m))
    return t


def one_shape(m, q, reps, chunk):
    import numpy as np
    import torch

    from vbs_amd import _lib as L
    from vbs_amd import analysis as A
    from vbs_amd import uncertainty as UN
    assert torch.cuda.is_available(), "needs a GPU"
    n = FRAMES
    K = np.array([[1500.0 * 1.01, 0, 963.3], [0, 1500.0 * 0.99, 597.9], [0, 0, 1]])
    a, b = 0.3, 0.2
    R = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @
         np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
    T = np.array([3.0, -2.0, 40.0])
    cam = L.make_camera(K, DIST, R, T, 2.0)
    tab = torch.from_numpy(recording(n, m, cam, m)).cuda()
    obs = np.ascontiguousarray(UN.obs_cov(0.05, 0.05).reshape(1, 6))
    if q == 5:
        fac = UN.camera_factor(omega_std=[1e-4] * 3, t_std=[0.02, 0.02, 0.0])
    else:
        r = np.random.default_rng(1)
        sd = np.array([0.5, 0.5, 0.3, 0.3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-3, 1e-4, 1e-4, 1e-4, 0.02, 0.02, 0.05, 0.01])
        fac = np.tril(r.normal(size=(16, 16))) * sd[:, None]
    fac = np.ascontiguousarray(fac)
    assert fac.shape == (16, q)
    dev = torch.device("cuda", 0)
    work = torch.empty((m * L.UNCERT_WORK_COLS,), dtype=torch.float64, device=dev)
    cov = torch.empty((n, m, L.UNCERT_COV_COLS), dtype=torch.float64, device=dev)
    dcov = torch.empty((n, m, L.UNCERT_DCOV_COLS), dtype=torch.float64, device=dev)
    total = torch.empty((n, L.UNCERT_TOTAL_COLS), dtype=torch.float64, device=dev)
    noise = torch.empty((m, L.NOISE_COLS), dtype=torch.float64, device=dev)
    hp, p = A._host_ptr, A._ptr

    def timed(fn, warm=2):
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

    res = {"frames": n, "slots": m, "q": q, "device": torch.cuda.get_device_name(0), "reps": reps, "chunk": chunk,
           "uncert_group": L.UNCERT_GROUP}
    res["uncert_cov"] = timed(lambda i: A._call("vbs_uncert_cov", "", dev, p(tab), n, m, C.byref(cam), hp(obs), 1, hp(fac), q, 0, 5.0,
                                                1e-12, 0, n, p(work), p(cov), p(dcov)))
    res["uncert_total"] = timed(lambda i: A._call("vbs_uncert_total", "", dev, p(tab), n, m, C.byref(cam), hp(obs), 1, hp(fac), q, 0,
                                                  None, 5.0, 0, n, p(work), p(total)))
    res["pixel_noise"] = timed(lambda i: A._call("vbs_pixel_noise", "", dev, p(tab), n, m, 0, n, p(noise)))
    res["usable_rows"] = float((cov[..., 0] == 1).double().mean())
    res["rows_per_us_cov"] = n * m / res["uncert_cov"]["median_us"]

    # ---- the yardstick: the same model in torch float64, differentiated by jacfwd under vmap -------------------------------------
    from torch.func import jacfwd, vmap
    f64 = dict(dtype=torch.float64, device=dev)
    Rt = torch.as_tensor(np.asarray(R, dtype=np.float32).astype(np.float64), **f64)
    theta = torch.as_tensor(np.concatenate([[np.float32(K[0, 0]), np.float32(K[1, 1]), np.float32(K[0, 2]), np.float32(K[1, 2])],
                                            np.asarray(DIST, dtype=np.float32), np.zeros(3), np.asarray(T, dtype=np.float32), [2.0]]),
                            **f64)

    def model(th, o):
        fx, fy, cx, cy, k1, k2, p1, p2, k3 = th[:9].unbind()
        w, Tt, dmm = th[9:12], th[12:15], th[15]
        x0, y0 = (o[0] - cx) / fx, (o[1] - cy) / fy
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dxx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dyy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dxx) * icd, (y0 - dyy) * icd
        du, dv = x * fx, y * fy
        fa = (fx + fy) / 2.0
        h = fa * ((dmm / fa) * torch.sqrt(du * du + dv * dv + fa * fa) / o[2])
        pc = torch.stack([h * du / fx - Tt[0], h * dv / fy - Tt[1], h - Tt[2]])
        pc = pc - torch.linalg.cross(w, pc)
        return Rt.t() @ pc

    jac = vmap(jacfwd(model, argnums=(0, 1)), in_dims=(None, 0))
    Lt = torch.as_tensor(fac, **f64)
    S = torch.as_tensor(np.array([[obs[0, 0], obs[0, 1], obs[0, 2]], [obs[0, 1], obs[0, 3], obs[0, 4]], [obs[0, 2], obs[0, 4], obs[0, 5]]]),
                        **f64)
    rows = tab[..., 1:4].reshape(-1, 3).to(torch.float64)
    rows = torch.where((tab[..., 0].reshape(-1, 1) == 3), rows, rows.new_tensor([900.0, 500.0, 16.0]))

    def parts(o):
        Jc, Jo = jac(theta, o)
        return Jc @ Lt, Jo @ S @ Jo.transpose(1, 2)

    def yard(i):
        G0, P0 = parts(rows[:m])
        sx = torch.empty((n * m, 3, 3), **f64)
        sd = torch.empty((n * m, 3, 3), **f64)
        dG = torch.empty((n * m, 3, q), **f64)
        for lo in range(0, n * m, chunk):
            hi = min(lo + chunk, n * m)
            G, Pf = parts(rows[lo:hi])
            slot = torch.arange(lo, hi, device=dev) % m
            d = G - G0[slot]
            sx[lo:hi] = Pf + G @ G.transpose(1, 2)
            sd[lo:hi] = Pf + P0[slot] + d @ d.transpose(1, 2)
            dG[lo:hi] = d
        B = dG.reshape(n, m, 3, q).sum(dim=1)
        var = torch.diagonal(sd, dim1=1, dim2=2).reshape(n, m, 3).sum(dim=1) - (dG * dG).sum(dim=2).reshape(n, m, 3).sum(dim=1)
        return sx, sd, var + (B * B).sum(dim=2), (B * B).sum(dim=2)
    res["jacfwd_vmap_f64_yardstick"] = timed(yard, warm=1)
    res["speedup_over_jacfwd"] = res["jacfwd_vmap_f64_yardstick"]["median_us"] / (res["uncert_cov"]["median_us"] +
                                                                                     res["uncert_total"]["median_us"])
    sx, sd, var, camv = yard(0)
    use = cov[..., 0].reshape(-1) == 1
    got = cov.reshape(-1, 7)[use][:, [1, 4, 6]]
    want = torch.diagonal(sx, dim1=1, dim2=2)[use]
    res["max_rel_difference_of_var_X_from_jacfwd"] = float(((got - want).abs() / want).max())
    full = total[:, 1] == 1
    res["complete_frames"] = int(full.sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="internal: slots,q of the one shape this process measures")
    a = ap.parse_args()
    if a.shape:
        m, q = (int(x) for x in a.shape.split(","))
        print(json.dumps(one_shape(m, q, a.reps, a.chunk)), flush=True)
        return 0
    for m, q in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{m},{q}", "--reps", str(a.reps), "--chunk", str(a.chunk)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"slots {m} q {q}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"slots {m} q {q}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
