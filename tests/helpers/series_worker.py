"""Child process of tests/test_gpu_analysis.py::test_series_stats_shard_two_ranks_on_one_gpu: one rank of a 2-rank gloo
group, both ranks on GPU 0 (the shard_worker.py pattern).  The rank renders and tracks its own block of the clip, reduces its
`disp` to per-chunk records, joins the one all-gather and merges.  argv: rank world port n_total outdir"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def gap_frames(n_total):
    """Frames in which the centre dot is painted out: a few early ones, and a run across the middle of the clip (the shard
    edge of two ranks), so that the displacement after it looks back across the edge."""
    e = n_total // 2
    return sorted({f for f in (3, 4, 9, e - 1, e, e + 1, n_total - 2) if 0 < f < n_total})


def make_clip(n_total, first=0, last=None, device="cuda"):
    """Frames [first, last) of `n_total` config-2 frames (1280x1024, 169 dots) on the device, the centre dot painted out in
    `gap_frames(n_total)` as shard_worker.make_clip does."""
    import vbs_amd.synth as S
    spec = S.config2()
    last = n_total if last is None else last
    frames = S.make_frames_torch(spec, range(first, last), seed=11, device=device)
    cx, cy = spec.width // 2, spec.height // 2
    for f in gap_frames(n_total):
        if first <= f < last:
            frames[f - first, cy - 30:cy + 30, cx - 30:cx + 30] = 190
    return spec, frames


def main():
    rank, world, port, n_total, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5]
    import torch
    import torch.distributed as td
    import vbs_amd.synth as S
    from vbs_amd import _lib as L
    from vbs_amd import dist as D
    from vbs_amd.engine import Engine
    from vbs_amd.pipeline import series_stats_shard, track_shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        a, b = D.shard_bounds(n_total, world, rank)
        spec, frames = make_clip(n_total, a, b)
        K, dist, R, T = S.default_camera(spec)
        cam = L.make_camera(K, dist, R, T, 2.0)
        eng = Engine(spec.height, spec.width, max_markers=512, max_batch=16, device=0)
        res = track_shard(eng, frames, n_total, cam=cam, warmup_frames=0)
        stats = series_stats_shard(eng, res, n_total)
        np.savez(os.path.join(outdir, f"series_rank{rank}.npz"), stats=stats.cpu().numpy(), disp=res.disp.cpu().numpy(),
                 span=np.array([res.frame_begin, res.frame_end]))
    finally:
        td.destroy_process_group()


if __name__ == "__main__":
    main()
