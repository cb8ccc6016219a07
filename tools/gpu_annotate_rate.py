"""Rates of the annotated-video path (`write_video`) for the 480x450 crop of a 640x480 Motion-JPEG clip (the reference's
camera frame and crop (1/8, 1/8, 1/16, 0)): frames/s of `MarkerTracker.process()` with and without `write_video`, and of the
device encoder alone (`MjpegDeviceEncoder`: encode + download of the files).  Prints one JSON line; with `--out DIR` also
writes it there.  Per-kernel times come from a separate run under the profiler, e.g.

    rocprofv3 --kernel-trace --stats -d OUT -o annotate -- python tools/gpu_annotate_rate.py --frames 512 --reps 1

    python tools/gpu_annotate_rate.py [--frames 1024] [--batch 64] [--reps 3] [--out DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import vbs_amd.synth as S
    from vbs_amd.marker_detection import MarkerTracker, _crop_box
    from vbs_amd.video_io import MjpegDeviceEncoder, write_avi
    assert torch.cuda.is_available(), "needs a GPU"
    crop = (1 / 8, 1 / 8, 1 / 16, 0)
    spec = S.config1()
    base = S.make_frames(spec, range(16), seed=1, channels=3)
    frames = base[np.arange(a.frames) % 16]
    td = tempfile.mkdtemp()
    clip = os.path.join(td, "clip.avi")
    write_avi(clip, frames, fps=30.0, quality=90)
    res = {"frames": a.frames, "batch": a.batch, "crop": "480x450", "device": torch.cuda.get_device_name(0)}

    def run(video):
        cfg = {"video_path": clip, "output_dir": os.path.join(td, "v" if video else "p"), "crop_ratios": crop,
               "batch": a.batch, "id_mode": "full", "write_video": video, "video_reader": "native"}
        t = MarkerTracker(cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.process()
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0)

    run(False)
    run(True)                                                       # warm-up of both
    best = {"process_fps": 0.0, "process_write_video_fps": 0.0}
    for _ in range(a.reps):                                         # alternated
        best["process_fps"] = max(best["process_fps"], run(False))
        best["process_write_video_fps"] = max(best["process_write_video_fps"], run(True))
    res.update(best)
    l, r, t, b = _crop_box(640, 480, crop)
    dev = torch.from_numpy(frames[:, t:b, l:r].copy()).cuda()
    enc = MjpegDeviceEncoder("cuda:0", r - l, b - t, a.batch, 95)
    for s in range(0, min(a.frames, 2 * a.batch), a.batch):
        enc.fetch(enc.encode(dev[s:s + a.batch]))
    rates, sizes = [], 0
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for s in range(0, a.frames, a.batch):
            files = enc.fetch(enc.encode(dev[s:s + a.batch]))
            n += len(files)
            sizes += sum(map(len, files))
        rates.append(n / (time.perf_counter() - t0))
    res["encode_fps"] = max(rates)
    res["jpeg_bytes_per_frame"] = sizes / (a.reps * a.frames)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        open(os.path.join(a.out, "annotate_rate.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
