"""Host against device entropy decode of the Motion-JPEG front end (`MjpegDeviceDecoder(entropy=...)`), in ONE process,
alternated: a 640x480 quality-70 4:2:0 clip (the camera's format) -> the decoder alone (entropy + reconstruct) and
MarkerTracker.process() AVI -> CSV, at batch 64 and 256, three repetitions each after a warm-up of every shape; the
subsequence lengths 512 / 1024 / 2048; the host cost per frame of `vbs_mjpeg_scan_batch` and of `vbs_mjpeg_entropy_batch` on
one thread; the bytes uploaded per frame.  One JSON line per figure.
usage: gpu_entropy_path.py [frames = 8192] [--kernels: one short pass of each path only, for a kernel trace]"""
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import vbs_amd.synth as S
from vbs_amd.marker_detection import MarkerTracker
from vbs_amd.video_io import AviReader, AviWriter, MjpegDeviceDecoder

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 8192
kernels_only = "--kernels" in sys.argv
dev = torch.device("cuda:0")


def say(**kw):
    print(json.dumps(kw), flush=True)


def make_clip(path):
    import io
    from PIL import Image
    spec = S.config1()
    frames = S.make_frames(spec, range(64), seed=0, channels=3)
    files = []
    for f in frames:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(bio, format="JPEG", quality=70, subsampling=2)
        files.append(bio.getvalue())
    with AviWriter(path, 12.0, spec.width, spec.height) as out:
        for i in range(n):
            out.write(files[i % 64])
    return sum(len(f) for f in files) / 64


def decoder_alone(path, entropy, batch, subseq_bits=0, threads=16):
    """entropy of batch k + 1 on a helper thread while batch k is reconstructed, as the tracker runs them"""
    from concurrent.futures import ThreadPoolExecutor
    dec = MjpegDeviceDecoder(AviReader(path), dev, batch, threads, entropy=entropy, subseq_bits=subseq_bits)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k, frames = 0, 0
    with ThreadPoolExecutor(1) as ahead:
        fut = ahead.submit(dec.entropy, 0)
        while True:
            m = fut.result()
            if not m:
                break
            fut = ahead.submit(dec.entropy, (k + 1) & 1)
            dec.reconstruct(k & 1)
            if entropy == "host":
                torch.cuda.synchronize()          # (the device path waits for its status words; the slot is free either way)
            frames += m
            k += 1
    torch.cuda.synchronize()
    return frames / (time.perf_counter() - t0), dec


def tracker(path, entropy, batch, out):
    with contextlib.redirect_stdout(sys.stderr):
        trk = MarkerTracker({"video_path": path, "output_dir": out, "mjpeg_entropy": entropy, "decode_threads": 16,
                             "crop_ratios": (1 / 8, 1 / 8, 1 / 16, 0), "id_mode": "full", "batch": batch})
        t0 = time.perf_counter()
        trk.process()
        dt = time.perf_counter() - t0
    assert trk.decode_path == "device" and trk.entropy_path == entropy
    return n / dt, open(trk.output_csv, "rb").read()


with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "clip.avi")
    kib = make_clip(path) / 1024
    say(clip=f"{n} frames 640x480 MJPG quality 70 4:2:0", kib_per_frame=round(kib, 1), gpu=torch.cuda.get_device_name(0))
    if kernels_only:
        for entropy in ("host", "device"):
            for sb in ((0,) if entropy == "host" else (512, 1024, 2048)):
                rate, _ = decoder_alone(path, entropy, 256, sb)
                say(what="decoder alone, traced", entropy=entropy, subseq_bits=sb, frames_per_s=round(rate))
        sys.exit(0)
    # host cost per frame on ONE thread
    for entropy in ("host", "device"):
        dec = MjpegDeviceDecoder(AviReader(path), dev, 256, 1, entropy=entropy)
        dec.entropy(0)
        t0 = time.perf_counter()
        k = 0
        while k < 2048:
            m = dec.entropy(0)
            if not m:
                break
            k += m
        dt = time.perf_counter() - t0
        say(what="host half on one thread", call="vbs_mjpeg_scan_batch" if entropy == "device" else "vbs_mjpeg_entropy_batch",
            frames_per_s=round(k / dt), us_per_frame=round(1e6 * dt / k, 1))
    # decoder alone
    for batch in (64, 256):
        for entropy in ("host", "device"):
            decoder_alone(path, entropy, batch)                        # warm-up of the shape
        rates = {"host": [], "device": []}
        for rep in range(3):
            for entropy in ("host", "device"):
                rate, dec = decoder_alone(path, entropy, batch)
                rates[entropy].append(round(rate))
                if rep == 0:
                    say(what="uploaded bytes per frame", entropy=entropy, batch=batch, bytes=round(dec.uploaded_bytes / n),
                        host_fallback_frames=dec.host_fallback_frames)
        say(what="decoder alone (entropy + reconstruct), frames/s", batch=batch, **rates)
    for sb in (512, 1024, 2048):
        decoder_alone(path, "device", 256, sb)
        say(what="decoder alone, device entropy, frames/s", batch=256, subseq_bits=sb,
            rates=[round(decoder_alone(path, "device", 256, sb)[0]) for _ in range(3)])
    # AVI -> CSV
    texts = set()
    for batch in (64, 256):
        for entropy in ("host", "device"):
            tracker(path, entropy, batch, os.path.join(td, f"w_{entropy}_{batch}"))
        rates = {"host": [], "device": []}
        for rep in range(3):
            for entropy in ("host", "device"):
                rate, text = tracker(path, entropy, batch, os.path.join(td, f"o_{entropy}_{batch}_{rep}"))
                rates[entropy].append(round(rate))
                texts.add(text)
        say(what="MarkerTracker.process() AVI -> CSV, frames/s", batch=batch, **rates)
    say(what="CSV files of both entropy paths and both batch sizes identical", same=len(texts) == 1)
    if len(texts) != 1:
        sys.exit(1)
