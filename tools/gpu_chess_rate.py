#!/usr/bin/env python3
"""Chessboard corner rate: 64 resident 640x480 frames with a rendered 6x6 board through Engine.find_chessboard_corners, then
finder + corner_subpix (11,11).  HIP events, a warm-up, the median of the repeats; one JSON line.

    timeout -k 10 120 python tools/gpu_chess_rate.py [--frames 64] [--repeats 20] > profiles/chess_rate.log
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import chess_cases as CC                                      # noqa: E402
from vbs_amd.engine import Engine                             # noqa: E402


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    gray, _ = CC.render((640, 480), (7, 7), CC.similarity(48.0, 12.0, 190.0, 40.0))
    frames = torch.from_numpy(np.repeat(gray[None], args.frames, axis=0)).cuda()
    eng = Engine(480, 640, max_markers=64, max_batch=args.frames)

    def finder():
        return eng.find_chessboard_corners(frames, (6, 6))

    def both():
        return eng.corner_subpix(frames, finder()[1])

    found = finder()[0]
    both()
    torch.cuda.synchronize()
    assert int(found.sum()) == args.frames, "the board was not found in every frame"
    t1, t2 = timed(finder, args.repeats), timed(both, args.repeats)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), frames=args.frames, finder_ms=t1, finder_fps=args.frames / t1 * 1e3,
                          finder_subpix_ms=t2, finder_subpix_fps=args.frames / t2 * 1e3)))


if __name__ == "__main__":
    main()
