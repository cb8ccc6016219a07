"""How many synchronisation rounds the device Huffman decoder (csrc/k_jpeg_huff.hip) needs: the debug library's emulation
(`vbs_dbg_mjpeg_huffman_emulate`, the kernel's five phases with loops in place of threads) counts, per frame, the rounds of
phase 2 and the longest chain (the subsequences one thread decoded before it met a stored state equal to its own).  Printed
as distributions over the test suite's stream variants and over 64 frames of the 640x480 quality-70 4:2:0 clip, at
S = 512 / 1024 / 2048 bits and 256 subsequences per chunk.  CPU only, exact, reproducible.  usage: mjpeg_sync_rounds.py"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np
import mjpeg_cases as M
import vbs_amd.synth as S
from vbs_amd import _lib as L

lib = L.lib()
frames = S.make_frames(S.config1(), range(64), seed=0, channels=3)
groups = {"test variants": [d for _, d in M.variant_streams()],
          "640x480 q70 4:2:0": [M.encode(f, quality=70, subsampling=2) for f in frames]}
for name, datas in groups.items():
    for sbits in (512, 1024, 2048):
        rounds, chain, subs = collections.Counter(), collections.Counter(), []
        for data in datas:
            _, info = M.probe(lib, data)
            sb = M.ScanBatch(lib, data, [0], [len(data)], info, threads=1)
            scan, bits, tset = sb.frame(0)
            rc, _, c = M.emulate(scan, bits, tset, info, sbits, 256)
            assert rc == 0
            rounds[int(c[2])] += 1
            chain[int(c[3])] += 1
            subs.append((bits + sbits - 1) // sbits)
        print(json.dumps({"streams": name, "frames": len(datas), "subseq_bits": sbits,
                          "subsequences_per_frame_median": int(np.median(subs)), "subsequences_per_frame_max": int(max(subs)),
                          "rounds_in_the_worst_chunk": dict(sorted(rounds.items())),
                          "longest_chain": dict(sorted(chain.items()))}), flush=True)
