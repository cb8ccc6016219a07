"""The device JPEG encoder as far as a CPU can check it.  (1) Every case of tests/helpers/jpeg_enc_cases.py reaches the place it
was built for, judged on PILLOW'S file: its tables, its coefficients (through the project's host entropy decoder), its last
bytes.  (2) The __host__ __device__ functions of csrc/k_jpeg_enc.hip, run with loops in place of threads by the debug library
(`vbs_dbg_jpeg_encode_emulate`: tables, colour conversion, downsampling, edge replication, DCT, quantisation, dummy blocks, code
emission, padding, stuffing), write Pillow's bytes on every case.  PackSink, the workgroup scans and k_jenc_write are not in
the emulation: tests/test_gpu_jpeg_enc.py.  (3) `vbs_jpeg_encode` refuses bad arguments before it launches anything.  Byte
equality throughout, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import jpeg_enc_cases as J  # noqa: E402

pytest.importorskip("PIL")

from vbs_amd import _lib as L  # noqa: E402

FORMER_QUALITIES = (50, 75, 95, 100)                    # of test_jpeg_encoder_bytes_equal_pillow
HEADER_BYTES = 623                                      # VBS_JPEG_HEADER_BYTES


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def _decoded(lib, cases):
    return [(name, i, q, J.Decoded(lib, J.pillow_jpeg(f, q))) for name, fr, q in cases for i, f in enumerate(fr)]


def test_quality_sweep_meets_every_divisor_of_pillows_tables(lib):
    d50 = J.Decoded(lib, J.pillow_jpeg(np.zeros((8, 8, 3), np.uint8), 50))
    # Pillow hands the tables out in natural order: at quality 50 they are Annex K.1 itself
    assert d50.q[0][:9].tolist() == [16, 11, 10, 16, 24, 40, 51, 61, 12] and d50.q[1][:5].tolist() == [17, 18, 24, 47, 99]
    cases = J.quality_sweep()
    assert [q for _, _, q in cases] == list(range(1, 101))
    every, met, former = set(), set(), set()
    for name, i, q, d in _decoded(lib, cases):
        assert (d.W, d.H) == (48, 48)
        every |= set(d.q.reshape(-1).tolist())
        met |= d.met_divisors()
        if q in FORMER_QUALITIES:
            former |= set(d.q.reshape(-1).tolist())
        if q == 1:                                                     # the clamp: 5000 % of anything is beyond 255
            assert (d.q == 255).all(), name
        if q == 2:                                                     # 2500 %: only Annex K's smallest entry, luma 10, stays below
            assert sorted(d.q.reshape(-1).tolist())[:2] == [250, 255] and d.q[0][2] == 250, name
        if q < 50:
            assert d.q.max() > 121, name                               # the 5000 / quality branch: Annex K's largest entry grew
    assert len(every) == 251 and len(former) == 76
    assert met == every, sorted(every - met)


def test_geometry_cases_fill_every_class():
    sizes = [(fr.shape[2], fr.shape[1]) for _, fr, _ in J.geometry()]
    assert len(set(sizes)) == len(J.SIZES) ** 2 + 2
    members = {c: [s for s in sizes if c in J.geometry_class(*s)] for c in J.GEOMETRY_CLASSES}
    assert all(len(v) >= 2 for v in members.values()), members
    assert {(8, 8), (24, 24), (40, 24), (8, 40)} <= set(members["both"])
    assert (17, 9) in members["right"] and (16, 8) in members["bottom"] and (16, 16) in members["none"]
    assert (J.LIBJPEG_MAX, 1) in sizes and (1, J.LIBJPEG_MAX) in sizes
    # the dummy blocks are in Pillow's file as jccoefct.c writes them: AC zero, DC of the block they copy
    d = J.Decoded(L.lib(), J.pillow_jpeg(J.geometry_frames(8, 8)[0], 90))
    assert d.nblk == 6 and not d.blocks[1:4, 1:].any() and d.blocks[0, 1:].any() and (d.blocks[1:4, 0] == d.blocks[0, 0]).all()


def test_entropy_cases_reach_their_codes(lib):
    dec = {name: d for name, _, _, d in _decoded(lib, J.entropy())}
    d = dec["entropy/dc11_luma"]
    assert max(J.category(v) for v in d.dcdiff[~d.chroma]) == 11
    d = dec["entropy/dc11_chroma"]
    assert 2040 in np.abs(d.dcdiff[d.chroma]) and max(J.category(v) for v in d.dcdiff[d.chroma]) == 11
    d = dec["entropy/ac10"]
    assert np.abs(d.blocks[:, 1:]).max() >= 512 and J.category(np.abs(d.blocks[:, 1:]).max()) == 10
    d = dec["entropy/zrl_and_last"]
    runs = d.zero_runs()
    assert ((runs >= 32) & (runs < 48)).any() and (runs >= 48).any()   # two ZRL in a row, three in a row
    assert (d.blocks[:, 63] != 0).any()                                # a block without EOB
    assert ((d.blocks != 0).sum(axis=1) <= 1).all()                    # (nothing else survived the quantisation)
    d = dec["entropy/many_blocks_per_word"]
    assert (d.q == 255).all() and d.scan_bits < 8 * d.nblk             # fewer than 8 bits a block: 4 or more share a word


def test_last_byte_cases_end_as_named(lib):
    assert J.search_last_byte(lib) == (J.LAST_BYTE_FF_SEEDS, J.LAST_BYTE_PLAIN_SEEDS)
    for name, i, q, d in _decoded(lib, J.last_byte()):
        if "/ff_" in name:
            assert d.data[-4:] == b"\xff\x00\xff\xd9", name
        else:
            assert d.scan_bits % 8 == 0 and d.data[-3] != 0xFF and d.data[-2:] == b"\xff\xd9", name


def test_batch_cases_shrink_and_mix_sizes(lib):
    cases = {name: (fr, q) for name, fr, q in J.batches()}
    assert [cases[k][0].shape[0] for k in ("batches/70", "batches/3_flat", "batches/1")] == [70, 3, 1]
    size = {k: [len(J.pillow_jpeg(f, q)) for f in fr] for k, (fr, q) in cases.items()}
    assert len(set(size["batches/70"])) > 20                           # offsets are sums of many different sizes
    assert max(size["batches/3_flat"]) < min(size["batches/70"][0::3]) # shorter scans than the noise frames in the same slots
    assert min(size["batches/70"]) - HEADER_BYTES < 64                 # scans of a few bytes and of a few hundred, all shorter
    assert 256 < max(size["batches/70"]) - HEADER_BYTES < 1024         # than the 1024 threads of k_jenc_count / k_jenc_write
    assert min(size["batches/333x217"]) - HEADER_BYTES > 4096          # ... and scans of several bytes a thread
    nblk = [6 * ((fr.shape[2] + 15) // 16) * ((fr.shape[1] + 15) // 16) for fr, _ in (cases["batches/333x217"], cases["batches/361x357"])]
    per = [(b + 1023) // 1024 for b in nblk]                           # blocks per thread of k_jenc_scan
    assert nblk == [1764, 3174] and per == [2, 4] and nblk[1] % per[1] != 0     # idle threads; a ragged last thread


def test_emulation_writes_pillows_bytes_on_every_case():
    n = 0
    for name, fr, q in J.all_cases():
        for i, f in enumerate(fr):
            assert J.emulate(f, q) == J.pillow_jpeg(f, q), (name, i, q)
            n += 1
    assert n > 800
    # a strided crop view: the bytes around the frame do not matter
    rng = np.random.default_rng(3)
    for w, h in ((17, 9), (8, 8), (33, 31)):
        big = rng.integers(0, 256, (h + 3, w + 5, 3), dtype=np.uint8)
        view = big[2:2 + h, 3:3 + w]
        assert J.emulate(view, 90) == J.pillow_jpeg(view, 90), (w, h)


def _device_or_host_buffer(nbytes):
    """real memory of the size the call is told about or more, on the GPU where there is one: were a refusal ever missing, the
    launch that follows would stay inside it"""
    try:
        import torch
        if torch.cuda.is_available():
            t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            return t, t.data_ptr()
    except ImportError:
        pass
    a = np.zeros(nbytes, np.uint8)
    return a, a.ctypes.data


def test_encode_refuses_bad_arguments_before_any_launch(lib):
    w, h, n = 24, 17, 2
    ws, pay, fb = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.vbs_jpeg_encode_workspace(w, h, n, C.byref(ws), C.byref(pay), C.byref(fb)) == 0
    assert pay.value == n * fb.value
    keep = [_device_or_host_buffer(x) for x in (n * h * 3 * w + 64, ws.value, pay.value, 8 * n, 4 * n)]
    frames, wsp, payp, offs, sizes = (p for _, p in keep)
    good = dict(n=n, sn=h * 3 * w, sr=3 * w, q=90, wsb=ws.value, payb=pay.value)

    def call(**over):
        a = {**good, **over}
        return lib.vbs_jpeg_encode(frames, a["n"], w, h, a["sn"], a["sr"], a["q"], wsp, a["wsb"], payp, a["payb"], offs, sizes, None)

    for over in (dict(q=0), dict(q=101), dict(sr=3 * w - 1), dict(sn=h * 3 * w - 1), dict(wsb=ws.value - 1), dict(payb=pay.value - 1)):
        assert call(**over) == L.VBS_EINVAL, over                      # (a launch without a GPU would have been VBS_EHIP)
    # one frame needs no frame stride
    ws1, pay1 = C.c_int64(), C.c_int64()
    assert lib.vbs_jpeg_encode_workspace(w, h, 1, C.byref(ws1), C.byref(pay1), None) == 0
    assert call(n=1, sn=0, q=0) == L.VBS_EINVAL and call(n=1, sn=0, wsb=ws1.value - 1) == L.VBS_EINVAL
    del keep
