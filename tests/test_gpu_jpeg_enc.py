"""The device JPEG encoder (`vbs_jpeg_encode`, csrc/k_jpeg_enc.hip) against Pillow byte for byte on the cases of
tests/helpers/jpeg_enc_cases.py: every quality, every kind of frame edge, the rare codes, the last byte of the scan, batches
that shrink on one encoder - and, by direct calls between guard bytes, that the kernels stay inside the workspace and the
payload they were given and read nothing of the bytes around a frame.  tests/test_jpeg_enc_host.py shows on a CPU that each
case reaches the place it is named after.  Byte equality throughout, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("PIL")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import jpeg_enc_cases as J  # noqa: E402

GUARD = 4096


def _embedded(frames, seed):
    """the frames as a strided crop view of a larger device buffer of random bytes"""
    n, h, w, _ = frames.shape
    rng = np.random.default_rng(seed)
    big = torch.from_numpy(rng.integers(0, 256, (n, h + 3, w + 5, 3), dtype=np.uint8)).cuda()
    big[:, 2:2 + h, 3:3 + w] = torch.from_numpy(frames).cuda()
    return big[:, 2:2 + h, 3:3 + w]


def _check(enc, name, frames, q, seed=1):
    """one batch through `enc` -> number of files compared"""
    before = enc.downloaded_bytes
    files = enc.fetch(enc.encode(_embedded(frames, seed)))
    assert len(files) == len(frames), name
    for i, f in enumerate(files):
        want = J.pillow_jpeg(frames[i], q)
        assert len(f) == len(want) and f == want, (name, i, q, len(f), len(want))
        assert len(f) <= enc.frame_bound, (name, i)
    assert enc.downloaded_bytes - before == sum(map(len, files)) + 4 * len(files), name
    return len(files)


def _run(cases):
    from vbs_amd.video_io import MjpegDeviceEncoder
    n = 0
    for name, frames, q in cases:
        enc = MjpegDeviceEncoder("cuda:0", frames.shape[2], frames.shape[1], batch=len(frames), quality=q)
        n += _check(enc, name, frames, q)
    return n


def test_every_quality_equals_pillow():
    assert _run(J.quality_sweep()) == 400


def test_every_frame_edge_equals_pillow():
    assert _run(J.geometry()) == 2 * len(J.SIZES) ** 2 + 2


def test_rare_codes_and_last_bytes_equal_pillow():
    assert _run(J.entropy()) == 5
    assert _run(J.last_byte()) == 4


def test_one_encoder_over_shrinking_batches_equals_pillow():
    from vbs_amd.video_io import MjpegDeviceEncoder
    cases = J.batches()
    enc = MjpegDeviceEncoder("cuda:0", 24, 24, batch=70, quality=J.BATCH_QUALITY)
    n = 0
    for k, (name, frames, q) in enumerate(cases[:3]):                  # 70 frames, 3 flat ones over their stale words, then 1
        n += _check(enc, name, frames, q, seed=k)
    # and both payload slots again, so that each has held a long batch before a short one
    for k, (name, frames, q) in enumerate(cases[:3]):
        n += _check(enc, name + " again", frames, q, seed=10 + k)
    assert n == 2 * 74
    assert _run(cases[3:]) == 3


def _direct(frames, q, seed):
    """`vbs_jpeg_encode` on a crop view, workspace and payload each followed by GUARD bytes of a fixed pattern -> (files, the
    device's offsets, sizes)"""
    n, h, w, _ = frames.shape
    lib = L.lib()
    ws, pay, fb = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.vbs_jpeg_encode_workspace(w, h, n, C.byref(ws), C.byref(pay), C.byref(fb)) == 0
    pattern = torch.arange(GUARD, dtype=torch.int32, device="cuda").mul(37).add(11).to(torch.uint8)
    rng = np.random.default_rng(seed)
    # the workspace starts dirty: nothing may depend on what an earlier call left in it
    wsb = torch.from_numpy(rng.integers(0, 256, ws.value + GUARD, dtype=np.uint8)).cuda()
    payb = torch.full((pay.value + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    wsb[ws.value:] = pattern
    payb[pay.value:] = pattern
    offs = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    sizes = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    view = _embedded(frames, seed)
    rc = lib.vbs_jpeg_encode(view.data_ptr(), n, w, h, view.stride(0), view.stride(1), q, wsb.data_ptr(), ws.value, payb.data_ptr(),
                             pay.value, offs[1:].data_ptr(), sizes[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(wsb[ws.value:], pattern), "bytes behind the workspace changed"
    assert torch.equal(payb[pay.value:], pattern), "bytes behind the payload changed"
    offs, sizes = offs.cpu().numpy(), sizes.cpu().numpy()
    assert offs[0] == -7 and offs[-1] == -7 and sizes[0] == -7 and sizes[-1] == -7, "offsets / sizes written beyond n entries"
    offs, sizes = offs[1:-1], sizes[1:-1]
    host = payb[:pay.value].cpu().numpy()
    total = int(sizes.sum())
    assert (host[total:] == 0x5A).all(), "payload written behind the last file"
    return [host[o:o + s].tobytes() for o, s in zip(offs, sizes)], offs, sizes


DIRECT_SIZES = {"none": (32, 16), "right": (17, 9), "bottom": (31, 24), "both": (40, 24), "w1": (1, 33), "h1": (31, 1),
                "oddw": (7, 16), "oddh": (16, 15)}


def test_direct_calls_stay_inside_workspace_and_payload():
    assert set(DIRECT_SIZES) == set(J.GEOMETRY_CLASSES)
    for cls, (w, h) in DIRECT_SIZES.items():
        assert cls in J.geometry_class(w, h), cls
        frames = np.concatenate([J.geometry_frames(w, h), J.geometry_frames(w, h, seed=99)[:1]])
        files, offs, sizes = _direct(frames, 90, seed=5)
        want = [J.pillow_jpeg(f, 90) for f in frames]
        lens = np.array([len(x) for x in want])
        assert sizes.tolist() == lens.tolist() and offs.tolist() == (np.cumsum(lens) - lens).tolist(), cls
        assert files == want, cls


def test_bytes_around_the_frame_do_not_reach_the_file():
    for cls, (w, h) in (("both", (24, 8)), ("odd", (33, 31))):
        frames = J.geometry_frames(w, h)
        a, b = (_direct(frames, 90, seed=s)[0] for s in (21, 22))
        assert a == b, cls
        assert a == [J.pillow_jpeg(f, 90) for f in frames], cls
