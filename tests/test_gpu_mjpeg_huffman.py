"""The device entropy path of the Motion-JPEG front end on the GPU (`MjpegDeviceDecoder(entropy="device")`,
csrc/k_jpeg_huff.hip): every BGR byte against Pillow's libjpeg and every coefficient against the host decoder, on the case
lists of `test_mjpeg_device_decode_equals_libjpeg`; table sets that change inside a batch; the frames the device hands back
to the host; `MarkerTracker` end to end.  Bad input meets the decoder's algorithm on a CPU
(tests/test_mjpeg_huffman_host.py), not here."""
import os
import sys

import numpy as np
import pytest

import vbs_amd.synth as S

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import mjpeg_cases as M  # noqa: E402

torch = pytest.importorskip("torch")
pytest.importorskip("PIL")
pytestmark = pytest.mark.gpu


def _device_coefficients(dec, m):
    """what `_huffman_on_device` left on the device, expanded as k_jpeg_idct expands it: [m, nblk, 64] int16"""
    ent, tab, fb = dec._dent.cpu().numpy(), dec._dtab[:m].cpu().numpy(), dec._dfb[:m].cpu().numpy()
    return np.stack([M.expand(ent[int(fb[i]):int(fb[i]) + dec._cap], tab[i]) for i in range(m)])


def _host_coefficients(path, first, m):
    from vbs_amd import _lib as L
    from vbs_amd.video_io import AviReader
    rd = AviReader(path)
    out = []
    for off, size in rd._frames[first:first + m]:
        data = bytes(rd._buf[off:off + size])
        _, info = M.probe(L.lib(), data)
        st, coef = M.host_coefficients(L.lib(), data, info)
        assert st == 0
        out.append(coef)
    return np.stack(out)


def _decode_all(path, batch, threads, check_coefficients=True, **kw):
    from vbs_amd.video_io import AviReader, MjpegDeviceDecoder
    dec = MjpegDeviceDecoder(AviReader(path), torch.device("cuda:0"), batch=batch, threads=threads, entropy="device", **kw)
    got, slot, first = [], 0, 0
    while True:
        m = dec.entropy(slot)
        if not m:
            break
        if dec.entropy_path == "device" and check_coefficients:       # read back before reconstruction
            dec._huffman_on_device(slot, m)
            assert np.array_equal(_device_coefficients(dec, m), _host_coefficients(path, first, m)), (path, first)
        got.append(dec.reconstruct(slot).cpu().numpy().copy())
        slot ^= 1
        first += m
    return dec, np.concatenate(got)


@pytest.mark.parametrize("sub", [0, 1, 2, "gray"])
def test_device_entropy_decode_equals_libjpeg_and_the_host_decoder(tmp_path, sub):
    from vbs_amd.video_io import AviReader, write_avi
    gray = sub == "gray"
    for q, (h, w), opts in M.libjpeg_cases(restart=True):
        fr = M.jpeg_test_frames(h, w, 5, 7 * h + w + q, gray)
        p = str(tmp_path / f"a_{q}_{h}_{w}_{len(opts)}_{list(opts)[:1]}.avi")
        write_avi(p, fr, quality=q, subsampling=0 if gray else sub, **opts)
        n, want = AviReader(p).read_batch(5, threads=1)
        dec, got = _decode_all(p, 4, 2)                                # batches of 4 + 1, both slots
        assert dec.entropy_path == ("host" if any(k.startswith("restart") for k in opts) else "device"), opts
        assert n == 5 and got.shape == want.shape and np.array_equal(got, want), (sub, q, h, w, opts)
        assert dec.host_fallback_frames == 0
    # camera-style frames: no DHT segment (the last clip above: 480x640, quality 70 - the camera's format)
    raw = bytearray(open(p, "rb").read())
    rd = AviReader(p)
    for off, size in rd._frames:
        keep = M.strip_dht(bytes(raw[off:off + size]))
        assert len(keep) < size
        raw[off:off + size] = keep + bytes(size - len(keep))
    p2 = str(tmp_path / "nodht.avi")
    open(p2, "wb").write(bytes(raw))
    n, want = AviReader(p2).read_batch(5, threads=1)
    for sbits in (512, 1024, 2048):
        dec, got = _decode_all(p2, 5, 1, subseq_bits=sbits)
        assert dec.entropy_path == "device" and np.array_equal(got, want) and dec.host_fallback_frames == 0, sbits


def test_table_sets_that_change_inside_a_batch(tmp_path):
    from vbs_amd.video_io import AviReader, AviWriter, write_avi
    fr = M.jpeg_test_frames(61, 83, 6, 3, False)
    p = str(tmp_path / "opt.avi")
    write_avi(p, fr, quality=75, optimize=True)                        # one optimised set per frame
    _, want = AviReader(p).read_batch(6, threads=1)
    dec, got = _decode_all(p, 6, 3)
    assert int(dec._nsets[0].value) == 6 and np.array_equal(got, want)
    # two sets in the first batch of four (frames 2 and 3 share one optimised set), a third in the clip
    q = str(tmp_path / "mixed.avi")
    opt = M.encode(fr[2], quality=75, optimize=True)
    with AviWriter(q, 30.0, 83, 61) as out:
        for d in (M.encode(fr[0], quality=75), M.encode(fr[1], quality=75), opt, opt, M.encode(fr[4], quality=75),
                  M.encode(fr[5], quality=75, optimize=True)):
            out.write(d)
    _, want = AviReader(q).read_batch(6, threads=1)
    dec, got = _decode_all(q, 5, 1)
    assert np.array_equal(got, want)
    dec, got = _decode_all(q, 4, 1, check_coefficients=False)
    assert int(dec._nsets[0].value) == 2 and dec._tset[0][:4].tolist() == [0, 0, 1, 1] and np.array_equal(got, want)


def test_frames_the_device_hands_back(tmp_path):
    """Two fixed inputs (both ran clean through the CPU emulation): a scan cut mid-way is padded by the host decoder as
    before; a frame without a header raises the IOError that names it, with the rows before it kept."""
    import pandas as pd
    from vbs_amd import _lib as L
    from vbs_amd.marker_detection import MarkerTracker
    from vbs_amd.video_io import AviReader, MjpegDeviceDecoder, write_avi
    spec = S.config1()
    frames = S.make_frames(spec, range(6), seed=6, channels=3)
    good = str(tmp_path / "good.avi")
    write_avi(good, frames, quality=70)
    b = bytearray(open(good, "rb").read())
    off, size = AviReader(good)._frames[3]
    b[off:off + size] = M.cut_scan(bytes(b[off:off + size]))
    cut = str(tmp_path / "cut.avi")
    open(cut, "wb").write(bytes(b))
    host = MjpegDeviceDecoder(AviReader(cut), torch.device("cuda:0"), batch=6, threads=2)
    assert host.entropy(0) == 6
    want = host.reconstruct(0).cpu().numpy().copy()
    dec, got = _decode_all(cut, 6, 2, check_coefficients=False)
    assert dec.host_fallback_frames == 1 and int(dec._dstatus[3].item()) == L.MJPEG_SHORT
    assert np.array_equal(got, want)
    # frame 4 of 6 loses its header
    b = bytearray(open(good, "rb").read())
    off, size = AviReader(good)._frames[4]
    b[off:off + 4] = bytes(4)
    bad = str(tmp_path / "bad.avi")
    open(bad, "wb").write(bytes(b))
    cfg = {"crop_ratios": (1 / 8, 1 / 8, 1 / 16, 0), "id_mode": "full", "batch": 2, "mjpeg_entropy": "device"}
    t = MarkerTracker({**cfg, "video_path": bad, "output_dir": str(tmp_path / "ob")})
    with pytest.raises(IOError, match="frame 4"):
        t.process()
    assert t.entropy_path == "device"
    kept = pd.read_csv(t.output_csv)
    assert sorted(kept["frameno"].unique()) == [0, 1, 2, 3]


def test_marker_tracker_csv_is_byte_identical_on_the_device_entropy_path(tmp_path):
    from vbs_amd.marker_detection import MarkerTracker
    from vbs_amd.video_io import write_avi
    try:
        import cv2  # noqa: F401
        pytest.skip("OpenCV present: VideoCapture is used, as in the reference")
    except ImportError:
        pass
    spec = S.config1()
    assert (spec.width, spec.height) == (640, 480)
    frames = S.make_frames(spec, range(9), seed=6, channels=3)
    path = str(tmp_path / "clip.avi")
    write_avi(path, frames, fps=30.0, quality=70)
    cfg = {"video_path": path, "crop_ratios": (1 / 8, 1 / 8, 1 / 16, 0), "num_layers": 5, "min_marker_distance": 20,
           "id_mode": "full", "batch": 4}
    t1 = MarkerTracker({**cfg, "output_dir": str(tmp_path / "o1")})
    t1.process()
    t2 = MarkerTracker({**cfg, "output_dir": str(tmp_path / "o2"), "mjpeg_entropy": "device"})
    t2.process()
    assert (t1.decode_path, t1.entropy_path) == ("device", "host") and (t2.decode_path, t2.entropy_path) == ("device", "device")
    a, b = open(t1.output_csv, "rb").read(), open(t2.output_csv, "rb").read()
    assert len(a) > 1000 and a == b
