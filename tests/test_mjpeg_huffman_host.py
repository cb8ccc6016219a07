"""The device entropy path of the Motion-JPEG front end, as far as a CPU can check it: the host half that stages the scans
(`vbs_mjpeg_scan_batch`), and the ALGORITHM of the device kernel - the decode step of csrc/jpeg_huff_common.h that
k_jpeg_huff.hip compiles, run through the same five phases with loops in place of threads (`vbs_dbg_mjpeg_huffman_emulate`,
debug library only) - against the host decoder, on valid and on mutated streams.  Exact equality throughout: there is no
tolerance in an entropy decoder."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vbs_amd.synth as S

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import mjpeg_cases as M  # noqa: E402

pytest.importorskip("PIL")


@pytest.fixture(scope="module")
def lib():
    from vbs_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def streams():
    return M.variant_streams()


def test_scan_batch_stages_destuffed_scans_and_numbers_the_table_sets(lib, streams):
    from vbs_amd import _lib as L
    assert L.MJPEG_HUFF_SET_BYTES == 6 * (4 * (18 + 17 + 17) + 2 * 512 + 256)
    saw_stuffing = 0
    for name, data in streams:
        rc, info = M.probe(lib, data)
        assert rc == 0 and info[5] == 0, name
        # the frame twice and a copy with other tables, in one buffer, on two threads
        other = M.strip_dht(data) if b"\xff\xc4" in data else data
        buf = data + other + data
        offs = [0, len(data), len(data) + len(other)]
        sb = M.ScanBatch(lib, buf, offs, [len(data), len(other), len(data)], info, threads=2)
        assert sb.rc == 0 and not sb.status[1:4].any() and sb.guards_intact(), name
        want = M.numpy_destuff(data)
        saw_stuffing += b"\xff\x00" in data[M.scan_start(data):]
        for i in (0, 2):
            scan, bits, _ = sb.frame(i)
            assert bits == 8 * len(want) and np.array_equal(scan[:len(want)], want), (name, i)
            assert not scan[len(want):].any() and int(sb.scan_off[1 + i]) % L.MJPEG_SCAN_ALIGN == 0, (name, i)
        assert sb.table_set[1] == sb.table_set[3], name
        same_tables = M.ScanBatch(lib, data + data, [0, len(data)], [len(data)] * 2, info, threads=1)
        assert same_tables.n_sets.value == 1 and list(same_tables.table_set[1:3]) == [0, 0]
        if other is not data and not np.array_equal(sb.frame(0)[2], sb.frame(1)[2]):
            assert sb.n_sets.value == 2 and sb.table_set[1] != sb.table_set[2], name
        else:
            assert sb.n_sets.value == 1, name
        # regions: what the threads report covers every staged scan
        reg = sb.regions[1:5].reshape(2, 2)
        for i in range(3):
            off, nbytes = int(sb.scan_off[1 + i]), int(sb.scan_bits[1 + i]) // 8
            assert any(a <= off and off + nbytes + L.MJPEG_SCAN_GUARD <= a + u for a, u in reg), name
    assert saw_stuffing > 10                                           # (FF 00 pairs did occur)
    # optimised tables differ from the standard ones: the two-set branch above was taken
    name, data = next((n, d) for n, d in streams if "optimize" in n and "sub 2" in n)
    _, info = M.probe(lib, data)
    other = M.strip_dht(data)
    sb = M.ScanBatch(lib, data + other, [0, len(data)], [len(data), len(other)], info)
    assert sb.n_sets.value == 2 and list(sb.table_set[1:3]) == [0, 1]


def test_scan_batch_refuses_chunks_outside_the_mapping_for_that_frame_only(lib, streams):
    name, data = streams[0]
    _, info = M.probe(lib, data)
    n = len(data)
    buf = data + data
    for offs, sizes, bad, buf_size in (
            ([0, n + 1], [n, n], 1, None),                             # offset + size beyond buf_size
            ([0, 0], [n, 2 * n + 1], 1, None),                         # size beyond buf_size
            ([-1, n], [n, n], 0, None),                                # negative offset
            ([0, n], [2 ** 31, n], 0, None),                           # size above INT32_MAX
            ([0, n], [n, 3], 1, None),                                 # size below 4
            ([0, n], [n, n], 1, 2 * n - 1),                            # the mapping is shorter than the chunk list says
            ([0, 2 ** 62], [n, 2 ** 62], 1, None)):                    # offset + size would wrap
        sb = M.ScanBatch(lib, buf, offs, sizes, info, threads=2, buf_size=buf_size)
        from vbs_amd import _lib as L
        assert sb.rc == 1 and sb.status[1 + bad] == L.VBS_EINVAL and sb.status[2 - bad] == 0, (offs, sizes)
        assert sb.guards_intact()
        scan, bits, _ = sb.frame(1 - bad)
        want = M.numpy_destuff(data)
        assert bits == 8 * len(want) and np.array_equal(scan[:len(want)], want)
    # a stage too small for the good chunks: the call is refused, nothing is written
    sb = M.ScanBatch(lib, buf, [0, n], [n, n], info)
    assert sb.rc == 0
    st = np.zeros(2, np.int32)
    ns = C.c_int32(0)
    rc = lib.vbs_mjpeg_scan_batch(buf, len(buf), sb.offs.ctypes.data, sb.sizes.ctypes.data, 2, info, sb.stage.ctypes.data, sb.cap - 16,
                                  sb.scan_off[1:].ctypes.data, sb.scan_bits[1:].ctypes.data, sb.table_set[1:].ctypes.data,
                                  sb.sets.ctypes.data, C.byref(ns), sb.regions[1:].ctypes.data, sb.qt[1:].ctypes.data, st.ctypes.data, 2)
    assert rc < 0


def test_emulated_device_decode_equals_the_host_decoder(lib, streams):
    """S = 512 / 1024 / 2048, chunks of 4 subsequences (the chunk-to-chunk carry, on small images too) and of 256."""
    multi_chunk = 0
    for name, data in streams:
        _, info = M.probe(lib, data)
        st, want = M.host_coefficients(lib, data, info)
        assert st == 0, name
        sb = M.ScanBatch(lib, data, [0], [len(data)], info, threads=1)
        scan, bits, tset = sb.frame(0)
        for sbits in (512, 1024, 2048):
            for chunk in (4, 256):
                rc, got, counters = M.emulate(scan, bits, tset, info, sbits, chunk)
                assert rc == 0 and np.array_equal(got, want), (name, sbits, chunk, rc)
                multi_chunk += counters[0] > 1
    assert multi_chunk > 100


def test_emulated_device_decode_on_corrupt_streams(lib):
    """The five mutation kinds of `test_mjpeg_host_half_survives_corrupt_streams`, 700 per base stream (its restart-interval
    stream replaced by a second 4:2:0 one): the emulation returns one of its three codes, VBS_OK only where the host
    decoder also says VBS_OK and the coefficients are equal; guard words intact (checked in the helper)."""
    from vbs_amd import _lib as L
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:40, 0:56]
    img = np.clip(np.stack([128 + 90 * np.sin(xx / 5.0), 128 + 90 * np.cos(yy / 4.0), 3.0 * (xx + yy)], axis=2)
                  + rng.normal(0, 15, (40, 56, 3)), 0, 255).astype(np.uint8)
    img2 = M.jpeg_test_frames(61, 83, 1, 11, False)[0]
    from PIL import Image
    import io
    bases = []
    for im, opts in ((img, dict(subsampling=2)), (img, dict(subsampling=0)), (img2[:, :, ::-1], dict(subsampling=2)), (img[:, :, 0], {})):
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(im)).save(bio, format="JPEG", quality=85, **opts)
        bases.append(bio.getvalue())
    checked = staged = ok = short = invalid = 0
    for bi, base in enumerate(bases):
        rc, info = M.probe(lib, base)
        assert rc == 0
        sos = base.index(b"\xff\xda")
        for it in range(700):
            d = bytearray(base)
            kind = it % 5
            if kind == 0:
                for _ in range(int(rng.integers(1, 12))):
                    d[int(rng.integers(2, len(d)))] = int(rng.integers(0, 256))
            elif kind == 1:
                for _ in range(int(rng.integers(1, 6))):
                    d[int(rng.integers(2, sos + 12))] = int(rng.integers(0, 256))
            elif kind == 2:
                d = d[:int(rng.integers(2, len(d)))]
            elif kind == 3:
                for _ in range(int(rng.integers(1, 5))):
                    k = int(rng.integers(sos, len(d) - 1))
                    d[k] = 0xFF
                    d[k + 1] = int(rng.choice([0x00, 0xD0, 0xD3, 0xD9, 0xC4, 0xFF]))
            else:
                k = bytes(d).index(b"\xff\xc4") + 5
                d[k + int(rng.integers(0, 4))] = int(rng.integers(3, 256))
            d = bytes(d)
            checked += 1
            sb = M.ScanBatch(lib, d, [0], [len(d)], info, threads=1)
            assert sb.rc in (0, 1) and sb.guards_intact()
            if sb.rc == 1 or len(d) < 4:
                continue
            staged += 1
            scan, bits, tset = sb.frame(0)
            sbits, chunk = (512, 1024, 2048)[it % 3], (4, 256)[(it // 3) % 2]
            rc, got, _ = M.emulate(scan, bits, tset, info, sbits, chunk)
            assert rc in (L.VBS_OK, L.MJPEG_SHORT, L.VBS_EINVAL), (bi, it, rc)
            if rc == L.VBS_OK:
                st, want = M.host_coefficients(lib, d, info)
                assert st == 0 and np.array_equal(got, want), (bi, it)
                ok += 1
            short += rc == L.MJPEG_SHORT
            invalid += rc == L.VBS_EINVAL
    print(f"checked {checked}, staged {staged}: device OK {ok}, short {short}, invalid {invalid}")
    assert checked == 2800 and 200 < ok < 2700 and short > 0 and invalid > 0      # every outcome occurs


def test_the_fixed_inputs_of_the_gpu_fallback_test_run_clean_through_the_emulation(lib, tmp_path):
    """tests/test_gpu_mjpeg_huffman.py::test_frames_the_device_hands_back feeds the GPU one scan cut mid-way: here the same
    frame goes through the emulation first - it returns, reports the scan short, and the host decoder pads it."""
    from vbs_amd import _lib as L
    from vbs_amd.video_io import AviReader, write_avi
    spec = S.config1()
    frames = S.make_frames(spec, range(6), seed=6, channels=3)
    good = str(tmp_path / "good.avi")
    write_avi(good, frames, quality=70)
    rd = AviReader(good)
    for k, (off, size) in enumerate(rd._frames):
        data = bytes(rd._buf[off:off + size])
        if k == 3:
            data = M.cut_scan(data)
        _, info = M.probe(lib, data)
        sb = M.ScanBatch(lib, data, [0], [len(data)], info, threads=1)
        assert sb.rc == 0
        scan, bits, tset = sb.frame(0)
        for sbits in (512, 1024, 2048):
            rc, got, _ = M.emulate(scan, bits, tset, info, sbits, 256)
            st, want = M.host_coefficients(lib, data, info)
            assert st == 0 and rc == (L.MJPEG_SHORT if k == 3 else 0), (k, sbits, rc)
            assert k == 3 or np.array_equal(got, want)


def test_decoder_class_keeps_restart_interval_clips_on_the_host_path(tmp_path):
    from vbs_amd.video_io import AviReader, MjpegDeviceDecoder, write_avi
    spec = S.config1()
    frames = S.make_frames(spec, range(5), seed=2, channels=3)
    p, q = str(tmp_path / "rst.avi"), str(tmp_path / "plain.avi")
    write_avi(p, frames, quality=70, restart_marker_rows=1)
    write_avi(q, frames, quality=70)
    dec = MjpegDeviceDecoder(AviReader(p), "cpu", batch=3, threads=2, entropy="device")
    assert dec.entropy_path == "host"
    assert [dec.entropy(0), dec.entropy(1), dec.entropy(0)] == [3, 2, 0] and int(dec._regions[0][1]) > 0
    assert MjpegDeviceDecoder(AviReader(q), "cpu", batch=3).entropy_path == "host"           # the default
    dec = MjpegDeviceDecoder(AviReader(q), "cpu", batch=3, threads=2, entropy="device")
    assert dec.entropy_path == "device"
    assert [dec.entropy(0), dec.entropy(1), dec.entropy(0)] == [3, 2, 0]                      # (host buffers only: the staging)
    assert int(dec._sbits[1][1]) > 0 and int(dec._nsets[1].value) == 1
    with pytest.raises(ValueError):
        MjpegDeviceDecoder(AviReader(q), "cpu", batch=3, entropy="gpu")
    # a frame without a header is still an IOError naming it
    b = bytearray(open(q, "rb").read())
    off, size = AviReader(q)._frames[4]
    b[off:off + 4] = bytes(4)
    bad = str(tmp_path / "bad.avi")
    open(bad, "wb").write(bytes(b))
    dec = MjpegDeviceDecoder(AviReader(bad), "cpu", batch=4, threads=3, entropy="device")
    assert dec.entropy(0) == 4
    with pytest.raises(IOError, match="frame 4"):
        dec.entropy(1)
