"""The annotated video's host side without a GPU: the OpenCV drawing restatement the device overlay is tested against
(tests/helpers/cv_draw.py), the streaming AVI writer, `write_avi` rebuilt on it, and the encoder's size contract."""
import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cv_draw  # noqa: E402

RED, YELLOW, BLUE = (0, 0, 255), (0, 255, 255), (255, 0, 0)


def _mask(img, color):
    return np.all(img == np.array(color, np.uint8), axis=2)


# ---- cv_draw invariants ---------------------------------------------------------------------------------------------
def test_filled_circle_radius_4_is_symmetric_with_the_midpoint_pixel_count():
    img = np.zeros((21, 21, 3), np.uint8)
    cv_draw.circle(img, (10, 10), 4, RED, -1)
    m = _mask(img, RED)
    assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1]) and np.array_equal(m, m.T)
    # spans of Circle(fill=1) for radius 4 (traced by hand through its (dx, dy) steps (4,0) (3,1) (3,2)): half-widths
    # 0, 2, 3, 3, 4, 3, 3, 2, 0 from the top row down
    assert [int(r.sum()) for r in m[6:15]] == [1, 5, 7, 7, 9, 7, 7, 5, 1]
    assert int(m.sum()) == 49
    r1 = np.zeros((5, 5, 3), np.uint8)
    cv_draw.circle(r1, (2, 2), 1, RED, -1)
    assert np.array_equal(_mask(r1, RED), np.array([[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0],
                                                    [0, 0, 0, 0, 0]], bool))


@pytest.mark.parametrize("p0,p1", [((3, 4), (40, 17)), ((40, 2), (5, 30)), ((20, 3), (21, 38)), ((2, 20), (44, 20)),
                                   ((30, 30), (6, 6)), ((10, 35), (35, 10))])
def test_thick_line_covers_its_bresenham_line(p0, p1):
    img = np.zeros((48, 48, 3), np.uint8)
    cv_draw.line(img, p0, p1, YELLOW, 2)
    m = _mask(img, YELLOW)
    assert all(m[y, x] for x, y in cv_draw.bresenham(p0, p1))
    # and stays within a band of about one and a half pixels around it (the round caps included)
    ys, xs = np.nonzero(m)
    d = np.abs((p1[1] - p0[1]) * xs - (p1[0] - p0[0]) * ys + p1[0] * p0[1] - p1[1] * p0[0]) / np.hypot(p1[0] - p0[0], p1[1] - p0[1])
    assert d.max() <= 2.0


def test_zero_length_arrow_is_two_radius_1_discs():
    a = np.zeros((9, 9, 3), np.uint8)
    cv_draw.arrowed_line(a, (4, 4), (4, 4), RED, 2, tip_length=0.25)
    b = np.zeros((9, 9, 3), np.uint8)
    cv_draw.circle(b, (4, 4), 1, RED, -1)
    cv_draw.circle(b, (4, 4), 1, RED, -1)
    assert np.array_equal(a, b) and int(_mask(a, RED).sum()) == 5


def test_primitives_crossing_every_border_clip_without_wrapping():
    h, w = 30, 40
    prims = [((-3, 5), (12, -6)), ((w - 5, -4), (w + 6, 9)), ((-6, h - 3), (8, h + 5)), ((w + 2, h - 8), (w - 9, h + 3)),
             ((-10, 15), (w + 10, 16)), ((20, -10), (21, h + 10)), ((-50, -50), (-40, -45))]
    for p0, p1 in prims:
        img = np.zeros((h, w, 3), np.uint8)
        cv_draw.line(img, p0, p1, BLUE, 2)
        ys, xs = np.nonzero(_mask(img, BLUE))
        # every painted pixel lies next to the segment (a wrapped index would land on the far side of the frame)
        v = np.array(p1, float) - p0
        t = np.clip(((xs - p0[0]) * v[0] + (ys - p0[1]) * v[1]) / (v @ v), 0, 1)
        assert np.all(np.hypot(xs - (p0[0] + t * v[0]), ys - (p0[1] + t * v[1])) <= 2.5), (p0, p1)
        inside = [q for q in (p0, p1) if 0 <= q[0] < w and 0 <= q[1] < h]
        assert all(_mask(img, BLUE)[q[1], q[0]] for q in inside)
    # discs at the corners and edges: exactly the part of the unclipped disc inside the frame
    big = np.zeros((h + 40, w + 40, 3), np.uint8)
    img = np.zeros((h, w, 3), np.uint8)
    for c in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (2, 15), (w + 3, 4), (-3, -3)]:
        cv_draw.circle(img, c, 4, RED, -1)
        cv_draw.circle(big, (c[0] + 20, c[1] + 20), 4, RED, -1)
    assert np.array_equal(img, big[20:20 + h, 20:20 + w])
    assert _mask(img, RED)[0, 0] and _mask(img, RED)[h - 1, w - 1] and _mask(img, RED)[4, w - 1]


def test_later_primitives_overwrite_earlier_ones():
    img = np.zeros((20, 20, 3), np.uint8)
    cv_draw.circle(img, (10, 10), 4, RED, -1)
    cv_draw.line(img, (2, 10), (18, 10), YELLOW, 2)
    assert tuple(img[10, 10]) == YELLOW and tuple(img[7, 10]) == RED
    cv_draw.circle(img, (10, 10), 4, BLUE, -1)
    assert tuple(img[10, 10]) == BLUE and not _mask(img, RED).any()


def test_draw_frame_paints_in_row_order_and_leaves_the_input():
    frame = np.full((40, 60, 3), 90, np.uint8)
    rows = [(20.7, 20.2, 25.9, 21.4, 14.0, 9.0, 30.0), (26.0, 22.0, 27.3, 22.8, 12.0, 8.0, -60.0)]
    out = cv_draw.draw_frame(frame, rows)
    assert (frame == 90).all() and not np.array_equal(out, frame)
    # the second marker's disc is drawn after the first marker's axes
    assert tuple(out[22, 27]) in (RED, YELLOW, BLUE)
    first = cv_draw.draw_frame(frame, rows[:1])
    second_only = cv_draw.draw_frame(first, rows[1:])
    assert np.array_equal(out, second_only)


# ---- AviWriter ---------------------------------------------------------------------------------------------------------
def _jpegs(n, h=24, w=40, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(b, "JPEG", quality=60 + i)
        out.append(b.getvalue())
    return out


def test_avi_writer_payloads_read_back_identical(tmp_path):
    pytest.importorskip("PIL")
    from vbs_amd.video_io import AviReader, AviWriter, CAP_PROP_FPS, CAP_PROP_FRAME_COUNT
    pays = _jpegs(5)
    p = str(tmp_path / "w.avi")
    wr = AviWriter(p, 25.0, 40, 24)
    assert wr.isOpened()
    for x in pays:
        wr.write(x)
    wr.release()
    assert not wr.isOpened()
    r = AviReader(p)
    assert r.isOpened() and (r.width, r.height) == (40, 24)
    assert r.get(CAP_PROP_FRAME_COUNT) == 5 and r.get(CAP_PROP_FPS) == 25.0
    assert [bytes(r._buf[o:o + s]) for o, s in r._frames] == pays
    ok, fr = r.read()
    assert ok and fr.shape == (24, 40, 3)


def test_avi_writer_patches_count_and_rate_on_release(tmp_path):
    pytest.importorskip("PIL")
    from vbs_amd.video_io import AviWriter
    pays = _jpegs(3)
    p = str(tmp_path / "w.avi")
    wr = AviWriter(p, 12.5, 40, 24)
    for x in pays:
        wr.write(x)
    wr.release()
    b = open(p, "rb").read()
    assert b[:4] == b"RIFF" and struct.unpack_from("<I", b, 4)[0] == len(b) - 8
    avih = b.index(b"avih") + 8
    usec, _, _, _, frames = struct.unpack_from("<5I", b, avih)
    assert usec == 80000 and frames == 3 and struct.unpack_from("<I", b, avih + 28)[0] == max(map(len, pays))
    strh = b.index(b"strh") + 8
    scale, rate = struct.unpack_from("<II", b, strh + 20)
    assert rate / scale == 12.5 and struct.unpack_from("<I", b, strh + 32)[0] == 3
    idx = b.index(b"idx1")
    assert struct.unpack_from("<I", b, idx + 4)[0] == 16 * 3


def test_avi_writer_continues_in_avix_chunks(tmp_path):
    pytest.importorskip("PIL")
    from vbs_amd.video_io import AviReader, AviWriter
    pays = _jpegs(9)
    p = str(tmp_path / "w.avi")
    wr = AviWriter(p, 30.0, 40, 24, riff_bytes=2 * max(map(len, pays)) + 1024)
    for x in pays:
        wr.write(x)
    wr.release()
    b = open(p, "rb").read()
    assert b.count(b"AVIX") >= 2
    pos, riffs = 0, 0
    while pos < len(b):                                        # RIFF chunks back to back, sizes consistent
        assert b[pos:pos + 4] == b"RIFF"
        pos += 8 + struct.unpack_from("<I", b, pos + 4)[0]
        riffs += 1
    assert pos == len(b) and riffs == b.count(b"AVIX") + 1
    r = AviReader(p)
    assert len(r._frames) == 9 and [bytes(r._buf[o:o + s]) for o, s in r._frames] == pays


def _old_write_avi(path, frames, fps=30.0, codec="MJPG", quality=95, subsampling=2, riff_frames=0, **jpeg_options):
    """`write_avi` as it was before it was rebuilt on AviWriter (kept here as the yardstick of its bytes)."""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    gray = frames.ndim == 3
    payloads = []
    if codec.upper() == "MJPG":
        from PIL import Image
        for fr in frames:
            im = Image.fromarray(fr if gray else np.ascontiguousarray(fr[:, :, ::-1]))
            bio = io.BytesIO()
            im.save(bio, format="JPEG", quality=quality, subsampling=0 if gray else subsampling, **jpeg_options)
            payloads.append(bio.getvalue())
        fourcc, bits = b"MJPG", 24
    else:
        bits = 8 if gray else 24
        stride = (w * bits // 8 + 3) & ~3
        for fr in frames:
            rows = np.zeros((h, stride), dtype=np.uint8)
            rows[:, :w * bits // 8] = fr.reshape(h, -1)
            payloads.append(rows[::-1].tobytes())
        fourcc = b"\x00\x00\x00\x00"
    tag = b"00dc" if fourcc == b"MJPG" else b"00db"

    def chunk(cc, data):
        return cc + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")

    def lst(kind, data):
        return b"LIST" + struct.pack("<I", len(data) + 4) + kind + data

    maxsz = max(len(p) for p in payloads) if payloads else 0
    avih = struct.pack("<14I", int(round(1e6 / fps)) if fps else 0, 0, 0, 0x10, n, 0, 1, maxsz, w, h, 0, 0, 0, 0)
    rate, scale = int(round(fps * 1000)), 1000
    strh = b"vids" + fourcc + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, scale, rate, 0, n, maxsz, 0xFFFFFFFF, 0,
                                         0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, bits, fourcc, maxsz, 0, 0, 256 if bits == 8 else 0, 0)
    if bits == 8:
        strf += b"".join(struct.pack("<4B", i, i, i, 0) for i in range(256))
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    first = payloads[:riff_frames] if riff_frames > 0 else payloads
    movi_body, index, off = b"", b"", 4
    for p in first:
        index += tag + struct.pack("<III", 0x10, off, len(p))
        c = chunk(tag, p)
        movi_body += c
        off += len(c)
    body = b"AVI " + hdrl + lst(b"movi", movi_body) + chunk(b"idx1", index)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
        for k in range(len(first), len(payloads), max(riff_frames, 1)):
            ext = b"AVIX" + lst(b"movi", b"".join(chunk(tag, p) for p in payloads[k:k + riff_frames]))
            f.write(b"RIFF" + struct.pack("<I", len(ext)) + ext)


@pytest.mark.parametrize("kw", [{}, {"riff_frames": 2}, {"codec": "DIB"}, {"fps": 25.0, "quality": 70, "subsampling": 0},
                                {"codec": "raw", "riff_frames": 3}, {"optimize": True}])
def test_write_avi_bytes_unchanged_by_the_rebuild(tmp_path, kw):
    pytest.importorskip("PIL")
    from vbs_amd.video_io import write_avi
    rng = np.random.default_rng(4)
    for frames in (rng.integers(0, 256, (5, 9, 17, 3), dtype=np.uint8), rng.integers(0, 256, (4, 10, 13), dtype=np.uint8),
                   np.zeros((0, 8, 8, 3), np.uint8)):
        _old_write_avi(str(tmp_path / "a.avi"), frames, **kw)
        write_avi(str(tmp_path / "b.avi"), frames, **kw)
        assert open(tmp_path / "a.avi", "rb").read() == open(tmp_path / "b.avi", "rb").read()


# ---- the device encoder's size contract (host-only query) -------------------------------------------------------------
def test_jpeg_encode_workspace_reports_the_documented_bound():
    from vbs_amd import _lib as L
    lib = L.lib()
    ws, pay, fb = C.c_int64(), C.c_int64(), C.c_int64()
    for w, h in [(480, 450), (640, 480), (17, 9), (1, 1), (1280, 1024)]:
        assert lib.vbs_jpeg_encode_workspace(w, h, 3, C.byref(ws), C.byref(pay), C.byref(fb)) == 0
        blocks = 6 * ((w + 15) // 16) * ((h + 15) // 16)
        bound = L.JPEG_HEADER_BYTES + 2 * ((blocks * L.JPEG_BLOCK_BITS_MAX + 7) // 8) + 2
        assert fb.value == bound and pay.value == 3 * bound and ws.value > blocks * 3 * 128
    assert lib.vbs_jpeg_encode_workspace(0, 10, 1, C.byref(ws), C.byref(pay), C.byref(fb)) == L.VBS_EINVAL
    assert lib.vbs_jpeg_encode_workspace(10, 10, -1, C.byref(ws), C.byref(pay), C.byref(fb)) == L.VBS_EINVAL
    # invalid arguments are refused before anything touches a device
    assert lib.vbs_jpeg_encode(None, 1, 16, 16, 768, 48, 0, None, 0, None, 0, None, None, None) == L.VBS_EINVAL
    assert lib.vbs_draw_tracking(None, 1, 0, 16, 0, 48, None, 0, None, None, 0, None, None, None) == L.VBS_EINVAL


def test_tracker_config_keys_default_off(tmp_path):
    """`write_video` absent: the tracker has no video state and `output_video` is only a path, as before."""
    from vbs_amd.marker_detection import MarkerTracker
    np.save(tmp_path / "c.npy", np.zeros((1, 16, 16, 3), np.uint8))
    t = MarkerTracker({"video_path": str(tmp_path / "c.npy"), "output_dir": str(tmp_path / "o"), "crop_ratios": (0, 0, 0, 0)})
    assert t.output_video.endswith("c_tracked.avi") and getattr(t, "_video", None) is None
    assert not os.path.exists(t.output_video)
