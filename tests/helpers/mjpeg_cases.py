"""Streams and small tools shared by the tests of the device entropy path (tests/test_mjpeg_huffman_host.py on a CPU,
tests/test_gpu_mjpeg_huffman.py on the GPU): the stream variants of `test_mjpeg_entropy_decode_host_half` and of
`test_mjpeg_device_decode_equals_libjpeg`, a NumPy de-stuffing of a scan, the host decoder's compact blocks expanded the way
`k_jpeg_idct` expands them, and the debug library's emulation of the device kernel."""
import ctypes as C
import io
import os

import numpy as np

GUARD = 0xA5A5A5A5


def jpeg_test_frames(h, w, n, seed, gray):
    """(the frames of tests/test_gpu_parity.py::test_mjpeg_device_decode_equals_libjpeg)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        base = 128 + 90 * np.sin(xx / (7.0 + i)) * np.cos(yy / (5.0 + 2 * i))
        img = np.stack([base, 255 - base, 128 + 100 * np.sin((xx + yy) / 11.0)], axis=2)
        img += rng.normal(0, 12 + 8 * i, img.shape)
        img[h // 4:h // 2, w // 3:w // 2] = rng.integers(0, 256, 3)
        img[:6, :9] = 255
        img[-5:, -7:] = 0
        img = np.clip(img, 0, 255).astype(np.uint8)
        out.append(img[:, :, 0] if gray else img)
    return np.stack(out)


def libjpeg_cases(restart=False):
    """(quality, (h, w), Pillow options) of test_mjpeg_device_decode_equals_libjpeg; its restart-interval cases on request"""
    cases = [(q, hw, {}) for q in (35, 75, 95, 100) for hw in ((48, 80), (61, 83), (17, 9))]
    cases += [(q, (h, w), {}) for q in (10, 90) for h in (1, 2, 5, 33) for w in (1, 2, 3, 4, 5)]
    opts = (dict(restart_marker_rows=1), dict(restart_marker_blocks=3), dict(optimize=True))
    cases += [(75, (61, 83), o) for o in opts if restart or "optimize" in o]
    cases += [(70, (480, 640), {})]
    return cases


def strip_dht(data):
    """a camera's frame: no DHT segment, the standard tables are implied"""
    i, keep = 2, bytearray(data[:2])
    while data[i + 1] != 0xDA:
        ln = 2 + ((data[i + 2] << 8) | data[i + 3])
        if data[i + 1] != 0xC4:
            keep += data[i:i + ln]
        i += ln
    return bytes(keep + data[i:])


def encode(img, **opts):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[:, :, ::-1])).save(bio, format="JPEG", **opts)
    return bio.getvalue()


def host_half_streams():
    """the gray 61x83 variants of test_mjpeg_entropy_decode_host_half that have no restart interval"""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:61, 0:83]
    img = np.clip(128 + 80 * np.sin(xx / 6.0) * np.cos(yy / 9.0) + rng.normal(0, 10, (61, 83)), 0, 255).astype(np.uint8)
    out = []
    for opts in ({}, {"optimize": True}, {"quality": 100}, {"no_dht": True}):
        data = encode(img, **{"quality": 80, **{k: v for k, v in opts.items() if k != "no_dht"}})
        out.append((f"host_half {opts}", strip_dht(data) if opts.get("no_dht") else data))
    return out


def variant_streams(frames_per_case=2):
    """[(name, jpeg bytes)]: every variant above without a restart interval, and the last of each sampling without its DHT"""
    out = host_half_streams()
    for sub in (0, 1, 2, "gray"):
        gray = sub == "gray"
        for q, (h, w), opts in libjpeg_cases():
            fr = jpeg_test_frames(h, w, frames_per_case, 7 * h + w + q, gray)
            for k, f in enumerate(fr):
                out.append((f"sub {sub} q {q} {h}x{w} {opts} frame {k}", encode(f, quality=q, subsampling=0 if gray else sub, **opts)))
        out.append((f"sub {sub} no DHT", strip_dht(out[-1][1])))
    return out


def scan_start(data):
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    return i + 2 + ((data[i + 2] << 8) | data[i + 3])


def cut_scan(data):
    """the frame with its scan cut mid-way: EOI there, zeros up to the old length (the chunk keeps its size)"""
    at = scan_start(data) + (len(data) - scan_start(data)) // 2
    return data[:at] + b"\xff\xd9" + bytes(len(data) - at - 2)


def numpy_destuff(data):
    """the scan of a JPEG file: bytes behind the SOS header, FF 00 -> FF, up to the first marker"""
    i = scan_start(data)
    a = np.frombuffer(data, np.uint8)[i:]
    ff = np.flatnonzero(a == 0xFF)
    nxt = np.where(ff + 1 < len(a), a[np.minimum(ff + 1, len(a) - 1)], 1)
    marker = ff[nxt != 0]
    end = int(marker[0]) if len(marker) else len(a)
    a, ff = a[:end], ff[ff < end]
    keep = np.ones(len(a), bool)
    keep[ff + 1] = False
    return a[keep]


class ScanBatch:
    """One `vbs_mjpeg_scan_batch` call over chunks laid out in `buf`, every output between guard words."""

    def __init__(self, lib, buf, offs, sizes, info, threads=2, buf_size=None):
        from vbs_amd import _lib as L
        n = len(offs)
        self.n = n
        good = [int(s) for o, s in zip(offs, sizes) if 0 <= o and 4 <= s <= 2 ** 31 - 1 and o + s <= (len(buf) if buf_size is None else buf_size)]
        cap = sum((s + 16 + 15) // 16 * 16 for s in good)
        self.cap = cap
        g32, g64 = np.uint32(GUARD), np.int64(0x5A5A5A5A5A5A5A5A)
        raw = np.full(cap + 64 + 16, 0xA5, np.uint8)
        at = (-raw.ctypes.data) % 16 + 16                                  # an aligned stage with guard bytes on both sides
        self._raw, self._at = raw, at
        self.stage = raw[at:at + cap]
        self.scan_off = np.full(n + 2, g64, np.int64)
        self.scan_bits = np.full(n + 2, g64, np.int64)
        self.table_set = np.full(n + 2, g32, np.uint32).view(np.int32)
        self.sets = np.full((n + 1) * L.MJPEG_HUFF_SET_BYTES, 0xA5, np.uint8)
        self.n_sets = C.c_int32(-7)
        self.regions = np.full(2 * threads + 2, g64, np.int64)
        self.qt = np.full((n * 3 * 64) + 2, 0xA5A5, np.uint16)
        self.status = np.full(n + 2, g32, np.uint32).view(np.int32)
        self.offs = np.asarray(offs, np.int64)
        self.sizes = np.asarray(sizes, np.int64)
        self.rc = lib.vbs_mjpeg_scan_batch(buf, len(buf) if buf_size is None else buf_size, self.offs.ctypes.data, self.sizes.ctypes.data,
                                           n, info, self.stage.ctypes.data, cap, self.scan_off[1:].ctypes.data,
                                           self.scan_bits[1:].ctypes.data, self.table_set[1:].ctypes.data, self.sets.ctypes.data,
                                           C.byref(self.n_sets), self.regions[1:].ctypes.data, self.qt[1:].ctypes.data,
                                           self.status[1:].ctypes.data, threads)

    def guards_intact(self):
        from vbs_amd import _lib as L
        g64, ns = 0x5A5A5A5A5A5A5A5A, max(int(self.n_sets.value), 0)
        return bool((self._raw[:self._at] == 0xA5).all() and (self._raw[self._at + self.cap:] == 0xA5).all()
                    and all(a[0] == g64 and a[-1] == g64 for a in (self.scan_off, self.scan_bits, self.regions))
                    and all(a.view(np.uint32)[0] == GUARD and a.view(np.uint32)[-1] == GUARD for a in (self.table_set, self.status))
                    and self.qt[0] == 0xA5A5 and self.qt[-1] == 0xA5A5
                    and (self.sets[ns * L.MJPEG_HUFF_SET_BYTES:] == 0xA5).all())

    def frame(self, i):
        """(staged scan bytes incl. guard as an aligned copy, scan_bits, the frame's table set bytes)"""
        from vbs_amd import _lib as L
        off, bits = int(self.scan_off[1 + i]), int(self.scan_bits[1 + i])
        nbytes = bits // 8
        k = int(self.table_set[1 + i])
        return (self.stage[off:off + nbytes + 16], bits, self.sets[k * L.MJPEG_HUFF_SET_BYTES:(k + 1) * L.MJPEG_HUFF_SET_BYTES])


def probe(lib, data):
    info = (C.c_int32 * 8)()
    return lib.vbs_mjpeg_probe(data, len(data), info), info


def host_coefficients(lib, data, info):
    """(status, [nblk, 64] int16): `vbs_mjpeg_entropy_batch` of one frame, its compact blocks expanded as k_jpeg_idct does"""
    cap, nblk = info[6] // 2, info[6] // 64
    ent = np.zeros(cap, np.uint32)
    tab = np.zeros(nblk, np.uint32)
    fb, reg, qt, st = np.zeros(1, np.int64), np.zeros(2, np.int64), np.zeros((1, 3, 64), np.uint16), np.zeros(1, np.int32)
    offs, sizes = np.zeros(1, np.int64), np.array([len(data)], np.int32)
    lib.vbs_mjpeg_entropy_batch(data, offs.ctypes.data, sizes.ctypes.data, 1, info, ent.ctypes.data, tab.ctypes.data, fb.ctypes.data,
                                reg.ctypes.data, qt.ctypes.data, st.ctypes.data, 1)
    if st[0] != 0:
        return int(st[0]), None
    return 0, expand(ent, tab)


def expand(ent, tab):
    """compact words of ONE frame (ent from the frame's first word) -> [nblk, 64] int16"""
    ent, tab = np.asarray(ent).view(np.uint32), np.asarray(tab).view(np.uint32)
    nblk = len(tab)
    coef = np.zeros((nblk, 64), np.int16)
    start, cnt = (tab >> 7).astype(np.int64), (tab & 127).astype(np.int64)
    dense = np.flatnonzero(cnt == 127)
    if len(dense):
        idx = start[dense, None] + np.arange(32)[None, :]
        coef[dense] = ent[idx].view(np.int16).reshape(len(dense), 64)
    sparse = np.flatnonzero(cnt != 127)
    c = cnt[sparse]
    if c.sum():
        blk = np.repeat(sparse, c)
        within = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        e = ent[np.repeat(start[sparse], c) + within]
        coef[blk, (e >> 16).astype(np.int64) & 63] = (e & 0xFFFF).astype(np.uint16).view(np.int16)
    return coef


_dbg = None


def debug_library():
    """libvbs_dbg.so (-DVBS_DEBUG_KNOBS): the only place the emulation of the device decoder exists"""
    global _dbg
    if _dbg is None:
        import vbs_amd._build as B
        path = B.LIB.replace(".so", "_dbg.so")
        if not os.path.exists(path):
            B.build(extra_flags=["-DVBS_DEBUG_KNOBS"], suffix="_dbg")
        _dbg = C.CDLL(path)
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
        _dbg.vbs_dbg_mjpeg_huffman_emulate.restype = i32
        _dbg.vbs_dbg_mjpeg_huffman_emulate.argtypes = [vp, i64, vp, vp, i32, i32, vp, vp]
    return _dbg


def emulate(scan, bits, table_set, info, subseq_bits, chunk_threads):
    """-> (status, [nblk, 64] int16 between guard words checked here, counters[4])"""
    nblk = info[6] // 64
    scan = np.ascontiguousarray(scan)
    buf = np.zeros(len(scan) + 8, np.uint8)
    at = (-buf.ctypes.data) % 4
    buf[at:at + len(scan)] = scan
    coef = np.full(nblk * 64 + 64, 0x5A5A, np.uint16).view(np.int16)
    counters = np.zeros(4, np.int64)
    tset = np.ascontiguousarray(table_set)
    rc = debug_library().vbs_dbg_mjpeg_huffman_emulate(buf[at:].ctypes.data, bits, tset.ctypes.data, info, subseq_bits, chunk_threads,
                                                       coef[32:].ctypes.data, counters.ctypes.data)
    assert (coef[:32].view(np.uint16) == 0x5A5A).all() and (coef[32 + nblk * 64:].view(np.uint16) == 0x5A5A).all(), "guard words"
    return rc, coef[32:32 + nblk * 64].reshape(nblk, 64), counters
