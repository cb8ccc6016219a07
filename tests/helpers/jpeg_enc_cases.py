"""Cases that hold the device JPEG encoder (csrc/k_jpeg_enc.hip) to Pillow byte for byte at the places its one generic test
does not reach, and the predicates that say a case really reaches its place.  A case is (name, BGR frames [n, H, W, 3] uint8,
quality); the reference is always Pillow's `Image.save(buf, "JPEG", quality=q)`.  Every predicate reads PILLOW'S file - its
coefficients through the project's host entropy decoder (`mjpeg_cases.host_coefficients`), its tables through
`Image.open(...).quantization`, its Huffman code lengths from its own DHT segments - never the encoder under test, so a
Pillow upgrade that moves a case off its edge fails the predicate, not the comparison.  Shared by tests/test_jpeg_enc_host.py
(CPU: predicates, the debug library's emulation) and tests/test_gpu_jpeg_enc.py (the kernels)."""
import ctypes as C
import functools
import io

import numpy as np

import mjpeg_cases as M

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40)
LIBJPEG_MAX = 65500                                     # JPEG_MAX_DIMENSION: beyond it there is no reference
GEOMETRY_CLASSES = ("none", "right", "bottom", "both", "w1", "h1", "oddw", "oddh")
# seeds the searches below ended on (Pillow 12.2 / libjpeg-turbo); the predicates fail if they stop holding
LAST_BYTE_FF_SEEDS = (12, 54)
LAST_BYTE_PLAIN_SEEDS = (7, 16)


def pillow_jpeg(bgr, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, "JPEG", quality=q)
    return b.getvalue()


# ---- what Pillow's file holds -------------------------------------------------------------------------------------------
def quant_tables(data):
    """[2][64] divisors in NATURAL order, as Pillow hands them out (test_jpeg_enc_host.py pins that convention at quality 50)"""
    from PIL import Image
    q = Image.open(io.BytesIO(data)).quantization
    return np.stack([np.asarray(q[c], np.int64) for c in (0, 1)])


def _code_lengths(data):
    """{(class, id): [256] code length by symbol} from the file's DHT segments"""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xC4:
            p = i + 4
            while p < i + 2 + ln:
                tc = data[p]
                bits = data[p + 1:p + 17]
                lens, v = np.zeros(256, np.int64), p + 17
                for l in range(16):
                    for _ in range(bits[l]):
                        lens[data[v]] = l + 1
                        v += 1
                out[(tc >> 4, tc & 15)] = lens
                p = v
        i += 2 + ln
    return out


class Decoded:
    """Pillow's file taken apart: `blocks` [nblk, 64] quantised coefficients in ZIGZAG order and SCAN order (per MCU: four
    luma blocks, Cb, Cr; dummy blocks included), `chroma` [nblk] bool, `dcdiff` [nblk] as coded, `q` [2][64] natural order,
    `scan_bits` the length of the entropy-coded segment before padding and stuffing."""

    def __init__(self, lib, data):
        rc, info = M.probe(lib, data)
        assert rc == 0 and info[2] == 3 and info[3] == 2 and info[4] == 2, "not a 4:2:0 baseline file"
        st, coef = M.host_coefficients(lib, data, info)
        assert st == 0
        self.W, self.H = info[0], info[1]
        mx, my = (self.W + 15) // 16, (self.H + 15) // 16
        ny = 4 * mx * my
        Y = coef[:ny].reshape(2 * my, 2 * mx, 64)
        Cb = coef[ny:ny + mx * my].reshape(my, mx, 64)
        Cr = coef[ny + mx * my:].reshape(my, mx, 64)
        Ym = Y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        mcu = np.concatenate([Ym, Cb[:, :, None], Cr[:, :, None]], axis=2)            # [my, mx, 6, 64] natural order
        self.blocks = mcu.reshape(-1, 64)[:, ZIGZAG].astype(np.int64)
        self.nblk = len(self.blocks)
        self.chroma = np.tile(np.array([0, 0, 0, 0, 1, 1], bool), mx * my)
        dc = mcu[..., 0].reshape(-1, 6).astype(np.int64)
        diff = np.zeros_like(dc)
        yflat = dc[:, :4].reshape(-1)
        diff[:, :4] = np.diff(yflat, prepend=0).reshape(-1, 4)
        diff[:, 4] = np.diff(dc[:, 4], prepend=0)
        diff[:, 5] = np.diff(dc[:, 5], prepend=0)
        self.dcdiff = diff.reshape(-1)
        self.q = quant_tables(data)
        self.data = data
        self._lens = _code_lengths(data)

    def met_divisors(self):
        """divisor values that sit, in either table, where a quantised coefficient is non-zero"""
        out = set()
        for c in (0, 1):
            nz = (self.blocks[self.chroma == bool(c)] != 0).any(axis=0)                # by zigzag position
            out |= set(self.q[c][ZIGZAG][nz].tolist())
        return out

    def zero_runs(self):
        """the longest run of zeros in front of a non-zero AC coefficient, per block"""
        out = np.zeros(self.nblk, np.int64)
        for b, zz in enumerate(self.blocks):
            nz = np.flatnonzero(zz[1:]) + 1
            if len(nz):
                out[b] = int(np.diff(np.concatenate([[0], nz])).max()) - 1
        return out

    @functools.cached_property
    def scan_bits(self):
        cat = lambda v: int(abs(int(v))).bit_length()                                  # noqa: E731
        total = 0
        for b, zz in enumerate(self.blocks):
            c = int(self.chroma[b])
            dcl, acl = self._lens[(0, c)], self._lens[(1, c)]
            s = cat(self.dcdiff[b])
            total += int(dcl[s]) + s
            r = 0
            for v in zz[1:]:
                if v == 0:
                    r += 1
                    continue
                while r > 15:
                    total += int(acl[0xF0])
                    r -= 16
                s = cat(v)
                total += int(acl[(r << 4) | s]) + s
                r = 0
            if r:
                total += int(acl[0])
        return total


def category(v):
    return int(abs(int(v))).bit_length()


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _gradient(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    d = (xx + yy) * 255.0 / max(w + h - 2, 1)
    img = np.stack([d, 255 - d, (3 * (xx + 2 * yy)) % 256], axis=2) + rng.integers(-6, 7, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _cells(rng, h, w):
    """2x2-pixel cells of saturated random colours: chroma as violent as luma after the 2x2 downsampling"""
    c = rng.integers(0, 2, ((h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8) * 255
    return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]


def _low_contrast(rng, h, w):
    return (128 + rng.integers(-3, 4, (h, w, 3))).astype(np.uint8)


def _salt(rng, h, w):
    """black and white pixels: the largest high-frequency luma there is (the big divisors of the low qualities sit there)"""
    return np.repeat(rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * 255, 3, axis=2)


def quality_sweep():
    """one case per quality 1..100: noise (luma), saturated 2x2 cells (chroma), +-3 about mid-grey (the rounding points of small
    divisors), black / white pixels (luma large enough for the largest divisors), 48x48"""
    out = []
    for q in range(1, 101):
        rng = np.random.default_rng(1000 + q)
        out.append((f"sweep/q{q}", np.stack([_noise(rng, 48, 48), _cells(rng, 48, 48), _low_contrast(rng, 48, 48), _salt(rng, 48, 48)]), q))
    return out


def geometry_class(w, h):
    """which of GEOMETRY_CLASSES a size belongs to (a size may be in several)"""
    right, bottom = ((w + 7) // 8) & 1, ((h + 7) // 8) & 1                             # the last MCU has a dummy column / row
    cls = {("none", "right", "bottom", "both")[right + 2 * bottom]}
    if w == 1:
        cls.add("w1")
    if h == 1:
        cls.add("h1")
    if w & 1:
        cls.add("oddw")
    if h & 1:
        cls.add("oddh")
    return cls


def geometry_frames(w, h, seed=None):
    rng = np.random.default_rng(7919 * w + h if seed is None else seed)
    return np.stack([_noise(rng, h, w), _gradient(rng, h, w)])


def geometry():
    out = [(f"geometry/{w}x{h}", geometry_frames(w, h), 90) for h in SIZES for w in SIZES]
    for w, h in ((LIBJPEG_MAX, 1), (1, LIBJPEG_MAX)):
        out.append((f"geometry/{w}x{h}", geometry_frames(w, h)[1:], 90))
    return out


def _gray(a):
    return np.repeat(np.clip(np.rint(a), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def _basis(u, v):
    x = np.arange(8)
    return np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))    # [y, x]


def _single_coefficient_frame(ks, amp):
    """gray blocks side by side, block i = mid-grey + the basis function of zigzag index ks[i] (an inverse DCT of that one
    coefficient), padded to whole MCUs with mid-grey"""
    h, w = 16, 16 * ((len(ks) + 1) // 2)
    img = np.full((h, w), 128.0)
    for i, k in enumerate(ks):
        nat = int(ZIGZAG[k])
        img[0:8, 8 * i:8 * i + 8] += amp * _basis(nat % 8, nat // 8)
    return _gray(img)


def entropy():
    out = []
    chk = (np.add.outer(np.arange(32) // 8, np.arange(32) // 8) & 1) * 255.0
    out.append(("entropy/dc11_luma", _gray(chk)[None], 100))
    by = np.zeros((32, 32, 3), np.uint8)
    sel = (np.add.outer(np.arange(32) // 16, np.arange(32) // 16) & 1).astype(bool)
    by[sel] = (255, 0, 0)                                                              # BGR: pure blue
    by[~sel] = (0, 255, 255)                                                           # pure yellow
    out.append(("entropy/dc11_chroma", by[None], 100))
    b44 = np.tile((_basis(4, 4) > 0) * 255.0, (2, 2))
    out.append(("entropy/ac10", _gray(b44)[None], 100))
    # one coefficient at zigzag k = k - 1 zeros in front of it: 33, 40, 48 take two ZRL (runs 32, 39, 47), 49, 50, 63 three (runs
    # 48, 49, 62), 63 leaves no EOB.  Quality 75: rounding the pixels leaves the other coefficients far below half their divisors
    out.append(("entropy/zrl_and_last", _single_coefficient_frame([40, 50, 63, 33, 48, 49], 120.0)[None], 75))
    out.append(("entropy/many_blocks_per_word", np.full((1, 64, 64, 3), 200, np.uint8), 1))
    return out


def _last_byte_frames(upto):
    rng = np.random.default_rng(0)
    return [rng.integers(0, 256, (16, 16, 3), dtype=np.uint8) for _ in range(upto + 1)]


def search_last_byte(lib, limit=200):
    """the seed search the fixed seeds came from: (first two draws whose file ends FF 00 FF D9, first two whose scan ends on a
    byte boundary in a byte that is not FF)"""
    ff, plain = [], []
    for i, f in enumerate(_last_byte_frames(limit)):
        data = pillow_jpeg(f, 90)
        if data[-4:] == b"\xff\x00\xff\xd9":
            ff.append(i)
        elif data[-3] != 0xFF and Decoded(lib, data).scan_bits % 8 == 0:
            plain.append(i)
    return tuple(ff[:2]), tuple(plain[:2])


def last_byte():
    fr = _last_byte_frames(max(LAST_BYTE_FF_SEEDS + LAST_BYTE_PLAIN_SEEDS))
    return ([(f"last_byte/ff_{s}", fr[s][None], 90) for s in LAST_BYTE_FF_SEEDS]
            + [(f"last_byte/plain_{s}", fr[s][None], 90) for s in LAST_BYTE_PLAIN_SEEDS])


BATCH_QUALITY = 85


def batches():
    """the first three run on ONE encoder, in this order: long scans, then shorter ones over their stale words, then n = 1; then
    two sizes of more blocks than k_jenc_scan has threads: 1764 (two a thread, the last 142 threads idle; 6 mcux mcuy is even, so
    no frame of up to 2048 blocks splits raggedly) and 3174 (four a thread, the last thread with two)"""
    rng = np.random.default_rng(24)
    kinds = (_noise, lambda r, h, w: np.full((h, w, 3), r.integers(0, 256, 3), np.uint8), _gradient)
    many = np.stack([kinds[i % 3](rng, 24, 24) for i in range(70)])
    flat = np.stack([np.full((24, 24, 3), v, np.uint8) for v in (0, 128, 255)])
    return [("batches/70", many, BATCH_QUALITY), ("batches/3_flat", flat, BATCH_QUALITY), ("batches/1", many[3:4], BATCH_QUALITY),
            ("batches/333x217", geometry_frames(333, 217, seed=5), BATCH_QUALITY),
            ("batches/361x357", geometry_frames(361, 357, seed=6)[:1], BATCH_QUALITY)]


def all_cases():
    return quality_sweep() + geometry() + entropy() + last_byte() + batches()


# ---- the debug library's host emulation ---------------------------------------------------------------------------------------
def emulate(frame, q):
    """one BGR frame [H, W, 3] (any row stride) -> the file `vbs_dbg_jpeg_encode_emulate` writes, between guard bytes"""
    dbg = M.debug_library()
    fn = dbg.vbs_dbg_jpeg_encode_emulate
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    from vbs_amd import _lib as L
    h, w = frame.shape[:2]
    assert frame.dtype == np.uint8 and frame.strides[2] == 1 and frame.strides[1] == 3
    bound = C.c_int64()
    assert L.lib().vbs_jpeg_encode_workspace(w, h, 1, None, None, C.byref(bound)) == 0
    out = np.full(bound.value + 64, 0xA5, np.uint8)
    size = C.c_int64(-1)
    rc = fn(frame.ctypes.data, w, h, frame.strides[0], q, out[32:].ctypes.data, bound.value, C.byref(size))
    assert rc == 0, rc
    assert (out[:32] == 0xA5).all() and (out[32 + size.value:] == 0xA5).all(), "the emulation wrote outside its file"
    return out[32:32 + size.value].tobytes()
