"""Ragged inputs for the diameter validation (test infrastructure): gray frames whose blurred, thresholded mask holds what the
smooth shots of `diameter_cases` never do - 1-px lines, diagonal necks, spurs, single pixels, components inside each other's
bounding boxes, boxes of exactly VBS_DIAM_MAX_EXTENT and one more, and component counts at and one over the limits.

The entry takes gray frames, so every case is a frame plus its threshold; the mask is ALWAYS taken from the helper
(`diameter_oracle.blur5_u8` + `threshold_inv`), never assumed from the drawing.  tests/test_diameter_edges_host.py states, on the
CPU, what each of these frames must contain for the GPU tests to mean anything.
"""
import functools

import numpy as np
from scipy import ndimage

import diameter_oracle as D

GEOMS = ((96, 130), (70, 200))          # H x W: widths that are no multiple of 64, three and four words per row
SMALLEST = (64, 128)                    # the smallest frame vbs_create takes
KINDS = ("white", "binary", "coarse", "sparse")
SEEDS = dict(white=(0, 1, 3), binary=(0, 1, 2), coarse=(0, 1, 2), sparse=(0, 1, 2))    # chosen on the CPU: see the host test
SMALL = (("white", 0), ("binary", 0), ("coarse", 0), ("sparse", 3))                     # kinds and seeds at SMALLEST
LINE_THRESHOLD = 190                    # a 1-px line at 0 on 255 stays one pixel wide at 186..190 (see line_frames)
SHAPE_THRESHOLD = 127
DOT_THRESHOLD = 170
EVERY = (-1.0, -1.0)                    # (min_area, min_circularity): every contour with a perimeter survives
MID = (20.25, 0.3)                      # areas are multiples of 1/2: 20.25 cannot tie


# ---- noise -------------------------------------------------------------------------------------------------------------
def white(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8), 127


def binary(H, W, seed):
    return ((np.random.default_rng(seed).random((H, W)) < 0.5) * 255).astype(np.uint8), 127


def coarse(H, W, seed):
    b = (np.random.default_rng(seed).random(((H + 1) // 2, (W + 1) // 2)) < 0.5) * 255
    return np.repeat(np.repeat(b, 2, axis=0), 2, axis=1)[:H, :W].astype(np.uint8), 127


def sparse(H, W, seed):
    return np.where(np.random.default_rng(seed).random((H, W)) < 0.12, 0, 255).astype(np.uint8), 190


GENERATORS = dict(white=white, binary=binary, coarse=coarse, sparse=sparse)


@functools.lru_cache(maxsize=None)
def noise(kind, geom, seed):
    """(frame, threshold); the frame is shared between the tests and must not be written to."""
    g, thr = GENERATORS[kind](geom[0], geom[1], seed)
    g.setflags(write=False)
    return g, thr


def noise_cases(geoms=GEOMS, kinds=KINDS):
    """[(name, frame, threshold)] of every kind, geometry and seed."""
    return [(f"{k}-{g[0]}x{g[1]}-s{s}", *noise(k, g, s)) for k in kinds for g in geoms for s in SEEDS[k]]


def small_noise_cases():
    return [(f"{k}-{SMALLEST[0]}x{SMALLEST[1]}-s{s}", *noise(k, SMALLEST, s)) for k, s in SMALL]


# ---- hand-made frames: drawn at 0 on 255 ---------------------------------------------------------------------------------
def _blank(H, W):
    return np.full((H, W), 255, np.uint8)


@functools.lru_cache(maxsize=None)
def line_frames():
    """Three 70 x 200 frames of 1-px lines, threshold LINE_THRESHOLD.  Blurred, the pixels of a horizontal or vertical line drop
    to 255 * 10 / 16 = 159 and their neighbours to 255 * 12 / 16 = 191; those of a diagonal line to 255 * 186 / 256 = 185 and
    their 4-neighbours to 255 * 200 / 256 = 199: at 186..190 the mask of the horizontal and vertical frames is the drawing,
    and a diagonal line loses its end pixels (202) or, at the image border, gains what the reflected border adds (the host
    test asserts all of it).
    Returns [(name, frame, threshold, drawing)]."""
    H, W = GEOMS[1]
    out = []
    # horizontal: across x = 63/64 and 127/128; on row 0 from column 0, on the last row up to the last column; a run of
    # exactly one word (64..127), one that ends at bit 63 and one that starts at bit 0
    d = np.zeros((H, W), bool)
    d[0, 0:140] = True
    d[H - 1, 50:W] = True
    d[8, 64:128] = True
    d[16, 20:64] = True
    d[24, 64:90] = True
    d[32, 60:132] = True
    d[40, 126:130] = True                                     # (a line of 2 px would blur away: 195 > 190)
    d[44, 128:150] = True
    d[48, 62:66] = True
    d[56, 0:W] = True
    out.append(("horizontal", d))
    # vertical: ON columns 0, 63, 64, 127, 128 and the last; from row 0 and down to the last row
    d = np.zeros((H, W), bool)
    d[0:H, 0] = True
    d[0:30, 63] = True
    d[36:H, 64] = True
    d[0:31, 127] = True
    d[37:H, 128] = True
    d[0:H, W - 1] = True
    d[5:60, 96] = True
    out.append(("vertical", d))
    # diagonal, both ways: from the corner (0, 0) down across x = 63/64 to the last row; from the last column's top down-left
    # across x = 128/127; short ones astride each seam
    d = np.zeros((H, W), bool)
    for k in range(H):
        d[k, k] = True                                        # (0, 0) .. (69, 69)
        d[k, W - 1 - k] = True                                # (199, 0) .. (130, 69)
    for k in range(12):
        d[10 + k, 100 + k + 22] = True                        # (122, 10) .. (133, 21): across 127/128, down-right
        d[30 + k, 70 - k] = True                              # (70, 30) .. (59, 41): across 64/63, down-left
        d[50 + k, 133 - k] = True                             # (133, 50) .. (122, 61): across 128/127, down-left
    out.append(("diagonal", d))
    frames = []
    for name, d in out:
        g = np.where(d, 0, 255).astype(np.uint8)
        g.setflags(write=False)
        frames.append((name, g, LINE_THRESHOLD, d))
    return frames


def _rect(g, x0, y0, x1, y1):
    g[y0:y1 + 1, x0:x1 + 1] = 0


@functools.lru_cache(maxsize=None)
def interleaved_frames():
    """96 x 130 frames, threshold SHAPE_THRESHOLD, of 6-px strokes whose bounding boxes hold pixels of another component.
    A blurred straight edge keeps its place at 127 (the edge pixel drops to 255 * 5 / 16 = 80, the one outside to 175; only the
    corner pixels are lost), so the boxes are the drawn ones; the host test asserts them.

    c_blob  : a 'C' open to the right over x = 64..127 with a blob inside its opening and a bar that pokes into the opening
              from beyond the box (cut at x1 = 127, x1 & 63 == 63, mid-run); a mirrored one open to the left over
              x = 64..123 whose bar is cut at x0 = 64 (x0 & 63 == 0) mid-run.
    nested_l: an 'L' and a turned 'L' hooked into each other, and a small 'L' inside the large one's box.
    plus    : a '+' over x = 64..127 with bars in the corners of its box - OUTSIDE its enclosing circle, cut mid-run at x0 and
              x1.  Rectangular strokes like 'C' and 'L' reach the corners of their boxes, so their enclosing circle covers the
              box and a foreign pixel inside it could never change the circle; the '+' is the frame on which it would.
    Returns [(name, frame, threshold, {label: (x0, y0, x1, y1)})]."""
    H, W = GEOMS[0]
    out = []
    g = _blank(H, W)
    _rect(g, 64, 4, 127, 9); _rect(g, 64, 4, 69, 40); _rect(g, 64, 35, 127, 40)             # 'C' open to the right
    _rect(g, 80, 14, 90, 22)                                                                    # the blob in its opening
    _rect(g, 100, 26, 129, 30)                                                                  # bar from the right, cut at 127
    _rect(g, 64, 50, 123, 55); _rect(g, 118, 50, 123, 90); _rect(g, 64, 85, 123, 90)          # 'C' open to the left
    _rect(g, 20, 67, 100, 72)                                                                   # bar from the left, cut at 64
    out.append(("c_blob", g, dict(c_right=(64, 4, 127, 40), blob=(80, 14, 90, 22), bar_right=(100, 26, 129, 30),
                                  c_left=(64, 50, 123, 90), bar_left=(20, 67, 100, 72))))
    g = _blank(H, W)
    _rect(g, 10, 5, 15, 70); _rect(g, 10, 65, 100, 70)                                          # 'L'
    _rect(g, 30, 15, 127, 20); _rect(g, 122, 15, 127, 90)                                       # turned 'L', hooked into it
    _rect(g, 30, 30, 35, 55); _rect(g, 30, 50, 64, 55)                                          # small 'L' inside both boxes
    out.append(("nested_l", g, dict(l_big=(10, 5, 100, 70), l_turned=(30, 15, 127, 90), l_small=(30, 30, 64, 55))))
    g = _blank(H, W)
    _rect(g, 64, 45, 127, 51); _rect(g, 93, 10, 99, 86)                                         # '+'
    _rect(g, 40, 12, 75, 17)                                                                    # corner bar, cut at x0 = 64
    _rect(g, 115, 80, 129, 85)                                                                  # corner bar, cut at x1 = 127
    _rect(g, 120, 12, 126, 16); _rect(g, 66, 78, 70, 84)                                        # blobs in the other corners
    out.append(("plus", g, dict(plus=(64, 10, 127, 86), bar_a=(40, 12, 75, 17), bar_b=(115, 80, 129, 85),
                                blob_a=(120, 12, 126, 16), blob_b=(66, 78, 70, 84))))
    res = []
    for name, g, boxes in out:
        g.setflags(write=False)
        res.append((name, g, SHAPE_THRESHOLD, boxes))
    return res


EXTENT_GEOM = (530, 640)


BANDS = dict(at_limit=((513, 512), (512, 512)),        # name: (drawn box, box of the helper's chain), width x height: the
             wide=((516, 300), (513, 300)),            # blur takes the band's corner pixels away, more of them the flatter
             tall=((301, 513), (300, 513)))            # it lies (the host test asserts the second column)


@functools.lru_cache(maxsize=None)
def band(name, thick=5):
    """A `thick`-px band from the top left to the bottom right of a box, and a small square next to it so that the frame has a
    second component.  530 x 640, SHAPE_THRESHOLD."""
    bw, bh = BANDS[name][0]
    H, W = EXTENT_GEOM
    g = _blank(H, W)
    x0, y0 = 70, 8
    for r in range(bh):
        xa = x0 + (r * (bw - thick)) // (bh - 1)
        g[y0 + r, xa:xa + thick] = 0
    _rect(g, 20, 400, 29, 409)
    g.setflags(write=False)
    return g, SHAPE_THRESHOLD


DOT_GEOM = (128, 256)


@functools.lru_cache(maxsize=None)
def dots(n, shift=0):
    """n dark dots at pitch 6 on 128 x 256, threshold DOT_THRESHOLD: 2 x 2 pixels, every fifth one 3 x 3 (were all diameters
    equal, their standard deviation would be rounding noise and no relative comparison of it could hold)."""
    H, W = DOT_GEOM
    g = _blank(H, W)
    cells = [(x, y) for y in range(2 + shift, H - 4, 6) for x in range(2 + shift, W - 4, 6)]
    assert n <= len(cells)
    for i, (x, y) in enumerate(cells[:n]):
        s = 3 if i % 5 == 4 else 2
        g[y:y + s, x:x + s] = 0
    g.setflags(write=False)
    return g, DOT_THRESHOLD


# ---- what a frame contains, by the helper alone ---------------------------------------------------------------------------
def mask_of(gray, thr):
    return D.threshold_inv(D.blur5_u8(gray), thr)


def neighbourhood_codes(mask):
    """The 8-neighbourhood codes (bit d = neighbour in chain direction d, 0 = E, 1 = NE, .. 7 = SE, y down; outside the image
    is background) that occur on foreground pixels of the hole-filled mask: what k_diam_measure's gather has to produce."""
    fg = D.fill_holes(mask)
    H, W = fg.shape
    p = np.zeros((H + 2, W + 2), np.int64)
    p[1:-1, 1:-1] = fg
    DX, DY = (1, 1, 0, -1, -1, -1, 0, 1), (0, -1, -1, -1, 0, 1, 1, 1)
    pat = np.zeros((H, W), np.int64)
    for d in range(8):
        pat |= p[1 + DY[d]:1 + DY[d] + H, 1 + DX[d]:1 + DX[d] + W] << d
    return set(int(v) for v in np.unique(pat[fg]))


def components(mask):
    """Per 8-connected component of the hole-filled mask, keyed by its first pixel (x, y) in raster order:
    dict(box=(x0, y0, x1, y1), own=[(x, y)], foreign=[(x, y) of other components inside the box])."""
    lab, n = D.component_pixels(mask)
    out = {}
    for i, sl in enumerate(ndimage.find_objects(lab)):
        sub = lab[sl]
        oy, ox = np.nonzero(sub == i + 1)
        fy, fx = np.nonzero((sub != 0) & (sub != i + 1))
        y0, x0 = sl[0].start, sl[1].start
        own = sorted(zip((oy + y0).tolist(), (ox + x0).tolist()))
        out[(own[0][1], own[0][0])] = dict(box=(x0, y0, sl[1].stop - 1, sl[0].stop - 1), own=[(x, y) for y, x in own],
                                           foreign=list(zip((fx + x0).tolist(), (fy + y0).tolist())))
    return out


def capacity(mask):
    """(runs of the mask, runs of its complement, 4-connected background components): what the labelling kernel has to hold
    (VBS_RUN_CAP runs per mask, 1024 components of the background) before the diameter kernels see a frame."""
    def runs(m):
        p = np.zeros((m.shape[0], m.shape[1] + 1), bool)
        p[:, 1:] = m
        return int((p[:, 1:] & ~p[:, :-1]).sum())
    return runs(mask), runs(~mask), int(ndimage.label(~mask)[1])


def measured_frames():
    """Every frame the GPU tests expect to be MEASURED (not reported): [(name, frame, threshold, max_markers of its engine)]."""
    out = [(n, g, t, 512) for n, g, t in noise_cases() + small_noise_cases()]
    out += [("lines-" + n, g, t, 512) for n, g, t, _ in line_frames()]
    out += [("boxes-" + n, g, t, 512) for n, g, t, _ in interleaved_frames()]
    out += [("band-at_limit", *band("at_limit"), 512)]
    out += [("dots-512", *dots(512), 1024), ("dots-64", *dots(64), 1024), ("dots-64", *dots(64), 64),
            ("dots-64-shifted", *dots(64, 1), 64)]
    return out
