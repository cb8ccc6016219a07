#!/usr/bin/env python3
"""Generate the fixtures of the diameter validation tests.

    python tests/golden/make_diameter_golden.py <path to the reference's code/ directory>

(1) tests/golden/diameter_scale.json, by RUNNING THE REFERENCE'S OWN STATEMENTS of `calculate_scale`;
(2) tests/golden/diameter_shot.npz from the reference's `img/diameter_shot.png` (README Figure 5 (a)), see `real_shot`.

In the manner of make_golden.py: `Precision_Validation/DiameterValidation.py` is parsed, the statements of `calculate_scale`
that compute the scale from the corners (:54-71: the two distance loops, the mean, the division) are pulled out by AST -
everything from the first assignment of `distances` to the assignment of `scale`, which leaves out the corner finder and the
prints - compiled on their own and executed with this machine's NumPy.  No reference source text is stored: the file holds the
corner arrays built below and the numbers those statements returned.

Cases: an exact 6x6 grid of 20.5 px pitch; the same rotated by 7 degrees with sub-pixel noise, float32 [36, 1, 2] as
findChessboardCorners returns; a 7x5 pattern (rows != columns) with perspective-like stretch; a 2x2 pattern.
"""
import ast
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diameter_scale.json")


def reference_scale(path):
    fn = next(n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == "calculate_scale")
    names = lambda st: {t.id for t in getattr(st, "targets", []) if isinstance(t, ast.Name)}
    first = next(i for i, st in enumerate(fn.body) if "distances" in names(st))
    last = next(i for i, st in enumerate(fn.body) if "scale" in names(st))
    new = ast.parse("def scale_of(corners, pattern_size, square_mm):\n    pass").body[0]
    new.body = fn.body[first:last + 1] + [ast.parse("return scale").body[0]]
    mod = ast.Module(body=[new], type_ignores=[])
    ast.fix_missing_locations(mod)
    env = {"np": np}
    exec(compile(mod, "<calculate_scale>", "exec"), env)
    return env["scale_of"]


def cases():
    rng = np.random.default_rng(11)
    out = []
    gy, gx = np.mgrid[0:6, 0:6]
    grid = np.stack([100 + 20.5 * gx, 80 + 20.5 * gy], axis=-1).reshape(-1, 2)
    out.append(("exact_6x6", grid.astype(np.float64), (6, 6), 3.0))
    a = np.deg2rad(7.0)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    rot = (grid - grid.mean(0)) @ R.T + grid.mean(0) + rng.normal(0, 0.15, grid.shape)
    out.append(("rotated_noisy_f32", rot.astype(np.float32).reshape(-1, 1, 2), (6, 6), 3.0))
    gy, gx = np.mgrid[0:5, 0:7]
    st = np.stack([40 + 31.0 * gx * (1 + 0.01 * gy), 30 + 29.0 * gy * (1 + 0.015 * gx)], axis=-1).reshape(-1, 2)
    out.append(("stretched_7x5", st.astype(np.float32).reshape(-1, 1, 2), (7, 5), 2.5))
    out.append(("tiny_2x2", np.array([[0, 0], [10, 0], [0, 12], [10, 12]], dtype=np.float32).reshape(-1, 1, 2), (2, 2), 1.0))
    return out


BOARD_SQUARES, SQUARE_MM = 7, 3.0          # the board of the published shot: 7 x 7 squares, "3 mm" written on the figure


def otsu(gray):
    """Otsu's level of a uint8 image: the t that maximises the between-class variance of {<= t} / {> t}."""
    hist = np.bincount(gray.ravel(), minlength=256).astype(np.float64)
    w0 = np.cumsum(hist)
    m0 = np.cumsum(hist * np.arange(256))
    w1, m1 = w0[-1] - w0, m0[-1] - m0
    with np.errstate(divide="ignore", invalid="ignore"):
        var = w0 * w1 * (m0 / w0 - m1 / w1) ** 2
    return int(np.nanargmax(var))


def real_shot(img_path):
    """`img/diameter_shot.png` -> diameter_shot.npz: the decoded pixels (BGR, like cv2.imread) and the two numbers
    `measure_markers` needs, both derived from the 3 mm chessboard IN THE SAME IMAGE by this fixed rule (the reference picks
    its threshold by hand on a slider and finds the corners with cv2; neither can be replayed):
      * gray = the oracle's BGR2GRAY; dark = gray <= Otsu's level of the whole image AND
        max(B, G, R) - min(B, G, R) <= 48 (the lettering and arrows drawn onto the reproduction are saturated red, green and
        blue and reach the board's top edge; the photo itself is neutral); dark is dilated twice with a 3 x 3
        element (in the photo the squares' corners do not quite touch) and the BOARD is the 8-connected component of that
        with the largest bounding-box area; its box is taken back by the 2 px of the dilation on every side;
      * scale [px/mm] = mean(box width, box height) / (BOARD_SQUARES * SQUARE_MM), the box measured edge to edge
        (x1 - x0 + 1): the outermost squares are dark on every side of this board;
      * threshold = the midpoint, rounded down, between the median gray of the board's dark pixels and the median gray of the
        other pixels inside its box (the light squares).
    The image is a downscaled, annotated reproduction (green outlines, blue labels, red lettering): pixels only are stored."""
    from PIL import Image
    from scipy import ndimage
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from oracle import stages as O
    rgb = np.array(Image.open(img_path).convert("RGB"))
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    gray = O.bgr2gray(bgr)
    chroma = bgr.max(axis=2).astype(np.int64) - bgr.min(axis=2)
    dark = (gray <= otsu(gray)) & (chroma <= 48)
    grow = 2
    lab, n = ndimage.label(ndimage.binary_dilation(dark, structure=np.ones((3, 3)), iterations=grow), structure=np.ones((3, 3)))
    boxes = ndimage.find_objects(lab)
    k = max(range(n), key=lambda i: (boxes[i][0].stop - boxes[i][0].start) * (boxes[i][1].stop - boxes[i][1].start))
    ys = slice(boxes[k][0].start + grow, boxes[k][0].stop - grow)
    xs = slice(boxes[k][1].start + grow, boxes[k][1].stop - grow)
    bw, bh = xs.stop - xs.start, ys.stop - ys.start
    scale = 0.5 * (bw + bh) / (BOARD_SQUARES * SQUARE_MM)
    inside, board = gray[ys, xs], dark[ys, xs]
    threshold = int((np.median(inside[board]) + np.median(inside[~board])) // 2)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diameter_shot.npz")
    np.savez_compressed(out, bgr=bgr, threshold=np.int64(threshold), scale=np.float64(scale),
                        board_box=np.array([xs.start, ys.start, xs.stop - 1, ys.stop - 1], dtype=np.int64))
    print(out, bgr.shape, "otsu", otsu(gray), "board", (xs.start, ys.start, bw, bh), "scale", scale, "threshold", threshold,
          os.path.getsize(out), "bytes")


def main():
    real_shot(os.path.join(os.path.dirname(os.path.abspath(sys.argv[1])), "img", "diameter_shot.png"))
    f = reference_scale(os.path.join(sys.argv[1], "Precision_Validation", "DiameterValidation.py"))
    doc = []
    for name, corners, pattern, sq in cases():
        doc.append(dict(name=name, dtype=str(corners.dtype), shape=list(corners.shape), corners=corners.ravel().tolist(),
                        pattern_size=list(pattern), square_mm=sq, scale=float(f(corners, pattern, sq))))
    json.dump(doc, open(OUT, "w"), indent=1)
    print(OUT, [d["scale"] for d in doc])


if __name__ == "__main__":
    main()
