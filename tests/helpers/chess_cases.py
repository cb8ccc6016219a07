"""Rendered chessboards with known inner corners for the chessboard tests: a board seen through a homography plus radial
distortion (k1, k2), area-sampled 8 x 8 per pixel, fixed seeds.  `cases()` builds every case once per process.

A case: name, gray uint8 [H,W] (a view for the strided crop), pattern (pw, ph) asked for, found (what the helper must say), truth
float64 [pw*ph,2] in the finder's output order (None when not found).  The cases keep every walk decision of the helper away from
ties - over every seed tried, `ties` of chess_oracle is 0, which tests/test_chess_host.py asserts; the equidistant first steps of
a seed on a regular board (`step_ties`) cannot be avoided with integer peaks and go to the lowest index."""
import functools

import numpy as np

import chess_oracle as CO

SS = 8                                        # sub-samples per pixel and axis
DARK, LIGHT, GROUND = 40, 215, 190


def _board_to_image(bx, by, Hm, k1, k2, size):
    """Board coordinates (squares) -> distorted pixel positions."""
    w, h = size
    f, cx, cy = float(max(w, h)), (w - 1) * 0.5, (h - 1) * 0.5
    d = Hm[2, 0] * bx + Hm[2, 1] * by + Hm[2, 2]
    ux = (Hm[0, 0] * bx + Hm[0, 1] * by + Hm[0, 2]) / d
    uy = (Hm[1, 0] * bx + Hm[1, 1] * by + Hm[1, 2]) / d
    xn, yn = (ux - cx) / f, (uy - cy) / f     # the renderer maps distorted -> undistorted; invert it by fixed point
    xd, yd = xn.copy(), yn.copy()
    for _ in range(50):
        r2 = xd * xd + yd * yd
        s = 1.0 + k1 * r2 + k2 * r2 * r2
        xd, yd = xn / s, yn / s
    return xd * f + cx, yd * f + cy


def render(size, squares, Hm, k1=0.0, k2=0.0, invert=False, cover=None, noise=0.0, seed=0):
    """gray uint8 [h,w] of a board of squares = (nx, ny) squares whose board -> pixel homography is Hm; and the inner corners
    float64 [ny-1, nx-1, 2].  cover = (i, j): a ground-coloured disc over inner corner (i, j)."""
    w, h = size
    nx, ny = squares
    f, cx, cy = float(max(w, h)), (w - 1) * 0.5, (h - 1) * 0.5
    sub = (np.arange(SS) + 0.5) / SS - 0.5
    xs = (np.arange(w)[:, None] + sub[None, :]).reshape(-1)
    ys = (np.arange(h)[:, None] + sub[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    xd, yd = (X - cx) / f, (Y - cy) / f
    r2 = xd * xd + yd * yd
    s = 1.0 + k1 * r2 + k2 * r2 * r2
    ux, uy = xd * s * f + cx, yd * s * f + cy
    Hi = np.linalg.inv(Hm)
    d = Hi[2, 0] * ux + Hi[2, 1] * uy + Hi[2, 2]
    bx = (Hi[0, 0] * ux + Hi[0, 1] * uy + Hi[0, 2]) / d
    by = (Hi[1, 0] * ux + Hi[1, 1] * uy + Hi[1, 2]) / d
    inside = (bx >= 0) & (bx < nx) & (by >= 0) & (by < ny)
    dark = ((np.floor(bx).astype(np.int64) + np.floor(by).astype(np.int64)) & 1) == 0
    lo, hi = (LIGHT, DARK) if invert else (DARK, LIGHT)
    val = np.where(inside, np.where(dark, lo, hi), GROUND).astype(np.float64)
    if cover is not None:
        val[(bx - cover[0] - 1) ** 2 + (by - cover[1] - 1) ** 2 < 0.45 ** 2] = GROUND
    img = val.reshape(h, SS, w, SS).mean(axis=(1, 3))
    if noise:
        img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
    gi, gj = np.meshgrid(np.arange(1, nx, dtype=np.float64), np.arange(1, ny, dtype=np.float64))
    tx, ty = _board_to_image(gi, gj, Hm, k1, k2, size)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), np.stack([tx, ty], axis=2)


def similarity(scale, angle_deg, tx, ty):
    a = np.deg2rad(angle_deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), tx], [scale * np.sin(a), scale * np.cos(a), ty], [0, 0, 1.0]])


def truth_in_output_order(corners, pattern):
    """The true corners [ny-1,nx-1,2] in the finder's order for `pattern`: rows of pw, positive handedness, corner 0 the one with
    the smallest (y, x) of its ROUNDED position (the finder orders integer peaks)."""
    pw, ph = pattern
    best = None
    for k in range(4):
        q = np.rot90(corners, -k, axes=(0, 1))
        if q.shape[:2] != (ph, pw):
            continue
        key = (int(np.rint(q[0, 0, 1])), int(np.rint(q[0, 0, 0])))
        if best is None or key < best[0]:
            best = (key, q.reshape(-1, 2))
    return best[1]


def _case(name, gray, pattern, found, corners):
    truth = truth_in_output_order(corners, pattern) if found else None
    return dict(name=name, gray=gray, pattern=pattern, found=found, truth=truth)


@functools.lru_cache(maxsize=1)
def cases():
    out = []
    g, c = render((160, 128), (5, 4), similarity(14.0, 0.0, 44.3, 35.6))
    out.append(_case("board_4x3", g, (4, 3), 1, c))
    size = (203, 157)
    flat = similarity(20.0, 0.0, 6.0, 6.0)                       # 7 x 7 squares of 20 px, the board 6 px from two edges
    g, c = render(size, (7, 7), flat)
    out.append(_case("board_6x6_edge", g, (6, 6), 1, c))
    rot = similarity(16.0, 30.0, 82.2, 2.4)
    g, c = render(size, (7, 7), rot)
    out.append(_case("rotated_30", g, (6, 6), 1, c))
    persp = similarity(17.0, 8.0, 38.0, 8.0)
    persp[2, :2] = (0.010, 0.015)
    g_persp, c_persp = render(size, (7, 7), persp, k1=-0.25, k2=0.08)
    out.append(_case("perspective_radial", g_persp, (6, 6), 1, c_persp))
    g, c = render(size, (7, 7), rot, invert=True)
    out.append(_case("inverted", g, (6, 6), 1, c))
    g, c = render(size, (7, 7), rot, noise=3.0, seed=11)
    out.append(_case("noise_sigma3", g, (6, 6), 1, c))
    g, c = render(size, (8, 5), similarity(17.0, -20.0, 30.5, 72.3))
    out.append(_case("asymmetric_7x4", g, (7, 4), 1, c))
    out.append(_case("uniform", np.full((157, 203), 128, dtype=np.uint8), (6, 6), 0, None))
    g, c = render(size, (7, 7), rot, cover=(2, 3))
    out.append(_case("covered_corner", g, (6, 6), 0, None))
    g, c = render(size, (8, 8), similarity(15.0, 10.0, 50.0, 10.0))
    out.append(_case("board_7x7_asked_6x6", g, (6, 6), 0, None))
    big = np.full((240, 320), GROUND, dtype=np.uint8)
    big[40:40 + 157, 70:70 + 203] = g_persp                      # the perspective case again, as a view with the frame's stride
    out.append(_case("strided_crop", big[40:40 + 157, 70:70 + 203], (6, 6), 1, c_persp))
    return tuple(out)


BATCH = ("rotated_30", "uniform", "perspective_radial", "covered_corner", "noise_sigma3")   # found, not, found, not, found


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def batch():
    """The batch of 5 that mixes found and not-found frames: (frames uint8 [5,157,203], cases)."""
    cs = [by_name(n) for n in BATCH]
    return np.stack([np.ascontiguousarray(c["gray"]) for c in cs]), cs


@functools.lru_cache(maxsize=1)
def helper_results():
    """The helper on every case, computed once: name -> dict (find_chessboard_corners(want=True) plus `refined`, the (11,11)
    refinement of the finder's corners, and its iteration counts)."""
    res = {}
    for c in cases():
        r = CO.find_chessboard_corners(c["gray"], c["pattern"], want=True)
        if r["found"]:
            r["refined"], r["refined_iters"] = CO.corner_subpix(c["gray"], r["corners"])
        res[c["name"]] = r
    return res


# Largest and rms distance (px) of the helper's corners to truth, per case: "finder" = window (2,2), 15 iterations, eps 0.1;
# "refined" = then window (11,11), 30 iterations, eps 0.001.  The reference's own numbers on these inputs, measured on the CPU by
# tests/test_chess_host.py::test_accuracy_record (which prints them); the GPU test adds eps to the per-corner distances.
HELPER_ERR_PX = {
    "board_4x3": dict(finder=(0.0487, 0.0487), refined=(0.0341, 0.0341)),   # peaks (0.5000, 0.5000)
    "board_6x6_edge": dict(finder=(0.0000, 0.0000), refined=(0.0000, 0.0000)),   # peaks (0.0000, 0.0000)
    "rotated_30": dict(finder=(0.1064, 0.0601), refined=(0.0675, 0.0449)),   # peaks (0.6674, 0.4056)
    "perspective_radial": dict(finder=(0.1439, 0.0826), refined=(0.5025, 0.1287)),   # peaks (0.7018, 0.4029)
    "inverted": dict(finder=(0.1064, 0.0602), refined=(0.0690, 0.0448)),   # peaks (0.6674, 0.4056)
    "noise_sigma3": dict(finder=(0.1139, 0.0660), refined=(0.0960, 0.0499)),   # peaks (0.6674, 0.4056)
    "asymmetric_7x4": dict(finder=(0.0941, 0.0704), refined=(0.0587, 0.0388)),   # peaks (1.3975, 0.6048)
    "strided_crop": dict(finder=(0.1439, 0.0826), refined=(0.5025, 0.1287)),   # peaks (0.7018, 0.4029)
}
