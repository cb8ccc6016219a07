"""What the GPU tests of the marker diameter validation assert about one frame of device output (test infrastructure, shared
by tests/test_gpu_diameter.py and tests/test_gpu_diameter_edges.py): the device against the sequential helper
`diameter_oracle.py`.

Exact: the thresholded mask bits, the survivor set and its order, area2, n_axis, n_diag, first pixel, pixel count and box.
Enclosing circle: the circle through the REPORTED support points, rebuilt in exact arithmetic, contains every pixel centre of the
component and equals the exact minimum as fractions; float64 columns and the statistics within REL of float64 Python / NumPy.
The threshold is the case module's (`diameter_cases.THRESHOLD`).
"""
import math

import numpy as np
import torch

import diameter_cases as K
import diameter_oracle as D

REL = 1e-12
MIN_AREA, MIN_CIRC = 100, 0.85


def close(a, b, rel=REL):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def helper_frame(gray, scale, offset=0.0, min_area=MIN_AREA, min_circ=MIN_CIRC):
    mask, allc, surv = D.measure_gray(gray, K.THRESHOLD, scale, min_area, min_circ, offset)
    for c in allc:                                           # the condition on the INPUTS (helper alone)
        assert abs(c["circularity"] - min_circ) > 1e-9 and c["area"] != min_area
    return mask, allc, surv


def check_frame(gray, rec, count, stats, mask_bits, scale, offset=0.0, min_area=MIN_AREA, min_circ=MIN_CIRC, expect=None):
    """One frame of device output against the helper.  Returns the helper's survivors."""
    H, W = gray.shape
    mask, allc, surv = helper_frame(gray, scale, offset, min_area, min_circ)
    if expect is not None:
        expect(allc, surv)
    if mask_bits is not None:
        assert np.array_equal(mask_bits.view(np.uint64), D.pack_bits(mask)), "thresholded mask bits differ"
    print(f"frame {H}x{W}: helper {len(allc)} contours, {len(surv)} survivors; device count {count}")
    assert count == len(surv)
    lab, _ = D.component_pixels(mask)
    for i, (r, c) in enumerate(zip(rec[:count], surv)):
        fx, fy = c["first"]
        # ---- exact integers, in the reference's contour order
        assert int(r[9]) == fy * W + fx, (i, "first pixel / order")
        assert (int(r[22]), int(r[7]), int(r[8])) == (c["area2"], c["n_axis"], c["n_diag"]), (i, "area2, n_axis, n_diag")
        ys, xs = np.nonzero(lab == lab[fy, fx])
        assert int(r[17]) == len(xs) and (int(r[18]), int(r[19]), int(r[20]), int(r[21])) == (xs.min(), ys.min(), xs.max(), ys.max())
        # ---- float64 from the integers
        assert close(r[4], c["area"]) and close(r[5], c["perimeter"]) and close(r[6], c["circularity"]), (i, r[4:7])
        # ---- the circle: rebuilt exactly from the reported support points
        ns = int(r[10])
        assert ns in (1, 2, 3)
        support = [(int(r[11 + 2 * k]), int(r[12 + 2 * k])) for k in range(ns)]
        cx, cy, r2 = D.circle_through(support)
        d2 = (xs.astype(object) - cx) ** 2 + (ys.astype(object) - cy) ** 2
        assert max(d2) <= r2, (i, "a pixel centre lies outside the reported circle")
        assert r2 == c["mec"][2], (i, "not the minimum circle", r2, c["mec"][2])
        assert (cx, cy) == c["mec"][:2]                       # (the minimum circle is unique)
        assert close(r[2], c["radius"]) and close(r[0], c["cx"]) and close(r[1], c["cy"]), (i, r[:3], c["radius"])
        assert close(r[3], c["diameter_mm"]), (i, r[3], c["diameter_mm"])
    d = np.array([c["diameter_mm"] for c in surv], dtype=np.float64)
    assert stats[0] == len(surv)
    if len(surv):
        assert close(stats[1], float(np.mean(d))) and close(stats[3], d.min()) and close(stats[4], d.max())
        assert close(stats[2], float(np.std(d))), (stats[2], float(np.std(d)))
    else:
        assert all(math.isnan(v) for v in stats[1:])
    return surv


def run(eng, frames, scale, offset=0.0, min_area=MIN_AREA, min_circ=MIN_CIRC):
    ft = torch.from_numpy(frames).to(eng.device)
    rec, counts, stats = eng.measure_markers(ft, K.THRESHOLD, scale, min_area, min_circ, offset)
    bits = eng.threshold_bits(ft, K.THRESHOLD)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy(), bits.cpu().numpy()
