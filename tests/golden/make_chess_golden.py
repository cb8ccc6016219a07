#!/usr/bin/env python3
"""Generate tests/golden/chess_shot.json: the chessboard of the published validation shot (tests/golden/diameter_shot.npz) as
the NumPy helper tests/helpers/chess_oracle.py finds it.

    python tests/golden/make_chess_golden.py

The shot's BGR image goes through the oracle's BGR2GRAY; the file holds the 36 integer peaks in output order, the finder's
corners (window (2,2), 15 iterations, eps 0.1), their (11,11) refinement, the number of candidates, and pixels per millimetre
from each of the three by `calculate_scale`'s arithmetic, next to the fixture's own box-rule scale.  Data only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import chess_oracle as CO                                    # noqa: E402
from oracle import stages as O                               # noqa: E402
from vbs_amd.diameter_validation import scale_from_corners    # noqa: E402

PATTERN, SQUARE_MM = (6, 6), 3.0


def shot_gray():
    d = np.load(os.path.join(HERE, "diameter_shot.npz"))
    return O.bgr2gray(d["bgr"]), float(d["scale"])


def main():
    gray, box_scale = shot_gray()
    r = CO.find_chessboard_corners(gray, PATTERN, want=True)
    assert r["found"] == 1 and r["ties"] == 0
    refined, _ = CO.corner_subpix(gray, r["corners"])
    out = dict(pattern=list(PATTERN), square_mm=SQUARE_MM, shape=list(gray.shape), n_candidates=int(r["n_candidates"]),
               peaks=r["peaks"].tolist(), corners=r["corners"].tolist(), refined=refined.tolist(),
               scale_peaks=float(scale_from_corners(r["peaks"], PATTERN, SQUARE_MM)),
               scale_corners=float(scale_from_corners(r["corners"], PATTERN, SQUARE_MM)),
               scale_refined=float(scale_from_corners(refined, PATTERN, SQUARE_MM)), scale_box_rule=box_scale)
    with open(os.path.join(HERE, "chess_shot.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: out[k] for k in ("n_candidates", "scale_peaks", "scale_corners", "scale_refined", "scale_box_rule")})


if __name__ == "__main__":
    main()
