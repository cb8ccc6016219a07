"""CPU tests of `tests/helpers/backend_oracle.py` (no GPU): the float64 restatement that the GPU tests of the 3-D back end
compare against reproduces the outputs of the reference's own function bodies (`tests/golden/solve3d.json`) when it is
driven through TABLES, the way the kernels are, and returns a known plane on integer data."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import backend_oracle as BO                                   # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return json.load(open(os.path.join(golden_dir, "solve3d.json")))


@pytest.mark.parametrize("cname", ["cam_a", "cam_b"])
def test_solve_table_reproduces_the_point_golden(gold, cname):
    """Both cameras (cam_b: rotated, fx != fy, three components of T), the rows on the principal point included: a float64
    table holding (u, v, d) in columns 1-3.  Zero distortion is normalise + re-project (1e-13 px), hence 1e-12 relative -
    the project's tolerance for float64 points - instead of equality."""
    cam, pts = gold[cname]["cam"], gold[cname]["pts"]
    tab = np.zeros((1, len(pts), 10))
    tab[0, :, 0] = BO.FLAG_TRACKED | BO.FLAG_XYZ              # (a stale XYZ flag must not survive on the refused rows)
    tab[0, :, 1:4] = [p[:3] for p in pts]
    tab[0, :, 6:9] = 77.0
    flags, xyz = BO.solve_table(tab, cam["K"], np.zeros(5), cam["R"], cam["T"], 2.0, 0.0)
    refused = np.array([p[3] is None for p in pts])
    assert refused.sum() == 3
    assert np.array_equal(flags[0], np.where(refused, BO.FLAG_TRACKED, BO.FLAG_TRACKED | BO.FLAG_XYZ))
    assert np.array_equal(xyz[0, refused], np.zeros((3, 3)))
    want = np.array([p[3:] for p in pts if p[3] is not None], dtype=np.float64)
    np.testing.assert_allclose(xyz[0, ~refused], want, rtol=1e-12, atol=1e-12)


def test_solve_table_filters_and_clears(gold):
    """`>= min_size` keeps the row that sits exactly on the bound; an untracked row loses a stale flag and stale values."""
    cam = gold["cam_b"]["cam"]
    tab = np.zeros((4, 10), dtype=np.float32)
    tab[:, 1:3] = [100.0, 50.0]
    tab[:, 0] = [1, 1, 2, 0]
    tab[:, 3] = [5.0, np.nextafter(np.float32(5), np.float32(0)), 20.0, 20.0]
    tab[:, 6:9] = 9.0
    flags, xyz = BO.solve_table(tab, cam["K"], np.zeros(5), cam["R"], cam["T"], 2.0, 5.0)
    assert flags.tolist() == [3, 1, 0, 0]
    assert np.isfinite(xyz[0]).all() and np.abs(xyz[0]).min() > 0 and not xyz[1:].any()


def test_displacement_reproduces_the_row_golden(gold):
    """The `disp` golden (gap frame, warm-up, > 50 mm jump and the step back) through solve_table + displacement on a
    float64 table [frames, ids, 10]."""
    g = gold["disp"]
    cam = g["cam"]
    ids = sorted({(r["row"], r["col"]) for r in g["rows_in"]})
    slot = {k: i for i, k in enumerate(ids)}
    n = max(r["frameno"] for r in g["rows_in"]) + 1
    tab = np.zeros((n, len(ids), 10))
    for r in g["rows_in"]:
        tab[r["frameno"], slot[(r["row"], r["col"])], :4] = [BO.FLAG_TRACKED, r["u"], r["v"], r["major_axis"]]
    flags, xyz = BO.solve_table(tab, cam["K"], np.zeros(5), cam["R"], cam["T"], 2.0, 0.0)
    tab[..., 0], tab[..., 6:9] = flags, xyz
    disp = BO.displacement(tab, g["warmup"], 0.0, g["limit"])
    f, s = np.nonzero(disp[..., 0])
    got = np.array([[fi, ids[si][0], ids[si][1], *tab[fi, si, 6:9], *disp[fi, si, 1:]] for fi, si in zip(f, s)])
    want = np.array(g["rows_out"])
    assert got.shape == want.shape
    key = lambda a: np.lexsort((a[:, 2], a[:, 1], a[:, 0]))      # noqa: E731
    got, want = got[key(got)], want[key(want)]
    np.testing.assert_array_equal(got[:, :3], want[:, :3])
    np.testing.assert_allclose(got[:, 3:], want[:, 3:], rtol=0, atol=1e-9)


def test_displacement_edges():
    """Nothing present, everything below the size filter, a warm-up beyond the table, a negative warm-up (= 0), and the
    `not mm > limit` boundary on an exact 3-4-5 step."""
    tab = np.zeros((6, 2, 10), dtype=np.float32)
    assert not BO.displacement(tab, 0, 5.0, 50.0).any()
    tab[..., 0], tab[..., 3] = 3, 4.0
    tab[:, 0, 6:9] = np.arange(6)[:, None] * np.array([3.0, 4.0, 0.0])
    assert not BO.displacement(tab, 0, 5.0, 50.0).any()
    tab[..., 3] = 5.0
    assert not BO.displacement(tab, 6, 5.0, 50.0).any()
    d = BO.displacement(tab, 0, 5.0, 5.0)
    assert np.array_equal(d, BO.displacement(tab, -3, 5.0, 5.0))
    assert np.array_equal(d[1:, 0], np.tile([1.0, 3.0, 4.0, 0.0, 5.0], (5, 1))) and not d[0].any()
    assert np.array_equal(d[1:, 1], np.tile([1.0, 0.0, 0.0, 0.0, 0.0], (5, 1)))
    assert not BO.displacement(tab, 0, 5.0, np.nextafter(5.0, 0))[:, 0].any()
    assert np.array_equal(BO.displacement(tab, 2, 5.0, 5.0)[..., 0].sum(0), [3, 3])


def test_plane_on_integer_data():
    """Z = 2 X - 3 Y + 5 on an integer lattice, the flagged rows scattered among TRACKED-only rows that hold garbage.  The
    count is exact; a, b, c come from `np.linalg.lstsq` (an SVD), which returns 2, -3, 5 to a few units in the last place
    and not bit for bit, hence 1e-13 relative where the data would allow equality."""
    rng = np.random.default_rng(0)
    tab = np.zeros((40, 10), dtype=np.float32)
    tab[:, 0] = BO.FLAG_TRACKED
    tab[:, 6:9] = 1e6
    rows = rng.permutation(40)[:12]
    X, Y = np.divmod(np.arange(12), 4)
    tab[rows, 0] = BO.FLAG_TRACKED | BO.FLAG_XYZ
    tab[rows, 6], tab[rows, 7], tab[rows, 8] = X - 1, Y + 2, 2 * (X - 1) - 3 * (Y + 2) + 5
    cnt, (a, b, c, tilt), ratio = BO.plane(tab)
    assert cnt == 12
    np.testing.assert_allclose([a, b, c], [2.0, -3.0, 5.0], rtol=1e-13, atol=0)
    assert abs(tilt - np.degrees(np.arctan(np.sqrt(13.0)))) < 1e-12
    s = np.linalg.svd(np.column_stack([X - 1, Y + 2, np.ones(12)]), compute_uv=False)
    assert abs(ratio - s[-1] / s[0]) < 1e-14 and ratio > 1e-2    # (the helper takes the rows in table order)
    # fewer than three points and exactly degenerate sets report their count and a ratio that says "no fit"
    tab[rows[3:], 0] = BO.FLAG_TRACKED
    assert BO.plane(tab)[0] == 3 and BO.plane(tab)[2] < 1e-12           # (-1,2), (-1,3), (-1,4): collinear
    tab[rows[2:], 0] = BO.FLAG_TRACKED
    assert BO.plane(tab)[0] == 2 and BO.plane(tab)[2] == 0.0
    tab[:, 0] = BO.FLAG_TRACKED
    assert BO.plane(tab) == (0, (0.0, 0.0, 0.0, 0.0), 0.0)
