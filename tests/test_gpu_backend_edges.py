"""The 3-D back end at its edges (run on the MI355X box: `pytest -m gpu`): `k_remap` / `k_undist_map`, the fused solve of
`k_track` and `k_finalize_track`, `k_solve3d`, `k_displacement`, `k_plane_fit` and `k_deviation_plane` against float64
restatements (`tests/helpers/backend_oracle.py`, `oracle/stages.py`) on hand-made tables and frames of at most 640x480, under
a GENERAL camera: `cam_b` of `tests/golden/solve3d.json` (rotated, fx != fy, three components of T) with distortion.

Bounds, none of them measured:
  flags, counts, bytes of an undistorted frame, the deviation columns   exact
  X, Y, Z and a, b, c, tilt of a float32 table against a float64 value  one float32 ulp of the expected value: device and
      restatement evaluate the same float64 expression on the same float32 inputs (they agree to 1e-12 on the float64 point
      interface, and the centred normal equations stay within 3e-14 of `lstsq` on well-conditioned points), so after the one
      float32 store they can only differ where they fall on opposite sides of a rounding boundary
  float64 displacement                                                   bit-equal (same operations in the same order)
  float32 displacement, deviation plane                                  the tolerances of the tests in test_gpu_parity.py
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import vbs_amd.synth as S                                     # noqa: E402
from vbs_amd import _lib as L                                 # noqa: E402
from oracle import stages as O                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import backend_oracle as BO                                   # noqa: E402

DIST = np.array([-0.21, 0.07, 0.0013, -0.0009, -0.011], dtype=np.float32)
TRK, XYZ = L.FLAG_TRACKED, L.FLAG_TRACKED | L.FLAG_XYZ
C = L.TABLE_COLS


def engine(h=480, w=640, **kw):
    from vbs_amd.engine import Engine
    kw.setdefault("max_markers", 512)
    kw.setdefault("max_batch", 4)
    return Engine(h, w, **kw)


@pytest.fixture(scope="module")
def camb(golden_dir):
    """The file's camera as the float32 arrays `load_parameters` hands over: (K, dist, R, T)."""
    cam = json.load(open(os.path.join(golden_dir, "solve3d.json")))["cam_b"]["cam"]
    return (np.array(cam["K"], dtype=np.float32), DIST, np.array(cam["R"], dtype=np.float32),
            np.array(cam["T"], dtype=np.float32))


def ulps_off(got32, want64):
    """|got - float32(want)| in units of the spacing of float32(want)."""
    w = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return np.abs(np.asarray(got32, dtype=np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)


def check_solved(got, source, cam, min_size, dmm=2.0):
    """A solved table against `BO.solve_table` of `source`'s own columns 1-3: flags equal, X, Y, Z within one float32 ulp
    (exact zeros where there is no 3-D point), every other column untouched.  Returns the expected flags."""
    flags, xyz = BO.solve_table(source, *cam, dmm, min_size)
    assert np.array_equal(got[..., 0], flags.astype(np.float32))
    assert np.array_equal(got[..., 1:6], source[..., 1:6]) and np.array_equal(got[..., 9], source[..., 9])
    has = (flags & L.FLAG_XYZ) != 0
    assert not got[~has][:, 6:9].any()
    off = ulps_off(got[has][:, 6:9], xyz[has])
    assert (off <= 1.0).all(), f"{(off > 1).sum()} of {off.size} values are more than one float32 ulp off, the worst by {off.max()}"
    return flags


# ---- the solve on the table routes ---------------------------------------------------------------------------------------
def test_three_table_routes_agree_under_the_general_camera(camb):
    """Fused `k_track` (a batch pass), `k_finalize_track` (one frame per call) and `track` + `Engine.solve3d` (`k_solve3d`)
    write the same bits, and those are the restatement's on the table's own Cx, Cy, major."""
    from vbs_amd.pipeline import reference_from_frame0
    spec = S.config1()
    ft = torch.from_numpy(S.make_frames(spec, range(3), seed=21)).cuda()
    cam = L.make_camera(*camb, 2.0)
    e4, e1 = engine(spec.height, spec.width, max_batch=4), engine(spec.height, spec.width, max_batch=1)
    e4.set_option(L.OPT_LATENCY_FRAMES, 0)                     # (a pass of 3 frames would otherwise take the few-frames launch too)
    _, xy = reference_from_frame0(e4, ft)

    def run(eng, fn):
        eng.profile(True)
        out = fn()
        torch.cuda.synchronize()
        kernels = set(eng.profile_read())
        eng.profile(False)
        return out, kernels

    ta, ka = run(e4, lambda: e4.track_to_3d(ft, xy, 20.0, cam, 5.0)[0])
    tb, kb = run(e1, lambda: torch.cat([e1.track_to_3d(ft[i:i + 1], xy, 20.0, cam, 5.0)[0] for i in range(3)]))
    tc, kc = run(e4, lambda: e4.solve3d(e4.track_to_3d(ft, xy, 20.0, None)[0], cam, 5.0))
    assert "k_track" in ka and "k_finalize_track" not in ka and "k_solve3d" not in ka
    assert "k_finalize_track" in kb and "k_track" not in kb and "k_solve3d" not in kb
    assert "k_solve3d" in kc
    assert torch.equal(ta, tb), "k_finalize_track differs from k_track"
    assert torch.equal(ta, tc), "track + solve3d differs from the fused solve"
    got = ta.cpu().numpy()
    flags = check_solved(got, got, camb, 5.0)
    assert ((flags & L.FLAG_XYZ) != 0).sum() == 3 * spec.n_markers
    # the rotation matters: the same rows under R = I, T = 0 are somewhere else entirely
    plain = BO.solve_table(got, camb[0], camb[1], np.eye(3), np.zeros(3), 2.0, 5.0)[1]
    assert np.linalg.norm(plain - got[..., 6:9], axis=-1).min() > 1.0
    e4.close()
    e1.close()


def edge_rows(camb):
    """name -> (frame, slot, (x, y, major_axis)) of the detections that sit on an edge of the solve; None keeps the random value."""
    cx, cy = float(camb[0][0, 2]), float(camb[0][1, 2])
    below5 = float(np.nextafter(np.float32(5), np.float32(0)))
    return {"near": (0, 0, (0.5 + 2.0 ** -20, 0.25, 20.0)),   # either side of Rr = 1e-6 for a camera with cx = 0.5, cy = 0.25 ...
            "far": (1, 0, (0.5 + 2.0 ** -19, 0.25, 20.0)),
            "on_pp_p": (2, 0, (0.5, 0.25, 20.0)),             # ... and on its principal point
            "on_pp": (0, 1, (cx, cy, 20.0)),                  # exactly on the general camera's principal point
            "at5": (0, 2, (None, None, 5.0)),                 # on the size bound, one float32 below it, no size at all
            "below5": (1, 2, (None, None, below5)),
            "size0": (2, 2, (None, None, 0.0))}


def edge_case_table(eng, n, m, camb, seed):
    """A float32 table [n, m, 10] through `Engine.track`: random detections around a lattice of reference positions (some
    missing, some below 5 px) with the detections of `edge_rows` in their (frame, slot); the reference positions of slots 0
    and 1 are the two principal points.  Every row then gets stale values in columns 6-8 and the XYZ flag, so that the solve
    has something to clear."""
    rng = np.random.default_rng(seed)
    edges = {(f, r): d for f, r, d in edge_rows(camb).values()}
    ref = np.stack([24.0 + 32.0 * (np.arange(m) % 19), 24.0 + 32.0 * (np.arange(m) // 19)], axis=1)
    ref[0], ref[1] = (0.5, 0.25), (float(camb[0][0, 2]), float(camb[0][1, 2]))
    det = np.zeros((n, eng.max_markers, L.DET_COLS))
    counts = np.zeros(n, dtype=np.int32)
    for f in range(n):
        rows = []
        for r in range(m):
            if rng.random() < 0.15 and (f, r) not in edges:
                continue
            major = rng.uniform(2.0, 4.9) if rng.random() < 0.1 else rng.uniform(6.0, 40.0)
            x, y = ref[r] + rng.uniform(-3, 3, 2)
            if (f, r) in edges:
                x, y, major = (v if e is None else e for v, e in zip((x, y, major), edges[(f, r)]))
            rows.append([x, y, major, 0.8 * major, rng.uniform(0, 180), 0.0])
        rows = [rows[i] for i in rng.permutation(len(rows))]
        det[f, :len(rows)] = rows
        counts[f] = len(rows)
    tab = eng.track(torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), ref).cpu().numpy()
    assert tab.shape == (n, m, C) and not tab[..., 6:9].any() and set(np.unique(tab[..., 0])) <= {0.0, float(TRK)}
    for name, (f, r, (x, y, major)) in edge_rows(camb).items():          # every edge row is where it was put
        assert tab[f, r, 0] == TRK and tab[f, r, 3] == np.float32(major), name
        assert x is None or (tab[f, r, 1] == np.float32(x) and tab[f, r, 2] == np.float32(y)), name
    tab[..., 0] += L.FLAG_XYZ
    tab[..., 6:9] = rng.uniform(-500, 500, (n, m, 3)).astype(np.float32)
    return tab


@pytest.mark.parametrize("n,m", [(4, 64), (3, 171)])
def test_solve3d_on_hand_made_tables(camb, n, m):
    """`k_solve3d` at n * m = 256 (one full block) and 513 (a last block of one thread): the refusals of the solve, the
    `>= min_size` comparison, clearing of stale values, a second camera, idempotence."""
    eng = engine()
    src = edge_case_table(eng, n, m, camb, seed=n * m)
    Kp = camb[0].copy()
    Kp[0, 2], Kp[1, 2] = 0.5, 0.25
    camp = (Kp, np.zeros(5, np.float32), camb[2], camb[3])    # the offsets 2^-20 and 2^-19 fit a float32 next to cx = 0.5
    at = {name: (f, r) for name, (f, r, _) in edge_rows(camb).items()}
    flag = lambda t, name: int(t[at[name]][0])                # noqa: E731
    tracked = (src[..., 0].astype(int) & TRK) != 0
    assert (~tracked).sum() > 10 and ((src[..., 3] < 5.0) & tracked).sum() > 3

    t = torch.from_numpy(src).cuda()
    g1 = eng.solve3d(t, L.make_camera(*camb, 2.0), 5.0).cpu().numpy()
    assert t.data_ptr() == eng.solve3d(t, L.make_camera(*camb, 2.0), 5.0).data_ptr()
    assert np.array_equal(t.cpu().numpy(), g1), "a second solve with the same camera changed the table"
    f1 = check_solved(g1, src, camb, 5.0)
    assert flag(g1, "on_pp") == TRK and (g1[..., 0][~tracked] == 0).all()
    assert flag(g1, "at5") == XYZ, "a major axis equal to min_size must be solved (>=)"
    assert flag(g1, "below5") == TRK and flag(g1, "size0") == TRK
    assert flag(g1, "near") == XYZ and flag(g1, "on_pp_p") == XYZ       # (nothing special about those points for THIS camera)

    g2 = eng.solve3d(t, L.make_camera(*camp, 2.0), 5.0).cpu().numpy()
    f2 = check_solved(g2, src, camp, 5.0)
    assert flag(g2, "near") == TRK and flag(g2, "on_pp_p") == TRK and flag(g2, "far") == XYZ and flag(g2, "on_pp") == XYZ
    both = ((f1 & f2) & L.FLAG_XYZ) != 0
    assert both.sum() > n * m // 2 and (g1[both][:, 6:9] != g2[both][:, 6:9]).all(), "a value of the first camera survived"

    g3 = eng.solve3d(t, L.make_camera(*camb, 2.0), 0.0).cpu().numpy()
    check_solved(g3, src, camb, 0.0)
    assert flag(g3, "size0") == TRK and flag(g3, "below5") == XYZ and flag(g3, "on_pp") == TRK
    solvable = tracked & (src[..., 3] > 0)
    solvable[at["on_pp"]] = False
    assert (g3[..., 0][solvable] == XYZ).all()
    eng.close()


@pytest.mark.parametrize("case", ["solved", "principal point", "below the size bound", "untracked"])
def test_solve3d_on_a_table_of_one_row(camb, case):
    """n * m = 1, written directly."""
    cx, cy = camb[0][0, 2], camb[0][1, 2]
    row = {"solved": [TRK, 100.25, 50.5, 5.0], "principal point": [XYZ, cx, cy, 20.0],
           "below the size bound": [XYZ, 100.25, 50.5, np.nextafter(np.float32(5), np.float32(0))],
           "untracked": [L.FLAG_XYZ, 100.25, 50.5, 20.0]}[case]
    src = np.zeros((1, 1, C), dtype=np.float32)
    src[0, 0, :4], src[0, 0, 4:6], src[0, 0, 6:9], src[0, 0, 9] = row, (4.0, 33.0), (7.0, -8.0, 9.0), 3.0
    eng = engine()
    guard = torch.full((3, C), 55.0, dtype=torch.float32, device="cuda")       # the row sits between two rows it must not touch
    guard[1] = torch.from_numpy(src[0, 0]).cuda()
    eng.solve3d(guard[1:2].unsqueeze(0), L.make_camera(*camb, 2.0), 5.0)
    got = guard.cpu().numpy()
    assert (got[0] == 55.0).all() and (got[2] == 55.0).all()
    flags = check_solved(got[1:2][None], src, camb, 5.0)
    assert int(flags[0, 0]) == {"solved": XYZ, "untracked": 0}.get(case, TRK)
    eng.close()


# ---- displacement --------------------------------------------------------------------------------------------------------
def random_table(n, m, seed=0):
    """The recipe of `test_displacement_range_and_gaps`: gaps, rows without a 3-D point, rows below the size filter, a jump."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((n, m, C), dtype=np.float32)
    present = rng.random((n, m)) < 0.8
    present[:3] = False
    present[10:60, 5 % m] = False                                  # a gap longer than a chunk for one ID
    ok = rng.random((n, m)) < 0.95
    tab[..., 0] = present * (1 + 2 * ok)
    tab[..., 3] = np.where(rng.random((n, m)) < 0.03, 4.0, 20.0)
    xyz = np.cumsum(rng.normal(0, 0.3, (n, m, 3)), axis=0) + 30
    for f, r in ((40, 7 % m), (50, 299 % m)):                  # a > 50 mm jump, one of them in the second column block
        xyz[f:, r] += 80.0
        tab[f - 1:f + 1, r, 0], tab[f - 1:f + 1, r, 3] = XYZ, 20.0
    tab[..., 6:9] = xyz
    return tab


def test_displacement_two_column_blocks_and_a_ragged_chunk():
    """n = 70 (chunks of 32, 32 and 6 frames), m = 300 (column blocks of 256 and 44): the float32 entry against the
    sequential loop within the suite's tolerance, the float64 entry BIT-equal to it, frame ranges equal to slices.
    The ranges run on the float32 entry: `vbs_displacement_f64` / `displacement_f64` take no frame range and always launch
    `k_displacement<double>` with f0 = 0, f1 = n, so the float64 instance cannot reach its f0 > 0 branch through any entry
    of the library; the branch is the template's, shared with the float32 instance that is run here."""
    from vbs_amd.engine import displacement_f64
    n, m, warm, minsz, lim = 70, 300, 10, 5.0, 50.0
    tab = random_table(n, m)
    want = BO.displacement(tab, warm, minsz, lim)
    assert want[..., 0].sum() > 5000 and want[:, 256:, 0].sum() > 500 and want[64:, :, 0].sum() > 500
    assert want[40, 7, 0] == 0 and want[50, 299, 0] == 0 and want[41:, 7, 0].any(), "the > 50 mm jumps are not in the table"
    eng = engine()
    tt = torch.from_numpy(tab).cuda()
    full = eng.displacement(tt, warm, minsz, lim).cpu().numpy()
    assert np.array_equal(full[..., 0], want[..., 0])
    np.testing.assert_allclose(full[..., 1:], want[..., 1:], rtol=1e-6, atol=1e-6)
    got64 = displacement_f64(tab.astype(np.float64), warm, minsz, lim).cpu().numpy()
    assert np.array_equal(got64, want), "vbs_displacement_f64 is not bit-equal to the sequential float64 loop"
    for a, b in ((33, 65), (64, 70)):
        part = eng.displacement(tt, warm, minsz, lim, frame_range=(a, b)).cpu().numpy()
        assert np.array_equal(part, full[a:b])
        assert np.array_equal(part[..., 0], want[a:b, :, 0])
        np.testing.assert_allclose(part[..., 1:], want[a:b, :, 1:], rtol=1e-6, atol=1e-6)
    eng.close()


def test_displacement_edge_tables():
    """Nothing present, everything below the size filter, warm-ups beyond the table and below zero, the `!(mm > limit)`
    boundary on an exact 3-4-5 step, and a look-back across two whole chunks - on both entries."""
    from vbs_amd.engine import displacement_f64
    n, m = 70, 3
    eng = engine()

    def both(tab, warm, minsz, lim):
        want = BO.displacement(tab, warm, minsz, lim)
        got = eng.displacement(torch.from_numpy(tab).cuda(), warm, minsz, lim).cpu().numpy()
        assert np.array_equal(got[..., 0], want[..., 0])
        np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=1e-6, atol=1e-6)
        assert np.array_equal(displacement_f64(tab.astype(np.float64), warm, minsz, lim).cpu().numpy(), want)
        return want

    empty = np.zeros((n, m, C), dtype=np.float32)
    empty[..., 6:9] = 3.0
    assert not both(empty, 0, 5.0, 50.0).any()                 # the "no frame survives" sentinel: nothing is emitted
    small = random_table(n, m, seed=1)
    small[..., 3] = np.nextafter(np.float32(5), np.float32(0))
    assert not both(small, 0, 5.0, 50.0).any()
    assert both(small, 0, float(small[0, 0, 3]), 50.0)[..., 0].sum() > 50      # (the same rows pass a bound they sit ON)
    tab = random_table(n, m, seed=2)
    assert not both(tab, n, 5.0, 50.0).any() and not both(tab, n - 3, 5.0, 50.0).any()    # (no row before frame 3)
    assert both(tab, n - 13, 5.0, 50.0)[..., 0].sum() > 0
    assert np.array_equal(both(tab, -3, 5.0, 50.0), both(tab, 0, 5.0, 50.0))
    step = np.zeros((n, m, C), dtype=np.float32)
    step[[0, 1], 0, 0], step[[0, 1], 0, 3] = XYZ, 20.0
    step[0, 0, 6:9], step[1, 0, 6:9] = (1.0, 2.0, 3.0), (4.0, 6.0, 3.0)
    assert np.array_equal(both(step, 0, 5.0, 5.0)[1, 0], [1.0, 3.0, 4.0, 0.0, 5.0])
    assert not both(step, 0, 5.0, float(np.nextafter(5.0, 0)))[..., 0].any()
    far = np.zeros((n, m, C), dtype=np.float32)
    far[[0, 69], 1, 0], far[[0, 69], 1, 3] = XYZ, 20.0
    far[0, 1, 6:9], far[69, 1, 6:9] = (1.5, 2.5, 30.0), (2.0, 2.25, 29.0)
    far[30:40, 1, 6:9] = 99.0                                  # (values in rows that are not tracked are not looked at)
    assert np.array_equal(both(far, 0, 5.0, 50.0)[69, 1, :4], [1.0, 0.5, -0.25, -1.0])
    eng.close()


# ---- plane fit -----------------------------------------------------------------------------------------------------------
TRIANGLE = np.array([[-10.0, -8.0], [12.0, -5.0], [1.0, 11.0]])


def plane_table(m, seed):
    """[8, m, 10]: frames with 0, 1, 2, 3 flagged rows, three with every row flagged on planes of tilt 0, 4 and 60 degrees, one
    with about half of them; the flagged rows lie scattered among TRACKED-only rows holding garbage.  The first three flagged
    rows of a frame sit near a fixed triangle, so that a frame of three points is well conditioned.  The tilted planes carry
    10 um of noise in Z.  The level one does not, and is level only to 0.16 degrees, a = b = 2^-9: an exactly level plane
    would be fitted as rounding noise around 0, whose ulp means nothing, and with noise the three-point frame could land
    anywhere near 0; as it is, the float32 rounding of Z (2e-6 mm over 20 mm) moves a and b by 1e-6 at most, so every
    fitted coefficient stays above the 1e-3 the test asks for whatever the seed."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((8, m, C), dtype=np.float32)
    tab[..., 0] = TRK
    tab[..., 6:9] = rng.uniform(1e5, 1e6, (8, m, 3)) * rng.choice([-1, 1], (8, m, 3))
    counts = [0, min(1, m), min(2, m), min(3, m), m, m, m, max(min(3, m), m // 2)]
    tilts = [4.0, 4.0, 4.0, 60.0, 0.0, 4.0, 60.0, 4.0]
    for f, (cnt, tilt) in enumerate(zip(counts, tilts)):
        rows = np.sort(rng.permutation(m)[:cnt])
        xy = rng.uniform(-15, 15, (cnt, 2))
        k = min(cnt, 3)
        xy[:k] = TRIANGLE[:k] + rng.uniform(-0.5, 0.5, (k, 2))
        az = 0.7 + f
        a, b = np.tan(np.radians(tilt)) * np.cos(az), np.tan(np.radians(tilt)) * np.sin(az)
        noise = rng.normal(0, 0.01, cnt)
        if tilt == 0.0:
            a, b, noise = 2.0 ** -9, 2.0 ** -9, 0.0
        z = a * xy[:, 0] + b * xy[:, 1] + 30.0 + noise
        tab[f, rows, 0] = XYZ
        tab[f, rows, 6:9] = np.column_stack([xy, z])
    return tab, counts


@pytest.mark.parametrize("m", [1, 3, 63, 64, 65, 200])
def test_plane_fit_counts_flags_and_well_conditioned_planes(m):
    """`Engine.plane_fit` directly, below, at and above the wave width: the count is exact, a kernel that ignores the XYZ flag
    meets garbage, fewer than 3 points give zeros, and a well-conditioned frame is `lstsq`'s plane to one float32 ulp."""
    tab, counts = plane_table(m, seed=100 + m)
    eng = engine()
    got = eng.plane_fit(torch.from_numpy(tab).cuda()).cpu().numpy()
    eng.close()
    assert got.shape == (8, L.PLANE_COLS)
    checked = 0
    for f in range(8):
        cnt, coeff, ratio = BO.plane(tab[f])
        assert cnt == counts[f] and got[f, 0] == cnt
        if cnt < 3:
            assert not got[f, 1:].any()
        elif ratio > 1e-3:
            off = ulps_off(got[f, 1:], coeff)
            assert (off <= 1.0).all(), f"frame {f} ({cnt} points, s_min / s_max {ratio:.3g}): {got[f, 1:]} against {coeff}, {off} ulp"
            assert min(abs(v) for v in coeff) > 1e-3            # (an expected value near 0 would have no ulp to speak of)
            checked += 1
    assert checked >= 4 or m < 3, "too few well-conditioned frames in this table"


@pytest.mark.parametrize("m", [3, 63, 64, 65, 200])
def test_plane_fit_exactly_degenerate_points_give_zeros(m):
    """All points on Y = 2.5, all on X = -1.25, all coincident, from exactly representable coordinates: the centred sums are
    exact, the determinant is exactly 0, and the kernel reports the count and ZEROS where `np.linalg.lstsq` returns the
    minimum-norm solution."""
    rng = np.random.default_rng(m)
    tab = np.zeros((3, m, C), dtype=np.float32)
    tab[..., 0] = TRK
    tab[..., 6:9] = 1e6
    cnt = max(3, (2 * m) // 3)
    for f in range(3):
        rows = rng.permutation(m)[:cnt]
        p = np.column_stack([rng.integers(-40, 40, cnt) * 0.25, rng.integers(-40, 40, cnt) * 0.25, rng.integers(100, 140, cnt) * 0.25])
        if f == 0:
            p[:, 1] = 2.5
        elif f == 1:
            p[:, 0] = -1.25
        else:
            p[:] = (3.75, -2.5, 30.25)
        tab[f, rows, 0], tab[f, rows, 6:9] = XYZ, p
    assert np.ptp(tab[0][tab[0, :, 0] == XYZ][:, 6]) > 0 and np.ptp(tab[1][tab[1, :, 0] == XYZ][:, 7]) > 0
    eng = engine()
    got = eng.plane_fit(torch.from_numpy(tab).cuda()).cpu().numpy()
    eng.close()
    for f in range(3):
        n_f, coeff, ratio = BO.plane(tab[f])
        assert n_f == cnt and ratio < 1e-12
        assert got[f].tolist() == [float(cnt), 0.0, 0.0, 0.0, 0.0]
    assert abs(BO.plane(tab[0])[1][2]) > 1.0                   # ... where lstsq has a minimum-norm plane that is not zero


# ---- deviation plane -----------------------------------------------------------------------------------------------------
RINGS = [(0, 1), (3.4, 6), (6.8, 12), (10.2, 18), (13.4, 24), (16.3, 30), (19.5, 36), (22.7, 42)]


def deviation_session(ref, tilt_deg, drop, rng):
    """The session recipe of `test_deviation_plane_against_the_oracle`: two frames (start, end) of a loading."""
    m = ref.shape[0]
    tab = np.zeros((2, m, C), np.float32)
    start = ref + rng.normal(0, 0.02, (m, 3))
    end = start + np.column_stack([np.zeros(m), 0.01 * start[:, 1], -0.6 - np.tan(np.radians(tilt_deg)) * start[:, 0]])
    end += rng.normal(0, 0.01, (m, 3))
    for f, xyz in enumerate((start, end)):
        tab[f, :, 0] = XYZ
        tab[f, :, 6:9] = xyz
    tab[1, drop, 0] = TRK
    return tab


def four(row):
    return np.column_stack([((row[:, 0].astype(int) & L.FLAG_XYZ) != 0).astype(float), row[:, 6:9].astype(np.float64)])


def check_deviation(eng, rows, ref, mode, scale):
    """`Engine.deviation_plane` on four table rows against `O.deviation_plane`, with the tolerances of
    `test_deviation_plane_against_the_oracle`; fewer than 3 common markers: the plane is zeros, the means are reported."""
    dev, out = eng.deviation_plane(*(torch.from_numpy(r).cuda() for r in rows), ref, mode, scale)
    dev, out = dev.cpu().numpy(), out.cpu().numpy()
    if not np.logical_and.reduce([four(r)[:, 0] != 0 for r in rows]).any():
        assert not out.any() and not dev.any()
        return 0, out
    common, want_dev, plane, mean_vec, mean_mag = O.deviation_plane(*(four(r) for r in rows), ref.astype(np.float32), mode, scale)
    cnt = int(common.sum())
    assert out[0] == cnt and np.array_equal(dev[:, 0] != 0, common)
    assert np.array_equal(dev[:, 1:4], want_dev.astype(np.float32))
    if cnt >= 3:
        np.testing.assert_allclose(out[1:5], plane, rtol=2e-4, atol=2e-5)
    else:
        assert not out[1:5].any()
    np.testing.assert_allclose(out[5:8], mean_vec, rtol=2e-4, atol=1e-6)
    assert abs(out[8] - mean_mag) <= 2e-4 * mean_mag
    return cnt, out


@pytest.mark.parametrize("m", [1, 2, 64, 130])
def test_deviation_plane_below_at_and_above_the_wave_width(m):
    rng = np.random.default_rng(9 + m)
    ref = np.array([[r * np.cos(2 * np.pi * k / n_), r * np.sin(2 * np.pi * k / n_), 0.02 * r * r]
                    for r, n_ in RINGS for k in range(n_)])[:m]
    drops = ([], []) if m < 3 else ([5, 30], [30, 31, m - 1])
    tv, tt = deviation_session(ref, 0.0, drops[0], rng), deviation_session(ref, 4.0, drops[1], rng)
    eng = engine()
    for mode in ("plane", "shell"):
        for scale in (1.0, 5.0):
            cnt, out = check_deviation(eng, (tv[0], tv[1], tt[0], tt[1]), ref, mode, scale)
            assert cnt == m - len(set(drops[0]) | set(drops[1]))
            if m >= 64 and mode == "plane" and scale == 1.0:
                assert abs(out[4] - 4.0) < 0.3                  # the synthetic misalignment comes back
    eng.close()


def test_deviation_plane_edge_cases():
    """No common marker (nine zeros), two common markers (means, no plane), a marker missing from each of the four rows in
    turn - which must drop it whichever row misses it."""
    m = 64
    rng = np.random.default_rng(3)
    ref = np.array([[r * np.cos(2 * np.pi * k / n_), r * np.sin(2 * np.pi * k / n_), 0.02 * r * r]
                    for r, n_ in RINGS for k in range(n_)])[:m]
    tv, tt = deviation_session(ref, 0.0, [], rng), deviation_session(ref, 4.0, [], rng)
    eng = engine()
    for mode in ("plane", "shell"):
        rows = [tv[0].copy(), tv[1].copy(), tt[0].copy(), tt[1].copy()]
        for k in range(4):                                     # slot 10 + k misses its 3-D point in row k only
            rows[k][10 + k, 0] = TRK
            cnt, _ = check_deviation(eng, rows, ref, mode, 2.0)
            assert cnt == m - 1 - k
        for k in range(4):                                     # every slot misses one of the four rows
            rows[k][k::4, 0] = TRK if k % 2 else 0
        cnt, out = check_deviation(eng, rows, ref, mode, 2.0)
        assert cnt == 0 and out.tolist() == [0.0] * L.DEVPLANE_COLS
        rows = [tv[0].copy(), tv[1].copy(), tt[0].copy(), tt[1].copy()]
        rows[2][:, 0] = TRK
        rows[2][[7, 40], 0] = XYZ
        cnt, out = check_deviation(eng, rows, ref, mode, 2.0)
        assert cnt == 2 and out[8] > 0 and out[5:8].any()
    eng.close()


# ---- frame undistortion --------------------------------------------------------------------------------------------------
# (size (W, H), K = (fx, fy, cx, cy), dist).  A handle takes frames of at least 128 x 64 (`vbs_create`), so the cameras run on
# 64 rows; what each map then offers at the border is asserted from the oracle's map in the test itself.
UNDISTORT_CASES = {
    "barrel": ((300, 64), (280.0, 284.0, 149.5, 30.25), (-0.25, 0.08, 0.001, -0.0005, 0.01)),
    "pincushion": ((300, 64), (280.0, 284.0, 149.5, 30.25), (0.3, 0.1, 0.0, 0.0, 0.0)),
    "off-centre": ((257, 64), (200.0, 190.0, 60.0, 30.0), (-0.3, 0.1, 0.02, -0.03, 0.0)),
    "identity": ((257, 64), (200.0, 190.0, 128.0, 18.0), (0.0, 0.0, 0.0, 0.0, 0.0)),
}
UNDISTORT_RUNS = [(c, False, ch) for c in UNDISTORT_CASES for ch in (1, 3)] + [("barrel", True, 1), ("off-centre", True, 3)]


def footprints(K, D, size):
    """From the ORACLE's map: (pixels whose 2x2 footprint is partly outside the frame, those among them where a tap outside
    carries weight, weight rows in use)."""
    W, H = size
    m1, m2 = O.init_undistort_rectify_map_16sc2(K, D, O.get_optimal_new_camera_matrix_alpha0(K, D, size), size)
    sx, sy = m1[..., 0].astype(int), m1[..., 1].astype(int)
    wts = O.bilinear_tab_i16()[m2.astype(int)]
    taps = [(sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)]
    inside = np.stack([(y >= 0) & (y < H) & (x >= 0) & (x < W) for y, x in taps], axis=-1)
    partly = inside.any(-1) & ~inside.all(-1)
    weighted = (~inside & (wts > 0)).any(-1)
    return int(partly.sum()), int((partly & weighted).sum()), len(np.unique(m2))


@pytest.mark.parametrize("case,view,channels", UNDISTORT_RUNS)
def test_undistort_random_frames_byte_equal(case, view, channels):
    """`k_undist_map` + `k_remap` on uniform random bytes - every tap and weight matters - equal `O.undistort_frame` byte for
    byte.  Every map has footprints that are partly outside the frame; in the off-centre one taps outside CARRY WEIGHT, so a
    tap that is read instead of taken as 0 shows (BORDER_CONSTANT), and the crop view surrounds the frame with random bytes
    such a tap would read."""
    (W, H), (fx, fy, cx, cy), D = UNDISTORT_CASES[case]
    K, D = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), np.array(D)
    partly, weighted, used = footprints(K, D, (W, H))
    assert partly > 0, "no footprint of this map crosses the border: the case no longer tests BORDER_CONSTANT"
    if case == "identity":
        assert (partly, weighted, used) == (W + H - 1, 0, 1)
    else:
        assert used == 1024, "the map no longer uses every row of the weight table"
        assert weighted > 0 or case != "off-centre"
    rng = np.random.default_rng(W + channels)
    shape = (2, H + 8, W + 11) + ((3,) if channels == 3 else ())
    big = rng.integers(0, 256, shape, dtype=np.uint8)
    frames = np.ascontiguousarray(big[:, 3:3 + H, 5:5 + W])
    ft = torch.from_numpy(big).cuda()[:, 3:3 + H, 5:5 + W] if view else torch.from_numpy(frames).cuda()
    assert ft.is_contiguous() != view
    eng = engine(H, W, max_batch=2)
    newK = eng.set_undistort(K, D)
    np.testing.assert_allclose(newK, O.get_optimal_new_camera_matrix_alpha0(K, D, (W, H)), rtol=1e-12, atol=1e-12)
    got = eng.undistort_frames(ft).cpu().numpy()
    eng.close()
    assert got.shape == frames.shape
    for i in range(2):
        want = O.undistort_frame(frames[i], K, D)
        diff = np.argwhere(got[i] != want)
        assert diff.size == 0, f"{len(diff)} bytes differ, the first at {diff[0]}: {got[i][tuple(diff[0])]} != {want[tuple(diff[0])]}"
        if case == "identity":
            assert np.array_equal(got[i], frames[i])
        else:
            assert (got[i] != frames[i]).mean() > 0.5
