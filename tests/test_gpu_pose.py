"""GPU tests of the pose-misalignment series (k_pose.hip; run on the MI355X box: `pytest -m gpu`): `Engine.pose_series`,
`pipeline.misalignment_analysis` and the sheet.

`deviation`, `field`, the flags, `count`, `n_used`, `complete`, `a`, `b` and `c` are held BIT FOR BIT to the NumPy restatement
(`tests/helpers/pose_oracle.py`: the same IEEE operations in the same order); `tilt_deg`, `azimuth_deg` and `rms` to 4 ulp.
rms^2 = SSR / n_used is no column of `pose`: it is held through `rms`, which must lie within 4 ulp of the square root of the
restated quotient.  No entry is skipped or masked.  Shapes are the smallest at which the kernel can go wrong: around the wave
(64 slots), around the staged chunk (64 VBS_POSE_GROUP slots) and around the frames a workgroup takes, not the workload's.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import filters as F                              # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as FO                                    # noqa: E402
import pose_oracle as O                                       # noqa: E402

G = L.POSE_GROUP
FRAMES = sorted({1, 2, G - 1, G, G + 1, 2 * G + 3} - {0})
SLOTS = (1, 2, 3, 4, 63, 64, 65, 128, 130, 441, 1024)


@pytest.fixture(scope="module")
def eng():
    from vbs_amd.engine import Engine
    e = Engine(480, 640, max_markers=256, max_batch=2)
    yield e
    e.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def run(eng, t, rd, ref, **kw):
    """`Engine.pose_series` -> three host arrays."""
    dev = t if isinstance(t, torch.Tensor) else torch.from_numpy(t).cuda()
    return tuple(x.cpu().numpy() for x in eng.pose_series(dev, rd, ref, **kw))


def make_case(n, m, i):
    """The i-th content for a shape: 20 % random dropouts, a slot dead in start_frame, a slot dead in ref_disp, frames with 0, 1,
    2 or 3 common slots, NaN / 1e30 in every cell that must not be read; mask, mode, scale, reject_k and start_frame rotate."""
    rng = np.random.default_rng(1000 * m + 10 * n + i)
    ref = O.grid_ref(m)
    t = O.tilted_table(ref, rng.uniform(0.0, 6.0, n), rng.uniform(-180.0, 180.0, n), 7 * m + n, 0.02,
                       0.2 if m > 4 or i % 2 else 0.0)      # (three or four slots: a plane needs them all, so not always)
    start = (3 * i) % (n - 4 if n > 4 else n)               # (not one of the thinned-out frames, where there is a choice)
    dead = np.zeros((n, m), dtype=bool)
    if m > 1 and (m > 4 or i % 3 == 1):
        dead[start, m // 2] = True                           # dead in start_frame: never common, never expected
    for k in range(4):                                       # the last four frames keep only 3, 2, 1, 0 slots; a short
        f = n - 4 + k if n >= 4 else n - 1                   # recording's last frame keeps i % 4
        if n < 4 and k != i % 4:
            continue
        keep = np.nonzero((t[f, :, 0].astype(int) & 2) != 0)[0][:(3 - k)]
        dead[f] = True
        dead[f, keep] = False
    O.poison(t, dead, rng)
    rd = np.zeros((m, 4))
    rd[:, 0] = rng.choice([1.0, 2.0, -1.0, 1e-300], m)       # any nonzero flag is valid
    rd[:, 1:] = rng.normal(0.0, 0.05, (m, 3))
    if m > 2 and (m > 4 or i % 3 == 2):
        rd[m // 3] = (0.0, np.nan, 1e30, np.nan)             # dead in the reference state
    kw = dict(start_frame=start, mode=("plane", "shell")[i % 2], scale=(1.0, 25.0)[(i // 2) % 2], reject_k=(0.0, 3.0, 1.0)[i % 3])
    mask = None
    if i % 4 == 3:
        mask = rng.random(m) < 0.7
        kw["slots"] = np.nonzero(mask)[0]
    return t, rd, ref, kw, mask


def want_of(t, rd, ref, kw, mask, frame_range=None):
    return O.pose_series(t, rd, ref, kw["start_frame"], mask, kw["mode"] == "shell", kw["scale"], kw["reject_k"], frame_range)


@pytest.mark.parametrize("m", SLOTS)
def test_pose_series_equals_the_restatement_on_every_edge_shape(eng, m):
    seen, worst = set(), 0.0
    for j, n in enumerate(FRAMES):
        i = SLOTS.index(m) + 5 * j                           # (content rotates through the shapes)
        t, rd, ref, kw, mask = make_case(n, m, i)
        got = run(eng, t, rd, ref, **kw)
        want = want_of(t, rd, ref, kw, mask)
        what = f"m {m} n {n} {kw['mode']} scale {kw['scale']} k {kw['reject_k']} start {kw['start_frame']} mask {mask is not None}"
        O.check_pose(got, want, what)
        worst = max(worst, O.check_against_independent(got[0], got[1], got[2], ref, kw["mode"] == "shell", kw["scale"], what))
        seen |= set(got[2][:, 0].tolist())
        assert set(got[2][:, 0].tolist()) <= {0.0, 1.0, 2.0} and (got[2][:, 7] <= got[1][:, 1]).all()
        if kw["reject_k"] == 0.0:
            assert (got[2][:, 0] != 2.0).all()               # no rejection asked, none made
        if n >= 4:                                           # the last four frames: at most 3, 2, 1, 0 common slots
            assert (got[1][-4:, 1] <= [3, 2, 1, 0]).all() and (got[2][-3:, :7] == 0).all() and (got[1][-1] == 0).all()
    print(f"m = {m}: flags seen {sorted(seen)}, worst plane difference from lstsq {worst:.2e}")
    assert 0.0 in seen and (m < 3 or 1.0 in seen)


def test_degenerate_reference_positions_give_no_plane(eng):
    """Exactly collinear and exactly coincident ref_xyz with integer data: det is exactly 0."""
    rng = np.random.default_rng(5)
    m, n = 70, G + 1
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0
    t[..., 8] = rng.integers(-3, 4, (n, m))
    zero = np.zeros((m, 4))
    zero[:, 0] = 1.0
    line = np.stack([np.arange(70.0), 2.0 * np.arange(70.0), np.zeros(70)], axis=1)
    for pts in (line, np.full((m, 3), 5.0)):
        for k in (0.0, 3.0):
            got = run(eng, t, zero, pts, reject_k=k)
            O.check_pose(got, O.pose_series(t, zero, pts, 0, reject_k=k), "degenerate")
            assert (got[2][:, :7] == 0).all() and (got[2][:, 7] == m).all() and (got[1][:, :2] == [1.0, m]).all()


def test_rejection_of_a_planted_outlier(eng):
    m, n = 65, 2 * G + 3
    ref = O.grid_ref(m)
    t = O.tilted_table(ref, np.full(n, 4.0), -120.0, 11)
    # bounded noise: a uniform residual never passes sqrt(3) of its own rms, so a frame without a planted outlier has none
    t[1:, :, 6:9] += np.random.default_rng(11).uniform(-0.01, 0.01, (n - 1, m, 3)).astype(np.float32)
    hit = [2, G, n - 1]
    for f in hit:
        t[f, 17 + f, 8] += np.float32(5.0)                    # one mistracked marker, 5 mm
    zero = np.zeros((m, 4))
    zero[:, 0] = 1.0
    p0 = run(eng, t, zero, ref)
    p3 = run(eng, t, zero, ref, reject_k=3.0)
    O.check_pose(p0, O.pose_series(t, zero, ref, 0), "k 0")
    O.check_pose(p3, O.pose_series(t, zero, ref, 0, reject_k=3.0), "k 3")
    clean = [f for f in range(n) if f not in hit]
    assert (p0[2][:, 0] == 1).all() and (p3[2][hit, 0] == 2).all() and (p3[2][clean, 0] == 1).all()
    assert (p3[2][hit, 7] == m - 1).all() and (p3[2][clean, 7] == m).all() and (p3[1][:, 1] == m).all()
    assert np.array_equal(bits(p3[2][clean]), bits(p0[2][clean])) and np.array_equal(bits(p3[1]), bits(p0[1]))
    use = p3[0][..., 0] != 0
    for f in hit:
        use[f, 17 + f] = False
    ind = O.independent(p3[0], ref, use=use)                 # the plane of the others
    for f in hit:
        assert np.abs(p3[2][f, 1:4] - ind[f, 1:4]).max() <= O.PLANE_TOL and abs(p3[2][f, 6] - ind[f, 4]) < 1e-9
        assert abs(p3[2][f, 4] - 4.0) < 0.1 and p3[2][f, 6] < 0.02 < 0.5 < p0[2][f, 6]     # the residual is the noise's again
    # m = 4: k = 3 can put nothing outside (r^2 <= SSR < 9 SSR / 4); a k that keeps fewer than three: the refit cannot stand
    r4 = O.grid_ref(4)
    t4 = O.tilted_table(r4, np.full(G + 1, 4.0), 30.0, 5, 0.05)
    a = run(eng, t4, zero[:4], r4)
    for k in (3.0, 0.05):
        b = run(eng, t4, zero[:4], r4, reject_k=k)
        O.check_pose(b, O.pose_series(t4, zero[:4], r4, 0, reject_k=k), f"m 4 k {k}")
        assert np.array_equal(bits(a[2]), bits(b[2])) and (b[2][1:, 0] == 1).all() and (b[2][:, 7] == 4).all()


@pytest.mark.parametrize("m", (130, 700))
def test_ranges_runs_inputs_and_alignment_do_not_change_a_bit(eng, m):
    n = 2 * G + 3
    t, rd, ref, kw, mask = make_case(n, m, 7)
    dev = torch.from_numpy(t).cuda()
    full = run(eng, dev, rd, ref, **kw)
    O.check_pose(full, want_of(t, rd, ref, kw, mask), f"m {m}")
    again = run(eng, dev, torch.from_numpy(rd).cuda(), torch.from_numpy(ref).cuda(), **kw)      # a second run, tensors for arrays
    cuts = (0, 1, G - 1, G + 2, n)
    parts = [run(eng, dev, rd, ref, frame_range=(cuts[j], cuts[j + 1]), **kw) for j in range(4)]
    for c in range(3):
        assert np.array_equal(bits(full[c]), bits(again[c])), c
        assert np.array_equal(bits(np.concatenate([p[c] for p in parts])), bits(full[c])), c
    assert [x.shape for x in run(eng, dev, rd, ref, frame_range=(5, 5), **kw)] == [(0, m, 4), (0, 6), (0, 8)]
    s = kw["start_frame"]
    for f in (0, G - 1, G, n - 1):                            # a frame alone: by range, and as a table of its own
        one = run(eng, dev, rd, ref, frame_range=(f, f + 1), **kw)
        two = run(eng, np.ascontiguousarray(t[[s, f]]), rd, ref, frame_range=(1, 2), **dict(kw, start_frame=0))
        for c in range(3):
            assert np.array_equal(bits(one[c][0]), bits(full[c][f])) and np.array_equal(bits(two[c][0]), bits(full[c][f])), (f, c)
    # a table that starts on 4 bytes, not 8: the kernel's other way of reading rows
    buf = torch.empty(t.size + 1, dtype=torch.float32, device="cuda")
    odd = buf[1:].view(t.shape)
    odd.copy_(dev)
    assert odd.data_ptr() % 8 == 4
    for c, x in enumerate(run(eng, odd, rd, ref, **kw)):
        assert np.array_equal(bits(x), bits(full[c])), c
    # outputs one at a time through the C entry, and what it refuses
    rdt, rxt = torch.from_numpy(rd).cuda(), torch.from_numpy(ref).cuda()
    msk = torch.zeros(m, dtype=torch.uint8, device="cuda")
    msk[torch.from_numpy(kw["slots"]).cuda()] = 1
    outs = [torch.empty(x.shape, dtype=torch.float64, device="cuda") for x in full]

    def call(n_=n, m_=m, start=s, scale=kw["scale"], k=kw["reject_k"], fb=0, fe=n, shell=int(kw["mode"] == "shell"), o=(0, 1, 2)):
        p = [outs[c].data_ptr() if c in o else None for c in range(3)]
        return eng.lib.vbs_pose_series(eng._h, dev.data_ptr(), n_, m_, start, rdt.data_ptr(), rxt.data_ptr(), msk.data_ptr(), shell,
                                       scale, k, fb, fe, p[0], p[1], p[2], None)
    for c in range(3):
        outs[c].fill_(-7.0)
        assert call(o=(c,)) == L.VBS_OK
        torch.cuda.synchronize()
        assert np.array_equal(bits(outs[c].cpu().numpy()), bits(full[c])), c
    for bad in (dict(start=n), dict(start=-1), dict(fb=-1), dict(fe=n + 1), dict(fb=3, fe=2), dict(k=-1.0), dict(k=float("nan")),
                dict(k=float("inf")), dict(scale=float("inf")), dict(scale=float("nan")), dict(m_=0), dict(n_=0, fe=0), dict(o=()),
                dict(shell=2)):
        assert call(**bad) == L.VBS_EINVAL, bad
    assert call(fb=4, fe=4) == L.VBS_OK
    for bad in (dict(start_frame=n), dict(mode="dome"), dict(reject_k=-1.0), dict(scale=float("nan")), dict(frame_range=(0, n + 1)),
                dict(slots=[m])):
        with pytest.raises(ValueError):
            eng.pose_series(dev, rd, ref, **dict(kw, **bad))
    with pytest.raises(ValueError):
        eng.pose_series(dev, rd[:-1], ref, **kw)


def test_frame_of_the_series_against_deviation_plane(eng):
    """The code that exists: frame `end` of the series = `Engine.deviation_plane` (float32, one wave) on the same four rows,
    within the tolerances `tests/test_gpu_backend_edges.py::check_deviation` holds that kernel to."""
    for m, mode, scale in ((65, "plane", 1.0), (130, "shell", 5.0)):
        ref = O.grid_ref(m)
        t = O.tilted_table(ref, np.full(G + 2, 4.0), 30.0, 40 + m, 0.01, 0.1)
        t_ref = O.tilted_table(ref, [0.0, 0.0], 0.0, 41 + m, 0.01)
        O.poison(t_ref, np.arange(m)[None, :] == np.array([[3], [9]]), np.random.default_rng(m))
        dt, dr = torch.from_numpy(t).cuda(), torch.from_numpy(t_ref).cuda()
        rd = eng.axis_displacement(dr, 0, frame_range=(1, 2))[0][0]
        dev, field, pose = (x.cpu().numpy() for x in eng.pose_series(dt, rd, ref, 0, mode, scale))
        O.check_pose((dev, field, pose), O.pose_series(t, rd.cpu().numpy(), ref, 0, None, mode == "shell", scale), f"m {m}")
        for end in (1, G + 1):
            d32, out = (x.cpu().numpy() for x in eng.deviation_plane(dr[0], dr[1], dt[0], dt[end], ref, mode, scale))
            assert out[0] == field[end, 1] and np.array_equal(d32[:, 0] != 0, dev[end, :, 0] != 0) and out[0] >= 3
            assert np.array_equal(d32[:, 1:4], dev[end, :, 1:4].astype(np.float32))
            np.testing.assert_allclose(out[1:5], pose[end, 1:5], rtol=2e-4, atol=2e-5)
            np.testing.assert_allclose(out[5:8], field[end, 2:5], rtol=2e-4, atol=1e-6)
            assert abs(out[8] - field[end, 5]) <= 2e-4 * field[end, 5]


def test_misalignment_analysis_on_a_tilt_ramp(eng, tmp_path):
    from vbs_amd.pipeline import POSE_FRAME_COLUMNS, POSE_TREND_COLUMNS, misalignment_analysis, to_pose_frame
    from vbs_amd.xlsx_io import read_xlsx
    n, m, k_taps = 240, 65, 31
    ref = O.grid_ref(m)
    ramp = np.linspace(0.0, 6.0, n)
    t = O.tilted_table(ref, ramp, 30.0, 2, 0.02, 0.1)
    t_ref = O.tilted_table(ref, [0.0, 0.0, 0.0], 0.0, 3, 0.02)
    taps = F.lowpass_taps(k_taps, .08)
    half = F.half_taps(taps)
    res = misalignment_analysis(eng, torch.from_numpy(t).cuda(), torch.from_numpy(t_ref).cuda(), ref, taps, reject_k=3.0)
    assert set(res) == {"ref_disp", "deviation", "field", "pose", "pose_filtered", "trend"}
    host = {k: v.cpu().numpy() for k, v in res.items()}
    rd = FO.axis_total(t_ref, 0, frame_range=(2, 3))[0][0]   # ref_end = -1: the reference table's last frame
    assert np.array_equal(bits(host["ref_disp"]), bits(rd))
    want = O.pose_series(t, rd, ref, 0, reject_k=3.0)
    O.check_pose((host["deviation"], host["field"], host["pose"]), want, "ramp")
    # the filter is held on the RESTATED pose: bit for bit (a, b and c are; the angle columns are not filtered)
    pf_want = FO.fir(want[2][:, None, :], half, 3)[:, 0]
    assert np.array_equal(bits(host["pose_filtered"]), bits(pf_want))
    assert (host["pose_filtered"][:, 0] == 3).all() and (host["trend"][:, 0] == 1).all()
    mid = slice(k_taps, n - k_taps)
    tilt_want = np.degrees(np.arctan(np.hypot(pf_want[:, 1], pf_want[:, 2])))
    assert np.abs(host["trend"][:, 1] - tilt_want).max() <= 1e-12
    worst = float(np.abs(host["trend"][mid, 1] - ramp[mid]).max())
    print(f"worst |trend tilt - ramp| = {worst:.4f} deg (bound {O.TREND_TOL_DEG})")
    assert worst <= O.TREND_TOL_DEG
    assert np.abs(host["trend"][n // 2:n - k_taps, 2] - 30.0).max() < 1.0
    bare = misalignment_analysis(eng, torch.from_numpy(t).cuda(), torch.from_numpy(t_ref).cuda(), ref, reject_k=3.0)
    assert set(bare) == {"ref_disp", "deviation", "field", "pose"} and np.array_equal(bits(bare["pose"].cpu().numpy()), bits(host["pose"]))
    with pytest.raises(ValueError):
        misalignment_analysis(eng, torch.from_numpy(t).cuda(), torch.from_numpy(t_ref).cuda(), ref, ref_end=3)
    # the sheet
    path = tmp_path / "pose_misalignment.xlsx"
    df = to_pose_frame(res["field"], res["pose"], res["pose_filtered"], path=path)
    back = read_xlsx(path)
    assert tuple(back.columns) == POSE_FRAME_COLUMNS + POSE_TREND_COLUMNS and len(back) == n
    for col in df.columns:
        assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64), equal_nan=True), col
    assert np.array_equal(df["a_f"].to_numpy(), host["pose_filtered"][:, 1]) and np.array_equal(df["rms"].to_numpy(), host["pose"][:, 6])
