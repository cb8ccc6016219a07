"""GPU tests of the probe-indentation analysis (k_steps.hip; run on the MI355X box: `pytest -m gpu`): the step response, the peak
search, the dwell statistics and `pipeline.indentation_analysis`.

Every result is held BIT FOR BIT to the NumPy restatement (`tests/helpers/step_oracle.py`: the same IEEE operations in the same
order; NaN where NaN, the same bits elsewhere); std, taken in Python on both sides, to 4 ulp.  Shapes are the smallest at which a
kernel can go wrong: around the window, around the tiles (64 or 32 frames x 64 series) and around the 64 lanes of the fold, not
the workload's.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as FO                                    # noqa: E402
import step_oracle as O                                       # noqa: E402

COLS = ((2, 1), (4, 1), (4, 3), (5, 1), (5, 3), (5, 4), (8, 1), (8, 3), (8, 7))    # n_values in {1, 3, cols - 1}
KINDS = ("none", "3 %", "40 %", "3 % and a dead series", "40 % and a dead series")


def response_dev(rec, w, nv=None, mc=None):
    from vbs_amd.engine import step_response_f64
    return step_response_f64(torch.from_numpy(rec).cuda(), w, nv, mc).cpu().numpy()


def steps_dev(resp, w, thr, ms=L.STEP_MAX_STEPS):
    from vbs_amd.engine import find_steps_f64
    return find_steps_f64(torch.from_numpy(resp).cuda(), w, thr, ms).cpu().numpy()


def dwell_dev(rec, steps, guard, nv=None):
    from vbs_amd.engine import dwell_stats_f64
    return dwell_stats_f64(torch.from_numpy(rec).cuda(), torch.from_numpy(steps).cuda(), guard, nv).cpu().numpy()


def std_within_4_ulp(got, want, nv):
    a, b = O.dwell_std(got, nv), O.dwell_std(want, nv)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and (np.abs(a - b)[~nan] <= 4 * np.spacing(np.abs(b[~nan]))).all()


def make_rec(rng, n, s, cols, kind):
    """[n, s, cols] float64: per series a staircase (jumps of a few units every so often) plus noise, with the gaps of `kind`;
    NaN and 1e30 in EVERY invalid entry (and random numbers in the columns past the values)."""
    jumps = np.where(rng.random((n, s, cols)) < 0.08, rng.normal(0.0, 4.0, (n, s, cols)), 0.0)
    rec = np.cumsum(jumps, axis=0) + rng.normal(0.0, 0.1, (n, s, cols))
    valid = np.ones((n, s), dtype=bool)
    if "3 %" in kind:
        valid &= rng.random((n, s)) >= 0.03
    if "40 %" in kind:
        valid &= rng.random((n, s)) >= 0.4
    if "dead" in kind:
        valid[:, s - 1] = False
    rec[..., 0] = np.where(valid, rng.choice([1.0, 2.0, -1.0, 1e-300], (n, s)), 0.0)       # any nonzero flag is valid
    junk = np.where(rng.random((n, s, cols - 1)) < 0.5, np.nan, 1e30)
    rec[..., 1:] = np.where(valid[..., None], rec[..., 1:], junk)
    return rec


def check_chain(rec, w, nv, mc, thr, guard, ms, what):
    """response -> steps -> dwell statistics of the device against the restatement, each stage on the stage before of the
    RESTATEMENT (equal bits, once shown, make the two the same input)."""
    resp = response_dev(rec, w, nv, mc)
    want = O.response(rec, w, nv, mc)
    assert not np.isnan(resp).any(), what
    assert resp.shape == want.shape and O.same(resp, want), f"{what}: response, {int((resp != want).sum())} entries differ"
    steps = steps_dev(want, w, thr, ms)
    want_steps = O.find_steps(want, w, thr * thr, ms)
    assert steps.dtype == np.int32 and np.array_equal(steps, want_steps), f"{what}: steps"
    st = dwell_dev(rec, want_steps, guard, nv)
    want_st = O.dwell_stats(rec, want_steps, guard, nv)
    assert O.same(st, want_st), f"{what}: dwell statistics"
    assert std_within_4_ulp(st, want_st, nv), f"{what}: std"
    return want, want_steps, want_st


@pytest.mark.parametrize("w", (1, 2, 8, 64))
def test_chain_equals_the_restatement_on_every_edge_shape(w):
    """n around the window and around the tile, s around the wave: every (n, s) pair, with the cols / n_values, the kinds of
    gap (9 and 5 are coprime: every combination of the two is met over the four windows), min_count and the guard rotating."""
    rng = np.random.default_rng(w)
    ns = sorted({1, 2, w, max(1, 2 * w - 1), 2 * w, 2 * w + 1, 63, 64, 65, 197})
    i, found, dwells = w, 0, 0
    for n in ns:
        for s in (1, 63, 64, 65, 130):
            (cols, nv), kind = COLS[i % 9], KINDS[i % 5]
            mc = (None, 1, w)[i % 3]
            guard = (0, 1, w)[(i // 3) % 3]
            i += 1
            rec = make_rec(rng, n, s, cols, kind)
            resp, steps, st = check_chain(rec, w, nv, mc, 1.0, guard, 16, f"w {w} n {n} s {s} cols {cols} nv {nv} {kind}")
            found += int(steps[:, 0].sum())
            dwells += int((st[..., 2] > 0).sum())
            if "dead" in kind:
                assert (resp[:, s - 1] == 0).all() and steps[s - 1, 0] == 0 and (steps[s - 1, 1:] == -1).all()
                assert (st[s - 1, 0, :3] == (0, n, 0)).all() and np.isnan(st[s - 1, 0, 3:3 + nv]).all()
    print(f"w = {w}: {i - w} shapes, {found} steps, {dwells} populated dwells")
    assert found > 0 and dwells > 0


def test_ties_the_earliest_wins_also_across_a_tile_boundary():
    """Integer-valued staircases, a power-of-two window, no gaps: every sum and quotient is exact, so a jump taken in two equal
    halves (x[c] half way) gives EXACTLY equal scores at c and c + 1.  c = 63, 127: the pair straddles the finder's 64-frame
    tiles; c = 31: the response's 32-frame tile (n_values > 3)."""
    w, n = 8, 200
    for cols, nv in ((2, 1), (4, 3), (8, 7)):
        rec = np.zeros((n, 66, cols))
        rec[..., 0] = 1.0
        cs = (31, 63, 100, 127, 160)
        for k, c in enumerate(cs):
            for v in range(nv):
                h = 4.0 * (k + 1) * (1 if v % 2 == 0 else -1)
                rec[c, :, 1 + v] += h / 2
                rec[c + 1:, :, 1 + v] += h
        rec[:, 65, 1:] *= 3.0
        resp, steps, _ = check_chain(rec, w, nv, None, 1.0, w, 8, f"ties cols {cols}")
        for c in cs:
            assert (resp[c, :, 1] == resp[c + 1, :, 1]).all() and (resp[c, :, 1] > 0).all()
        assert (steps[:, 0] == len(cs)).all() and (steps[:, 1:1 + len(cs)] == np.asarray(cs)[None, :]).all()
    # equal jumps exactly w + 1 apart are both steps; w apart, the later one lies in the earlier one's window and loses the tie
    rec = np.zeros((n, 1, 2))
    rec[..., 0] = 1.0
    for c in (40, 49, 120, 128):
        rec[c:, 0, 1] += 5.0
    _, steps, _ = check_chain(rec, w, 1, None, 1.0, 0, 8, "ties at the window's edge")
    assert steps[0, :5].tolist() == [3, 40, 49, 120, -1]


def test_overflow_is_counted_and_four_frames_are_stored():
    w, n, s = 2, 197, 65
    rec = np.zeros((n, s, 2))
    rec[..., 0] = 1.0
    rec[..., 1] = (np.arange(n)[:, None] // 6 % 2) * 3.0 + np.arange(s)[None, :]        # a step every 6 frames
    resp, steps, st = check_chain(rec, w, 1, None, 1.0, 1, 4, "overflow")
    assert (steps[:, 0] == (n - 1) // 6).all() and (steps[:, 1:] == np.asarray([6, 12, 18, 24])[None, :]).all()
    assert (st[:, 4, 0] == 25).all() and (st[:, 4, 1] == n).all()                        # the last dwell kept runs over the rest
    full = steps_dev(resp, w, 1.0)
    assert np.array_equal(full, O.find_steps(resp, w, 1.0)) and (full[:, 1 + 32] == -1).all() and (full[:, 32] == 192).all()


@pytest.mark.parametrize("guard", (0, 1, 8, 70))
def test_dwell_lengths_around_the_fold_and_guards(guard):
    """Dwells of 0, 1, 2, 63, 64, 65 and 130 frames at guard 0 (lane sums of one or three rounds, lanes with nothing); a guard
    longer than a dwell leaves count 0 and NaN."""
    rng = np.random.default_rng(guard)
    n, s = 330, 66
    rec = make_rec(rng, n, s, 5, "3 %")
    rec[:, 1, 0] = 1.0                                       # one series without gaps: its counts are the lengths
    rec[:, 1, 1:] = rng.normal(5.0, 2.0, (n, 4))
    own = np.full((s, 9), -1, dtype=np.int32)
    own[:, :8] = (7, 0, 1, 3, 66, 130, 195, 325)
    own[2, :8] = (7, 1, 2, 4, 67, 131, 196, 326)             # each series reads ITS row
    for steps in (own, own[:1].copy()):
        got, want = dwell_dev(rec, steps, guard, 3), O.dwell_stats(rec, steps, guard, 3)
        assert O.same(got, want) and std_within_4_ulp(got, want, 3)
        O.check_dwell_means(got, rec, 3)
        lengths = np.maximum(0, np.asarray([0, 1, 2, 63, 64, 65, 130, 5]) - guard * np.asarray([1, 2, 2, 2, 2, 2, 2, 1]))
        assert got[1, :8, 2].tolist() == lengths.tolist()
        assert np.isnan(got[1, :8, 3][lengths == 0]).all() and (got[1, :8, 6:][lengths == 0] == 0).all()
        assert (got[:, 8, 0] == -1).all() and np.isnan(got[:, 8, 3:]).all()
    shared = dwell_dev(rec, own[:1].copy(), guard, 3)
    assert O.same(shared, dwell_dev(rec, np.repeat(own[:1], s, axis=0), guard, 3))       # one shared list = the list s times
    assert not O.same(shared[2], dwell_dev(rec, own, guard, 3)[2])


def test_runs_and_neighbours_do_not_change_a_bit():
    rng = np.random.default_rng(5)
    n, s, w = 197, 130, 8
    rec = make_rec(rng, n, s, 4, "3 %")
    resp, steps, st = check_chain(rec, w, 3, None, 1.0, w, 16, "s = 130")
    assert O.same(response_dev(rec, w, 3), resp) and np.array_equal(steps_dev(resp, w, 1.0, 16), steps)      # two runs
    assert O.same(dwell_dev(rec, steps, w, 3), st)
    for j in (0, 63, 64, 65, 129):                           # a series alone
        one = np.ascontiguousarray(rec[:, j:j + 1])
        r1 = response_dev(one, w, 3)
        assert O.same(r1[:, 0], resp[:, j]), j
        s1 = steps_dev(r1, w, 1.0, 16)
        assert np.array_equal(s1[0], steps[j]), j
        assert O.same(dwell_dev(one, s1, w, 3)[0], st[j]), j


def test_wrappers_refuse_bad_arguments():
    from vbs_amd.engine import dwell_stats_f64, find_steps_f64, step_response_f64
    rec = torch.ones((10, 2, 4), dtype=torch.float64, device="cuda")
    resp = step_response_f64(rec, 4)
    assert resp.shape == (10, 2, 5) and step_response_f64(rec, 64, 1, 64).shape == (10, 2, 3)
    steps = find_steps_f64(resp, 4, 0.5)
    assert steps.shape == (2, 65) and steps.dtype == torch.int32 and find_steps_f64(resp, 64, 0.0, 1).shape == (2, 2)
    assert dwell_stats_f64(rec, steps, 0).shape == (2, 65, 9) and dwell_stats_f64(rec, steps[:1], 3, 1).shape == (2, 65, 5)
    for kw in (dict(window=0), dict(window=65), dict(min_count=0), dict(min_count=5), dict(n_values=4), dict(n_values=0),
               dict(rec=torch.ones((10, 2, 9), dtype=torch.float64, device="cuda")),
               dict(rec=torch.ones((10, 2, 1), dtype=torch.float64, device="cuda")),
               dict(rec=torch.ones((10, 8), dtype=torch.float64, device="cuda"))):
        args = dict(rec=rec, window=4)
        args.update(kw)
        with pytest.raises(ValueError):
            step_response_f64(**args)
    for kw in (dict(window=0), dict(window=65), dict(threshold=float("nan")), dict(max_steps=0), dict(max_steps=65),
               dict(resp=torch.ones((10, 2, 1), dtype=torch.float64, device="cuda")),
               dict(resp=torch.ones((10, 2, 10), dtype=torch.float64, device="cuda")),
               dict(resp=torch.ones((10, 2), dtype=torch.float64, device="cuda"))):
        args = dict(resp=resp, window=4, threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            find_steps_f64(**args)
    for kw in (dict(guard=-1), dict(n_values=4), dict(n_values=0), dict(steps=steps[:, :1]), dict(steps=steps[0]),
               dict(steps=torch.zeros((3, 9), dtype=torch.int32, device="cuda")),
               dict(steps=torch.zeros((2, 66), dtype=torch.int32, device="cuda")),
               dict(rec=torch.ones((10, 2, 9), dtype=torch.float64, device="cuda"))):
        args = dict(rec=rec, steps=steps, guard=1)
        args.update(kw)
        with pytest.raises(ValueError):
            dwell_stats_f64(**args)


# ---------------------------------------------------------------------------------------------------------------------
def figure6_table(rng, m, slots, dwell, ramp, noise):
    """A float32 table [n, m, 10]: the selected slots sit at their own (X, Y, Z) and all move in Z by the figure's signal; the
    others wander; 3 % of the rows (frame 0 apart) lack VBS_FLAG_XYZ and hold 1e30 where no 3-D point is."""
    z, begins = O.figure6_signal(dwell, ramp, noise)
    n = z.size
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = np.where(rng.random((n, m)) >= 0.03, 3.0, 1.0)
    t[0, :, 0] = 3.0
    base = rng.uniform(-20.0, 20.0, (m, 3))
    t[..., 6:9] = (base[None] + np.cumsum(rng.normal(0.0, 0.3, (n, m, 3)), axis=0)).astype(np.float32)
    for j in slots:
        t[:, j, 6] = np.float32(base[j, 0])
        t[:, j, 7] = np.float32(base[j, 1])
        t[:, j, 8] = (base[j, 2] + z).astype(np.float32)
    t[..., 6:9][t[..., 0] != 3.0] = np.float32(1e30)
    return t, z, begins


@pytest.mark.parametrize("component", ("z", "xyz"))
def test_indentation_analysis_on_the_figure_6b_signal(component, tmp_path):
    from vbs_amd.engine import Engine
    from vbs_amd.pipeline import indentation_analysis, to_step_frame
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    rng = np.random.default_rng(6)
    dwell, ramp, noise, window, guard, m = 24, 3, 0.02, 8, 8, 65
    slots = np.asarray([0, 3, 17, 31, 40, 52, 63, 64])
    t, z, begins = figure6_table(rng, m, slots, dwell, ramp, noise)
    n = z.size
    res = indentation_analysis(eng, torch.from_numpy(t).cuda(), O.STEP_MM, window, slots=slots, component=component)
    # the restatement chain
    mask = np.zeros(m, dtype=bool)
    mask[slots] = True
    axis, total = FO.axis_total(t, 0, mask)
    cols = {"z": [3], "xyz": [1, 2, 3]}[component]
    with np.errstate(all="ignore"):
        series = np.concatenate([total[:, 0:1], total[:, cols] / total[:, 4:5]], axis=1)[:, None, :]
    a = O.analyse(series, window, O.STEP_MM / 2, guard, O.STEP_MM)
    assert np.array_equal(res.step_frames, a["step_frames"]) and res.overflow is False
    for key in ("begin", "end", "count", "cumulative", "delta", "abs_error"):
        assert O.same(getattr(res, key), a[key]), key
    nan = np.isnan(a["std"])
    assert np.array_equal(np.isnan(res.std), nan) and (np.abs(res.std - a["std"])[~nan] <= 4 * np.spacing(a["std"][~nan])).all()
    per_marker = O.dwell_stats(axis, a["steps"], guard, 3)
    assert res.marker_means.shape == (m, 13, 3) and O.same(res.marker_means, per_marker[:, :13, 3:6])
    assert np.isnan(res.marker_means[~mask]).all() and not np.isnan(res.marker_means[mask]).any()
    # what the figure shows: 12 steps, each on its ramp (a dropout next to a ramp moves the peak by a frame or two) ...
    centre = begins[1:] - ramp + ramp // 2
    print("steps:", res.step_frames.tolist(), "counts:", res.count.tolist())
    assert res.step_frames.size == 12 and (np.abs(res.step_frames - centre) <= 3).all()
    # ... and the single-step errors.  Every kept frame of a dwell is level - z[0] +- noise; were no frame missing the signs
    # would alternate and leave at most one over: |mean - level| <= noise / count.  Each missing frame of the span can unbalance
    # the signs by one more, so with `miss` = end - begin - count the bound is noise (miss + 1) / count; the table is float32:
    # Z and Z_ref are each rounded once, 2 * 2^-24 * max|Z|; the float64 sums add count 2^-52 max|d|, far below.  A step's
    # error has the bounds of its two dwells.  Stated with the smallest count and the largest miss, so one number holds for all:
    miss = (a["end"] - a["begin"] - a["count"]).max()
    c_min = a["count"].min()
    f32 = 2 * 2.0 ** -24 * float(np.abs(t[:, slots, 8][t[:, slots, 0] == 3.0]).max())
    bound = 2 * (noise * (miss + 1) / c_min + f32 + c_min * O.U2 * 10.0)
    print(f"smallest count {c_min}, most missing {miss}: bound {bound:.5f}; worst {np.abs(res.abs_error - O.ERRORS).max():.5f}")
    # ("xyz" is a norm: dwell 0 lies at -noise against frame 0 and is folded to +noise, so its first step is left out there)
    first = 0 if component == "z" else 1
    assert c_min >= 4 and (np.abs(res.abs_error - np.abs(np.diff(O.LEVELS) - O.STEP_MM))[first:] <= bound).all()
    df = to_step_frame(res, path=tmp_path / "indentation_steps.xlsx")
    assert len(df) == 13 and np.isnan(df["abs_error_mm"][0]) and np.array_equal(df["abs_error_mm"].to_numpy()[1:], res.abs_error)
    eng.close()
