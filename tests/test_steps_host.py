"""CPU tests of the probe-indentation analysis' host side (no GPU): the new C symbols and what they refuse, the NumPy restatement
the GPU tests hold the device to bit for bit (`tests/helpers/step_oracle.py`) against sides that do not share its order
(`np.convolve`, `math.fsum`), the published Figure 6(b) on the restatement alone, and the sheet.  Bounds: see the helper."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import step_oracle as O                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbs_step_response_f64", "vbs_find_steps_f64", "vbs_dwell_stats_f64")


def _rec(n, s, cols, seed, gaps=0.0):
    rng = np.random.default_rng(seed)
    rec = rng.normal(0.0, 3.0, (n, s, cols))
    rec[..., 0] = (rng.random((n, s)) >= gaps).astype(np.float64)
    return rec


def test_new_header_symbols_are_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.STEP_MAX_WINDOW, L.STEP_MAX_STEPS) == (defs["VBS_STEP_MAX_WINDOW"], defs["VBS_STEP_MAX_STEPS"]) == (64, 64)
    assert (O.MAX_WINDOW, O.MAX_STEPS) == (64, 64)


def test_entries_refuse_bad_arguments_before_touching_a_device():
    """Every VBS_EINVAL condition is decided on the host, ahead of hipSetDevice: checkable without a GPU (non-null dummies)."""
    lib = L.lib()
    p = C.c_void_p(8)

    def response(rec=p, n=10, s=2, cols=4, nv=3, w=4, mc=2, out=p):
        return lib.vbs_step_response_f64(0, rec, n, s, cols, nv, w, mc, out, None)
    for kw in (dict(w=0, mc=0), dict(w=65, mc=1), dict(mc=0), dict(mc=5), dict(w=-1, mc=-1), dict(cols=9), dict(cols=1, nv=1),
               dict(nv=4), dict(nv=0), dict(n=0), dict(s=0), dict(rec=None), dict(out=None)):
        assert response(**kw) == L.VBS_EINVAL, kw

    def find(resp=p, n=10, s=2, cols=5, w=4, thr2=0.1, ms=8, steps=p):
        return lib.vbs_find_steps_f64(0, resp, n, s, cols, w, thr2, ms, steps, None)
    for kw in (dict(w=0), dict(w=65), dict(thr2=float("nan")), dict(thr2=-1.0), dict(ms=0), dict(ms=65), dict(cols=1), dict(cols=10),
               dict(n=0), dict(s=0), dict(resp=None), dict(steps=None)):
        assert find(**kw) == L.VBS_EINVAL, kw

    def dwell(rec=p, n=10, s=2, cols=4, nv=3, steps=p, rows=2, ms=8, guard=1, out=p):
        return lib.vbs_dwell_stats_f64(0, rec, n, s, cols, nv, steps, rows, ms, guard, out, None)
    for kw in (dict(rows=0), dict(rows=3), dict(ms=0), dict(ms=65), dict(guard=-1), dict(cols=9), dict(nv=4), dict(nv=0), dict(n=0),
               dict(s=0), dict(rec=None), dict(steps=None), dict(out=None)):
        assert dwell(**kw) == L.VBS_EINVAL, kw


@pytest.mark.parametrize("w", (1, 2, 8, 64))
def test_response_against_np_convolve_on_gap_free_data(w):
    rec = _rec(3 * w + 70, 3, 3, w)
    out = O.response(rec, w)
    worst = O.check_response_gap_free(out, rec, w)
    print(f"w = {w}: worst |r - convolve| / bound = {worst:.3f}")
    mc = (w + 1) // 2                                        # fewer frames than that on a side: not ok, all zero
    assert (out[:mc] == 0).all() and (out[mc:-mc + 1 or None, :, 0] == 1).all() and (out[rec.shape[0] - mc + 1:] == 0).all()
    r = out[..., 2:]
    assert np.array_equal(out[..., 1], r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])


def test_response_counts_gaps_and_never_reads_an_invalid_entry():
    rec = _rec(90, 5, 4, 2, 0.4)
    rec[:, 3, 0] = 0.0                                       # a series never seen
    junk = rec[..., 0] == 0
    rec[..., 1:][junk] = np.nan
    for w, mc in ((8, None), (8, 8), (8, 1), (3, 2)):
        out = O.response(rec, w, 3, mc)
        assert not np.isnan(out).any() and (out[:, 3] == 0).all()
        need = (w + 1) // 2 if mc is None else mc
        v = rec[..., 0] != 0
        for f in (0, 5, 44, 89):
            for i in (0, 4):
                left, right = v[max(0, f - w):f, i], v[f:f + w, i]
                ok = left.sum() >= need and right.sum() >= need
                assert out[f, i, 0] == ok
                if ok:
                    want = rec[f:f + w, i, 1:4][right].mean(axis=0) - rec[max(0, f - w):f, i, 1:4][left].mean(axis=0)
                    assert np.abs(out[f, i, 2:] - want).max() <= 64 * O.U2 * np.abs(rec[..., 1:][~junk]).max()


def test_find_steps_rules_on_hand_made_scores():
    def steps_of(score, ok=None, w=2, thr2=1.0, ms=8):
        score = np.asarray(score, dtype=np.float64)
        ok = np.ones_like(score) if ok is None else np.asarray(ok, dtype=np.float64)
        st = O.find_steps(np.stack([ok, score], axis=1)[:, None, :], w, thr2, ms)[0]
        return int(st[0]), st[1:1 + min(int(st[0]), ms)].tolist()
    assert steps_of([0, 3, 0, 0, 0, 2, 0]) == (2, [1, 5])
    assert steps_of([0, 3, 0, 2, 0, 0, 0]) == (1, [1])                     # inside the window of a larger one
    assert steps_of([0, 3, 3, 3, 0, 0, 0]) == (1, [1])                     # the earliest of equal maxima ...
    assert steps_of([3, 0, 0, 3, 0, 0, 3]) == (3, [0, 3, 6])               # ... equal ones further apart than w all count
    assert steps_of([0, 3, 0, 0, 0, 0.5, 0]) == (1, [1])                   # below the threshold
    assert steps_of([0, 1, 0, 0, 0, 0, 0]) == (1, [1])                     # at the threshold
    assert steps_of([0, 3, 9, 0, 0, 0, 0], ok=[1, 1, 0, 1, 1, 1, 1]) == (1, [1])         # what is not ok does not suppress
    assert steps_of([0, 3, np.nan, 0, 0, np.nan, 0]) == (1, [1])           # NaN neither suppresses nor is a step
    assert steps_of([5, 0, 0] * 5, ms=4) == (5, [0, 3, 6, 9])              # an overflow: counted, four kept
    st = O.find_steps(np.zeros((4, 2, 2)), 2, 0.0, 3)
    assert (st[:, 0] == 0).all() and (st[:, 1:] == -1).all()


def test_dwell_stats_against_fsum_and_their_edges():
    rec = _rec(300, 4, 4, 9, 0.1)
    rec[..., 1:][rec[..., 0] == 0] = np.nan
    steps = np.full((4, 9), -1, dtype=np.int32)
    steps[0, :4] = (3, 40, 41, 170)                          # dwells of 40 - 2 g, 1 - 2 g, 129 - 2 g, 130 - g frames
    steps[1, :1] = 0                                         # no step: one dwell, the whole series
    steps[2, :9] = (12, 10, 20, 30, 40, 50, 60, 70, 80)      # an overflow: 8 kept, the last dwell runs to the end
    steps[3, :3] = (2, 0, 299)
    for guard in (0, 1, 8):
        st = O.dwell_stats(rec, steps, guard, 3)
        O.check_dwell_means(st, rec, 3)
        assert st[0, 1, 2] == (1 if guard == 0 else 0) or rec[40, 0, 0] == 0
        assert (st[0, 4:, 0] == -1).all() and np.isnan(st[0, 4:, 3:]).all() and (st[0, 4:, 2] == 0).all()
        assert (st[1, 0, :2] == (0, 300)).all() and (st[1, 1:, 0] == -1).all()
        assert st[2, 8, 0] == 80 + guard and st[2, 8, 1] == 300
        assert (st[3, 0, :3] == (0, 0, 0)).all() and np.isnan(st[3, 0, 3:6]).all() and (st[3, 0, 6:] == 0).all()
        std = O.dwell_std(st, 3)
        for j in range(4):
            b, e, c = (int(v) for v in st[0, j, :3])
            x = rec[b:e, 0, 1][rec[b:e, 0, 0] != 0]
            if c >= 2:                                       # two-pass M2 against NumPy's own two-pass variance
                assert abs(std[0, j, 0] - x.std(ddof=1)) <= 4 * c * O.U2 * np.abs(x).max()
            else:
                assert np.isnan(std[0, j, 0])
    shared = O.dwell_stats(rec, steps[:1], 1, 3)
    assert O.same(shared, O.dwell_stats(rec, np.repeat(steps[:1], 4, axis=0), 1, 3))


CASES = {(24, 0, 0.0): [24 * k for k in range(1, 13)],
         (24, 3, 0.02): [25, 52, 80, 106, 133, 160, 187, 215, 241, 269, 295, 322]}


@pytest.mark.parametrize("dwell,ramp,noise", sorted(CASES))
def test_figure_6b_on_the_restatement(dwell, ramp, noise):
    """The published bar heights as a synthetic recording: 12 steps where they are, 13 levels, 12 errors.  The means are held to
    noise / count (an odd count leaves one +-noise over; an even count nothing) plus the rounding of the sum itself,
    count 2^-52 max|x|, without which the odd counts - whose exact deviation EQUALS noise / count - fail by their last bits."""
    window, guard, threshold = 8, 8, 0.35
    assert ramp < window                                     # a longer ramp lowers the response below the threshold
    z, begins = O.figure6_signal(dwell, ramp, noise)
    assert z.size == 13 * dwell + 12 * ramp and begins.tolist() == [k * (dwell + ramp) for k in range(13)]
    rec = np.stack([np.ones(z.size), z], axis=1)[:, None, :]
    a = O.analyse(rec, window, threshold, guard, O.STEP_MM)
    assert a["step_frames"].tolist() == CASES[(dwell, ramp, noise)] and not a["overflow"]
    assert (a["count"] >= dwell - 2 * guard - ramp).all()
    for k in range(13):                                      # every dwell lies inside the flat part it measures
        assert begins[k] <= a["begin"][k] and a["end"][k] <= begins[k] + dwell
    bound = noise / a["count"] + a["count"] * O.U2 * np.abs(z).max()
    print("mean - level:", a["cumulative"] - O.LEVELS)
    assert (np.abs(a["cumulative"] - O.LEVELS) <= bound).all()
    print("abs_error - figure:", a["abs_error"] - O.ERRORS)
    assert (np.abs(a["abs_error"] - O.ERRORS) <= 0.005).all()
    if noise == 0:
        assert (a["std"] == 0).all()
    else:                                                    # an alternating +-noise: std is noise sqrt(c / (c - 1)) or just below
        assert (a["std"] <= noise * np.sqrt(a["count"] / (a["count"] - 1.0)) * (1 + 1e-12)).all() and (a["std"] > 0.9 * noise).all()


def test_the_golden_figure_is_consistent_with_itself():
    assert O.LEVELS.size == 13 and O.ERRORS.size == 12 and O.STEP_MM == 0.7
    assert O.FIGURE["image"] == "img/Sensor_Error_Analysis.png"
    assert (np.abs(np.abs(np.diff(O.LEVELS) - O.STEP_MM) - O.ERRORS) < 1e-12).all()


def test_to_step_frame_schema_nan_row_and_xlsx_round_trip(tmp_path):
    from vbs_amd.pipeline import IndentationResult, to_step_frame
    from vbs_amd.xlsx_io import read_xlsx
    z, _ = O.figure6_signal(24, 3, 0.02)
    a = O.analyse(np.stack([np.ones(z.size), z], axis=1)[:, None, :], 8, 0.35, 8, O.STEP_MM)
    res = IndentationResult(step_mm=O.STEP_MM, component="z", step_frames=a["step_frames"], begin=a["begin"], end=a["end"],
                            count=a["count"], cumulative=a["cumulative"], std=a["std"], delta=a["delta"], abs_error=a["abs_error"],
                            marker_means=np.zeros((1, 13, 3)), overflow=False)
    path = tmp_path / "indentation_steps.xlsx"
    df = to_step_frame(res, path=path)
    assert list(df.columns) == ["step", "frame_first", "frame_last", "count", "cumulative_mm", "std_mm", "step_mm", "abs_error_mm"]
    assert len(df) == 13 and df["step"].tolist() == list(range(13)) and df["count"].dtype == np.int64
    assert np.isnan(df["step_mm"][0]) and np.isnan(df["abs_error_mm"][0]) and not df.iloc[1:].isna().any().any()
    assert np.array_equal(df["step_mm"].to_numpy()[1:], a["delta"]) and np.array_equal(df["abs_error_mm"].to_numpy()[1:], a["abs_error"])
    assert df["frame_first"][1] == a["begin"][1] and df["frame_last"][1] == a["end"][1] - 1
    back = read_xlsx(path)
    assert list(back.columns) == list(df.columns) and len(back) == 13
    for c in df.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64), equal_nan=True), c
