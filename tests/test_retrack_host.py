"""Host tests of the re-tracker (no GPU): the two forms of the rule's restatement against each other, the recording the rule was
made for, the pieces of `vbs_amd.retrack`, the wrapper's checker, and `vbs_retrack`'s refusals, which come before a device is
selected (device -1, dummy pointers)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from vbs_amd import _lib as L
from vbs_amd import retrack as R

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import retrack_oracle as O                                    # noqa: E402


# ---- the rule: the sort is the definition, the rounds are what the kernel runs ----------------------------------------------------
def _lattice_cases(n_cases=300, seed=1):
    rng = np.random.default_rng(seed)
    for _ in range(n_cases):
        m, cnt = int(rng.integers(1, 31)), int(rng.integers(0, 31))
        q = rng.integers(0, 12, (m, 2)).astype(np.float64)
        xy = rng.integers(0, 12, (cnt, 2)).astype(np.float64)
        yield O.candidates(q, q, xy, 4.0, np.inf)


def test_sort_form_equals_round_form_on_tie_heavy_lattices():
    """Integer coordinates from a 12 x 12 lattice, gate 4: exact ties of d2 across slots and across detections everywhere.  The
    rounds in which a detection chooses among ALL free slots that hold it equal the sort; the form in which it chooses among
    the slots that named it does not, and a bounded number of rounds is enough."""
    namers_differ, most_rounds, ties = 0, 0, 0
    for d2 in _lattice_cases():
        a = O.match_sorted(d2)
        b, rounds = O.match_rounds(d2)
        assert np.array_equal(a, b)
        assert rounds <= min(d2.shape) + 1
        taken = a[a >= 0]
        assert len(set(taken.tolist())) == taken.size                # one-to-one
        namers_differ += not np.array_equal(a, O.match_rounds(d2, only_namers=True)[0])
        most_rounds = max(most_rounds, rounds)
        v = d2[d2 >= 0]
        ties += v.size - np.unique(v).size
    assert ties > 1000 and most_rounds >= 3
    assert namers_differ > 0


# ---- the recording: 61 markers at pitch 40, a 45 px drag and 8 degrees of torsion, 3 % dropouts -----------------------------------
@pytest.fixture(scope="module")
def recording():
    det, counts, ref, truth = O.scenario(n=120, ramp=60, drag=45.0, torsion_deg=8.0, noise=0.05, dropout=0.03, seed=0)
    return det, counts, ref, truth, O.retrack(det, counts, ref, state=R.initial_state(ref), **R.DEFAULTS)


def test_scenario_retracker_has_no_wrong_and_no_missed_row_and_the_per_frame_rule_loses_a_quarter(recording):
    det, counts, ref, truth, res = recording
    assert ref.shape == (61, 2) and truth.shape == (120, 61) and (counts[1:] < 61).any()
    assert O.score(res["assign"], truth) == (0, 0)
    legacy = O.legacy_track(det, counts, ref, 20.0)
    wrong, missed = O.score(legacy, truth)
    assert wrong + missed >= 0.25 * truth.size                       # (measured: 3211 wrong + 2321 missed of 7320 = 75 %)
    # the same through compare_tables: the rows the two tables disagree on are the per-frame rule's errors
    lt = np.zeros_like(res["table"])
    f, s = np.nonzero(legacy >= 0)
    lt[f, s, 0], lt[f, s, 9] = 1.0, legacy[f, s]
    cmp_ = R.compare_tables(res["table"], lt)
    assert cmp_["total"]["differ"] + cmp_["total"]["only_a"] + cmp_["total"]["only_b"] == wrong + missed
    assert cmp_["same"].shape == (120,) and cmp_["same"][0] == 61
    assert cmp_["total"]["same"] + cmp_["total"]["differ"] + cmp_["total"]["only_a"] == int((res["assign"] >= 0).sum())


def test_scenario_round_form_and_ranges_give_the_same_bits(recording):
    det, counts, ref, truth, res = recording
    part = O.retrack(det[:40], counts[:40], ref, match=O.match_rounds)
    assert np.array_equal(part["assign"], res["assign"][:40])
    rest = O.retrack(det[40:], counts[40:], ref, state=part["state"])
    for key in ("assign", "table", "dist2", "info"):
        assert np.array_equal(rest[key], res[key][40:]), key
    assert np.array_equal(rest["state"].view(np.uint64), res["state"].view(np.uint64))


# ---- what the rule promises ---------------------------------------------------------------------------------------------------------
def _det(frames, max_det=4):
    det = np.zeros((len(frames), max_det, 6))
    counts = np.zeros(len(frames), dtype=np.int32)
    for f, pts in enumerate(frames):
        counts[f] = len(pts)
        for i, p in enumerate(pts):
            det[f, i, 0:2] = p
            det[f, i, 2:5] = (12.0, 11.0, 30.0)
    return det, counts


@pytest.mark.parametrize("gate", [10.0, 20.0])
def test_a_neighbours_detection_across_a_one_frame_dropout_goes_to_nobody(gate):
    """Two markers 15 px apart; the first drops out for one frame.  The per-frame rule hands its ID to the neighbour's detection
    (15 px < min_dist 20).  Here the detection is outside the gate (gate 10), or inside it but taken by its own slot (gate 20:
    the row is then counted as contested)."""
    a, b = (100.0, 100.0), (115.0, 100.0)
    det, counts = _det([[a, b], [b], [b, a]])
    ref = np.array([a, b])
    assert O.legacy_track(det, counts, ref).tolist() == [[0, 1], [0, 0], [1, 0]]
    res = O.retrack(det, counts, ref, gate=gate)
    assert res["assign"].tolist() == [[0, 1], [-1, 0], [1, 0]]
    assert res["info"].tolist() == [[1, 2, 2, 0], [1, 1, 2 if gate == 20.0 else 1, 1 if gate == 20.0 else 0], [1, 2, 2, 0]]
    assert res["dist2"][1].tolist() == [-1.0, 0.0]


def test_vel_gain_zero_holds_the_velocity_and_coasting_ends_after_max_coast():
    ref = np.array([[50.0, 50.0]])
    walk = [[(50.0 + 2.0 * f, 50.0)] for f in range(4)]
    det, counts = _det(walk + [[]] * 4)
    held = O.retrack(det[:4], counts[:4], ref, vel_gain=0.0)
    assert held["state"][0].tolist() == [56.0, 50.0, 0.0, 0.0, 0.0, 1.0]
    # vel_gain 1: v is the last step; the first match (seen == 0) leaves it at 0
    one = O.retrack(det[:1], counts[:1], ref, vel_gain=1.0)
    assert one["state"][0].tolist() == [50.0, 50.0, 0.0, 0.0, 0.0, 1.0]
    moving = O.retrack(det[:4], counts[:4], ref, vel_gain=1.0)
    assert moving["state"][0].tolist() == [56.0, 50.0, 2.0, 0.0, 0.0, 1.0]
    # unmatched frames: age counts up and v survives until age > max_coast
    for coast, frames, want_v, want_age in ((2, 2, 2.0, 2.0), (2, 3, 0.0, 3.0), (0, 1, 0.0, 1.0), (5, 4, 2.0, 4.0)):
        st = O.retrack(det[4:4 + frames], counts[4:4 + frames], ref, max_coast=coast, state=moving["state"])["state"][0]
        assert st.tolist() == [56.0, 50.0, want_v, 0.0, want_age, 1.0], (coast, frames)
    # the prediction runs ahead by v * (age + 1): after two missed frames the marker is found 6 px on, outside a gate around p
    back, cb = _det([[], [], [(62.0, 50.0)]])
    res = O.retrack(back, cb, ref, gate=1.0, state=moving["state"])
    assert res["assign"][:, 0].tolist() == [-1, -1, 0] and res["dist2"][2, 0] == 0.0
    assert res["state"][0].tolist() == [62.0, 50.0, 2.0, 0.0, 0.0, 1.0]        # ux = (62 - 56) / 3


def test_an_unusable_frame_and_a_count_above_max_det():
    ref = np.array([[10.0, 10.0], [30.0, 10.0]])
    det, counts = _det([[(10.0, 10.0), (30.0, 10.0)]] * 3, max_det=2)
    counts[1] = L.VBS_ECAPACITY
    counts[2] = 7                                                # above max_det: the rows there are
    res = O.retrack(det, counts, ref)
    assert res["info"].tolist() == [[1, 2, 2, 0], [0, 0, 0, 0], [1, 2, 2, 0]]
    assert res["assign"].tolist() == [[0, 1], [-1, -1], [0, 1]]


def test_initial_state_and_config_key():
    ref = np.array([[1.5, 2.5], [3.0, 4.0]])
    st = R.initial_state(ref)
    assert st.dtype == np.float64 and st.tolist() == [[1.5, 2.5, 0, 0, 0, 0], [3.0, 4.0, 0, 0, 0, 0]]
    assert np.array_equal(st, O.initial_state(ref)) and st.shape[1] == L.RETRACK_STATE_COLS
    assert R.params(None) is None and R.params(False) is None
    assert R.params(True) == R.DEFAULTS == {"gate": 10.0, "max_travel": float("inf"), "vel_gain": 0.5, "max_coast": 5}
    assert R.params({"gate": 6.0}) == {**R.DEFAULTS, "gate": 6.0}
    with pytest.raises(ValueError, match="unknown keys"):
        R.params({"gait": 6.0})
    with pytest.raises(ValueError):
        R.params(3)
    with pytest.raises(ValueError):
        R.compare_tables(np.zeros((2, 3, 10)), np.zeros((2, 4, 10)))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,text", [
    (dict(n=-1), "det must be"), (dict(m=0), "det must be"), (dict(m=L.RETRACK_MAX + 1), "VBS_RETRACK_MAX"),
    (dict(max_det=L.RETRACK_MAX + 1), "VBS_RETRACK_MAX"), (dict(gate=-1.0), "gate"), (dict(gate=float("nan")), "gate"),
    (dict(max_travel=float("nan")), "max_travel"), (dict(vel_gain=1.5), "vel_gain"), (dict(vel_gain=-0.1), "vel_gain"),
    (dict(vel_gain=float("nan")), "vel_gain"), (dict(max_coast=-1), "max_coast"), (dict(max_coast=2.5), "max_coast"),
    (dict(want=("assign", "rows")), "unknown outputs")])
def test_the_checker_refuses(defect, text):
    pytest.importorskip("torch")
    from vbs_amd.engine import _retrack_args
    good = dict(n=3, m=4, max_det=8, gate=10.0, max_travel=float("inf"), vel_gain=0.5, max_coast=5, want=("assign",))
    assert _retrack_args(**good) == (10.0, float("inf"), 0.5, 5, ("assign",))
    assert _retrack_args(**{**good, "want": "table", "gate": 0, "max_coast": 0})[3:] == (0, ("table",))
    with pytest.raises(ValueError, match=text):
        _retrack_args(**{**good, **defect})


P = C.c_void_p(64)                       # a pointer that is never followed: every case is answered before a device is selected
NULL = C.c_void_p(0)
GOOD = dict(det=P, counts=P, n=3, max_det=16, ref_xy=P, m_ref=4, state_in=NULL, gate=10.0, max_travel=float("inf"), vel_gain=0.5,
            max_coast=5, assign=P, table=P, dist2=P, info=P, state_out=P, workspace=P)


@pytest.mark.parametrize("defect,status", [
    (dict(det=NULL), L.VBS_EINVAL), (dict(counts=NULL), L.VBS_EINVAL), (dict(ref_xy=NULL), L.VBS_EINVAL),
    (dict(workspace=NULL), L.VBS_EINVAL), (dict(assign=NULL, table=NULL, state_out=NULL), L.VBS_EINVAL),
    (dict(n=-1), L.VBS_EINVAL), (dict(m_ref=0), L.VBS_EINVAL), (dict(max_det=0), L.VBS_EINVAL), (dict(gate=-0.5), L.VBS_EINVAL),
    (dict(gate=float("nan")), L.VBS_EINVAL), (dict(vel_gain=1.0001), L.VBS_EINVAL), (dict(vel_gain=-1e-9), L.VBS_EINVAL),
    (dict(vel_gain=float("nan")), L.VBS_EINVAL), (dict(max_coast=-1), L.VBS_EINVAL),
    (dict(m_ref=L.RETRACK_MAX + 1), L.VBS_ECAPACITY), (dict(max_det=L.RETRACK_MAX + 1), L.VBS_ECAPACITY),
    (dict(m_ref=L.RETRACK_MAX + 1, gate=-1.0), L.VBS_EINVAL),        # a bad argument comes before a capacity
    (dict(), L.VBS_EHIP),                                            # nothing wrong: only now is device -1 selected, and refused
    (dict(assign=NULL, dist2=NULL, info=NULL), L.VBS_EHIP), (dict(assign=NULL, table=NULL), L.VBS_EHIP)],
    ids=lambda v: ",".join(v) if isinstance(v, dict) else str(v))
def test_the_entry_answers_a_defect_before_it_selects_a_device(defect, status):
    args = {**GOOD, **defect}
    assert L.lib().vbs_retrack(-1, *args.values(), NULL) == status


def test_workspace_size_and_names():
    lib = L.lib()
    assert lib.vbs_retrack_workspace(-1, 4, 16) == L.VBS_EINVAL and lib.vbs_retrack_workspace(1, 0, 16) == L.VBS_EINVAL
    assert lib.vbs_retrack_workspace(1, 4, 0) == L.VBS_EINVAL
    assert lib.vbs_retrack_workspace(1, L.RETRACK_MAX + 1, 16) == L.VBS_ECAPACITY
    small, large = lib.vbs_retrack_workspace(0, 1, 1), lib.vbs_retrack_workspace(120, 61, 512)
    assert 0 < small <= 64 and large >= 120 * 61 * 4 + 120 * 2 * (1025 + 512)
    assert lib.vbs_retrack_workspace(240, 61, 512) > large
    # the record entries are the *_f64 symbols after vbs_fir_series_f64: these two are not among them
    for name in ("vbs_retrack", "vbs_retrack_workspace"):
        assert name in L.SYMBOLS and not name.endswith("_f64")
    assert (L.RETRACK_MAX, L.RETRACK_STATE_COLS, L.RETRACK_INFO_COLS) == (1024, 6, 4)
