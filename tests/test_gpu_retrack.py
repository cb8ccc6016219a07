"""GPU tests of the re-tracker (k_retrack.hip; run on the MI355X box: `pytest -m gpu`): `engine.retrack`, `pipeline.retrack_table`
and `MarkerTracker` with the `"retrack"` key.

An assignment plus a handful of stated IEEE operations has no order of summation, so EVERY output - assign, table, dist2, info,
state - is held BIT FOR BIT to the restatement of `tests/helpers/retrack_oracle.py` (the sort over (d2, j, i); the kernel runs
mutual rounds over a cell grid).  Shapes are the smallest at which the kernel can go wrong: slots around the wave and around the
workgroup sizes the walk is launched with (256, 512, 1024), detections at the table's ends, recordings of 1, 2 and 120 frames
(the double buffer), counts of 0, 1, max_det and above it.  Coordinates are multiples of 5 on a pitch of 40, so d2 ties across
slots and across detections are everywhere.  Every row of det at or beyond the count holds NaN or 1e300."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import retrack as R                              # noqa: E402
import vbs_amd.synth as S                                     # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import retrack_oracle as O                                    # noqa: E402

KEYS = ("assign", "table", "dist2", "info", "state")
PITCH = 40.0


def dev(det, counts, ref, tensors=True, **kw):
    from vbs_amd.engine import retrack
    if tensors:
        det, counts, ref = torch.from_numpy(det).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(ref).cuda()
        if kw.get("state") is not None:
            kw["state"] = torch.from_numpy(np.ascontiguousarray(kw["state"])).cuda()
    return {k: v.cpu().numpy() for k, v in retrack(det, counts, ref, **kw).items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, keys=KEYS, what=""):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{what}: {k} differs in {len(bad)} entries, first at {bad[0].tolist()}: " \
                              f"{got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


def checked(det, counts, ref, what="", **kw):
    got = dev(det, counts, ref, **kw)
    same(got, O.retrack(det, counts, ref, **kw), what=what)
    return got


def lattice_ref(m):
    side = int(np.ceil(np.sqrt(m)))
    k = np.arange(m)
    return np.stack([100.0 + PITCH * (k % side), 60.0 + PITCH * (k // side)], axis=1)


def make_case(rng, n, m, max_det, drift=(5.0, 0.0)):
    """A recording on the lattice: each marker drifts by `drift` per frame, is detected at its place or 5 px beside it, drops out
    now and then; false detections sit midway between two markers (the same d2 to both) and at random lattice points.  The
    counts walk through 0, 1, max_det, above max_det and everything between; rows at or beyond the count hold junk."""
    ref = lattice_ref(m)
    det = np.empty((n, max_det, 6))
    det[0::2], det[1::2] = np.nan, 1e300
    counts = np.zeros(n, dtype=np.int32)
    special = [max_det, 0, 1, max_det + 5]
    for f in range(n):
        pos = ref + np.asarray(drift) * f
        own = pos[rng.random(m) >= 0.1]
        own = own + 5.0 * rng.integers(-1, 2, own.shape)
        mid = pos[rng.random(m) < 0.3] + np.array([PITCH / 2, 0.0])
        far = np.stack([100.0 + 5.0 * rng.integers(-8, 8 * int(np.sqrt(m)) + 8, 8), 60.0 + 5.0 * rng.integers(-8, 80, 8)], axis=1)
        pts = np.concatenate([own, mid, far])
        pts = pts[rng.permutation(len(pts))]
        want = special[f // 2] if f % 2 == 1 and f // 2 < len(special) else int(rng.integers(0, max_det + 1))
        if f == 0:
            want = max_det
        cnt = min(want, max_det)
        while len(pts) < cnt:                                    # not enough: lattice points around the markers, duplicates too
            pts = np.concatenate([pts, pts + 5.0 * rng.integers(-2, 3, pts.shape)])
        pts = pts[:cnt]
        det[f, :cnt, 0:2] = pts
        det[f, :cnt, 2:6] = rng.uniform(5.0, 30.0, (cnt, 4))
        counts[f] = want
    return det, counts, ref


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 16), (1, 2, 1024), (61, 120, 512), (64, 2, 16), (65, 2, 1024), (130, 120, 16), (257, 2, 512), (257, 11, 1024),
          (1024, 1, 16), (1024, 2, 1024), (1024, 9, 512), (513, 3, 512)]


@pytest.mark.parametrize("gate", [10.0, 100.0])
@pytest.mark.parametrize("m,n,max_det", SHAPES)
def test_every_output_equals_the_restatement_bit_for_bit(m, n, max_det, gate):
    rng = np.random.default_rng(1000 * m + 10 * n + max_det + int(gate))
    det, counts, ref = make_case(rng, n, m, max_det)
    got = checked(det, counts, ref, what=f"m={m} n={n} max_det={max_det} gate={gate}", gate=gate)
    if gate == 100.0 and n >= 9:
        assert got["info"][:, 3].sum() > 0                         # contested slots: the ties and the shared candidates are there
    if n >= 9:
        assert (counts == 0).any() and (counts == 1).any() and (counts == max_det).any() and (counts > max_det).any()


@pytest.mark.parametrize("kw", [dict(gate=0.0), dict(gate=100.0, max_travel=60.0), dict(gate=30.0, vel_gain=0.0, max_coast=0),
                                dict(gate=30.0, vel_gain=1.0, max_coast=1), dict(gate=5000.0), dict(gate=float("inf")),
                                dict(gate=4095.0), dict(gate=7.0, max_travel=0.0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_parameters(kw):
    rng = np.random.default_rng(7)
    det, counts, ref = make_case(rng, 12, 130, 512, drift=(5.0, 5.0))
    got = checked(det, counts, ref, what=str(kw), **kw)
    if kw["gate"] == 0.0:
        assert got["info"][:, 1].sum() > 0 and (got["dist2"][got["assign"] >= 0] == 0.0).all()     # exact coincidences only
    if kw["gate"] >= 100.0 and "max_travel" not in kw:
        assert got["info"][:, 3].sum() > 50                        # many candidates per slot, chains of rounds


def edge_recording():
    """65 slots, 9 frames, every frame with its own trouble: negative coordinates throughout (the recording is shifted), NaN and
    inf coordinates, a frame with a detection beyond 2^30 cells (the plain scan; the others take the lists), a frame with a
    status instead of a count, a slot whose reference lies beyond 2^30 cells (that slot alone scans)."""
    rng = np.random.default_rng(11)
    det, counts, ref = make_case(rng, 9, 65, 512)
    det[..., 0:2] -= 1000.0
    ref = ref - 1000.0
    ref[64] = (3.0e13, -2.0e13)
    for f, i in ((1, 0), (2, 3), (2, 4), (6, 1)):
        counts[f] = max(counts[f], 8)
        det[f, :8, 2:6] = 7.0
        det[f, :8, 0:2] = np.where(np.abs(det[f, :8, 0:2]) < 1e6, det[f, :8, 0:2], ref[:8])
    det[2, 3, 0], det[2, 4, 1], det[6, 1, 0] = np.nan, np.inf, -np.inf
    counts[4] = L.VBS_ECAPACITY
    counts[5] = 300
    det[5, :300, 0:2] = np.where(np.abs(det[5, :300, 0:2]) < 1e6, det[5, :300, 0:2], ref[rng.integers(0, 64, 300)])
    det[5, :300, 2:6] = 9.0
    det[5, 17, 0:2] = (1.0e12, 5.0)                                  # 1e12 / 16 > 2^30: the whole frame scans
    det[5, 18, 0:2] = ref[64]                                       # and there the far slot finds its marker
    return det, counts, ref


def test_edges_lists_and_plain_scan_agree_with_the_restatement():
    det, counts, ref = edge_recording()
    got = checked(det, counts, ref, what="edges")
    assert got["info"][4].tolist() == [0, 0, 0, 0] and got["info"][5, 0] == 1
    assert got["assign"][5, 64] == 18 and (got["assign"][[0, 1, 2, 3, 6, 7, 8], 64] == -1).all()
    assert not (got["assign"][2] == 3).any() and not (got["assign"][2] == 4).any() and not (got["assign"][6] == 1).any()
    # the frame that scanned gives what its lists give: the same frame with the far detection moved out of the count's reach
    near = det.copy()
    near[5, 17, 0:2] = np.nan
    a, b = dev(det, counts, ref), dev(near, counts, ref)
    keep = np.ones(65, dtype=bool)
    keep[64] = False
    assert np.array_equal(a["assign"][5, keep], b["assign"][5, keep])
    assert np.array_equal(bits(a["dist2"][5, keep]), bits(b["dist2"][5, keep]))


@pytest.fixture(scope="module")
def recording():
    rng = np.random.default_rng(5)
    det, counts, ref = make_case(rng, 120, 61, 512)
    return det, counts, ref, checked(det, counts, ref, what="recording", gate=30.0)


@pytest.mark.parametrize("k", [1, 7, 119])
def test_range_by_range_with_the_returned_state(recording, k):
    det, counts, ref, whole = recording
    first = dev(det[:k], counts[:k], ref, gate=30.0)
    rest = dev(det[k:], counts[k:], ref, gate=30.0, state=first["state"])
    for key in ("assign", "table", "dist2", "info"):
        assert np.array_equal(bits(np.concatenate([first[key], rest[key]])), bits(whole[key])), key
    assert np.array_equal(bits(rest["state"]), bits(whole["state"]))


def test_run_to_run_arrays_and_each_output_alone(recording):
    from vbs_amd.engine import retrack
    det, counts, ref, whole = recording
    same(dev(det, counts, ref, gate=30.0), whole, what="second run")
    same(dev(det, counts, ref, tensors=False, gate=30.0), whole, what="arrays")
    same(dev(det, counts, ref, gate=30.0, state=R.initial_state(ref)), whole, what="explicit initial state")
    for key in ("assign", "table", "dist2", "info"):
        alone = dev(det, counts, ref, gate=30.0, want=(key,))
        assert set(alone) == {key, "state"}
        same(alone, whole, keys=(key, "state"), what=f"{key} alone")
    only_state = dev(det, counts, ref, gate=30.0, want=())
    assert set(only_state) == {"state"}
    same(only_state, whole, keys=("state",), what="state alone")
    empty = retrack(det[:0], counts[:0], ref, state=whole["state"])
    assert empty["assign"].shape == (0, 61) and np.array_equal(bits(empty["state"].cpu().numpy()), bits(whole["state"]))
    with pytest.raises(ValueError, match="gate"):
        retrack(det, counts, ref, gate=-1.0)
    with pytest.raises(ValueError, match="state must be"):
        retrack(det, counts, ref, state=np.zeros((3, 6)))


# ---- the drag-plus-torsion recording as real frames, through the front end ------------------------------------------------------------
W, H, N_FRAMES, RAMP = 480, 400, 40, 30


@pytest.fixture(scope="module")
def clip():
    """The scenario rendered by synth.py: 61 dots of 20 px at pitch 40 (the smallest frame that holds the rings, the drag and the
    front end's margin), 45 px of drag and 8 degrees of torsion over 30 of 40 frames, 3 % of the dots after frame 0 not drawn."""
    rng = np.random.default_rng(0)
    pos = O.trajectory(n=N_FRAMES, ramp=RAMP, drag=45.0, torsion_deg=8.0, pitch=PITCH, centre=(215.0, 200.0))
    drawn = rng.random(pos.shape[:2]) >= 0.03
    drawn[0] = True
    frames = torch.empty((N_FRAMES, H, W, 3), dtype=torch.uint8, device="cuda")
    for f in range(N_FRAMES):
        spec = S.FrameSpec(W, H, np.round(pos[f][drawn[f]] * 16).astype(np.int64), 20 * 16, jitter16=0, djitter16=0, name="retrack")
        frames[f] = S.make_frames_torch(spec, [f], seed=3, channels=3)[0]
    return frames, pos, drawn


def _tracker(tmp_path, name, **extra):
    from vbs_amd.marker_detection import MarkerTracker
    np.save(tmp_path / f"{name}.npy", np.zeros((1, 2, 2), dtype=np.uint8))         # (the path must exist; the frames are passed in)
    return MarkerTracker({"video_path": str(tmp_path / f"{name}.npy"), "output_dir": str(tmp_path / name), "crop_ratios": (0, 0, 0, 0),
                          "num_layers": 4, "id_mode": "full", "min_marker_distance": 20, **extra})


def _csv(trk, frames):
    trk._save_results(trk.process_frames(frames))
    return open(trk.output_csv, "rb").read()


def _errors(csv_path, pos, drawn):
    """(wrong, missed) of a CSV against the rendered truth: a row is wrong when it lies more than 3 px from where its marker (the
    one drawn nearest to Ox, Oy in frame 0) was drawn in that frame, or the marker was not drawn at all."""
    import pandas as pd
    df = pd.read_csv(csv_path)
    o = df[["Ox", "Oy"]].to_numpy()
    j = np.sqrt(((o[:, None, :] - pos[0][None, :, :]) ** 2).sum(axis=2)).argmin(axis=1)
    f = df["frameno"].to_numpy()
    err = np.sqrt(((df[["Cx", "Cy"]].to_numpy() - pos[f, j]) ** 2).sum(axis=1))
    wrong = int(((err > 3.0) | ~drawn[f, j]).sum())
    return wrong, int(drawn.sum()) - (len(df) - wrong)


def test_marker_tracker_retracks_in_any_batch_size_and_is_untouched_without_the_key(clip, tmp_path):
    frames, pos, drawn = clip
    whole = _tracker(tmp_path, "whole", batch=64, retrack=True)
    by7 = _tracker(tmp_path, "by7", batch=7, retrack={"gate": 10.0})
    a, b = _csv(whole, frames), _csv(by7, frames)
    assert a == b
    assert np.array_equal(whole.retrack_report["info"], by7.retrack_report["info"]) and whole.retrack_report["info"].shape == (N_FRAMES, 4)
    plain, off, none = (_csv(_tracker(tmp_path, name, batch=7, **kw), frames)
                        for name, kw in (("plain", {}), ("off", {"retrack": False}), ("none", {"retrack": None})))
    assert plain == off == none and plain != a
    assert not hasattr(_tracker(tmp_path, "unused"), "retrack_report")
    wrong, missed = _errors(whole.output_csv, pos, drawn)
    legacy_wrong, legacy_missed = _errors(tmp_path / "plain" / "plain_markers.csv", pos, drawn)
    print(f"retrack: {wrong} wrong, {missed} missed; per-frame rule: {legacy_wrong} wrong, {legacy_missed} missed of {int(drawn.sum())}")
    assert (wrong, missed) == (0, 0)
    assert legacy_wrong + legacy_missed >= 0.25 * drawn.sum()


def test_retrack_table_with_a_camera_equals_solve3d_on_the_retracked_table(clip):
    from vbs_amd import pipeline as P
    from vbs_amd.engine import Engine, retrack
    frames, pos, drawn = clip
    eng = Engine(H, W, max_markers=256, max_batch=N_FRAMES)
    _, det, counts = eng.track_to_3d(frames, None, want_det=True)
    assert int(counts[0]) == 61 and np.array_equal(counts.cpu().numpy(), drawn.sum(axis=1))
    ref = det[0, :61, 0:2].clone()
    cam = L.make_camera(*S.default_camera(S.FrameSpec(W, H, np.zeros((1, 2), dtype=np.int64), 320)), 2.0)
    table, report = P.retrack_table(eng, det, counts, ref, cam=cam)
    out = retrack(det, counts, ref)
    want = eng.solve3d(out["table"].clone(), cam, 5.0)
    assert np.array_equal(bits(table.cpu().numpy()), bits(want.cpu().numpy()))
    assert int(((table[..., 0].to(torch.int64) & L.FLAG_XYZ) != 0).sum()) == int(drawn.sum())
    assert np.array_equal(report["info"].cpu().numpy(), out["info"].cpu().numpy()) and report["lost"].numel() == 0
    legacy = eng.track(det, counts, ref, 20.0)
    again = R.compare_tables(out["table"], legacy)
    assert all(np.array_equal(report["comparison"][k], again[k]) for k in ("same", "only_a", "only_b", "differ"))
    total = report["comparison"]["total"]
    assert total["same"] + total["differ"] + total["only_a"] == int(drawn.sum()) and total["differ"] + total["only_a"] > 0
    sheet = P.to_retrack_frame(report)
    assert list(sheet.columns) == ["frameno", "used", "matched", "with_candidate", "contested", "same", "only_retrack",
                                   "only_per_frame", "differ"]
    assert len(sheet) == N_FRAMES and sheet["matched"].tolist() == drawn.sum(axis=1).tolist()
