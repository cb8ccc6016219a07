"""GPU tests of the grey-level refinement (k_refine.hip; run on the MI355X box: `pytest -m gpu`): `Engine.refine_markers`,
`pipeline.refine_table`, the sheet and `MarkerTracker` with `"refine"`.

Against the restatement of the rule (`tests/helpers/refine_oracle.py`, written from include/vbs.h): `sums` and the status
exactly; every `rec` column that does not end in a root or an arc tangent (cx, cy, A, the two levels) bit for bit, the rest
(major', minor', angle, d_area, edge_var, shift) to 4 ulp, the precedent of test_gpu_motion.py; `table_out` bit for bit given
`rec`.  Frames are 96 x 160 with n = 3 and m_ref = 9 unless a case needs more room (R = 63 needs 127 rows)."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import pipeline as P                             # noqa: E402
from vbs_amd import synth as S                                # noqa: E402
from vbs_amd.engine import Engine                             # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import refine_cases as RC                                     # noqa: E402
import refine_oracle as O                                     # noqa: E402
BOUND = RC.BOUND

H, W = 96, 160
ROUND, LONG = (30.3, 29.6, 8.0, 8.0, 0.0), (84.4, 31.2, 9.0, 6.3, 30.0)      # the second: ratio 0.7


@pytest.fixture(scope="module")
def eng():
    e = Engine(H, W, max_markers=64, max_batch=4, device=0)
    yield e
    e.close()


def run(e, frames, table, **kw):
    rec, sums, out = e.refine_markers(frames, table, **kw)
    return rec.cpu().numpy(), sums.cpu().numpy(), out.cpu().numpy()


def main_frames():
    """Three frames of the same two markers: 200/60 sharp, 120/90 sharp, 200/60 blurred by 1 px; noise 1.5 levels."""
    return np.stack([RC.render(H, W, [ROUND, LONG], 200.0, 60.0, 0.0, noise=1.5, seed=1),
                     RC.render(H, W, [ROUND, LONG], 120.0, 90.0, 0.0, noise=1.5, seed=2),
                     RC.render(H, W, [ROUND, LONG], 200.0, 60.0, 1.0, noise=1.5, seed=3)])


def main_table(n=3):
    """m_ref = 9: a round and an elongated marker (the first with VBS_FLAG_XYZ and a 3-D point to clear), an untracked row full of
    NaN, a NaN centre, an infinite diameter, a flat patch, a start two radii off, a diameter below 2 and a window over the border."""
    nan, inf = float("nan"), float("inf")
    rows = [RC.row(30.9, 29.0, 17.0, 15.0, 100.0, flags=3, det_index=4, xyz=(1.0, 2.0, 30.0)),
            RC.row(84.0, 31.9, 17.2, 12.0, 200.0, det_index=2),
            RC.row(nan, nan, nan, nan, nan, flags=0, det_index=7, xyz=(nan, nan, nan)),
            RC.row(nan, 40.0, 16.0, det_index=1),
            RC.row(40.0, 40.0, inf, det_index=3),
            RC.row(130.0, 70.0, 12.0, det_index=5),
            RC.row(30.3 + 16.0, 29.6, 16.0, det_index=6),
            RC.row(40.0, 40.0, 1.5, det_index=8),
            RC.row(5.0, 50.0, 16.0, det_index=9)]
    return np.stack([np.stack(rows)] * n)


@pytest.fixture(scope="module")
def main_case():
    frames, table = main_frames(), main_table()
    return frames, table, {k: O.refine(frames, table, keep_unrefined=k) for k in (0, 1)}


@pytest.mark.parametrize("keep", [0, 1])
def test_markers_at_both_contrasts_and_every_early_status(eng, main_case, keep):
    """Cases a, d, e and k: round and elongated markers at 200/60 and 120/90, untracked and non-finite rows, a flat patch
    (status 5), a start two radii off (7 or 5), with keep_unrefined 0 and 1."""
    frames, table, want = main_case
    rec, sums, out = run(eng, frames, table, keep_unrefined=keep)
    O.check(rec, sums, out, want[keep], f"keep_unrefined {keep}")
    st = rec[..., 0]
    assert (st[:, :2] == 0).all() and (st[:, 2] == 1).all() and (st[:, 3] == 2).all() and (st[:, 4] == 2).all()
    assert (st[:, 5] == 5).all() and np.isin(st[:, 6], (5, 7)).all() and (st[:, 7] == 2).all() and (st[:, 8] == 4).all()
    # every row: VBS_FLAG_XYZ clear, X Y Z zero, det_index kept
    assert ((out[..., 0].astype(int) & L.FLAG_XYZ) == 0).all() and (out[..., 6:9] == 0).all() and np.array_equal(out[..., 9], table[..., 9])
    gap = (st != 0) if keep == 0 else (st == 1)
    assert (out[gap][:, :9] == 0).all() and (out[st == 0][:, 0] == 1).all()
    if keep:
        kept = st >= 2
        assert np.array_equal(out[kept][:, 1:6].view(np.int32), table[kept][:, 1:6].view(np.int32)) and (out[kept][:, 0] == 1).all()
    # the rule's accuracy on these markers, at both contrasts and under blur
    for f in range(3):
        assert abs(rec[f, 0, 3] - 16.0) <= BOUND["major"] and abs(rec[f, 1, 3] - 18.0) <= BOUND["major"]
        assert abs(rec[f, 1, 6] - 2 * math.sqrt(9.0 * 6.3)) <= BOUND["d_area"]
        assert math.hypot(rec[f, 1, 1] - LONG[0], rec[f, 1, 2] - LONG[1]) <= BOUND["centre"]
        assert abs((rec[f, 1, 5] - 30.0 + 90.0) % 180.0 - 90.0) < 3.0


def test_large_windows_use_the_second_column_of_a_lane():
    """Case b: R <= 31, R in 32 .. 63, R = 63 exactly (the whole 127-pixel width), and R = 64 is status 3."""
    h, w = 128, 160
    e = Engine(h, w, max_markers=64, max_batch=4, device=0)
    mk = (80.3, 63.8, 26.0, 24.0, 60.0)
    frames = np.stack([RC.render(h, w, [mk], 200.0, 60.0, 0.0, noise=1.5, seed=4), RC.render(h, w, [mk], 120.0, 90.0, 1.0, noise=1.5, seed=5),
                       RC.render(h, w, [mk], 60.0, 200.0, 2.0, noise=1.5, seed=6)])
    over = float(np.nextafter(np.float32(62.0), np.float32(63.0)))
    majors = (62.0, 61.3, 52.0, 40.0, 31.0, 30.0, over, 63.0, 200.0)
    table = np.stack([np.stack([RC.row(80.0, 64.0, m, det_index=i) for i, m in enumerate(majors)])] * 3)
    assert [RC_R(m) for m in majors[:6]] == [63, 63, 53, 41, 32, 31]
    for pol in (0, 1):
        rec, sums, out = run(e, frames, table, polarity=pol, max_shift_f=1.0)
        O.check(rec, sums, out, O.refine(frames, table, polarity=pol), f"polarity {pol}")
        assert (rec[:, 6:, 0] == 3).all()
        dark = rec[:2] if pol == 0 else rec[2:]
        assert (dark[:, :3, 0] == 0).all()                     # the starts near the true diameter refine the marker they see as dark
        assert (np.abs(dark[:, 2, 6] - 2 * math.sqrt(26.0 * 24.0)) <= BOUND["d_area"]).all()
    e.close()


def RC_R(major):
    return int(math.ceil(2.0 * 0.5 * float(np.float32(major)))) + 1


def test_windows_flush_with_each_border_and_one_pixel_over(eng):
    """Case c: R = 13; flush with the left, right, top and bottom border and in a corner: status 0; one pixel over: status 4."""
    centres = [(13, 48), (W - 14, 48), (80, 13), (80, H - 14), (13, 13)]
    over = [(12, 48), (W - 13, 48), (80, 12), (80, H - 13)]
    mks = [(x + 0.2, y - 0.3, 6.0, 5.4, 45.0) for x, y in centres]
    frames = np.stack([RC.render(H, W, mks, 200.0, 60.0, s, noise=1.5, seed=10 + i) for i, s in enumerate((0.0, 0.5, 1.0))])
    table = np.stack([np.stack([RC.row(x, y, 12.0, det_index=i) for i, (x, y) in enumerate(centres + over)])] * 3)
    table[1, :, 1:3] += 0.49                                    # still rounds to the same pixel
    table[2, :, 1:3] -= 0.5                                     # x - 0.5 rounds up to x
    rec, sums, out = run(eng, frames, table)
    O.check(rec, sums, out, O.refine(frames, table), "borders")
    assert (rec[:, :5, 0] == 0).all() and (rec[:, 5:, 0] == 4).all()


def test_a_bright_blob_or_a_neighbours_edge_in_the_ring_does_not_move_the_background_level(eng):
    """Case f, on noise-free frames: a highlight and a dark neighbour's edge inside the ring leave B8 - the trimmed level - and
    with it every sum what the clean frame gives."""
    clean = RC.render(H, W, [ROUND], 200.0, 60.0, 0.7)
    blob = clean.copy()
    blob[29 - 2:29 + 3, 30 + 13:30 + 16] = 255                  # a highlight in the ring (r = 8: the ring is 12 < d <= 17)
    blob[29 + 13:29 + 17, 30 - 6:30 + 6] = 40                   # the edge of a dark neighbour
    table = np.stack([np.stack([RC.row(30.0, 29.0, 16.0)] * 9)] * 3)
    table[:, 1:, 0] = 0
    frames = np.stack([clean, blob, blob])
    rec, sums, out = run(eng, frames, table)
    O.check(rec, sums, out, O.refine(frames, table), "blob")
    assert sums[0, 0, 0] == 8 * 200 and np.array_equal(sums[1, 0], sums[0, 0]) and rec[1, 0, 0] == 0
    assert np.array_equal(rec[1, 0], rec[0, 0])


def test_polarity_1_on_the_inverted_frame_gives_the_same_sums(eng, main_case):
    """Case g."""
    frames, table, want = main_case
    rec, sums, out = run(eng, 255 - frames, table, polarity=1)
    assert np.array_equal(sums, want[0][1]) and np.array_equal(rec.view(np.int64), run(eng, frames, table)[0].view(np.int64))
    O.check(rec, sums, out, O.refine(255 - frames, table, polarity=1), "polarity 1")


def test_a_strided_crop_view_equals_its_dense_copy(eng, main_case):
    """Case h."""
    frames, table, want = main_case
    big = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (3, H + 24, W + 40)).astype(np.uint8)).cuda()
    big[:, 10:10 + H, 20:20 + W] = torch.from_numpy(frames).cuda()
    view = big[:, 10:10 + H, 20:20 + W]
    assert not view.is_contiguous()
    a = run(eng, view, table)
    b = run(eng, view.contiguous(), table)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    O.check(*a, want[0], "crop view")


def test_bgr_frames_equal_the_gray_that_bgr2gray_gives(eng, main_case):
    """Case i."""
    frames, table, _ = main_case
    rng = np.random.default_rng(1)
    bgr = np.clip(frames[..., None].astype(np.int64) + rng.integers(-20, 21, (3, H, W, 3)), 0, 255).astype(np.uint8)
    gray = eng.bgr2gray(torch.from_numpy(bgr).cuda())
    a = run(eng, bgr, table)
    b = run(eng, gray, table)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    O.check(*a, O.refine(gray.cpu().numpy(), table), "bgr")
    assert (a[0][:, :2, 0] == 0).all()


@pytest.mark.parametrize("n,m", [(5, 9), (3, 8)])
def test_batching_does_not_change_a_bit(eng, main_case, n, m):
    """Case j: frames [0, k) and [k, n) equal [0, n); n m_ref = 45 is no multiple of the rows a workgroup takes, 24 is."""
    frames, table, _ = main_case
    assert (n * m) % L.REFINE_WAVES == (1 if (n, m) == (5, 9) else 0)
    idx = [0, 1, 2, 1, 0][:n]
    fr, tb = frames[idx], main_table(n)[:, :m].copy()
    tb[:, :, 1] += np.linspace(-0.4, 0.4, n, dtype=np.float32)[:, None]
    whole = run(eng, fr, tb)
    O.check(*whole, O.refine(fr, tb), f"n {n} m {m}")
    for k in (1, 2):
        first, second = run(eng, fr[:k], tb[:k]), run(eng, fr[k:], tb[k:])
        for x, a, b in zip(whole, first, second):
            assert np.array_equal(x.view(np.uint8), np.concatenate([a, b]).view(np.uint8)), (n, m, k)


def test_wanted_outputs_and_refusals(eng, main_case):
    frames, table, want = main_case
    rec, sums, out = eng.refine_markers(frames, table, want=("sums",))
    assert rec is None and out is None and np.array_equal(sums.cpu().numpy(), want[0][1])
    rec, sums, out = eng.refine_markers(frames[0], table[0], want=("table",))
    assert rec is None and sums is None and np.array_equal(out.cpu().numpy().view(np.int32)[0, 2:], want[0][2][0, 2:].view(np.int32))
    for bad in (dict(ring_f=1.0), dict(min_contrast=0.0), dict(polarity=3), dict(nope=1), dict(want=()), dict(want=("x",)), dict(passes=0)):
        with pytest.raises(ValueError):
            eng.refine_markers(frames, table, **bad)
    with pytest.raises(ValueError):
        eng.refine_markers(frames, table[:2])
    # a tight max_shift_f: the markers are status 7, with every column filled in
    moved = run(eng, frames, table, max_shift_f=0.01)
    O.check(*moved, O.refine(frames, table, max_shift_f=0.01), "moved")
    assert (moved[0][:, :2, 0] == 7).all() and (moved[0][:, :2, 1:] != 0).all() and (moved[2][:, :2, :9] == 0).all()
    # two passes are the rule applied to what the first pass (with keep_unrefined) wrote
    rec2, sums2, out2 = run(eng, frames, table, passes=2)
    O.check(rec2, sums2, out2, O.refine(frames, want[1][2]), "passes 2")


def test_refined_angle_agrees_with_the_binary_paths_column_5():
    """Case l: ratio-0.7 markers (a = 12, b = 8.4 px, major axis at 30 degrees) through the detector itself - DoG, threshold,
    contour, k_finalize's ellipse - and then refined: the two column-5 values agree within 3 degrees modulo 180, for all 15
    markers, and the refined one lies within 1 degree of the rendered direction.  The markers are centred on pixel centres: the
    comparison is about the CONVENTION of column 5, and the binary path's own angle depends on where the pixel grid cuts the
    contour.  Restated on the CPU (the oracle pipeline, the restatement): here the binary angle is 2.0 - 2.6 degrees below the
    rendered 30 and the largest difference is 2.5; with centres moved by fractions of a pixel the binary angle is up to 3.7
    degrees off the rendered direction (the refined one stays within 0.5), which a 3-degree comparison would charge to the
    refinement."""
    mks = [(120.0 + 100 * i, 100.0 + 100 * j, 12.0, 8.4, 30.0) for i in range(5) for j in range(3)]
    frame = RC.render(480, 640, mks, 190.0, 40.0, 0.7, noise=1.5, seed=1)
    e = Engine(480, 640, max_markers=256, max_batch=2, device=0)
    ft = torch.from_numpy(frame[None]).cuda()
    _, det, counts = e.track_to_3d(ft, None, want_det=True)
    assert int(counts[0]) == len(mks)
    table, _, _ = e.track_to_3d(ft, det[0, :len(mks), :2].contiguous(), 20.0)
    rec, _, out = run(e, ft, table)
    binary = table.cpu().numpy()[0, :, 5].astype(np.float64)
    assert (rec[0, :, 0] == 0).all() and ((binary >= 90.0) & (binary < 270.0)).all() and ((out[0, :, 5] > 90.0) & (out[0, :, 5] <= 270.0)).all()
    diff = np.abs((out[0, :, 5].astype(np.float64) - binary + 90.0) % 180.0 - 90.0)
    print(f"binary - rendered: {np.min((binary - 30.0 + 90.0) % 180.0 - 90.0):+.2f} .. {np.max((binary - 30.0 + 90.0) % 180.0 - 90.0):+.2f} deg; "
          f"refined - rendered: {np.min((rec[0, :, 5] - 30.0 + 90.0) % 180.0 - 90.0):+.2f} .. "
          f"{np.max((rec[0, :, 5] - 30.0 + 90.0) % 180.0 - 90.0):+.2f} deg; largest |refined - binary| {diff.max():.2f} deg")
    assert (diff < 3.0).all() and (np.abs((rec[0, :, 5] - 30.0 + 90.0) % 180.0 - 90.0) < 1.0).all()
    e.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
CONTRASTS = ((190, 40), (150, 100))
E2E_PASSES = 3
E2E_REFINED = {(190, 40): 147, (150, 100): 132}           # rows refined, as the restatement gives them on the oracle's detections


@pytest.fixture(scope="module")
def e2e():
    """`synth.grid_spec` frames (640 x 480, 7 x 7 dots of 20 +- 2 px) at two contrasts with the same geometry, through
    `track_to_3d` and then `refine_table`."""
    out = {}
    for bg, fg in CONTRASTS:
        spec = S.grid_spec(640, 480, 7, 60, 20, bg=bg, fg=fg)
        frames = torch.from_numpy(S.make_frames(spec, [0, 1, 2], seed=0)).cuda()
        e = Engine(480, 640, max_markers=256, max_batch=4, device=0)
        truth = S.dot_truth(spec, 0, [0, 1, 2])
        ref_xy = truth[0, :, :2].copy()
        cam = L.make_camera(*S.default_camera(spec), 2.0)
        table, _, counts = e.track_to_3d(frames, ref_xy, 20.0, cam, 5.0)
        assert (counts.cpu().numpy() == 49).all()
        out[(bg, fg)] = dict(eng=e, frames=frames, truth=truth, cam=cam, table=table, ref_xy=ref_xy)
    yield out
    for v in out.values():
        v["eng"].close()


def test_refined_diameter_is_the_rendered_one_at_both_contrasts(e2e):
    """The refined `major` of every refined marker lies within the accuracy bound of the rendered diameter at BOTH contrasts.
    The binary path's `major` is printed, not asserted: at 150/100 it is about 9 px short of the rendered 20 px, far outside the
    +-1.5 px start the rule's accuracy set assumes - the disc of a single pass (1.5 x the start's radius) does not even cover
    the marker there - so the table is refined with `passes = 3`, each pass starting from the last one's rows.  The figures of a
    single pass are printed next to it.  Restated on the CPU (oracle detections, the restatement, 3 passes): max |error| 0.172 px
    at 190/40 and 0.258 px at 150/100, where 15 of 147 rows stay status 5 (their start's ring lies inside the marker) and are
    gaps, not refined markers."""
    for (bg, fg), c in e2e.items():
        truth_d = c["truth"][..., 2]
        binary = c["table"].cpu().numpy()
        tracked = (binary[..., 0].astype(int) & 1) != 0
        assert tracked.all()
        print(f"{bg}/{fg}: binary major - rendered: mean {np.mean(binary[..., 3] - truth_d):+.3f}, min {np.min(binary[..., 3] - truth_d):+.3f}, "
              f"max {np.max(binary[..., 3] - truth_d):+.3f} px")
        for passes in (1, E2E_PASSES):
            table, rep = P.refine_table(c["eng"], c["frames"], c["table"], cam=c["cam"], passes=passes)
            t = table.cpu().numpy()
            ok = (t[..., 0].astype(int) & 1) != 0
            err = np.abs(t[..., 3].astype(np.float64) - truth_d)[ok]
            print(f"{bg}/{fg}: passes {passes}: refined {int(ok.sum())} of {ok.size}, status counts {rep['status_per_slot'].sum(axis=0).tolist()}, "
                  f"uncovered {int(rep['uncovered'].sum())}, max |major' - rendered| {err.max():.3f} px, mean {err.mean():.3f} px")
            # a single pass from a start far too small reports status 0 and is short: the report names exactly those rows
            short = np.abs(t[..., 3].astype(np.float64) - truth_d) > BOUND["major"]
            assert np.array_equal(rep["uncovered"] & short, ok & short) and (passes == 1 or not rep["uncovered"].any())
            if (bg, fg) == (150, 100) and passes == 1:
                assert rep["uncovered"].sum() == ok.sum()
        assert ok.sum() == E2E_REFINED[(bg, fg)] and rep["status_per_slot"][:, 5].sum() == ok.size - ok.sum()
        assert (err <= BOUND["major"]).all(), (bg, fg, float(err.max()))
        cerr = np.hypot(t[..., 1] - c["truth"][..., 0], t[..., 2] - c["truth"][..., 1])[ok]
        assert (cerr <= BOUND["centre"] + 2.0 ** -10).all(), (bg, fg, float(cerr.max()))      # (+ float32 rounding at 640 px)


def test_refined_table_goes_through_solve3d_despike_and_fill_and_the_sheet(e2e, tmp_path):
    c = e2e[CONTRASTS[0]]
    e = c["eng"]
    table, rep = P.refine_table(e, c["frames"], c["table"], cam=c["cam"])
    assert table.dtype == torch.float32 and tuple(table.shape) == tuple(c["table"].shape) and table.data_ptr() != c["table"].data_ptr()
    t = table.cpu().numpy()
    rec = rep["rec"].cpu().numpy()
    ok = rec[..., 0] == 0
    assert ok.all() and ((t[..., 0].astype(int) & 3) == 3).all() and np.isfinite(t).all()      # refined, then solved
    assert np.array_equal(t[..., 9], c["table"].cpu().numpy()[..., 9])
    again = e.solve3d(e.refine_markers(c["frames"], c["table"])[2], c["cam"]).cpu().numpy()
    assert np.array_equal(again.view(np.int32), t.view(np.int32))
    assert rep["status_per_frame"].tolist() == [[49, 0, 0, 0, 0, 0, 0, 0]] * 3 and rep["never_refined"].size == 0
    assert np.isfinite(rep["dmajor_mean"]).all() and np.isfinite(rep["edge_var_median"])
    clean, _ = P.despike_table(e, table, half_window=1, k_sigma=3.0, min_scale=0.05)
    filled, _ = P.fill_table(e, clean, half_window=1, degree=1)
    for x in (clean, filled):
        assert x.dtype == torch.float32 and tuple(x.shape) == tuple(table.shape)
    df = P.to_refine_frame(rep, path=str(tmp_path / "refine.csv"))
    assert list(df.columns)[:2] == ["slot", "refined"] and len(df) == 49 and (df["refined"] == 3).all()
    assert os.path.getsize(tmp_path / "refine.csv") > 0


def _tracker(tmp_path, name, **extra):
    from vbs_amd.marker_detection import MarkerTracker
    np.save(tmp_path / f"{name}.npy", np.zeros((1, 2, 2), dtype=np.uint8))         # (the path must exist; the frames are passed in)
    return MarkerTracker({"video_path": str(tmp_path / f"{name}.npy"), "output_dir": str(tmp_path / name), "crop_ratios": (0, 0, 0, 0),
                          "num_layers": 5, "id_mode": "full", "min_marker_distance": 20, "batch": 2, **extra})


def _csv(trk, frames):
    rows = trk.process_frames(frames)
    trk._save_results(rows)
    return open(trk.output_csv, "rb").read(), list(rows)


def test_marker_tracker_follows_the_refined_table_and_is_unchanged_without_the_key(e2e, tmp_path):
    """Without `"refine"` (absent, None, False) the CSV is byte for byte one file, and its rows are the detections' own float64
    values - what the tracker has always written; with it the rows equal `refine_table`'s, in any batch size."""
    from vbs_amd import ids as I
    spec = S.grid_spec(640, 480, 7, 60, 20)
    frames = S.make_frames(spec, [0, 1, 2], seed=0)
    (plain, rows0), (off, _), (none, _) = (_csv(_tracker(tmp_path, name, **kw), frames)
                                           for name, kw in (("plain", {}), ("off", {"refine": False}), ("none", {"refine": None})))
    assert plain == off == none and not hasattr(_tracker(tmp_path, "unused"), "refine_report")
    trk = _tracker(tmp_path, "refined", refine=True)
    refined, rows1 = _csv(trk, frames)
    by3, _ = _csv(_tracker(tmp_path, "by3", batch=3, refine={"min_contrast": 16.0}), frames)
    assert refined == by3 and refined != plain
    assert len(rows1) == len(rows0) == 147 and trk.refine_report["status_per_frame"].tolist() == [[49, 0, 0, 0, 0, 0, 0, 0]] * 3
    ids, ref_xy = I.reference_arrays(trk.first_frame_markers)
    e = e2e[CONTRASTS[0]]["eng"]
    ft = torch.from_numpy(frames).cuda()
    table, det, _ = e.track_to_3d(ft, ref_xy, 20, want_det=True)
    want, _ = P.refine_table(e, ft, table)
    want, table, det = want.cpu().numpy(), table.cpu().numpy(), det.cpu().numpy()
    fi, si = np.nonzero(want[..., 0].astype(int) & 1)
    assert len(fi) == len(rows1)
    names = ("Cx", "Cy", "major_axis", "minor_axis", "angle")
    for r0, r1, f, s in zip(rows0, rows1, fi, si):
        key = (int(f),) + tuple(int(v) for v in np.asarray(ids)[s])
        assert (r1["frameno"], r1["row"], r1["col"]) == key == (r0["frameno"], r0["row"], r0["col"])
        assert tuple(r1[k] for k in names) == tuple(float(v) for v in want[f, s, 1:6])
        assert tuple(r0[k] for k in names) == tuple(float(v) for v in det[f, int(table[f, s, 9]), :5])
    assert any(r0["major_axis"] != r1["major_axis"] for r0, r1 in zip(rows0, rows1))


def test_marker_tracker_refines_after_retracking(e2e, tmp_path):
    """`"refine"` together with `"retrack"`: the rows are `refine_table` of `retrack_table`."""
    from vbs_amd import ids as I
    spec = S.grid_spec(640, 480, 7, 60, 20)
    frames = S.make_frames(spec, [0, 1, 2], seed=0)
    trk = _tracker(tmp_path, "both", retrack=True, refine=True)
    _, rows = _csv(trk, frames)
    ids, ref_xy = I.reference_arrays(trk.first_frame_markers)
    e = e2e[CONTRASTS[0]]["eng"]
    ft = torch.from_numpy(frames).cuda()
    _, det, counts = e.track_to_3d(ft, ref_xy, 20, want_det=True)
    tracked, _ = P.retrack_table(e, det, counts, ref_xy)
    want, _ = P.refine_table(e, ft, tracked)
    want = want.cpu().numpy()
    fi, si = np.nonzero(want[..., 0].astype(int) & 1)
    assert len(rows) == len(fi) == 147 and trk.retrack_report["info"].shape == (3, 4) and trk.refine_report["uncovered"] == 0
    for r, f, s in zip(rows, fi, si):
        assert (r["frameno"], r["row"], r["col"]) == (int(f),) + tuple(int(v) for v in np.asarray(ids)[s])
        assert tuple(r[k] for k in ("Cx", "Cy", "major_axis", "minor_axis", "angle")) == tuple(float(v) for v in want[f, s, 1:6])


def test_marker_tracker_refines_the_undistorted_crop_and_draws_the_refined_ellipses(tmp_path):
    """`"refine"` with `calibration_params`, a crop, BGR frames and `write_video`: refinement reads the undistorted crop the
    detector saw (rows equal `refine_table` on `undistort_frames`), and the video shows the refined ellipses - every frame of
    the AVI is the overlay of the CSV's own rows on the undistorted crop, byte for byte (the CSV is what the video follows)."""
    import io
    Image = pytest.importorskip("PIL.Image")
    import cv_draw
    from vbs_amd import ids as I
    from vbs_amd.marker_detection import MarkerTracker, _crop_box
    from vbs_amd.video_io import AviReader
    import pandas as pd
    crop = (1 / 8, 1 / 8, 1 / 16, 0)
    frames = S.make_frames(S.config1(), range(3), seed=4, channels=3)
    np.save(tmp_path / "clip.npy", np.zeros((1, 2, 2), dtype=np.uint8))
    calib = {"camera_matrix": [[520.0, 0, 240.0], [0, 520.0, 225.0], [0, 0, 1]], "dist_coeffs": [0.04, -0.01, 0.0, 0.0, 0.0]}
    cfg = {"video_path": str(tmp_path / "clip.npy"), "crop_ratios": crop, "calibration_params": calib, "batch": 2, "id_mode": "full",
           "refine": True, "video_quality": 90}
    trk = MarkerTracker({**cfg, "output_dir": str(tmp_path / "v"), "write_video": True})
    rows = trk.process_frames(torch.from_numpy(frames).cuda())
    trk._save_results(rows)
    rows = list(rows)
    l, r, t, b = _crop_box(640, 480, crop)
    e = Engine(b - t, r - l, max_markers=256, max_batch=4, device=0)
    e.set_undistort(calib["camera_matrix"], calib["dist_coeffs"])
    ft = torch.from_numpy(frames).cuda()[:, t:b, l:r]
    ids, ref_xy = I.reference_arrays(trk.first_frame_markers)
    table, _, _ = e.track_to_3d(ft, ref_xy, 20)
    und = e.undistort_frames(ft)
    want, _ = P.refine_table(e, und, table)
    want = want.cpu().numpy()
    fi, si = np.nonzero(want[..., 0].astype(int) & 1)
    assert len(rows) == len(fi) > 100
    for row, f, s in zip(rows, fi, si):
        assert tuple(row[k] for k in ("Cx", "Cy", "major_axis", "minor_axis", "angle")) == tuple(float(v) for v in want[f, s, 1:6])
    # the refined rows differ from the detections, so a video drawn from the detections would not match the CSV
    plain = list(MarkerTracker({**cfg, "refine": None, "output_dir": str(tmp_path / "p")}).process_frames(torch.from_numpy(frames).cuda()))
    assert any(a["major_axis"] != c["major_axis"] for a, c in zip(plain, rows))
    rd = AviReader(trk.output_video)
    assert rd.isOpened() and len(rd._frames) == 3
    df = pd.read_csv(trk.output_csv, float_precision="round_trip")
    crops = und.cpu().numpy()
    for i, (off, size) in enumerate(rd._frames):
        drawn = cv_draw.draw_frame(crops[i], [tuple(x) for x in df[df.frameno == i][["Ox", "Oy", "Cx", "Cy", "major_axis", "minor_axis", "angle"]]
                                              .to_numpy(dtype=np.float64)])
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(drawn[:, :, ::-1])).save(buf, "JPEG", quality=90)
        assert bytes(rd._buf[off:off + size]) == buf.getvalue(), i
    e.close()
