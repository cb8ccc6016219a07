"""GPU tests of the time-axis reductions (k_series.hip; run on the MI355X box: `pytest -m gpu`): per-marker displacement
statistics, cumulative series, window means and the distance from a reference frame, each against the pandas / NumPy oracle
(`tests/helpers/analysis_oracle.py`, pinned to the reference's own statements by `tests/test_analysis_host.py`) on the same
float32 inputs promoted to float64.

Tolerances (derived from the float64 summation error, stated in analysis_oracle.py): count / max / flags exact; totals,
cumulative entries and window sums n 2^-52 sum|x|; means that over the count plus 2^-52 |mean|; std relative
n kappa 2^-52; distances, difference vectors and norms 1e-12 relative.  No slot is skipped or masked to get under one.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import vbs_amd.synth as S                                     # noqa: E402
from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import analysis_oracle as A                                   # noqa: E402

CH = L.SERIES_CHUNK


def engine(h=480, w=640, **kw):
    from vbs_amd.engine import Engine
    kw.setdefault("max_markers", 256)
    kw.setdefault("max_batch", 2)
    return Engine(h, w, **kw)


def bits(t):
    return t.contiguous().view(torch.int64)


def random_disp(rng, n, m, missing):
    """float32 disp [n, m, 5]: per-slot levels spread over three decades, some slots with a mean hundreds of times their
    standard deviation; `missing` = the share of entries that are no rows (their values are junk that must not be read)."""
    level = 10.0 ** rng.uniform(-2, 1, m)
    spread = level * np.where(rng.random(m) < 0.3, 1.0 / 300.0, 0.4)
    x = np.abs(level[None, :] + spread[None, :] * rng.standard_normal((n, m)))
    flag = rng.random((n, m)) >= missing if 0 < missing < 1 else np.full((n, m), missing == 0)
    d = np.zeros((n, m, 5), dtype=np.float32)
    d[..., 0] = flag
    d[..., 1:4] = rng.standard_normal((n, m, 3))
    d[..., 4] = np.where(flag, x, 1e30 * rng.standard_normal((n, m)))
    return d


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "analysis.npz")))


# ---------------------------------------------------------------------------------------------------------------------
def test_golden_case_through_every_entry_point(gold, tmp_path):
    from vbs_amd.engine import series_stats_f64
    from vbs_amd.pipeline import window_displacement
    from vbs_amd.reconstruction3d import Config, MarkerAnalysis
    eng = engine()
    disp, table, ids = gold["disp"], gold["table"], gold["ids"]
    d32 = torch.from_numpy(disp).cuda()
    t32 = torch.from_numpy(table).cuda()
    # statistics + cumulative series: float32 entry, float64 entry, the two halves
    st, cum = eng.series_stats(d32, cumulative=True)
    A.check_series(st.cpu().numpy(), cum.cpu().numpy(), disp, ids, "series_stats")
    A.check_stats(st.cpu().numpy(), gold["stats"], disp, "series_stats vs the reference's numbers")
    assert torch.equal(bits(eng.series_stats(d32)), bits(st))
    st64, cum64 = series_stats_f64(torch.from_numpy(disp.astype(np.float64)).cuda(), cumulative=True)
    A.check_series(st64.cpu().numpy(), cum64.cpu().numpy(), disp, ids, "series_stats_f64")
    assert torch.equal(bits(st64), bits(st)) and torch.equal(bits(cum64), bits(cum))     # same values, same order of operations
    assert torch.equal(bits(eng.series_merge(eng.series_partial(d32))), bits(st))
    rows = disp[..., 0] != 0
    assert np.array_equal(np.isnan(gold["cumulative"]), ~rows)
    x = np.where(rows, np.abs(disp[..., 4].astype(np.float64)), 0)
    assert (np.abs(cum.cpu().numpy() - gold["cumulative"])[rows] <= (np.cumsum(rows, 0) * A.EPS * np.cumsum(x, 0))[rows]).all()
    # analyze_tables: the reference's statistics frame, empty slots dropped
    ma = MarkerAnalysis(Config(data_dir=tmp_path / "d", output_dir=tmp_path / "o", plots_dir=tmp_path / "p"))
    for frame in (ma.analyze_tables(d32, ids, engine=eng, path=tmp_path / "stats.csv"),
                  ma.analyze_tables(torch.from_numpy(disp.astype(np.float64)).cuda(), ids)):
        assert list(frame.index.names) == ["row", "col"] and len(frame) == int((gold["stats"][:, 0] > 0).sum())
        assert [tuple(c) for c in frame.columns] == [("displacement", "mean"), ("displacement", "std"), ("displacement", "max"),
                                                     ("cumulative_displacement", "last")]
        A.check_stats(A.stats_from_frame(frame, ids, rows.sum(axis=0)), gold["stats"], disp, "analyze_tables")
    assert (tmp_path / "stats.csv").exists() and not (tmp_path / "p" / "displacement_statistics.csv").exists()
    # window means and LocalAnalysis's flow
    windows = [tuple(w) for w in gold["windows"].tolist()]
    wm = eng.window_means(t32, windows).cpu().numpy()
    A.check_window_means(wm, table, windows, "window_means")
    for w in range(2):
        assert np.array_equal(np.isnan(wm[w, :, 1]), np.isnan(gold[f"win_all_{w}"][:, 0]))
    for tag, slots in (("all", None), ("sel", gold["target_slots"])):
        got = window_displacement(eng, t32, windows[0], windows[1], slots)
        assert np.array_equal(got["slots"].cpu().numpy(), gold[f"merged_{tag}_slots"])
        want = gold[f"merged_{tag}_d"]
        assert (np.abs(got["d"].cpu().numpy() - want) <= A.REL_POINT * np.abs(want)).all()
        assert abs(float(got["mean"]) - float(gold[f"merged_{tag}_mean"])) <= A.REL_POINT * float(gold[f"merged_{tag}_mean"])
    # distance from frame 0 (and from another frame)
    sc = eng.displacement_from_frame(t32, 0).cpu().numpy()
    A.check_disp_from_frame(sc, table, 0, "displacement_from_frame")
    ok = ~np.isnan(gold["scalar"])
    assert np.array_equal(sc[..., 0] == 1, ok)
    assert (np.abs(sc[..., 1][ok] - gold["scalar"][ok]) <= A.REL_POINT * np.abs(gold["scalar"][ok])).all()
    A.check_disp_from_frame(eng.displacement_from_frame(t32, 77).cpu().numpy(), table, 77, "displacement_from_frame(77)")
    eng.close()


def test_tracked_sequence_against_the_oracle_and_the_existing_csv(tmp_path):
    """288 config-2 frames through track_shard (synthetic camera), the centre dot painted out in a few frames so that gaps
    exist; every reduction against the oracle, and analyze_tables against the CSV the existing analyze_displacement writes
    from the flattened rows."""
    import pandas as pd
    import series_worker as SW
    from vbs_amd.pipeline import track_shard
    from vbs_amd.reconstruction3d import Config, MarkerAnalysis
    n = 288
    spec, frames = SW.make_clip(n)
    K, dist, R, T = S.default_camera(spec)
    cam = L.make_camera(K, dist, R, T, 2.0)
    eng = engine(spec.height, spec.width, max_markers=512, max_batch=32)
    res = track_shard(eng, frames, n, cam=cam, warmup_frames=0)
    del frames
    table, disp = res.table.cpu().numpy(), res.disp.cpu().numpy()
    m = table.shape[1]
    assert m == spec.n_markers and disp.shape == (n, m, 5)
    centre = int(np.nonzero((table[SW.gap_frames(n)[0], :, 0].astype(int) & 1) == 0)[0][0])
    assert (disp[SW.gap_frames(n), centre, 0] == 0).all() and 0 < disp[:, centre, 0].sum() < n - 1      # gaps exist
    st, cum = eng.series_stats(res.disp, cumulative=True)
    A.check_series(st.cpu().numpy(), cum.cpu().numpy(), disp, res.ids, "tracked series_stats")
    windows = [(1, 30), (120, 150), (0, n - 1), (SW.gap_frames(n)[0], SW.gap_frames(n)[0])]
    A.check_window_means(eng.window_means(res.table, windows).cpu().numpy(), table, windows, "tracked window_means")
    A.check_disp_from_frame(eng.displacement_from_frame(res.table, 0).cpu().numpy(), table, 0, "tracked from frame 0")
    # analyze_tables against the oracle and against the EXISTING analyze_displacement's CSV on the flattened rows
    cfg = Config(data_dir=tmp_path / "d", output_dir=tmp_path / "o", plots_dir=tmp_path / "p")
    ma = MarkerAnalysis(cfg)
    frame = ma.analyze_tables(res.disp, res.ids, engine=eng)
    counts = (disp[..., 0] != 0).sum(axis=0)
    got = A.stats_from_frame(frame, res.ids, counts)
    A.check_stats(got, A.series_stats(disp, res.ids)[0], disp, "analyze_tables vs oracle")
    rows = A.disp_rows(disp, res.ids).drop(columns=["slot"])
    ma.analyze_displacement(rows.sample(frac=1.0, random_state=0))
    csv = pd.read_csv(tmp_path / "p" / "displacement_statistics.csv", header=[0, 1], index_col=[0, 1],
                      float_precision="round_trip")       # (the default parser may be an ulp off the digits written)
    assert len(csv) == len(frame) == int((counts > 0).sum())
    A.check_stats(got, A.stats_from_frame(csv, res.ids, counts), disp, "analyze_tables vs analyze_displacement's CSV")
    eng.close()


SHAPES = [(n, m) for n in (1, CH - 1, CH, CH + 1, 4096) for m in (1, 65, 441)]


@pytest.mark.parametrize("case", range(len(SHAPES) + 8))
def test_shapes_that_exercise_the_grid(case):
    """n = 1, CHUNK - 1, CHUNK, CHUNK + 1, 4096 x m_ref = 1, 65, 441, with frame_begin cycling through 0 and values that are
    no multiple of CHUNK and the missing share through 0 %, 3 %, 97 %, 100 %; then every (frame_begin, missing) pair on
    4096 x 65 / CHUNK + 1 x 65."""
    begins, missing = (0, 7, CH + 5, 3 * CH - 1), (0.0, 0.03, 0.97, 1.0)
    if case < len(SHAPES):
        (n, m), fb, miss = SHAPES[case], begins[case % 4], missing[(case // 2) % 4]
    else:
        k = case - len(SHAPES)
        n, m, fb, miss = (4096 if k < 4 else CH + 1), 65, begins[1 + k % 3], missing[k % 4]
    from vbs_amd.engine import series_stats_f64
    rng = np.random.default_rng(1000 + case)
    disp = random_disp(rng, n, m, miss)
    eng = engine()
    d32 = torch.from_numpy(disp).cuda()
    st, cum = eng.series_stats(d32, frame_begin=fb, cumulative=True)
    what = f"n={n} m={m} frame_begin={fb} missing={miss}"
    A.check_series(st.cpu().numpy(), cum.cpu().numpy(), disp, None, what)
    st2, cum2 = eng.series_stats(d32, frame_begin=fb, cumulative=True)                        # determinism
    assert torch.equal(bits(st), bits(st2)) and torch.equal(bits(cum), bits(cum2))
    rec = eng.series_partial(d32, frame_begin=fb)
    assert rec.shape[0] == len({f // CH for f in range(fb, fb + n)})
    assert torch.equal(bits(eng.series_merge(rec)), bits(st))
    st64 = series_stats_f64(torch.from_numpy(disp.astype(np.float64)).cuda(), frame_begin=fb)
    A.check_series(st64.cpu().numpy(), None, disp, None, what + " f64")
    # table-side kernels on the same grid: flags from the same pattern
    table = np.zeros((n, m, 10), dtype=np.float32)
    table[..., 0] = np.where(disp[..., 0] != 0, 3, rng.integers(0, 2, (n, m)))
    table[..., 6:9] = (50 * rng.standard_normal((n, m, 3))).astype(np.float32)
    t32 = torch.from_numpy(table).cuda()
    windows = [(0, n - 1), (n // 2, n // 2), (n // 3, min(n - 1, n // 3 + CH)), (0, min(n - 1, CH - 1))] + \
              [(min(i, n - 1), n - 1) for i in range(17)]                                  # more windows than one launch takes
    wm = eng.window_means(t32, windows)
    A.check_window_means(wm.cpu().numpy(), table, windows, what + " window_means")
    assert torch.equal(bits(wm), bits(eng.window_means(t32, windows)))
    ref = n // 2
    out = eng.displacement_from_frame(t32, ref)
    A.check_disp_from_frame(out.cpu().numpy(), table, ref, what + " from_frame")
    assert torch.equal(bits(out), bits(eng.displacement_from_frame(t32, ref)))
    eng.close()


def test_scratch_is_sized_by_the_call_and_kept():
    """The handle's scratch follows the call (a 4096-frame sequence on a handle built for passes of 2 frames), and a smaller
    call afterwards reuses it: results stay right in either order."""
    rng = np.random.default_rng(5)
    eng = engine(max_batch=2)
    small, big = random_disp(rng, 40, 7, 0.03), random_disp(rng, 4096, 441, 0.03)
    for d in (small, big, small):
        st, cum = eng.series_stats(torch.from_numpy(d).cuda(), cumulative=True)
        A.check_series(st.cpu().numpy(), cum.cpu().numpy(), d, None, f"{d.shape}")
    eng.close()


def test_bad_arguments_raise_and_launch_nothing(gold):
    eng = engine()
    lib, h = eng.lib, eng._h
    d32 = torch.from_numpy(gold["disp"]).cuda()
    t32 = torch.from_numpy(gold["table"]).cuda()
    n, m = d32.shape[0], d32.shape[1]
    out = torch.zeros((n, m, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((m, 5), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    eng.profile(True)
    for bad in ([(0, n)], [(-1, 3)], [(5, 4)], [(1, 30), (120, n)], []):
        with pytest.raises(ValueError):
            eng.window_means(t32, bad)
    for ref in (-1, n, n + 100):
        with pytest.raises(ValueError):
            eng.displacement_from_frame(t32, ref)
    with pytest.raises(ValueError):
        eng.series_stats(d32, frame_begin=-1)
    with pytest.raises(ValueError):
        eng.series_stats(d32[:0])
    with pytest.raises(ValueError):
        eng.series_partial(d32, frame_begin=-3)
    with pytest.raises(ValueError):
        eng.series_stats(t32)                                 # a table is not a disp
    # the C entry points themselves: n <= 0, null required pointers
    w = np.array([[1, 30]], dtype=np.int32)
    wp = w.ctypes.data_as(C.c_void_p)
    assert lib.vbs_series_stats(h, p(d32), 0, m, 0, p(stats), None, None) == L.VBS_EINVAL
    assert lib.vbs_series_stats(h, p(d32), -4, m, 0, p(stats), None, None) == L.VBS_EINVAL
    assert lib.vbs_series_stats(h, None, n, m, 0, p(stats), None, None) == L.VBS_EINVAL
    assert lib.vbs_series_stats(h, p(d32), n, m, 0, None, None, None) == L.VBS_EINVAL
    assert lib.vbs_series_stats_f64(0, p(d32), n, m, 0, p(stats), None, None, None) == L.VBS_EINVAL      # no scratch
    assert lib.vbs_series_partial(h, p(d32), n, m, 0, None, None) == L.VBS_EINVAL
    assert lib.vbs_series_merge(h, None, 1, m, p(stats), None, None) == L.VBS_EINVAL
    assert lib.vbs_series_merge(h, p(stats), 0, m, p(stats), None, None) == L.VBS_EINVAL
    assert lib.vbs_window_means(h, p(t32), 0, m, wp, 1, p(out), None) == L.VBS_EINVAL
    assert lib.vbs_window_means(h, p(t32), n, m, None, 1, p(out), None) == L.VBS_EINVAL
    assert lib.vbs_window_means(h, p(t32), n, m, wp, 1, None, None) == L.VBS_EINVAL
    assert lib.vbs_displacement_from_frame(h, p(t32), 0, m, 0, p(out), None) == L.VBS_EINVAL
    assert lib.vbs_displacement_from_frame(h, p(t32), n, m, 0, None, None) == L.VBS_EINVAL
    assert eng.profile_read() == {}, "a refused call launched a kernel"
    # ... and the same handle still works, its launches seen by the profiler under the kernels' names
    eng.series_stats(d32, cumulative=True)
    eng.window_means(t32, [(1, 30)])
    eng.displacement_from_frame(t32, 0)
    assert set(eng.profile_read()) == {"k_series_partial", "k_series_finalize", "k_series_cumsum", "k_window_partial",
                                       "k_window_finalize", "k_disp_from_frame"}
    eng.profile(False)
    eng.close()


@pytest.mark.parametrize("n_total,aligned", [(100, False), (4 * CH, True)])
def test_series_stats_shard_two_ranks_on_one_gpu(tmp_path, n_total, aligned):
    """Two ranks as fresh child processes sharing GPU 0 (gloo): each reduces its own frames to chunk records, one
    all-gather, the same ordered merge on both.  Shard edge inside a chunk: the ranks agree bit for bit and match the
    single-process statistics within the bounds; chunk-aligned edge: bit-identical to the single process as well.
    (No scaling number follows from this: both ranks share one GPU and the transport is gloo.)"""
    import socket
    import subprocess
    import series_worker as SW
    from vbs_amd.pipeline import series_stats_shard, track_shard
    assert ((n_total // 2) % CH == 0) == aligned
    spec, frames = SW.make_clip(n_total)
    K, dist, R, T = S.default_camera(spec)
    cam = L.make_camera(K, dist, R, T, 2.0)
    eng = engine(spec.height, spec.width, max_markers=512, max_batch=16)
    one = track_shard(eng, frames, n_total, cam=cam, warmup_frames=0)
    del frames
    stats1 = eng.series_stats(one.disp)
    assert torch.equal(bits(series_stats_shard(eng, one, n_total)), bits(stats1))        # world of one: the same numbers
    disp1, stats1 = one.disp.cpu().numpy(), stats1.cpu().numpy()
    A.check_series(stats1, None, disp1, one.ids, "single process")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = os.path.join(os.path.dirname(__file__), "helpers", "series_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(n_total), str(tmp_path)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    z = [np.load(tmp_path / f"series_rank{r}.npz") for r in range(2)]
    e = n_total // 2
    assert [tuple(x["span"]) for x in z] == [(0, e), (e, n_total)]
    for r, (a, b) in enumerate(((0, e), (e, n_total))):
        assert np.array_equal(z[r]["disp"], disp1[a:b])
    assert np.array_equal(z[0]["stats"].view(np.int64), z[1]["stats"].view(np.int64))      # rank 0 == rank 1, bit for bit
    A.check_stats(z[0]["stats"], A.series_stats(disp1, one.ids)[0], disp1, "two ranks vs oracle")
    A.check_stats(z[0]["stats"], stats1, disp1, "two ranks vs single process")
    if aligned:
        assert np.array_equal(z[0]["stats"].view(np.int64), stats1.view(np.int64))
    # the gaps around the edge made the displacement after them look back across it
    centre = int(np.nonzero(disp1[e, :, 0] == 0)[0][0])
    assert disp1[e + 1, centre, 0] == 0 and disp1[e + 2, centre, 0] == 1
    eng.close()
