"""CPU tests of the analysis layer's host side (no GPU): the pandas / NumPy oracle the GPU tests compare against is pinned to
the golden made from the reference's own statements (`tests/golden/analysis.npz`, `make_analysis_golden.py`); the marker
numbering against the numbers printed in the reference's figure; the L4 sheet and its .xlsx round trip; the new C symbols.
Bounds: see `tests/helpers/analysis_oracle.py` (derived from the float64 summation error, not from what the code gives)."""
import json
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import ids as I

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import analysis_oracle as A                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vbs_series_chunks", "vbs_series_stats", "vbs_series_stats_f64", "vbs_series_partial", "vbs_series_merge",
               "vbs_window_means", "vbs_displacement_from_frame")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "analysis.npz")))


def test_golden_holds_the_cases_it_is_meant_to(gold):
    st, d, t = gold["stats"], gold["disp"], gold["table"]
    assert d.dtype == np.float32 and t.dtype == np.float32 and d.shape == (160, 19, 5) and t.shape == (160, 19, 10)
    xyz = (t[..., 0].astype(int) & 2) != 0
    (a0, b0), (a1, b1) = gold["windows"].tolist()
    assert (st[:, 0] == 0).sum() >= 1 and not xyz[:, 3].any()                       # a slot never seen
    assert (st[:, 0] == 1).sum() >= 1 and np.isnan(st[st[:, 0] == 1, 2]).all()     # exactly one displacement row: std NaN
    assert xyz[a0:b0 + 1, 9].any() and not xyz[a1:b1 + 1, 9].any()                  # missing from one of the two windows
    assert (st[:, 1] >= 100 * st[:, 2]).any()                                       # the cancellation case
    assert (~xyz[a0:b0 + 1, 2]).any() and (~xyz[a1:b1 + 1, 2]).any() and xyz[a0:b0 + 1, 2].any() and xyz[a1:b1 + 1, 2].any()
    assert xyz[0].sum() > 19 // 2 and not xyz[0].all()                              # frame 0 for most slots, not all


def test_oracle_series_stats_equal_the_reference_statements(gold):
    A.check_series(gold["stats"], None, gold["disp"], gold["ids"], "golden vs oracle")
    st, cum, rows = A.series_stats(gold["disp"], gold["ids"])
    # the oracle IS those statements on the same rows: expect it bit for bit where the reference has a value
    assert np.array_equal(st, gold["stats"], equal_nan=True)
    assert np.array_equal(np.isnan(gold["cumulative"]), ~rows)
    assert np.array_equal(cum[rows], gold["cumulative"][rows])
    # carried over the entries that are no rows, 0 before the first
    assert (cum[:, 3] == 0).all() and (cum[:11, 5] == 0).all() and (cum[11:, 5] == cum[11, 5]).all()


def test_oracle_window_means_and_displacement_equal_the_reference_statements(gold):
    windows = [tuple(w) for w in gold["windows"].tolist()]
    wm = A.window_means(gold["table"], windows)
    for w in range(2):
        assert np.array_equal(wm[w, :, 1:], gold[f"win_all_{w}"], equal_nan=True)
        assert np.array_equal(wm[w, :, 0] == 0, np.isnan(gold[f"win_all_{w}"][:, 0]))
    for tag, slots in (("all", None), ("sel", gold["target_slots"])):
        got = A.window_displacement(gold["table"], windows[0], windows[1], slots)
        assert np.array_equal(got["slots"], gold[f"merged_{tag}_slots"])
        want = gold[f"merged_{tag}_d"]
        assert (np.abs(got["d"] - want) <= A.REL_POINT * np.abs(want)).all()
        assert abs(got["mean"] - float(gold[f"merged_{tag}_mean"])) <= A.REL_POINT * float(gold[f"merged_{tag}_mean"])
    assert 9 not in gold["merged_all_slots"] and 3 not in gold["merged_all_slots"]


def test_oracle_distance_from_frame_0_equals_the_reference_statements(gold):
    got = A.disp_from_frame(gold["table"], 0)
    want = gold["scalar"]
    assert np.array_equal(got[..., 0] == 1, ~np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[..., 1][ok] - want[ok]) <= A.REL_POINT * np.abs(want[ok])).all()
    assert (got[..., 1][~ok] == 0).all()


def test_marker_ids_are_the_numbers_printed_in_the_reference_figure(golden_dir):
    """The figure's 65 measured centres through the frame-0 assignment (`full`), then `marker_ids`: every marker must get
    the number the reference printed next to it (65 of 65)."""
    with open(os.path.join(golden_dir, "figure_2d.json")) as f:
        ms = json.load(f)["markers"]
    assert sorted(m["label"] for m in ms) == list(range(1, 66))
    perm = np.random.default_rng(0).permutation(65)                  # (detection order must not matter)
    markers = [{"center": (ms[i]["u"], ms[i]["v"]), "major_axis": ms[i]["major_axis"], "minor_axis": ms[i]["minor_axis"],
                "angle": ms[i]["angle"]} for i in perm]
    table = I.assign_ids(markers, 5, "full", "optimal")
    ids, xy = I.reference_arrays(table)
    got = I.marker_ids(ids)
    label_at = {(m["u"], m["v"]): m["label"] for m in ms}
    want = np.array([label_at[(x, y)] for x, y in xy.tolist()])
    assert int((got == want).sum()) == 65, np.nonzero(got != want)
    assert np.array_equal(got, np.array([1 + [0, 1, 7, 19, 37, 61][lay] + k for lay, k in ids.tolist()]))


def test_marker_ids_on_a_full_7x7_table():
    import vbs_amd.synth as S
    spec = S.config1()
    truth = S.dot_truth(spec, 5, [0])
    markers = [{"center": (float(x), float(y)), "major_axis": float(d), "minor_axis": float(d), "angle": 0.0} for x, y, d in truth[0]]
    ids, _ = I.reference_arrays(I.assign_ids(markers, 5, "full", "optimal"))
    assert len(ids) == 49
    got = I.marker_ids(ids)
    assert got.dtype.kind == "i" and sorted(got.tolist()) == list(range(1, 50))
    order = np.argsort(got)
    assert [tuple(k) for k in ids[order].tolist()] == sorted(tuple(k) for k in ids.tolist())
    assert got[0] == 1 and tuple(ids[0]) == (0, 0)


def test_to_marker_frame_schema_and_xlsx_round_trip(gold, tmp_path):
    from vbs_amd.pipeline import to_marker_frame
    from vbs_amd.xlsx_io import read_xlsx
    t = gold["table"]
    path = tmp_path / "marker_3d_coordinates.xlsx"
    df = to_marker_frame(t, gold["ids"], frame_offset=0, path=path)
    assert list(df.columns) == ["frameno", "marker_id", "Xw", "Yw", "Zw"]
    assert df["frameno"].dtype == np.int64 and df["marker_id"].dtype == np.int64
    assert all(df[c].dtype == np.float64 for c in ("Xw", "Yw", "Zw"))
    xyz = (t[..., 0].astype(int) & L.FLAG_XYZ) != 0
    assert len(df) == int(xyz.sum())
    assert np.array_equal(df["marker_id"].to_numpy(), np.broadcast_to(gold["marker_id"], xyz.shape)[xyz])
    assert np.array_equal(df["Xw"].to_numpy(), t[..., 6][xyz].astype(np.float64))
    assert (np.diff(df["frameno"].to_numpy()) >= 0).all()
    assert to_marker_frame(t, gold["ids"], frame_offset=100)["frameno"].min() == 100
    back = read_xlsx(path)
    assert list(back.columns) == list(df.columns) and len(back) == len(df)
    for c in df.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64)), c
    # the sheet is what the oracle's (= the reference's) window means read
    want = A.marker_rows(t, gold["marker_id"])
    assert np.array_equal(want[["frameno", "marker_id"]].to_numpy(), df[["frameno", "marker_id"]].to_numpy())


def test_new_header_symbols_are_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.SERIES_CHUNK, L.SERIES_REC_COLS, L.STATS_COLS, L.WINDOW_COLS) == (
        defs["VBS_SERIES_CHUNK"], defs["VBS_SERIES_REC_COLS"], defs["VBS_STATS_COLS"], defs["VBS_WINDOW_COLS"])


def test_series_chunks_counts_the_global_chunks_a_call_touches():
    lib, ch = L.lib(), L.SERIES_CHUNK
    for n, fb in ((1, 0), (ch - 1, 0), (ch, 0), (ch + 1, 0), (4096, 0), (1, ch - 1), (2, ch - 1), (ch, 1), (3 * ch, 5), (7, 123)):
        want = len({f // ch for f in range(fb, fb + n)})
        assert lib.vbs_series_chunks(n, fb) == want, (n, fb)
    assert lib.vbs_series_chunks(0, 0) == L.VBS_EINVAL and lib.vbs_series_chunks(4, -1) == L.VBS_EINVAL
    assert lib.vbs_series_chunks(2, 2**31 - 2) == L.VBS_EINVAL
