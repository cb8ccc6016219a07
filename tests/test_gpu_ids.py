"""GPU tests of the first-frame identity assignment on the device (`k_assign_ids`, csrc/k_ids.hip, through `Engine.assign_ids` and
`vbs_assign_ids` itself; run on the MI355X box: `pytest -m gpu`).

Expected values (tests/helpers/ids_cases.py says why no comparison here hangs on the last bit of an atan2, a sqrt or a sum):
  * margin cases - the exact integer oracle (tests/helpers/ids_oracle.py): keys in dict order and float64 coordinates bit for
    bit, detection order within every exact angle tie included (equal bits from atan2 on collinear points, stable rank);
  * tie cases - the host restatement `ids.assign_ids` bit for bit, the oracle's centre, and cuts that the oracle prices as
    exactly optimal (1e-12 relative);
  * the 256-thread stride and the IDS_MAXN sizes - `ids.assign_ids` and `oracle.process_first_frame` bit for bit (the latter's
    scalar DP takes 12 s at 1024 markers and 16 layers, so that one size is held to `ids.assign_ids` alone).
Every `det` buffer has more rows than markers, NaN and +-1e300 in every cell that must not be read, and is presented both dense
and as a strided slice of a larger tensor.  tests/test_ids_host.py vets the cases and both references on the CPU."""
import ctypes as C
import functools
import os
import sys
from decimal import Decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import ids as I                                  # noqa: E402
from oracle import stages as O                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ids_cases as K                                         # noqa: E402
import ids_oracle as X                                        # noqa: E402

PAD = 5                                                       # rows of junk past `count`


def make_engine():
    from vbs_amd.engine import Engine
    return Engine(480, 640, max_markers=1024, max_batch=1)


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


def det_tensors(case):
    """The case's `det` twice: dense [1, maxm, 6], and the same rows as a strided 2-D slice of a larger NaN-filled tensor."""
    n = len(case["pts"])
    det = torch.from_numpy(K.det_rows(case, n + PAD)).cuda()
    big = torch.full((2 * (n + PAD) + 1, 9), float("nan"), dtype=torch.float64, device="cuda")
    view = big[1::2, 2:8]
    view.copy_(det)
    assert not view.is_contiguous()
    return det[None], view, torch.tensor([n], dtype=torch.int32, device="cuda")


def device_table(eng, case, mode, both_layouts=True):
    dense, view, counts = det_tensors(case)
    ids, xy = eng.assign_ids(dense, counts, case["layers"], mode)
    ids, xy = ids.cpu().numpy().astype(np.int64), xy.cpu().numpy()
    if both_layouts:
        ids2, xy2 = eng.assign_ids(view, counts, case["layers"], mode)
        assert np.array_equal(ids2.cpu().numpy(), ids) and xy2.cpu().numpy().tobytes() == xy.tobytes(), "the slice changed the result"
    return ids, xy


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


@functools.lru_cache(maxsize=None)
def host_table(name, mode):
    case = K.BY_NAME[name]
    return K.arrays(I.assign_ids(K.markers(case), case["layers"], mode, "optimal"))


@functools.lru_cache(maxsize=None)
def stages_table(name, mode):
    case = K.BY_NAME[name]
    return K.arrays(O.process_first_frame(K.markers(case), case["layers"], mode, "optimal"))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.names("margin"))
def test_margin_cases_equal_the_exact_oracle(eng, name, mode):
    got = device_table(eng, K.BY_NAME[name], mode)
    want = K.exact_table(name, mode)
    assert got[0].tolist() == want[0].tolist()
    assert same(got, want), np.where((got[1] != want[1]).any(axis=1))[0]


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.names("tie"))
def test_tie_cases_equal_the_host_restatement_with_optimal_cuts(eng, name, mode):
    case, rep = K.BY_NAME[name], K.report(name)
    got = device_table(eng, case, mode)
    assert got[1][0].tobytes() == K.xy(case)[rep["ci"]].tobytes(), "not the oracle's centre"
    if mode == "full":
        groups = K.layer_r2(case, *got)
        assert sum(len(g) for g in groups) == rep["n"] - 1
        assert abs(X.sse_of_groups(groups) - rep["sse"]) <= Decimal("1e-12") * rep["sse"], "the device's cuts are not optimal"
    assert same(got, host_table(name, mode))


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.names(group="stride") + K.names(group="capacity"))
def test_stride_and_capacity_sizes_equal_the_restatements(eng, name, mode):
    case = K.BY_NAME[name]
    got = device_table(eng, case, mode, both_layouts=len(case["pts"]) < 1000)
    assert same(got, host_table(name, mode)), "ids.assign_ids"
    if not (case["group"] == "capacity" and case["layers"] == 16):
        assert same(got, stages_table(name, mode)), "oracle.process_first_frame"
    assert len(got[0]) == (len(case["pts"]) if mode == "full" else 1 + min(case["layers"], len(case["pts"]) - 1))


def test_calls_are_deterministic_and_leave_nothing_behind(eng):
    """Two calls give the same bits; a small case after the IDS_MAXN one on the same handle gives what a fresh handle gives
    (the kernel's LDS tables and the handle carry nothing over)."""
    big, small = K.BY_NAME["capacity_n1024_L16"], K.BY_NAME["fewer_n4_L16"]
    fresh = make_engine()
    first = {m: device_table(fresh, small, m, both_layouts=False) for m in K.MODES}
    fresh.close()
    for name in ("capacity_n1024_L16", "sweep_exact_L16", "rays8_L2"):
        for mode in K.MODES:
            a = device_table(eng, K.BY_NAME[name], mode, both_layouts=False)
            assert same(a, device_table(eng, K.BY_NAME[name], mode, both_layouts=False)), (name, mode)
    for mode in K.MODES:
        device_table(eng, big, "full", both_layouts=False)
        after = device_table(eng, small, mode, both_layouts=False)
        assert same(after, first[mode]) and same(after, K.exact_table(small["name"], mode)), mode


# ---------------------------------------------------------------------------------------------------------------------
IDS_FILL, XY_FILL, M_FILL = -77, -7.5, 12345


def raw_call(eng, det, count, layers, mode, cap, rows, null=None):
    """`vbs_assign_ids` itself on sentinel-filled outputs of `rows` rows: (status, m_out, ids, ref_xy)."""
    ids = torch.full((rows, 2), IDS_FILL, dtype=torch.int32, device="cuda")
    xy = torch.full((rows, 2), XY_FILL, dtype=torch.float64, device="cuda")
    m = torch.full((1,), M_FILL, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = {k: C.c_void_p(t.data_ptr()) for k, t in (("det", det), ("count", cnt), ("ids", ids), ("xy", xy), ("m", m))}
    if null:
        p[null] = None
    rc = eng.lib.vbs_assign_ids(eng._h, p["det"], p["count"], layers, mode, p["ids"], p["xy"], cap, p["m"], None)
    torch.cuda.synchronize()
    return rc, int(m.item()), ids.cpu().numpy(), xy.cpu().numpy()


def untouched(ids, xy):
    return (ids == IDS_FILL).all() and (xy == XY_FILL).all()


def test_refusals_and_statuses(eng):
    case = K.BY_NAME["sweep_jitter_L5"]
    n = len(case["pts"])
    dense, _, counts = det_tensors(case)
    det = dense[0]
    rows = n + 4
    for mode, name in enumerate(K.MODES):
        want = K.exact_table(case["name"], name)
        M = len(want[0])
        # cap == M succeeds and writes M rows, no more
        rc, m, ids, xy = raw_call(eng, det, n, 5, mode, M, rows)
        assert (rc, m) == (L.VBS_OK, M) and same((ids[:M].astype(np.int64), xy[:M]), want) and untouched(ids[M:], xy[M:])
        # cap == M - 1: refused on the device, nothing written
        rc, m, ids, xy = raw_call(eng, det, n, 5, mode, M - 1, rows)
        assert (rc, m) == (L.VBS_OK, -2) and untouched(ids, xy)
        # no markers; a device status in place of the count
        rc, m, ids, xy = raw_call(eng, det, 0, 5, mode, rows, rows)
        assert (rc, m) == (L.VBS_OK, -1) and untouched(ids, xy)
        rc, m, ids, xy = raw_call(eng, det, -3, 5, mode, rows, rows)
        assert (rc, m) == (L.VBS_OK, -3000) and untouched(ids, xy)
        # more layers than VBS_IDS_MAX_LAYERS: refused on the host
        rc, m, ids, xy = raw_call(eng, det, n, L.IDS_MAX_LAYERS + 1, mode, rows, rows)
        assert (rc, m) == (L.VBS_EINVAL, M_FILL) and untouched(ids, xy)
        assert b"VBS_IDS_MAX_LAYERS" in eng.lib.vbs_last_error(eng._h)
        # the largest legal layer count is not refused
        rc, m, ids, xy = raw_call(eng, det, n, L.IDS_MAX_LAYERS, mode, rows, rows)
        assert rc == L.VBS_OK and m == (n if mode else 1 + L.IDS_MAX_LAYERS)
    # more markers than VBS_IDS_MAX_MARKERS: refused on the device (the count lives there), never truncated
    over = L.IDS_MAX_MARKERS + 1
    wide = torch.from_numpy(K.det_rows(K.BY_NAME["capacity_n1024_L16"], over + PAD)).cuda()
    wide[L.IDS_MAX_MARKERS, :2] = torch.tensor([17.0, 23.0], dtype=torch.float64)
    for mode in (0, 1):
        rc, m, ids, xy = raw_call(eng, wide, over, 5, mode, over + 1, over + 1)
        assert (rc, m) == (L.VBS_OK, -3) and untouched(ids, xy)
    # ... and the same through Engine.assign_ids
    with pytest.raises(L.VbsError, match=str(L.IDS_MAX_MARKERS)):
        eng.assign_ids(wide[None], torch.tensor([over], dtype=torch.int32, device="cuda"), 5, "full")
    with pytest.raises(ValueError, match=f"{L.IDS_MAX_LAYERS} "):
        eng.assign_ids(dense, counts, L.IDS_MAX_LAYERS + 1, "full")
    with pytest.raises(ValueError, match="No markers detected in first frame!"):
        eng.assign_ids(dense, torch.zeros_like(counts), 5, "full")
    with pytest.raises(L.VbsError, match="device status -3 in frame 0"):
        eng.assign_ids(dense, torch.full_like(counts, -3), 5, "as_written")
    with pytest.raises(ValueError):
        eng.assign_ids(dense, counts, 5, "nope")
    ok = eng.assign_ids(wide[None], torch.tensor([L.IDS_MAX_MARKERS], dtype=torch.int32, device="cuda"), L.IDS_MAX_LAYERS, "full")
    assert len(ok[0]) == L.IDS_MAX_MARKERS


def test_bad_arguments_raise_and_launch_nothing(eng):
    case = K.BY_NAME["fewer_n6_L5"]
    dense, _, counts = det_tensors(case)
    n = len(case["pts"])
    eng.profile(True)
    try:
        for layers in (L.IDS_MAX_LAYERS + 1, 0, -1, 1 << 20):
            with pytest.raises(ValueError):
                eng.assign_ids(dense, counts, layers, "full")
            rc, m, ids, xy = raw_call(eng, dense[0], n, layers, 1, n + 1, n + 1)
            assert (rc, m) == (L.VBS_EINVAL, M_FILL) and untouched(ids, xy), layers
        for null in ("det", "count", "ids", "xy", "m"):
            rc, m, ids, xy = raw_call(eng, dense[0], n, 5, 1, n + 1, n + 1, null=null)
            assert (rc, m) == (L.VBS_EINVAL, M_FILL) and untouched(ids, xy), null
        for cap, mode in ((0, 1), (-1, 0), (n + 1, 2), (n + 1, -1)):
            rc, m, ids, xy = raw_call(eng, dense[0], n, 5, mode, cap, n + 1)
            assert (rc, m) == (L.VBS_EINVAL, M_FILL) and untouched(ids, xy), (cap, mode)
        assert eng.lib.vbs_assign_ids(None, None, None, 5, 0, None, None, 1, None, None) == L.VBS_EINVAL
        assert eng.profile_read() == {}, "a refused call launched a kernel"
        # ... and the same handle still works, its launch seen by the profiler under the kernel's name
        got = eng.assign_ids(dense, counts, 5, "full")
        assert set(eng.profile_read()) == {"k_assign_ids"}
        assert same((got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy()), K.exact_table(case["name"], "full"))
    finally:
        eng.profile(False)
