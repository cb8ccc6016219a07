"""GPU tests of the despiking entry (k_robust.hip; run on the MI355X box: `pytest -m gpu`): the gap-aware rolling median and
MAD, the Hampel rule, the clean record, and `pipeline.despike_table`.

An order statistic has no order of summation, so EVERY entry of every result is held BIT FOR BIT (uint64 views) to the
restatement of `tests/helpers/robust_oracle.py`, which shares no algorithm with the kernel; nothing is skipped or masked.  Shapes
are the smallest at which the kernel can go wrong: n around the window and around the tile (VBS_ROBUST_TILE frames), s around the
wave (64 series), not the workload's.

The restatement has two forms.  The loops of `hampel` (`sorted` on (x, g) pairs per frame, series and value) are the definition,
but too slow for every entry of the sweep; `hampel_np` (one stable sort per window) is what every entry of the device's result is
compared with, and the loops are evaluated beside it on whole shapes of up to `LOOP_ENTRIES` entries and otherwise on the first,
middle and last series, where they must give `hampel_np`'s bits.  `tests/test_robust_host.py` holds the two forms to each other.
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
import robust_oracle as O                                     # noqa: E402

TILE = L.ROBUST_TILE
COLS = ((2, 1), (4, 3), (5, 3), (8, 7))                       # (cols, n_values): a bare series, `axis`, `total`, the widest
GAPS = ("none", "random", "long", "dead series", "random and dead")
SERIES = (1, 63, 64, 65, 130)


def engine(h=480, w=640, **kw):
    from vbs_amd.engine import Engine
    kw.setdefault("max_markers", 256)
    kw.setdefault("max_batch", 2)
    return Engine(h, w, **kw)


def dev(rec, nv, h, **kw):
    from vbs_amd.engine import hampel_series_f64
    out, clean = hampel_series_f64(torch.from_numpy(rec).cuda(), h, n_values=nv, **kw)
    return out.cpu().numpy(), (None if clean is None else clean.cpu().numpy())


def checked(rec, nv, h, what="", **kw):
    """The device's (out, clean) for rec, held to the restatement in every bit."""
    out, clean = dev(rec, nv, h, **kw)
    O.check(out, clean, rec, nv, h, what=what, **kw)
    return out, clean


def make_rec(rng, n, s, cols, kind, window):
    """[n, s, cols] float64 with the gaps of `kind`; NaN and 1e30 in EVERY invalid entry and in every column past the values
    (the caller's n_values decides which those are: all columns carry junk where invalid, the values past nv are never read)."""
    rec = rng.normal(0.0, 3.0, (n, s, cols)) + 10.0 * rng.standard_normal((1, s, 1))
    valid = np.ones((n, s), dtype=bool)
    if "random" in kind:
        valid &= rng.random((n, s)) >= 0.2
    if kind == "long" and n > 2:
        a = min(n // 3, max(0, n - window - 3))
        valid[a:a + window + 2, s // 2] = False
        if a + window + 2 < n:
            valid[a + window + 2, s // 2] = True
    if "dead" in kind:
        valid[:, s - 1] = False
    rec[..., 0] = np.where(valid, rng.choice([1.0, 2.0, -1.0, 1e-300], (n, s)), 0.0)       # any nonzero flag is valid
    junk = np.where(rng.random((n, s, cols - 1)) < 0.5, np.nan, 1e30)
    rec[..., 1:] = np.where(valid[..., None], rec[..., 1:], junk)
    return rec


def junk_past(rec, nv, rng):
    """NaN or 1e30 in every column past the values, valid rows included."""
    extra = rec.shape[2] - 1 - nv
    if extra:
        rec[..., 1 + nv:] = np.where(rng.random(rec.shape[:2] + (extra,)) < 0.5, np.nan, 1e30)
    return rec


@pytest.mark.parametrize("h", (0, 1, 7, 31))
def test_hampel_equals_the_restatement_on_every_edge_shape(h):
    rng = np.random.default_rng(100 + h)
    ns = sorted({1, 2, max(1, 2 * h), 2 * h + 1, 2 * h + 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5})
    i, seen = 0, set()
    for n in ns:
        for s in SERIES:
            (cols, nv), kind = COLS[i % 4], GAPS[(i // 4 + i) % 5]
            i += 1
            rec = junk_past(make_rec(rng, n, s, cols, kind, 2 * h + 1), nv, rng)
            out, clean = checked(rec, nv, h, what=f"h {h} n {n} s {s} cols {cols} nv {nv} {kind}")
            seen |= set(np.unique(out[..., 0]).tolist())
            assert not np.isnan(out).any()
            if "dead" in kind:
                assert (out[:, s - 1] == 0).all()
            if h == 0:                                           # the window is the frame itself
                v = rec[..., 0] != 0
                assert np.array_equal(O.bits(out[..., 2:2 + nv][v]), O.bits(rec[..., 1:1 + nv][v])) and (out[..., 2 + nv:] == 0).all()
                assert np.array_equal(out[..., 0], 3.0 * v) and np.array_equal(O.bits(clean), O.bits(rec))
    print(f"h = {h}: {i} shapes, flags seen {sorted(seen)}")
    # at h = 0 an invalid frame has an empty window (never 2) and a valid one is its own median (never 7)
    assert seen >= ({0.0, 3.0} if h == 0 else {0.0, 2.0, 3.0, 7.0}) and seen <= {0.0, 1.0, 2.0, 3.0, 7.0}


def test_more_frames_than_the_flag_kernel_has_workgroups_for():
    """`k_hampel_flags` runs at most 65535 workgroups of 4 frames and strides over the rest: one series of 4 x 65535 + 7 frames,
    so that the last frames belong to the second stride, with jumps put into both strides."""
    rng = np.random.default_rng(65535)
    n = 4 * 65535 + 7
    rec = np.empty((n, 1, 2))
    rec[:, 0, 0] = rng.random(n) >= 0.1
    rec[:, 0, 1] = np.where(rec[:, 0, 0] != 0, rng.normal(0.0, 1.0, n), np.nan)
    for f in (100, n - 3):                                       # a jump between two valid neighbours
        rec[f - 1:f + 2, 0, 0] = 1.0
        rec[f - 1:f + 2, 0, 1] = (0.25, 50.0, -0.5)
    out, clean = checked(rec, 1, 1, what="two strides", min_scale=0.5)
    assert out[100, 0, 0] == 7 and out[n - 3, 0, 0] == 7 and clean[n - 3, 0, 0] == 0.0 and set(np.unique(out[..., 0])) >= {0.0, 2.0, 3.0, 7.0}


@pytest.mark.parametrize("h", (1, 4, 31))
def test_ties_and_both_zeros(h):
    """Values drawn from {-1, -0.0, 0.0, 1} only: nearly everything ties, and which zero a median is depends on the (x, g)
    order.  Series 0 is all equal; series 1 loses one frame of every 2h + 1, so with min_count = 2h every judged window has an
    even count."""
    rng = np.random.default_rng(h)
    n, s = TILE + 2 * h + 9, 65
    rec = rng.choice([-1.0, -0.0, 0.0, 1.0], (n, s, 4))
    valid = rng.random((n, s)) >= 0.2
    valid[:, :2] = True
    valid[h::2 * h + 1, 1] = False
    rec[:, 0, 1:] = 0.3
    rec[..., 0] = np.where(valid, 1.0, 0.0)
    rec[..., 1:] = np.where(valid[..., None], rec[..., 1:], np.nan)
    for mc in (1, 2 * h):
        out, _ = checked(rec, 3, h, what=f"ties h {h} min_count {mc}", min_count=mc)
        whole = out[:, 0, 0] == 3                                # the all-equal series: its own median, mad 0, never a spike
        assert whole[h:n - h].all() and set(out[:, 0, 0].tolist()) <= {1.0, 3.0}
        assert (out[whole, 0, 2:5] == 0.3).all() and (out[:, 0, 5:] == 0).all()
    judged = out[:, 1, 0] >= 2
    assert judged.any() and (out[judged, 1, 1] == 2 * h).all()
    med = out[..., 2:5][out[..., 0] >= 2]
    assert (np.signbit(med) & (med == 0)).any() and (~np.signbit(med) & (med == 0)).any()       # both zeros came out as medians


def test_the_comparisons_are_strict():
    """min_scale exactly equal to a deviation, and thr * mad exactly equal to one (built from dyadic values): neither is a spike;
    one ulp less on the right-hand side, or more on the left, is."""
    x = np.ones(9)
    x[4] = 1.5                                                   # med 1, mad 0, dev 0.5
    rec = np.stack([np.ones(9), x], axis=1)[:, None, :]
    out, _ = checked(rec, 1, 2, what="min_scale = dev", min_scale=0.5)
    assert (out[:, 0, 0] == 3).all()
    out, clean = checked(rec, 1, 2, what="min_scale < dev", min_scale=float(np.nextafter(0.5, 0.0)))
    assert out[4, 0, 0] == 7 and (np.delete(out[:, 0, 0], 4) == 3).all() and clean[4, 0, 0] == 0.0
    thr = 2.0 * 1.4826                                           # the product the entry forms
    for top, flag in ((thr, 3.0), (float(np.nextafter(thr, np.inf)), 7.0)):
        x = np.array([0.0, 0.0, -1.0, 0.0, top, 0.0, 1.0, 0.0, 0.0])       # window of frame 4: med 0, mad 1, dev = top
        rec = np.stack([np.ones(9), x], axis=1)[:, None, :]
        out, _ = checked(rec, 1, 2, what=f"thr mad against dev {top!r}", k_sigma=2.0)
        assert out[4, 0].tolist() == [flag, 5.0, 0.0, 1.0]
        out, _ = checked(0.25 * rec + np.array([0.75, 0.0]), 1, 2, what="the same scaled by a power of two", k_sigma=2.0)
        assert out[4, 0].tolist() == [flag, 5.0, 0.0, 0.25]


def test_min_count_decides_judged_at_the_ends_and_around_a_long_gap():
    rng = np.random.default_rng(7)
    h, n, s = 7, 3 * TILE + 5, 65
    rec = make_rec(rng, n, s, 4, "long", 2 * h + 1)
    a, j = n // 3, s // 2                                        # the gap: frames a .. a + 2h + 2 of series j
    assert not rec[a:a + 2 * h + 3, j, 0].any() and rec[a - 1, j, 0] != 0 and rec[a + 2 * h + 3, j, 0] != 0
    for mc in (1, h + 1, 2 * h + 1):
        out, _ = checked(rec, 3, h, what=f"min_count {mc}", min_count=mc)
        fl = out[..., 0]
        assert (fl[a + h + 1, j], out[a + h + 1, j, 1]) == (0.0, 0.0)                  # nothing in reach: never judged
        assert out[0, 0, 1] == h + 1 and out[n - 1, 0, 1] == h + 1 and out[a, j, 1] == h and out[a - 1, j, 1] == h + 1
        if mc == 1:
            assert fl[a, j] == 2 and fl[a + 2 * h + 2, j] == 2 and fl[0, 0] >= 3 and fl[a - 1, j] >= 3
        elif mc == h + 1:
            assert fl[a, j] == 0 and fl[0, 0] >= 3 and fl[n - 1, 0] >= 3 and fl[a - 1, j] >= 3
        else:
            assert fl[0, 0] == 1 and fl[n - 1, 0] == 1 and fl[a - 1, j] == 1 and fl[a + 2 * h + 3, j] == 1 and fl[a, j] == 0
            assert (fl[h:n - h, 0] >= 3).all() and (out[..., 2:][fl < 2] == 0).all()


@pytest.mark.parametrize("h", (7, 31))
def test_ranges_runs_series_and_inputs_do_not_change_a_bit(h):
    from vbs_amd.engine import hampel_series_f64
    rng = np.random.default_rng(11 + h)
    n, s = 3 * TILE + 5, 130
    rec = make_rec(rng, n, s, 4, "random", 2 * h + 1)
    full, full_clean = checked(rec, 3, h, what=f"h {h}")
    again = dev(rec, 3, h)
    assert np.array_equal(O.bits(full), O.bits(again[0])) and np.array_equal(O.bits(full_clean), O.bits(again[1]))      # two runs
    cuts = (0, 37, TILE + 1, n)
    parts = [dev(rec, 3, h, frame_range=(cuts[k], cuts[k + 1])) for k in range(3)]
    assert [p[0].shape[0] for p in parts] == [37, TILE + 1 - 37, n - TILE - 1]
    assert np.array_equal(O.bits(np.concatenate([p[0] for p in parts])), O.bits(full))                                     # ranges
    assert np.array_equal(O.bits(np.concatenate([p[1] for p in parts])), O.bits(full_clean))
    empty = dev(rec, 3, h, frame_range=(5, 5))
    assert empty[0].shape == (0, s, 8) and empty[1].shape == (0, s, 4)
    for j in (0, 63, 64, 65, 129):                                                                                          # alone
        alone = dev(np.ascontiguousarray(rec[:, j:j + 1]), 3, h)
        assert np.array_equal(O.bits(alone[0][:, 0]), O.bits(full[:, j])), j
        assert np.array_equal(O.bits(alone[1][:, 0]), O.bits(full_clean[:, j])), j
    out, clean = hampel_series_f64(rec, h, n_values=3)                                                                      # an array
    assert np.array_equal(O.bits(out.cpu().numpy()), O.bits(full)) and np.array_equal(O.bits(clean.cpu().numpy()), O.bits(full_clean))
    out, clean = dev(rec, 3, h, want_clean=False)
    assert clean is None and np.array_equal(O.bits(out), O.bits(full))


def test_refusals_through_the_python_entry():
    from vbs_amd.engine import hampel_series_f64
    rec = torch.ones((10, 2, 4), dtype=torch.float64, device="cuda")
    assert hampel_series_f64(rec, 31, min_count=63)[0].shape == (10, 2, 8)
    for kw in (dict(half_window=32), dict(half_window=-1), dict(min_count=0), dict(min_count=8), dict(k_sigma=0.0),
               dict(k_sigma=float("nan")), dict(min_scale=-1.0), dict(min_scale=float("inf")), dict(n_values=4), dict(n_values=0),
               dict(frame_range=(3, 2)), dict(frame_range=(0, 11)), dict(rec=rec[..., :1]), dict(rec=rec[:, 0]),
               dict(rec=torch.ones((10, 2, 9), dtype=torch.float64, device="cuda"))):
        args = dict(rec=rec, half_window=3)
        args.update(kw)
        with pytest.raises(ValueError):
            hampel_series_f64(**args)


def test_clean_is_the_record_with_its_spikes_turned_into_gaps():
    """Bit-equal to rec outside col 0 of the spike entries (NaN payloads included), and a record the FIR takes as it is: what
    the device filters from it is what the f10 restatement gives on the restated clean record."""
    from vbs_amd.engine import fir_series_f64, hampel_series_f64
    rng = np.random.default_rng(5)
    n, s, h = 3 * TILE + 5, 65, 7
    rec = make_rec(rng, n, s, 5, "random", 2 * h + 1)
    rec.view(np.uint64)[..., 4][rec[..., 0] == 0] = 0x7ff8dead0000beef                    # a NaN with a payload of its own
    rec[rng.random((n, s)) < 0.02, 1] += 40.0                                             # jumps of 13 noise amplitudes
    out, clean = checked(rec, 3, h, what="clean")
    spike = out[..., 0] == 7
    assert spike.sum() >= 20 and np.array_equal(O.bits(clean[..., 1:]), O.bits(rec[..., 1:]))
    assert np.array_equal(O.bits(clean[..., 0][~spike]), O.bits(rec[..., 0][~spike])) and (clean[..., 0][spike] == 0).all()
    assert not np.signbit(clean[..., 0][spike]).any()
    taps = F.lowpass_taps(31, .08)
    dclean = hampel_series_f64(torch.from_numpy(rec).cuda(), h, n_values=3)[1]
    got = fir_series_f64(dclean, taps, 3).cpu().numpy()
    want = FO.fir(O.hampel_np(rec, 3, h)[1], F.half_taps(taps), 3)
    assert np.array_equal(O.bits(got), O.bits(want))
    assert not np.array_equal(O.bits(got), O.bits(FO.fir(rec, F.half_taps(taps), 3)))      # ... and the spikes did change it


def test_despike_table_end_to_end(tmp_path):
    from vbs_amd.pipeline import despike_table, polishing_analysis, to_spike_frame
    eng = engine()
    rng = np.random.default_rng(3)
    n, m, h = 3 * TILE + 5, 65, 7
    t = FO.figure11_table(n, m, 60, 0)
    drop = rng.random((n, m)) < 0.03                             # tracked, but no 3-D point
    t[drop, 0] = 1.0
    t[drop, 6:9] = np.float32(1e30)
    injected = [(0, 4), (5, 0), (40, 64), (TILE - 1, 63), (TILE, 31), (2 * TILE + 1, 7), (n - 3, 12)]
    for f, j in injected:                                        # the neighbour's blob, one marker pitch away, for one frame
        t[f, j, 0] = 3.0
        near = f - 1 if f > 0 and t[f - 1, j, 0] == 3.0 else f + 1
        t[f, j, 6:9] = t[near, j, 6:9] + np.array([2.0, -2.0, 0.0], dtype=np.float32)
    tab = torch.from_numpy(t).cuda()
    clean, rep = despike_table(eng, tab, half_window=h, k_sigma=3.0, min_scale=0.05)
    want_out, _ = O.hampel_np(O.table_record(t), 3, h, 3.0, 0.05)
    spike = want_out[..., 0] == 7
    assert np.array_equal(rep["spike"].cpu().numpy(), spike) and all(spike[f, j] for f, j in injected)
    assert np.array_equal(rep["fill"].cpu().numpy(), want_out[..., 0] == 2) and rep["fill"].any()
    assert np.array_equal(O.bits(rep["median"].cpu().numpy()), O.bits(want_out[..., 2:5]))
    assert np.array_equal(O.bits(rep["mad"].cpu().numpy()), O.bits(want_out[..., 5:8]))
    assert np.array_equal(rep["per_marker"].cpu().numpy(), spike.sum(axis=0)) and np.array_equal(rep["per_frame"].cpu().numpy(), spike.sum(axis=1))
    assert rep["ref_spikes"].cpu().tolist() == np.nonzero(spike[0])[0].tolist() and 4 in rep["ref_spikes"].cpu().tolist()
    by_hand = t.copy()
    by_hand[spike, 0] = 1.0                                      # the same rows removed by hand: VBS_FLAG_XYZ cleared
    assert np.array_equal(clean.cpu().numpy().view(np.uint32), by_hand.view(np.uint32))
    taps = F.lowpass_taps(31, .08)
    a, b = polishing_analysis(eng, clean, taps), polishing_analysis(eng, torch.from_numpy(by_hand).cuda(), taps)
    for key in ("axis", "total", "total_filtered", "marker_filtered", "amplitude"):
        assert np.array_equal(O.bits(a[key].cpu().numpy()), O.bits(b[key].cpu().numpy())), key
    raw = polishing_analysis(eng, tab, taps)
    assert not np.array_equal(O.bits(a["total"].cpu().numpy()), O.bits(raw["total"].cpu().numpy()))
    df = to_spike_frame(rep, tab, path=tmp_path / "spikes.csv")
    assert len(df) == int(spike.sum()) and (tmp_path / "spikes.csv").exists()
    f0, j0 = injected[1]
    row = df[(df["frameno"] == f0) & (df["marker_id"] == j0 + 1)]
    assert len(row) == 1 and float(row["Xw"].iloc[0]) == float(t[f0, j0, 6]) and abs(float(row["Xw"].iloc[0]) - float(row["Xw_med"].iloc[0])) > 1.9
