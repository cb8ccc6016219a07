"""GPU tests of the dynamic-polishing analysis (k_filter.hip; run on the MI355X box: `pytest -m gpu`): the gap-aware zero-phase
FIR, the signed displacement with its totals, and `pipeline.polishing_analysis`.

Every result is held BIT FOR BIT to the NumPy restatement (`tests/helpers/filter_oracle.py`: the same IEEE operations in the same
order) and, within the bounds of the summation error derived there, to sides that do not share its order (`np.convolve`,
`math.fsum`).  No entry is skipped or masked to get under a bound.  Shapes are the smallest at which the kernel can go wrong:
around the filter length and around the tile (VBS_FIR_TILE frames x 64 series), not the workload's.
"""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import filters as F                              # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as O                                     # noqa: E402

TILE = L.FIR_TILE
DESIGN = {1: .3, 3: .5, 31: .08, 255: .02}
COLS = ((2, 1), (4, 3), (5, 3), (8, 7))                       # (cols, n_values): a bare series, `axis`, `total`, the widest
GAPS = ("none", "random", "long", "dead series", "random and dead")


def engine(h=480, w=640, **kw):
    from vbs_amd.engine import Engine
    kw.setdefault("max_markers", 256)
    kw.setdefault("max_batch", 2)
    return Engine(h, w, **kw)


def fir_dev(rec, taps, nv, mc=0.5, frame_range=None):
    from vbs_amd.engine import fir_series_f64
    return fir_series_f64(torch.from_numpy(rec).cuda(), taps, nv, mc, frame_range).cpu().numpy()


def make_rec(rng, n, s, cols, kind, k_taps):
    """[n, s, cols] float64 with the gaps of `kind`; NaN and 1e30 in EVERY invalid entry (and in the columns past the values)."""
    rec = rng.normal(0.0, 3.0, (n, s, cols)) + 10.0 * rng.standard_normal((1, s, 1))
    valid = np.ones((n, s), dtype=bool)
    if "random" in kind:
        valid &= rng.random((n, s)) >= 0.2
    if kind == "long" and n > 2:
        a = min(n // 3, max(0, n - k_taps - 3))
        valid[a:a + k_taps + 2, s // 2] = False
        if a + k_taps + 2 < n:
            valid[a + k_taps + 2, s // 2] = True
    if "dead" in kind:
        valid[:, s - 1] = False
    rec[..., 0] = np.where(valid, rng.choice([1.0, 2.0, -1.0, 1e-300], (n, s)), 0.0)       # any nonzero flag is valid
    junk = np.where(rng.random((n, s, cols - 1)) < 0.5, np.nan, 1e30)
    rec[..., 1:] = np.where(valid[..., None], rec[..., 1:], junk)
    return rec


@pytest.mark.parametrize("k_taps", sorted(DESIGN))
def test_fir_equals_the_restatement_on_every_edge_shape(k_taps):
    """n around the filter length and around the tile, s around the wave: every (n, s) pair, the cols / n_values and the kinds
    of gap rotating through them (4 and 5 are coprime: every combination of the two is met)."""
    rng = np.random.default_rng(k_taps)
    taps = F.lowpass_taps(k_taps, DESIGN[k_taps])
    half = F.half_taps(taps)
    ns = sorted({1, 2, max(1, k_taps - 1), k_taps, TILE - 1, TILE, TILE + 1, 3 * TILE + 5})
    i, worst, seen = 0, 0.0, set()
    for n in ns:
        for s in (1, 63, 64, 65, 130):
            (cols, nv), kind = COLS[i % 4], GAPS[i % 5]
            i += 1
            rec = make_rec(rng, n, s, cols, kind, k_taps)
            got = fir_dev(rec, taps, nv)
            worst = max(worst, O.check_fir(got, rec, half, nv, what=f"K {k_taps} n {n} s {s} cols {cols} {kind}"))
            seen |= set(np.unique(got[..., 0]).tolist())
            if "dead" in kind:
                assert (got[:, s - 1] == 0).all()
            if k_taps == 1:                                  # the identity: (1.0 x) / 1.0
                v = rec[..., 0] != 0
                assert np.array_equal(got[..., 1:1 + nv][v], rec[..., 1:1 + nv][v]) and (got[..., 1 + nv:] == 0).all()
                assert np.array_equal(got[..., 0], 3.0 * v)
    print(f"K = {k_taps}: {i} shapes, worst |y - convolve| / bound = {worst:.3f}, flags seen {sorted(seen)}")
    assert seen >= {0.0, 3.0}


def test_fir_flag_is_1_where_a_valid_frame_lacks_coverage():
    rng = np.random.default_rng(7)
    taps = F.lowpass_taps(31, .08)
    rec = make_rec(rng, 3 * TILE + 5, 65, 4, "long", 31)
    a = (3 * TILE + 5) // 3
    for mc in (0.5, 0.9, 1.0):
        got = fir_dev(rec, taps, 3, mc)
        O.check_fir(got, rec, F.half_taps(taps), 3, mc, what=f"coverage {mc}")
        if mc > 0.5:
            assert got[a + 33, 32, 0] == 1.0 and got[a - 1, 32, 0] == 1.0 and (got[a + 33, 32, 1:] == 0).all()
            assert got[0, 0, 0] == 1.0 and got[TILE, 0, 0] == 3.0
    assert (got[a:a + 33, 32] == 0).all()


def test_fir_ranges_runs_and_series_do_not_change_a_bit():
    rng = np.random.default_rng(11)
    n, s = 3 * TILE + 5, 130
    for k_taps in (31, 255):
        taps = F.lowpass_taps(k_taps, DESIGN[k_taps])
        rec = make_rec(rng, n, s, 4, "random", k_taps)
        full = fir_dev(rec, taps, 3)
        assert np.array_equal(full.view(np.uint64), fir_dev(rec, taps, 3).view(np.uint64))           # two runs
        cuts = (0, 37, TILE + 1, n)
        parts = [fir_dev(rec, taps, 3, frame_range=(cuts[j], cuts[j + 1])) for j in range(3)]
        assert [p.shape[0] for p in parts] == [37, TILE + 1 - 37, n - TILE - 1]
        assert np.array_equal(np.concatenate(parts).view(np.uint64), full.view(np.uint64))           # three ranges
        assert fir_dev(rec, taps, 3, frame_range=(5, 5)).shape == (0, s, 7)
        for j in (0, 63, 64, 65, 129):                                                                # a series alone
            alone = fir_dev(np.ascontiguousarray(rec[:, j:j + 1]), taps, 3)
            assert np.array_equal(alone[:, 0].view(np.uint64), full[:, j].view(np.uint64)), j


def test_fir_refuses_bad_arguments():
    from vbs_amd.engine import fir_series_f64
    rec = torch.ones((10, 2, 4), dtype=torch.float64, device="cuda")
    ok = F.moving_average_taps(5)
    assert fir_series_f64(rec, ok).shape == (10, 2, 7) and fir_series_f64(rec, np.ones(255)).shape == (10, 2, 7)
    for kw in (dict(taps=np.ones(257)), dict(taps=[1.0, 2.0, 3.0]), dict(taps=np.ones(4)), dict(taps=[-1.0, 1.0, -1.0]),
               dict(taps=[-1.0, 2.0, -1.0]), dict(min_coverage=0.0), dict(min_coverage=1.5), dict(min_coverage=-1.0),
               dict(n_values=4), dict(n_values=0), dict(frame_range=(3, 2)), dict(frame_range=(0, 11)), dict(frame_range=(-1, 4)),
               dict(rec=torch.ones((10, 2, 9), dtype=torch.float64, device="cuda")),
               dict(rec=torch.ones((10, 2, 1), dtype=torch.float64, device="cuda")),
               dict(rec=torch.ones((10, 8), dtype=torch.float64, device="cuda"))):
        args = dict(rec=rec, taps=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            fir_series_f64(**args)


# ---------------------------------------------------------------------------------------------------------------------
def random_table(rng, n, m):
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = rng.choice([0.0, 1.0, 3.0, 3.0, 3.0, 3.0], (n, m))
    t[..., 6:9] = (rng.normal(0.0, 40.0, (1, m, 3)) + rng.normal(0.0, 2.0, (n, m, 3))).astype(np.float32)
    t[..., 6:9][t[..., 0] != 3.0] = np.float32(1e30)         # what is no 3-D point must not be read
    return t


@pytest.mark.parametrize("m", (1, 64, 65, 169))
def test_axis_and_total_equal_the_restatement(m):
    eng = engine()
    rng = np.random.default_rng(m)
    n, ref = 9, 2
    t = random_table(rng, n, m)
    t[ref, :, 0] = 3.0
    t[ref, :, 6:9] = rng.normal(0.0, 40.0, (m, 3)).astype(np.float32)
    t[4, :, 0] = 3.0
    t[4, :, 6:9] = rng.normal(0.0, 40.0, (m, 3)).astype(np.float32)      # a frame where everything is seen ...
    t[5] = t[4]
    if m > 1:
        t[ref, m - 1, 0] = 1.0                               # a slot without a 3-D point in the reference frame
        t[5, 0, 0] = 1.0                                     # ... and the same frame with one dropout
    dev = torch.from_numpy(t).cuda()
    axis, total = (x.cpu().numpy() for x in eng.axis_displacement(dev, ref))
    O.check_axis_total(axis, total, t, ref, what=f"m {m}")
    exp = m - (m > 1)
    assert total[4, 0] == 1.0 and total[4, 4] == exp and total[ref, 0] == 1.0 and (total[ref, 1:4] == 0).all()
    if m > 1:
        assert (axis[:, m - 1] == 0).all()                   # flag 0 everywhere, and `complete` does not wait for it
        assert total[5, 0] == 0.0 and total[5, 4] == exp - 1
    # the range form, in pieces
    parts = [eng.axis_displacement(dev, ref, frame_range=r) for r in ((0, 3), (3, 4), (4, n))]
    assert np.array_equal(np.concatenate([p[0].cpu().numpy() for p in parts]).view(np.uint64), axis.view(np.uint64))
    assert np.array_equal(np.concatenate([p[1].cpu().numpy() for p in parts]).view(np.uint64), total.view(np.uint64))
    assert eng.axis_displacement(dev, ref, frame_range=(4, 4))[1].shape == (0, 5)
    # a selection of slots = the same table with the other slots' flags cleared
    slots = np.nonzero(rng.random(m) < 0.6)[0] if m > 1 else np.array([0])
    mask = np.zeros(m, dtype=bool)
    mask[slots] = True
    cleared = t.copy()
    cleared[:, ~mask, 0] = 0.0
    a_s, t_s = (x.cpu().numpy() for x in eng.axis_displacement(dev, ref, slots=slots))
    a_c, t_c = (x.cpu().numpy() for x in eng.axis_displacement(torch.from_numpy(cleared).cuda(), ref))
    assert np.array_equal(a_s.view(np.uint64), a_c.view(np.uint64)) and np.array_equal(t_s.view(np.uint64), t_c.view(np.uint64))
    O.check_axis_total(a_s, t_s, t, ref, mask, what=f"m {m}, selected")
    for bad in (dict(ref_frame=n), dict(ref_frame=-1), dict(frame_range=(2, 1)), dict(frame_range=(0, n + 1)), dict(slots=[m])):
        with pytest.raises(ValueError):
            eng.axis_displacement(dev, **bad)
    buf = torch.empty((n, 5), dtype=torch.float64, device="cuda")
    call = eng.lib.vbs_axis_displacement
    assert call(eng._h, dev.data_ptr(), n, m, n, None, 0, n, None, buf.data_ptr(), None) == L.VBS_EINVAL       # ref_frame
    assert call(eng._h, dev.data_ptr(), n, m, 0, None, 0, n, None, None, None) == L.VBS_EINVAL                 # nothing to write
    assert call(eng._h, dev.data_ptr(), n, m, 0, None, 0, n, None, buf.data_ptr(), None) == L.VBS_OK           # total alone
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), O.axis_total(t, 0)[1].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
def test_polishing_analysis_on_the_figure_11_signal(tmp_path):
    from vbs_amd.engine import fir_series_f64, series_stats_f64
    from vbs_amd.pipeline import polishing_analysis, to_total_frame
    from vbs_amd.xlsx_io import read_xlsx
    eng = engine()
    n, m, ramp, k_taps = 300, 65, 100, 31
    taps = F.lowpass_taps(k_taps, .08)
    half = F.half_taps(taps)
    t = O.figure11_table(n, m, ramp, 0)
    res = polishing_analysis(eng, torch.from_numpy(t).cuda(), taps)
    axis, total, tf, mf, amp = (res[k].cpu().numpy() for k in ("axis", "total", "total_filtered", "marker_filtered", "amplitude"))
    O.check_axis_total(axis, total, t, 0, what="figure 11")
    O.check_fir(mf, axis, half, 3, what="figure 11, per marker")
    O.check_fir(tf[:, None, :], total[:, None, :], half, 3, what="figure 11, total")
    direct = fir_series_f64(res["total"][:, None, :], taps, 3)[:, 0].cpu().numpy()
    assert np.array_equal(tf.view(np.uint64), direct.view(np.uint64))
    # amplitude = series_stats_f64 of the residuals packed into the disp layout
    packed = np.zeros((n, m, 5))
    packed[..., 0] = mf[..., 0] == 3.0
    for a in range(3):
        packed[..., 4] = mf[..., 4 + a]
        st = series_stats_f64(packed).cpu().numpy()
        packed[..., 4] = np.abs(mf[..., 4 + a])
        mx = series_stats_f64(packed).cpu().numpy()
        want = np.stack([st[:, 0], st[:, 2], mx[:, 3]], axis=1)
        assert np.array_equal(amp[:, a].view(np.uint64), want.view(np.uint64)), a
    assert (amp[:, :, 0] == n).all()
    # what the figure shows: the trend follows the ramp, the amplitude left is the oscillation's (per marker, scaled as rendered)
    zstd = mf[ramp + k_taps:n - k_taps, :, 6].std(axis=0, ddof=1)
    gain = 1.0 - 0.3 * np.arange(m) / m
    assert (np.abs(zstd / gain - O.OSC_MM / np.sqrt(2)) <= 0.05 * O.OSC_MM / np.sqrt(2)).all()
    assert np.abs(tf[ramp + k_taps:n - k_taps, 3] - O.RAMP_MM * gain.sum()).max() < 2.0    # (65 slots' noise in frame 0)
    # no gaps: by linearity the trend of the total is the sum of the markers' trends, within the summation error of both sides
    # (2 K for the two filter sums, m for the rounding of the total the filter was given, 4 for the divisions; see the helper)
    assert (total[:, 0] == 1).all() and (mf[..., 0] == 3).all()
    w = np.abs(O.full_taps(half))
    h = k_taps // 2
    for c in range(3):
        slot_sum = np.array([math.fsum(mf[f, :, 1 + c].tolist()) for f in range(n)])
        mass = np.convolve(np.abs(axis[..., 1 + c]).sum(axis=1), w)[h:h + n]
        den = np.convolve(np.ones(n), O.full_taps(half))[h:h + n]
        bound = (2 * k_taps + m + 4) * O.U2 * mass / np.abs(den)
        assert (np.abs(tf[:, 1 + c] - slot_sum) <= bound).all(), c
    # the sheet
    path = tmp_path / "total_marker_displacement.xlsx"
    df = to_total_frame(res["total"], res["total_filtered"], path=path)
    back = read_xlsx(path)
    assert list(back.columns) == ["frameno", "count", "complete", "dX", "dY", "dZ", "dX_f", "dY_f", "dZ_f"] and len(back) == n
    for col in df.columns:
        assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64), equal_nan=True), col
    assert np.array_equal(df["dZ_f"].to_numpy(), tf[:, 3]) and (df["count"] == m).all()
