"""CPU tests of the despiking entry's host side (no GPU): the header against the binding, every refusal of the C entry and of
`engine._robust_args`, the restatement the GPU tests hold the device to bit for bit (`tests/helpers/robust_oracle.py`) against
`np.median`, its two forms against each other, what the Hampel rule detects on a synthetic series, and `despike_table`'s flag
arithmetic with the device call replaced by the restatement."""
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd.engine import _robust_args

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import robust_oracle as O                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rec(n, s, cols, seed, gaps=0.0, scale=3.0):
    rng = np.random.default_rng(seed)
    rec = rng.normal(0.0, scale, (n, s, cols))
    rec[..., 0] = (rng.random((n, s)) >= gaps).astype(np.float64)
    return rec


def test_header_defines_are_bound_and_the_entry_is_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    name = "vbs_hampel_series_f64"
    assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.ROBUST_MAX_HALF, L.ROBUST_TILE) == (defs["VBS_ROBUST_MAX_HALF"], defs["VBS_ROBUST_TILE"])
    assert L.ROBUST_MAX_HALF == 31 and L.ROBUST_TILE >= 1
    import vbs_amd._build as B
    assert "k_robust.hip" in B.SOURCES


BAD = (dict(h=-1), dict(h=32), dict(mc=0), dict(mc=8), dict(h=0, mc=2), dict(k=0.0), dict(k=-1.0), dict(k=float("nan")),
       dict(k=float("inf")), dict(ms=-1e-300), dict(ms=float("nan")), dict(ms=float("inf")), dict(fb=-1), dict(fe=11),
       dict(fb=6, fe=5), dict(cols=9), dict(cols=1, nv=1), dict(nv=4), dict(nv=0), dict(n=0, fe=0), dict(s=0))


def test_the_entry_refuses_bad_arguments_before_touching_a_device():
    """Every VBS_EINVAL condition is decided on the host, ahead of hipSetDevice: checkable without a GPU (non-null dummies)."""
    import ctypes as C
    lib = L.lib()
    p = C.c_void_p(8)

    def call(n=10, s=2, cols=4, nv=3, h=3, mc=4, k=3.0, ms=0.0, fb=0, fe=10, rec=p, out=p, clean=p):
        return lib.vbs_hampel_series_f64(0, rec, n, s, cols, nv, h, mc, k, ms, fb, fe, out, clean, None)
    for kw in BAD + (dict(rec=None), dict(out=None)):
        assert call(**kw) == L.VBS_EINVAL, kw
    assert call(rec=None, clean=None) == L.VBS_EINVAL            # a null `clean` alone is no error; with a null rec it still is


def test_robust_args_refuses_the_same_and_sets_the_defaults():
    def args(n=10, s=2, cols=4, nv=3, h=3, mc=4, k=3.0, ms=0.0, fb=0, fe=10):
        return _robust_args(n, s, cols, h, k, ms, mc, nv, (fb, fe))
    assert args() == (0, 10, 3, 3, 4)
    for kw in BAD + (dict(h=2.5), dict(mc=2.5)):
        with pytest.raises(ValueError):
            args(**kw)
    assert _robust_args(10, 2, 4, 7, 3.0, 0.0, None, None, None) == (0, 10, 3, 7, 8)           # min_count h + 1, cols - 1, all
    assert _robust_args(10, 2, 8, 0, 1e-3, 5.0, None, 7, (5, 5)) == (5, 5, 7, 0, 1)
    assert _robust_args(1, 1, 2, 31, 3.0, 0.0, 63, None, None) == (0, 1, 1, 31, 63)
    with pytest.raises(ValueError, match=str(L.ROBUST_MAX_HALF)):
        args(h=32)


@pytest.mark.parametrize("h,gaps", ((1, 0.0), (3, 0.0), (3, 0.3), (7, 0.2), (31, 0.1)))
def test_restated_median_is_np_median_of_every_window(h, gaps):
    """Finite values far below 1e150: halving is exact and 0.5 a + 0.5 b is the rounded (a + b) / 2 `np.median` forms.  The ends
    of the recording and the gaps give odd and even counts."""
    rec = _rec(2 * h + 40, 3, 3, 10 + h, gaps, scale=1e6)
    n = rec.shape[0]
    out, _ = O.hampel(rec, 2, h, min_count=1)
    parity = set()
    for i in range(3):
        for f in range(n):
            g = np.arange(max(0, f - h), min(n, f + h + 1))
            g = g[rec[g, i, 0] != 0]
            assert out[f, i, 1] == g.size
            parity.add(g.size & 1)
            for v in range(2):
                if g.size:
                    assert out[f, i, 2 + v] == np.median(rec[g, i, 1 + v]), (f, i, v)
                    assert out[f, i, 4 + v] == np.median(np.abs(rec[g, i, 1 + v] - out[f, i, 2 + v])), (f, i, v)
                else:
                    assert out[f, i, 0] == 0.0 and (out[f, i, 2:] == 0).all()
    assert parity == {0, 1}


def _tie_rec(n, s, cols, seed, gaps):
    rng = np.random.default_rng(seed)
    rec = rng.choice([-1.0, -0.0, 0.0, 1.0], (n, s, cols))
    valid = rng.random((n, s)) >= gaps
    rec[..., 0] = np.where(valid, rng.choice([1.0, 2.0, -1.0, 1e-300], (n, s)), 0.0)
    rec[..., 1:] = np.where(valid[..., None], rec[..., 1:], np.where(rng.random((n, s, cols - 1)) < 0.5, np.nan, 1e30))
    return rec


@pytest.mark.parametrize("h", (0, 1, 4, 31))
def test_the_two_forms_of_the_restatement_agree_in_bits(h):
    """`hampel` (loops, `sorted` on (x, g) pairs) and `hampel_np` (one stable sort) on noise with gaps, on values drawn from
    {-1, -0.0, 0.0, 1} where almost everything ties and the sign of a zero median depends on the order, and on a range."""
    n = 2 * h + 9
    for rec, nv in ((_rec(n, 4, 5, h, 0.25), 3), (_tie_rec(n, 5, 4, h, 0.2), 3), (_tie_rec(n, 3, 3, h + 1, 0.0), 2)):
        rec[:, -1, 0] = 0.0                                       # a dead series
        for mc in (1, h + 1, 2 * h + 1):
            for kw in (dict(), dict(min_scale=0.5, k_sigma=1.0), dict(frame_range=(3, n - 2))):
                a, b = O.hampel(rec, nv, h, min_count=mc, **kw), O.hampel_np(rec, nv, h, min_count=mc, **kw)
                assert np.array_equal(O.bits(a[0]), O.bits(b[0])) and np.array_equal(O.bits(a[1]), O.bits(b[1])), (h, mc, kw)
    zeros = np.signbit(O.hampel(_tie_rec(40, 8, 2, 5, 0.0), 1, 2)[0][..., 2])
    assert zeros.any() and not zeros.all()                       # medians of both signs of zero (and -1) were produced


def test_h0_returns_the_input():
    rec = _rec(30, 3, 4, 1, 0.2)
    out, clean = O.hampel(rec, 3, 0, k_sigma=1e-6)
    v = rec[..., 0] != 0
    assert np.array_equal(O.bits(out[..., 2:5][v]), O.bits(rec[..., 1:4][v])) and (out[..., 5:] == 0).all()
    assert np.array_equal(out[..., 0], 3.0 * v) and np.array_equal(out[..., 1], 1.0 * v) and (out[..., 2:][~v] == 0).all()
    assert np.array_equal(O.bits(clean), O.bits(rec))


def test_a_constant_series_has_no_spike_and_one_sample_off_is_exactly_one():
    rec = np.ones((50, 1, 2))
    rec[..., 1] = 0.3
    out, clean = O.hampel(rec, 1, 7, min_scale=0.0)
    assert (out[..., 0] == 3).all() and (out[..., 3] == 0).all() and np.array_equal(clean, rec)
    rec[20, 0, 1] = 0.3 + 1e-9
    out, clean = O.hampel(rec, 1, 7, min_scale=0.0)               # mad = 0: anything off the median is a spike without a floor
    assert np.argwhere(out[..., 0] == 7).tolist() == [[20, 0]] and (out[..., 0] >= 3).all()
    assert clean[20, 0, 0] == 0.0 and clean[..., 0].sum() == 49 and np.array_equal(clean[..., 1], rec[..., 1])
    assert (O.hampel(rec, 1, 7, min_scale=1e-8)[0][..., 0] == 3).all()       # ... and the floor is what says it is not one


def test_detection_on_a_sinusoid_with_noise_gaps_and_injected_spikes():
    """Every injected spike (>= 10 noise amplitudes) is flagged at h = 7, k = 3.  The rule tells a glitch from motion only where
    the motion across a window is small against the noise: the sinusoid (amplitude 1, period 2000 frames) moves by at most
    2 pi 7 / 2000 = 0.022 across a half window, one noise amplitude (0.02), so the MAD stays the noise's (about 0.67 sigma, the
    threshold about 3 to 4.5 sigma) and 10 sigma is far outside it even with a second spike in the window."""
    rng = np.random.default_rng(2024)
    n, sigma = 3000, 0.02
    t = np.arange(n)
    x = np.sin(2 * np.pi * t / 2000.0) + rng.normal(0.0, sigma, n)
    valid = rng.random(n) >= 0.03
    inject = valid & (rng.random(n) < 0.02)
    x[inject] += rng.choice([-1.0, 1.0], int(inject.sum())) * rng.uniform(10.0, 30.0, int(inject.sum())) * sigma
    rec = np.stack([valid.astype(np.float64), np.where(valid, x, np.nan)], axis=1)[:, None, :]
    out, clean = O.hampel(rec, 1, 7, 3.0, 0.0)
    spike = out[:, 0, 0] == 7
    print(f"{int(inject.sum())} injected, {int(spike.sum())} flagged, {int((spike & ~inject).sum())} others")
    assert inject.sum() >= 40 and spike[inject].all()
    # The number of OTHER flagged samples: Gaussian noise passes 3 scaled MADs of 15 samples now and then (33 of 2840 here).  It
    # is the count this restatement gave on the CPU with this seed - a recorded result that pins the rule, not a target.
    assert int((spike & ~inject).sum()) == 33
    assert np.array_equal(clean[:, 0, 0] != 0, valid & ~spike)



def test_despike_table_flag_arithmetic(monkeypatch):
    """A hand-built table through `pipeline.despike_table` with the device call replaced by the restatement."""
    torch = pytest.importorskip("torch")
    import vbs_amd.engine as E
    from vbs_amd.pipeline import despike_table, to_spike_frame
    calls = []

    def fake(rec, half_window, k_sigma=3.0, min_scale=0.0, min_count=None, n_values=None, frame_range=None, want_clean=True,
             device=None):
        r = rec.cpu().numpy()
        calls.append((r.copy(), half_window, k_sigma, min_scale, want_clean))
        out, clean = O.hampel(r, r.shape[2] - 1, half_window, k_sigma, min_scale, min_count, frame_range)
        return torch.from_numpy(out), (torch.from_numpy(clean) if want_clean else None)
    monkeypatch.setattr(E, "hampel_series_f64", fake)

    class Eng:
        device = torch.device("cpu")
    n, m = 12, 4
    t = np.zeros((n, m, 10), dtype=np.float32)
    t[..., 0] = 3.0 + 8.0                                        # a bit of someone else's beside the two of the table
    t[..., 1:3] = np.array([100.0, 200.0], dtype=np.float32) + 10 * np.arange(m, dtype=np.float32)[None, :, None]
    t[..., 6:9] = np.arange(m, dtype=np.float32)[None, :, None]
    t[..., 9] = 7.0
    t[0, 1, 8] += 5.0                                            # a jump in Z of slot 1 in frame 0, the reference frame
    t[6, 2, 1] += 30.0                                           # a jump in Cx of slot 2, which its X does not show
    t[6, 2, 6] += 1e-4                                           # ... but for less than the floor
    t[4, 3, 0] = 1.0 + 8.0                                       # slot 3 has no 3-D point in frame 4
    t[4, 3, 6:9] = 1e30
    t[5, 0, 0] = 8.0                                             # slot 0 is not tracked in frame 5
    t[5, 0, 1:9] = np.nan
    tab = torch.from_numpy(t)

    clean, rep = despike_table(Eng(), tab, half_window=2, min_scale=0.01)
    rec = calls[-1][0]
    assert calls[-1][1:] == (2, 3.0, 0.01, False) and np.array_equal(O.bits(rec), O.bits(O.table_record(t, "xyz")))
    spike = np.zeros((n, m), bool)
    spike[0, 1] = True
    assert np.array_equal(rep["spike"].numpy(), spike)
    want = t.copy()
    want[0, 1, 0] = 1.0 + 8.0                                    # VBS_FLAG_XYZ cleared, every other bit and column as it was
    assert np.array_equal(clean.numpy().view(np.uint32), want.view(np.uint32)) and clean is not tab
    assert np.array_equal(tab.numpy().view(np.uint32), t.view(np.uint32))            # the input is not written
    assert rep["ref_spikes"].tolist() == [1] and rep["per_marker"].tolist() == [0, 1, 0, 0] and rep["per_frame"].tolist()[0] == 1
    fill = np.zeros((n, m), bool)
    fill[4, 3] = fill[5, 0] = True
    assert np.array_equal(rep["fill"].numpy(), fill) and rep["median"][4, 3].tolist() == [3.0, 3.0, 3.0]
    assert rep["median"].shape == (n, m, 3) and rep["mad"].shape == (n, m, 3)
    df = to_spike_frame(rep, tab, frame_offset=100)
    assert list(df.columns) == ["frameno", "marker_id", "Xw", "Yw", "Zw", "Xw_med", "Yw_med", "Zw_med", "Xw_mad", "Yw_mad", "Zw_mad"]
    assert len(df) == 1 and df["frameno"][0] == 100 and df["marker_id"][0] == 2 and df["Zw"][0] == 6.0 and df["Zw_med"][0] == 1.0

    clean, rep = despike_table(Eng(), tab, half_window=2, min_scale=1.0, source="pixel")
    assert np.array_equal(O.bits(calls[-1][0]), O.bits(O.table_record(t, "pixel")))
    spike = np.zeros((n, m), bool)
    spike[6, 2] = True
    assert np.array_equal(rep["spike"].numpy(), spike) and rep["ref_spikes"].numel() == 0
    want = t.copy()
    want[6, 2, 0] = 8.0                                          # both bits cleared: the 3-D row derives from the 2-D one
    assert np.array_equal(clean.numpy().view(np.uint32), want.view(np.uint32))
    assert rep["fill"].numpy().sum() == 1 and rep["fill"][5, 0] and rep["median"].shape == (n, m, 2)
    df = to_spike_frame(rep, tab, path=None)
    assert list(df.columns) == ["frameno", "marker_id", "Cx", "Cy", "Cx_med", "Cy_med", "Cx_mad", "Cy_mad"] and len(df) == 1
    assert df["Cx"][0] == 150.0 and df["Cx_med"][0] == 120.0

    _, rep = despike_table(Eng(), tab, half_window=2, min_scale=0.01, slots=[0, 2, 3])          # slot 1 is not looked at
    assert not rep["spike"].any() and np.array_equal(O.bits(calls[-1][0]), O.bits(O.table_record(t, "xyz", [0, 2, 3])))
    with pytest.raises(TypeError):
        despike_table(Eng(), tab)                                # min_scale has no default
    for bad in (dict(source="uv"), dict(slots=[m])):
        with pytest.raises(ValueError):
            despike_table(Eng(), tab, min_scale=0.01, **bad)
    with pytest.raises(ValueError):
        despike_table(Eng(), tab[..., :9], min_scale=0.01)
