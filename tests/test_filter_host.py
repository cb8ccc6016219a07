"""CPU tests of the dynamic-polishing analysis' host side (no GPU): the tap designs, the NumPy restatement the GPU tests hold the
device to bit for bit (`tests/helpers/filter_oracle.py`) against sides that do not share its order (`np.convolve`, `math.fsum`),
the coverage at the edges, the synthetic Figure-11 signal, and the new C symbols.  Bounds: see the helper."""
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import filters as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as O                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESIGNS = ((31, .08), (63, .05), (255, .02))


def _rec(n, s, cols, seed, gaps=0.0):
    rng = np.random.default_rng(seed)
    rec = rng.normal(0.0, 3.0, (n, s, cols))
    rec[..., 0] = (rng.random((n, s)) >= gaps).astype(np.float64)
    return rec


@pytest.mark.parametrize("n_taps,cutoff", DESIGNS + ((1, .3), (3, .5), (101, .25)))
def test_lowpass_taps_are_firwin(n_taps, cutoff):
    from scipy.signal import firwin
    w = F.lowpass_taps(n_taps, cutoff)
    assert w.shape == (n_taps,) and np.abs(w - firwin(n_taps, cutoff)).max() <= 1e-15
    assert np.array_equal(w, w[::-1]) and abs(w.sum() - 1.0) <= 1e-15 * n_taps


def test_tap_helpers_refuse_what_they_must():
    assert np.array_equal(F.moving_average_taps(5), np.full(5, 0.2))
    assert np.array_equal(F.half_taps([1.0, 2.0, 3.0, 2.0, 1.0]), [3.0, 2.0, 1.0])
    assert np.array_equal(F.half_taps([7.0]), [7.0])
    w = F.lowpass_taps(31, .08)
    assert np.array_equal(O.full_taps(F.half_taps(w)), w)
    bad = w.copy()
    bad[3] += 1e-9 * w.max()
    for wrong in (bad, [1.0, 2.0, 3.0], [1.0, 2.0], [], np.ones((3, 3)), [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError):
            F.half_taps(wrong)
    near = w.copy()
    near[3] += 1e-13 * w.max()                               # inside the tolerance: accepted, the pair's mean is used
    assert F.half_taps(near)[15 - 3] == 0.5 * (near[3] + near[27])
    for n in (0, 4, -3, 2.5):
        with pytest.raises(ValueError):
            F.lowpass_taps(n, .1)
        with pytest.raises(ValueError):
            F.moving_average_taps(n)
    for c in (0.0, 1.0, -.1):
        with pytest.raises(ValueError):
            F.lowpass_taps(5, c)


def test_scipy_firwin_is_not_bit_symmetric_which_is_why_only_the_half_travels():
    from scipy.signal import firwin
    assert any(not np.array_equal(w, w[::-1]) for w in (firwin(n, c) for n, c in DESIGNS))


@pytest.mark.parametrize("n_taps,cutoff", DESIGNS)
def test_restatement_against_np_convolve_same_on_gap_free_interiors(n_taps, cutoff):
    """The form the bound is stated for, and the ratio it leaves (printed: a CPU trial gave 0.04-0.08)."""
    w = F.lowpass_taps(n_taps, cutoff)
    half, h = F.half_taps(w), n_taps // 2
    rec = _rec(3 * n_taps + 7, 3, 3, n_taps)
    out = O.fir(rec, half, 2)
    sw = math.fsum(w.tolist())
    worst = 0.0
    for j in range(3):
        for c in range(2):
            x = rec[:, j, 1 + c]
            ref = np.convolve(x, w, "same") / sw
            bound = n_taps * O.U2 * np.convolve(np.abs(x), np.abs(w), "same") / abs(sw) + 2 * O.U2 * np.abs(ref)
            err = np.abs(out[:, j, 1 + c] - ref)[h:-h]
            assert (err <= bound[h:-h]).all()
            worst = max(worst, float((err / bound[h:-h]).max()))
    print(f"K = {n_taps}: worst |y - ref| / bound = {worst:.3f}")
    assert (out[..., 0] == 3).all()


@pytest.mark.parametrize("gaps", (0.0, 0.2))
def test_restatement_against_the_independent_check_with_gaps_and_junk(gaps):
    for n_taps, cutoff in DESIGNS + ((1, .3), (3, .5)):
        half = F.half_taps(F.lowpass_taps(n_taps, cutoff))
        rec = _rec(2 * n_taps + 9, 4, 5, 100 + n_taps, gaps)
        rec[:, 2, 0] = 0.0                                   # a series never seen
        a = max(0, n_taps // 2 - 1)
        rec[a:a + n_taps + 2, 1, 0] = 0.0                    # a gap longer than the filter
        rec[a + n_taps + 2, 1, 0] = 1.0
        junk = rec[..., 0] == 0
        rec[..., 1:][junk] = np.where(np.arange(int(junk.sum()) * 4).reshape(-1, 4) % 2 == 0, np.nan, 1e30)
        out = O.fir(rec, half, 3)
        O.check_fir(out, rec, half, 3, what=f"K {n_taps}")
        assert (out[:, 2] == 0).all()
        assert set(np.unique(out[..., 0]).tolist()) <= {0.0, 1.0, 3.0}
        if n_taps >= 31:                                     # next to the long gap: valid, but not covered to 90 %
            strict = O.fir(rec, half, 3, 0.9)
            O.check_fir(strict, rec, half, 3, 0.9, what=f"K {n_taps}, coverage 0.9")
            assert strict[a + n_taps + 2, 1, 0] == 1.0 and (strict[a + n_taps + 2, 1, 1:] == 0).all()


def test_k1_is_the_identity():
    rec = _rec(40, 3, 4, 5, 0.2)
    out = O.fir(rec, F.half_taps(F.lowpass_taps(1, .3)), 3)       # the tap is 1.0: (1.0 x) / 1.0 is x
    v = rec[..., 0] != 0
    assert np.array_equal(out[..., 1:4][v], rec[..., 1:4][v]) and (out[..., 4:] == 0).all() and (out[..., 0][v] == 3).all()


def test_totals_against_fsum_and_their_flags():
    rng = np.random.default_rng(3)
    for m in (1, 64, 65, 169):
        t = np.zeros((12, m, 10), dtype=np.float32)
        t[..., 0] = 3.0
        t[..., 6:9] = rng.normal(0.0, 50.0, (12, m, 3)).astype(np.float32)
        if m > 1:
            t[:, m - 1, 0] = 1.0                             # never a 3-D point: not in the reference frame, not expected
            t[5, 0, 0] = 1.0                                 # a dropout
        axis, total = O.axis_total(t, 2)
        O.check_axis_total(axis, total, t, 2)
        exp = m - (m > 1)
        assert (total[:, 4] == np.where((np.arange(12) == 5) & (m > 1), exp - 1, exp)).all()
        assert (total[:, 0] == ((np.arange(12) != 5) | (m == 1))).all()
        assert (axis[2, :, 1:] == 0).all()
        if m > 1:
            assert (axis[:, m - 1] == 0).all()
    t[:, :, 0] = 1.0
    assert (O.axis_total(t, 0)[1][:, 0] == 0).all()           # nothing valid in the reference frame: never complete


@pytest.mark.parametrize("n_taps,cutoff,floor", ((31, .08, 0.544), (63, .05, 0.525), (255, .02, 0.510)))
def test_every_frame_of_a_gap_free_series_passes_half_coverage(n_taps, cutoff, floor):
    half = F.half_taps(F.lowpass_taps(n_taps, cutoff))
    rec = _rec(2 * n_taps + 3, 1, 2, 1)
    assert (O.fir(rec, half, 1, 0.5)[..., 0] == 3).all()
    w = O.full_taps(half)
    cover = np.convolve(np.ones(rec.shape[0]), w)[n_taps // 2:n_taps // 2 + rec.shape[0]] / w.sum()
    print(f"K = {n_taps}: minimum coverage {cover.min():.3f}")
    assert abs(cover.min() - floor) < 2e-3
    assert (O.fir(rec, half, 1, 1.0)[[0, -1], 0, 0] == 1).all()     # and full coverage is refused at the ends


def test_figure_11_signal_trend_and_amplitude():
    n, ramp = 600, 200
    half = F.half_taps(F.lowpass_taps(31, .08))
    for seed in range(4):
        z = O.figure11_signal(n, ramp, seed)
        rec = np.stack([np.ones(n), z], axis=1)[:, None, :]
        out = O.fir(rec, half, 1)
        res = out[ramp + 31:n - 31, 0, 2]
        std = res.std(ddof=1)
        print(f"seed {seed}: residual std {std:.4f} against {O.OSC_MM / math.sqrt(2):.4f}")
        assert abs(std - O.OSC_MM / math.sqrt(2)) <= 0.03 * O.OSC_MM / math.sqrt(2)
        mid = slice(31, ramp - 31)                           # zero phase: the trend follows the ramp without lag
        want = O.RAMP_MM * np.arange(n)[mid] / ramp
        assert np.abs(out[mid, 0, 1] - want).max() < 4 * O.NOISE_MM
        assert np.abs(out[ramp + 31:n - 31, 0, 1] - O.RAMP_MM).max() < 4 * O.NOISE_MM


def test_to_total_frame_schema_and_xlsx_round_trip(tmp_path):
    from vbs_amd.pipeline import to_total_frame
    from vbs_amd.xlsx_io import read_xlsx
    t = O.figure11_table(80, 5, 20, 0)
    t[7, 2, 0] = 1.0
    _, total = O.axis_total(t, 0)
    half = F.half_taps(F.moving_average_taps(9))
    tf = O.fir(total[:, None, :], half, 3)[:, 0]
    path = tmp_path / "total_marker_displacement.xlsx"
    df = to_total_frame(total, tf, frame_offset=10, path=path)
    assert list(df.columns) == ["frameno", "count", "complete", "dX", "dY", "dZ", "dX_f", "dY_f", "dZ_f"]
    assert df["frameno"].tolist() == list(range(10, 90)) and df["count"].dtype == np.int64 and df["complete"].dtype == np.int64
    assert df["complete"][7] == 0 and df["count"][7] == 4 and np.isnan(df["dZ_f"][7]) and df["complete"].sum() == 79
    assert np.array_equal(df["dZ"].to_numpy(), total[:, 3]) and np.array_equal(df["dZ_f"].to_numpy()[8:], tf[8:, 3])
    back = read_xlsx(path)
    assert list(back.columns) == list(df.columns) and len(back) == len(df)
    for c in df.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64), equal_nan=True), c
    with pytest.raises(ValueError):
        to_total_frame(total[:, :4], tf)


def test_new_header_symbols_are_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in ("vbs_axis_displacement", "vbs_fir_series_f64"):
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.FIR_MAX_TAPS, L.FIR_TILE, L.AXIS_COLS, L.TOTAL_COLS) == (
        defs["VBS_FIR_MAX_TAPS"], defs["VBS_FIR_TILE"], defs["VBS_AXIS_COLS"], defs["VBS_TOTAL_COLS"])
    assert L.FIR_MAX_TAPS == 255 and L.AXIS_COLS == 4 and L.TOTAL_COLS == 5


def test_fir_entry_refuses_bad_arguments_before_touching_a_device():
    """Every VBS_EINVAL condition is decided on the host, ahead of hipSetDevice: checkable without a GPU (non-null dummies)."""
    import ctypes as C
    lib = L.lib()
    half = (C.c_double * 128)(*([1.0] * 128))
    p = C.c_void_p(8)

    def call(n=10, s=2, cols=4, nv=3, hp=half, n_half=3, mc=0.5, fb=0, fe=10, rec=p, out=p):
        return lib.vbs_fir_series_f64(0, rec, n, s, cols, nv, hp, n_half, mc, fb, fe, out, None)
    for kw in (dict(n_half=0), dict(n_half=129), dict(mc=0.0), dict(mc=1.5), dict(mc=float("nan")), dict(mc=-0.5),
               dict(fb=-1), dict(fe=11), dict(fb=6, fe=5), dict(cols=9), dict(cols=1, nv=1), dict(nv=4), dict(nv=0), dict(n=0, fe=0),
               dict(s=0), dict(rec=None), dict(out=None), dict(hp=None)):
        assert call(**kw) == L.VBS_EINVAL, kw
    neg = (C.c_double * 2)(1.0, -0.5)                        # sw = 0
    assert call(hp=neg, n_half=2) == L.VBS_EINVAL


def test_filters_module_does_not_import_scipy():
    src = open(os.path.join(ROOT, "vision-basedsensor_amd", "filters.py")).read()
    assert not re.search(r"^\s*(import|from)\s+scipy", src, re.M)
    import subprocess
    code = "import sys; import vbs_amd.filters as F; F.lowpass_taps(31, .08); assert 'scipy' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
