"""CPU tests of the pose-misalignment series' host side (no GPU): the new C symbol and its constants, what is refused before a
device is touched, the sheet, and the NumPy restatement the GPU tests hold the device to bit for bit
(`tests/helpers/pose_oracle.py`) against sides that do not share its order or its algorithm: `np.linalg.lstsq` on the end points,
`math.fsum` means, and the project's own four-row oracle (`oracle.stages.deviation_plane`).  Bounds: see the helper."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from oracle import stages as S

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as FO                                    # noqa: E402
import pose_oracle as O                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbol_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    assert "vbs_pose_series" in declared and "vbs_pose_series" in L.SYMBOLS and hasattr(L.lib(), "vbs_pose_series")
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    assert (L.POSE_COLS, L.POSEFIELD_COLS, L.POSE_GROUP) == (defs["VBS_POSE_COLS"], defs["VBS_POSEFIELD_COLS"], defs["VBS_POSE_GROUP"])
    assert L.POSE_COLS == 8 and L.POSEFIELD_COLS == 6 and 1 <= L.POSE_GROUP <= 16
    assert L.POSE_COLS <= 8                                   # `pose` as [F, 1, 8] is a FIR record: cols <= 8, n_values 3 < cols
    fn = L.lib().vbs_pose_series
    assert len(fn.argtypes) == 17 and fn.argtypes[9] is C.c_double and fn.argtypes[10] is C.c_double


def test_refusals_without_a_gpu():
    """The C entry without a handle, and every argument check of `Engine.pose_series` (decided before a device is touched)."""
    from vbs_amd.engine import _pose_args
    p = C.c_void_p(8)
    assert L.lib().vbs_pose_series(None, p, 4, 3, 0, p, p, None, 0, 1.0, 0.0, 0, 4, p, p, p, None) == L.VBS_EINVAL
    good = dict(n=10, m=5, start_frame=0, mode="plane", scale=1.0, slots=None, reject_k=0.0, frame_range=None)
    assert _pose_args(**good) == (0, 10, 0)
    assert _pose_args(**dict(good, mode="shell", frame_range=(2, 7), slots=[0, 4], reject_k=3.0, start_frame=9)) == (2, 7, 1)
    assert _pose_args(**dict(good, frame_range=(4, 4))) == (4, 4, 0)
    for bad in (dict(start_frame=10), dict(start_frame=-1), dict(mode="dome"), dict(scale=math.inf), dict(scale=math.nan),
                dict(reject_k=-1.0), dict(reject_k=math.nan), dict(reject_k=math.inf), dict(frame_range=(3, 2)),
                dict(frame_range=(0, 11)), dict(frame_range=(-1, 4)), dict(slots=[5]), dict(slots=[-1])):
        with pytest.raises(ValueError):
            _pose_args(**dict(good, **bad))


def _case(m, tilt, az, seed, n=5, noise=0.01, drop=0.1):
    ref = O.grid_ref(m)
    t = O.tilted_table(ref, np.full(n, tilt), az, seed, noise, drop if m > 3 else 0.0)
    t_ref = O.tilted_table(ref, [0.0, 0.0], 0.0, seed + 1000, noise)
    rd = FO.axis_total(t_ref, 0, frame_range=(1, 2))[0][0]
    return ref, t, t_ref, rd


@pytest.mark.parametrize("m", (3, 65, 441))
def test_restatement_against_lstsq_and_fsum(m):
    """Planes of 0, 4 and 60 degrees at azimuths in all four quadrants (a < 0 and b < 0 among them), both modes and scales.
    Printed: the worst plane difference, which PLANE_TOL is 10 x of (a CPU trial: see the helper)."""
    worst, i = 0.0, 0
    for tilt in (0.0, 4.0, 60.0):
        for az in (0.0, 30.0, 135.0, -120.0, -45.0):
            shell, scale = bool(i % 2), (1.0, 25.0)[(i // 2) % 2]
            i += 1
            ref, t, _, rd = _case(m, tilt, az, 7 * i + m)
            dev, field, pose, rms2 = O.pose_series(t, rd, ref, 0, None, shell, scale)
            w = O.check_against_independent(dev, field, pose, ref, shell, scale, what=f"m {m} tilt {tilt} az {az}")
            worst = max(worst, w)
            have = pose[:, 0] != 0
            assert have[1:].all() or m == 3
            assert np.array_equal(pose[:, 6], np.sqrt(rms2)) and (pose[:, 7] == field[:, 1]).all()
            if scale == 1.0 and not shell and m > 3 and tilt > 0:       # the tilt and the steep direction come back
                assert np.abs(pose[1:, 4] - tilt).max() < 0.2
                want_az = az
                assert np.abs((pose[1:, 5] - want_az + 180.0) % 360.0 - 180.0).max() < (3.0 if tilt < 10 else 0.2)
                a_sign, b_sign = np.cos(np.radians(az)), np.sin(np.radians(az))
                assert (np.sign(pose[1:, 1]) == np.sign(round(a_sign, 9))).all() or abs(a_sign) < 1e-9
                assert (np.sign(pose[1:, 2]) == np.sign(round(b_sign, 9))).all() or abs(b_sign) < 1e-9
    print(f"m = {m}: worst |restatement - lstsq| / max(1, |a|, |b|, |c|) = {worst:.3e} (PLANE_TOL {O.PLANE_TOL:.1e})")
    assert worst <= O.PLANE_TOL


def test_restatement_rules_counts_flags_and_zeros():
    ref = O.grid_ref(70)
    t = O.tilted_table(ref, np.full(8, 4.0), 30.0, 3, 0.01)
    rng = np.random.default_rng(0)
    rd = np.zeros((70, 4))
    rd[:, 0] = 1.0
    rd[:, 1:] = rng.normal(0.0, 0.05, (70, 3))
    rd[5] = (0.0, np.nan, 1e30, np.nan)                       # dead in the reference state: never read
    dead = np.zeros((8, 70), dtype=bool)
    dead[0, 6] = True                                        # dead in start_frame
    dead[2, 7] = True                                        # a dropout
    dead[3, :] = True                                        # frames with 0, 1, 2 and 3 common slots
    dead[4, 1:] = True
    dead[5, 2:] = True
    dead[6, 3:] = True
    dead[4:7, 0] = False
    O.poison(t, dead, rng)
    dev, field, pose, _ = O.pose_series(t, rd, ref, 0)
    assert not np.isnan(dev).any() and not np.isnan(field).any() and not np.isnan(pose).any()
    assert field[:, 1].tolist() == [68, 68, 67, 0, 1, 2, 3, 68] and field[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    assert (dev[:, [5, 6]] == 0).all() and (dev[2, 7] == 0).all() and (dev[3] == 0).all()
    assert pose[:, 0].tolist() == [1, 1, 1, 0, 0, 0, 1, 1] and (pose[3:6, 1:7] == 0).all() and pose[3:6, 7].tolist() == [0, 1, 2]
    assert (field[3] == 0).all() and field[4, 5] > 0
    assert (dev[0, :, 1:] == -np.where(rd[:, :1] != 0, rd[:, 1:], 0.0) * dev[0, :, :1]).all()       # frame 0 against itself
    # a slot mask = the same table with the other slots' flags cleared
    mask = rng.random(70) < 0.6
    cleared = t.copy()
    cleared[:, ~mask, 0] = 0.0
    for x, y in zip(O.pose_series(t, rd, ref, 0, mask), O.pose_series(cleared, rd, ref, 0)):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    # collinear and coincident reference positions (integer data: exactly degenerate) give no plane and zeros
    line = np.stack([np.arange(70.0), 2.0 * np.arange(70.0), np.zeros(70)], axis=1)
    tz = np.zeros((3, 70, 10), dtype=np.float32)
    tz[..., 0] = 3.0
    tz[..., 8] = rng.integers(-3, 4, (3, 70))
    zero = np.zeros((70, 4))
    zero[:, 0] = 1.0
    for pts in (line, np.full((70, 3), 5.0)):
        _, f2, p2, _ = O.pose_series(tz, zero, pts, 0)
        assert (p2[:, :7] == 0).all() and (p2[:, 7] == 70).all() and (f2[:, 1] == 70).all()


def test_restatement_rejection():
    m = 65
    ref = O.grid_ref(m)
    t = O.tilted_table(ref, np.full(6, 4.0), -120.0, 11, 0.01)
    t[2, 17, 8] += np.float32(5.0)                            # one mistracked marker, 5 mm
    t[4, 40, 6] += np.float32(5.0)                            # in the plane's own X: far smaller in the residual, but still out
    zero = np.zeros((m, 4))
    zero[:, 0] = 1.0
    dev, field, p0, _ = O.pose_series(t, zero, ref, 0)
    _, _, p3, rms2 = O.pose_series(t, zero, ref, 0, reject_k=3.0)
    assert (p0[:, 0] == 1).all() and p3[:, 0].tolist() == [1, 1, 2, 1, 2, 1] and p3[2, 7] == p3[4, 7] == m - 1
    assert np.array_equal(p3[[0, 1, 3, 5]], p0[[0, 1, 3, 5]])       # no outlier: the first plane, bit for bit
    use = dev[..., 0] != 0
    use[2, 17] = False
    ind = O.independent(dev, ref, use=use)                   # the plane of the others
    assert np.abs(p3[2, 1:4] - ind[2, 1:4]).max() <= O.PLANE_TOL and abs(p3[2, 6] - ind[2, 4]) < 1e-9
    assert abs(p3[2, 4] - 4.0) < 0.1 < abs(p0[2, 4] - 4.0) and p3[2, 6] < 0.05 < p0[2, 6]
    # m = 4: with k = 3 nothing can lie outside (r^2 <= SSR < 9 SSR / 4); with a k so small that fewer than three are kept
    # the refit cannot stand and the first plane does
    t4 = O.tilted_table(O.grid_ref(4), np.full(3, 4.0), 30.0, 5, 0.05)
    z4 = zero[:4]
    a = O.pose_series(t4, z4, O.grid_ref(4), 0)[2]
    for k in (3.0, 0.05):
        b = O.pose_series(t4, z4, O.grid_ref(4), 0, reject_k=k)[2]
        assert np.array_equal(a, b) and (b[1:, 0] == 1).all() and (b[:, 7] == 4).all()


def test_restatement_against_the_four_row_oracle():
    """Frame f of the series = `deviation_plane` on (reference start, reference end, start, f)."""
    four = lambda row: np.column_stack([((row[:, 0].astype(int) & L.FLAG_XYZ) != 0).astype(float), row[:, 6:9].astype(np.float64)])  # noqa: E731
    for m, shell, scale in ((65, False, 1.0), (130, True, 5.0)):
        ref, t, t_ref, _ = _case(m, 4.0, 30.0, 40 + m, n=4)
        rng = np.random.default_rng(m)
        O.poison(t_ref, np.arange(m)[None, :] == np.array([[3], [9]]), rng)       # a slot dead in each reference row
        rd = FO.axis_total(t_ref, 0, frame_range=(1, 2))[0][0]
        dev, field, pose, _ = O.pose_series(t, rd, ref, 0, None, shell, scale)
        for f in (1, 3):
            common, want_dev, plane, mean_vec, mean_mag = S.deviation_plane(four(t_ref[0]), four(t_ref[1]), four(t[0]), four(t[f]),
                                                                            ref, "shell" if shell else "plane", scale)
            assert np.array_equal(dev[f, :, 0] != 0, common) and field[f, 1] == common.sum() and not common[[3, 9]].any()
            assert np.abs(dev[f, :, 1:] - want_dev).max() <= 4 * O.U2 * np.abs(t[..., 6:9][np.isfinite(t[..., 6:9])]).max()
            np.testing.assert_allclose(pose[f, 1:5], plane, rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(field[f, 2:5], mean_vec, rtol=1e-11, atol=1e-13)
            assert abs(field[f, 5] - mean_mag) <= 1e-12 * mean_mag


def test_trend_on_the_synthetic_ramp_and_the_bound_it_sets():
    """The ramp of the end-to-end GPU test, on the restatement: the filtered plane's tilt follows 0 -> 6 degrees.  Printed: the
    worst deviation, which TREND_TOL_DEG is 10 x of."""
    from vbs_amd import filters as F
    n, m, k_taps = 240, 65, 31
    ref = O.grid_ref(m)
    ramp = np.linspace(0.0, 6.0, n)
    t = O.tilted_table(ref, ramp, 30.0, 2, 0.02, 0.1)
    zero = np.zeros((m, 4))
    zero[:, 0] = 1.0
    pose = O.pose_series(t, zero, ref, 0)[2]
    half = F.half_taps(F.lowpass_taps(k_taps, .08))
    pf = FO.fir(pose[:, None, :], half, 3)[:, 0]
    assert (pf[:, 0] == 3).all()
    tilt_f = np.degrees(np.arctan(np.hypot(pf[:, 1], pf[:, 2])))
    mid = slice(k_taps, n - k_taps)
    worst = float(np.abs(tilt_f[mid] - ramp[mid]).max())
    print(f"worst |trend tilt - ramp| = {worst:.4f} deg (TREND_TOL_DEG {O.TREND_TOL_DEG})")
    assert worst <= O.TREND_TOL_DEG
    az_f = np.degrees(np.arctan2(pf[:, 2], pf[:, 1]))
    assert np.abs(az_f[n // 2:n - k_taps] - 30.0).max() < 1.0


def test_to_pose_frame_columns_nan_rules_and_round_trip(tmp_path):
    from vbs_amd import filters as F
    from vbs_amd.pipeline import POSE_FRAME_COLUMNS, POSE_TREND_COLUMNS, to_pose_frame
    from vbs_amd.xlsx_io import read_xlsx
    ref = O.grid_ref(9)
    t = O.tilted_table(ref, np.linspace(0.0, 6.0, 40), 30.0, 1, 0.01)
    rng = np.random.default_rng(1)
    dead = np.zeros((40, 9), dtype=bool)
    dead[7, 2:] = True                                       # two common slots: no plane, so a gap of the trend as well
    O.poison(t, dead, rng)
    zero = np.zeros((9, 4))
    zero[:, 0] = 1.0
    _, field, pose, _ = O.pose_series(t, zero, ref, 0)
    pf = FO.fir(pose[:, None, :], F.half_taps(F.moving_average_taps(9)), 3)[:, 0]
    df = to_pose_frame(field, pose, frame_offset=100)
    assert tuple(df.columns) == POSE_FRAME_COLUMNS == ("frameno", "count", "complete", "n_used", "flag", "a", "b", "c", "tilt_deg",
                                                       "azimuth_deg", "rms", "mean_dX", "mean_dY", "mean_dZ", "mean_mag")
    path = tmp_path / "pose_misalignment.xlsx"
    df = to_pose_frame(field, pose, pf, frame_offset=100, path=path)
    assert tuple(df.columns) == POSE_FRAME_COLUMNS + POSE_TREND_COLUMNS == POSE_FRAME_COLUMNS + ("a_f", "b_f", "c_f", "tilt_f", "azimuth_f")
    assert df["frameno"].tolist() == list(range(100, 140))
    for c in ("count", "complete", "n_used", "flag"):
        assert df[c].dtype == np.int64
    assert df["flag"][7] == 0 and df["count"][7] == 2 and df["n_used"][7] == 2 and df["complete"][7] == 0
    nan_cols = ["a", "b", "c", "tilt_deg", "azimuth_deg", "rms", "a_f", "b_f", "c_f", "tilt_f", "azimuth_f"]
    assert np.isnan(df.loc[7, nan_cols].to_numpy(dtype=np.float64)).all()
    assert not np.isnan(df.drop(index=7).to_numpy(dtype=np.float64)).any() and not np.isnan(df.loc[7, ["mean_dZ", "mean_mag"]].to_numpy(dtype=np.float64)).any()
    keep = np.arange(40) != 7
    assert np.array_equal(df["a"].to_numpy()[keep], pose[keep, 1]) and np.array_equal(df["rms"].to_numpy()[keep], pose[keep, 6])
    assert np.array_equal(df["b_f"].to_numpy()[keep], pf[keep, 2]) and np.array_equal(df["mean_mag"].to_numpy(), field[:, 5])
    assert np.allclose(df["tilt_f"].to_numpy()[keep], np.degrees(np.arctan(np.hypot(pf[keep, 1], pf[keep, 2]))), rtol=1e-14)
    back = read_xlsx(path)
    assert list(back.columns) == list(df.columns) and len(back) == len(df)
    for c in df.columns:
        assert np.array_equal(back[c].to_numpy(dtype=np.float64), df[c].to_numpy(dtype=np.float64), equal_nan=True), c
    for bad in ((field[:, :5], pose), (field, pose[:, :7]), (field, pose[:-1])):
        with pytest.raises(ValueError):
            to_pose_frame(*bad)
    with pytest.raises(ValueError):
        to_pose_frame(field, pose, pf[:, :6])
