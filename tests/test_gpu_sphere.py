"""GPU tests of the bonnet contact geometry (`vbs_sphere_series`) against the NumPy restatement
`tests/helpers/sphere_oracle.py`: `sphere`, `radial` and `decomp` bit for bit, +0 and -0 told apart, but the five columns that pass
through a root or an arc tangent last (4 ulp), nothing masked, in BOTH modes (the sphere fitted per frame, the sphere given).  Shapes
are the smallest at which the kernel can go wrong - around the four slots a sphere needs and the three a plane needs, around one and
two lane strides (64 slots), the workload's 441, around the frames a workgroup takes (VBS_SPHERE_GROUP) - the tables hold rows
without a 3-D point, a frame with every slot missing next to full ones, a fit mask and a slot mask that differ, source slots with
flag 0, planted slots for the rejection, contact sets of 0, 1, 2, 3, 3 collinear and many slots, and NaN / 1e30 / 1e300 in every
cell that must not be read.  Every case's decisions have a margin (`sphere_cases.with_margins`), so the restatement alone decides."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import vbs_amd._lib as L                                       # noqa: E402
from vbs_amd import engine as E                                # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import field_oracle as FO                                      # noqa: E402
import filter_oracle as FI                                     # noqa: E402
import sphere_cases as SC                                      # noqa: E402
import sphere_oracle as O                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.SPHERE_GROUP
WANT = ("sphere", "radial", "decomp")
HELD = (0.0, 0.0, 27.0, 27.0)
REJECT_K = 3.0
#        m,   F,         masks, outliers, empty frame
CASES = [(1,   1,         False, 0, None),
         (3,   G,         False, 0, None),
         (4,   G + 1,     False, 0, None),
         (5,   G,         False, 0, 2),
         (63,  2 * G + 3, False, 2, 6),
         (64,  G,         True,  0, 1),
         (65,  2 * G + 3, True,  1, 4),
         (129, G + 1,     False, 3, 2),
         (441, G + 1,     True,  4, 2)]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(480, 640, max_markers=256, max_batch=2)
    yield e
    e.close()


def _masks(k, m, masked, seed):
    """fit_slots = the rim (the outer 40 % of the slots, where the planted slots lie), slots = a random 80 %: they differ."""
    if not masked:
        return None, None
    c = k["centre"]
    rr = ((k["layout"][:, :2] - c[:2]) ** 2).sum(axis=1)
    fit = np.sort(np.argsort(-rr, kind="stable")[:int(np.ceil(0.4 * m))])
    return fit, np.flatnonzero(np.random.default_rng(seed).random(m) < 0.8)


@pytest.fixture(scope="module")
def cases():
    """Every recording with its restatement in both modes, computed once; every decision has a margin."""
    out = {}
    for i, (m, n, masked, outliers, empty) in enumerate(CASES):
        def make(seed, i=i, m=m, n=n, masked=masked, outliers=outliers, empty=empty):
            k = SC.recording(n, m, seed=100 * seed + i, drop=0.0 if m < 10 else 0.1, outliers=outliers, empty_frame=empty,
                             bad_src=0.0 if m < 10 else 0.05)
            k["fit_slots"], k["slots"] = _masks(k, m, masked, i)
            k["given"] = tuple(k["centre"]) + (SC.R0,)
            return k

        def run(k, margins, m=m):
            sel = lambda s: None if s is None else np.isin(np.arange(m), s)                        # noqa: E731
            a = dict(fit_mask=sel(k["fit_slots"]), slot_mask=sel(k["slots"]), source=k["source"], margins=margins)
            return dict(fit=O.sphere_series(k["table"], None, reject_k=REJECT_K, **a), given=O.sphere_series(k["table"], k["given"], **a))

        k, want = SC.with_margins(make, run)
        k.update(want=want, n=n, m=m)
        out[m] = k
    return out


def _run(k, mode, **over):
    a = dict(table=k["table"], sphere=k["given"] if mode == "given" else None, fit_slots=k["fit_slots"], slots=k["slots"],
             source=k["source"], reject_k=REJECT_K if mode == "fit" else 0.0)
    a.update(over)
    out = E.sphere_series(**a)
    return tuple(out[w].cpu().numpy() if w in out else None for w in WANT)


def _assert_what_the_case_is_for_occurs(k, m, mode):
    """What the case was made for occurs in the RESTATEMENT's output (no device needed)."""
    want = k["want"][mode]
    assert all(np.isfinite(w).all() for w in want)
    rows = want[0]
    flag = rows[:, O.FLAG]
    case = CASES[[c[0] for c in CASES].index(m)]
    if case[4] is not None:
        e = case[4]
        assert rows[e, O.N_USED] == 0.0 and rows[e, O.N_FIT] == 0.0 and flag[e] == (1.0 if mode == "given" else 0.0), "no empty frame"
        assert (want[1][e] == 0.0).all() and (rows[np.arange(len(rows)) != e, O.N_USED] > 0.0).all()
    if case[2]:
        assert (rows[:, O.N_FIT] != rows[:, O.N_USED]).any(), "the two masks select the same slots"
    if m >= 63:
        assert (k["source"][:, 0] == 0).any() and (want[2][..., 0].sum(axis=0)[k["source"][:, 0] == 0] == 0.0).all()
        assert (want[2][..., 0] == 1.0).any() and (flag >= 1.0).any()
    if mode == "fit":
        if m < 4:
            assert (flag == 0.0).all() and (rows[:, O.N_FIT] == float(m)).all()
        if case[3]:
            rej = rows[:, O.REJECTED] == 1.0
            assert rej.any() and (rows[rej, O.N_FIT_USED] < rows[rej, O.N_FIT]).all(), "the planted slots were not rejected"
            assert ((flag >= 1.0) & ~rej).any(), "no frame keeps its first fit"
    else:
        assert flag[0] == 1.0 and (m < 3 or (flag == 3.0).any()), "no frame without contact / with a contact plane"
        if m >= 63:
            assert (rows[:, O.N_CONTACT] >= 10.0).any()


@pytest.mark.parametrize("mode", ["fit", "given"])
@pytest.mark.parametrize("m", [c[0] for c in CASES])
def test_every_output_equals_the_restatement(cases, m, mode):
    k = cases[m]
    O.check(_run(k, mode), k["want"][mode], f"m = {m}, {mode}")
    _assert_what_the_case_is_for_occurs(k, m, mode)

@pytest.mark.parametrize("mode", ["fit", "given"])
@pytest.mark.parametrize("m", [4, 65, 441])
def test_an_output_alone_and_device_resident_inputs_give_the_same_bits(cases, m, mode):
    k = cases[m]
    got = _run(k, mode)
    # any one output alone equals the same output requested with the others
    for w, i in zip(WANT, range(3)):
        alone = _run(k, mode, want=(w,))
        assert [x is None for x in alone] == [j != i for j in range(3)]
        assert np.array_equal(alone[i].view(np.uint64), got[i].view(np.uint64)), w
    # a table and a source that live on the device already give the same bits as host arrays
    dev = _run(k, mode, table=torch.from_numpy(k["table"]).cuda(), source=torch.from_numpy(k["source"]).cuda())
    for a, b in zip(dev, got):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_contact_sets_of_every_size():
    """Contact sets of 0, 1, 2, 3 (not collinear), 3 collinear, 3 coincident and many slots against the given sphere."""
    tab, n_contact, flag = SC.special_contacts()
    margins = []
    want = O.sphere_series(tab, HELD, margins=margins)
    O.assert_margins(margins, "the special contact sets")
    assert want[0][:, O.N_CONTACT].tolist() == n_contact.tolist() and want[0][:, O.FLAG].tolist() == flag.tolist()
    assert n_contact[-1] >= 10.0
    out = E.sphere_series(tab, HELD)
    assert sorted(out) == ["radial", "sphere"]
    O.check((out["sphere"].cpu().numpy(), out["radial"].cpu().numpy(), None), want, "the special contact sets")


@pytest.mark.parametrize("mode", ["fit", "given"])
@pytest.mark.parametrize("m", [65, 129])
def test_frame_ranges_equal_the_rows_of_the_full_call(cases, m, mode):
    k = cases[m]
    full = _run(k, mode)
    n = k["n"]
    for cut in (G - 1, G, G + 1):
        for a, b in ((0, cut), (cut, n)):
            part = _run(k, mode, frame_range=(a, b))
            for g, f in zip(part, full):
                assert g.shape[0] == b - a and np.array_equal(g.view(np.uint64), f[a:b].view(np.uint64)), (cut, a, b)
    empty = _run(k, mode, frame_range=(2, 2))
    assert empty[0].shape == (0, 31) and empty[1].shape == (0, m, 2) and empty[2].shape == (0, m, 4)


def test_refusals_leave_the_outputs_untouched(cases):
    k = cases[5]
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m = k["n"], 5
    t = torch.from_numpy(k["table"]).to(dev)
    src = torch.from_numpy(k["source"]).to(dev)
    sph = torch.full((n, 31), -7.5, dtype=torch.float64, device=dev)
    rad = torch.full((n, m, 2), -7.5, dtype=torch.float64, device=dev)
    dec = torch.full((n, m, 4), -7.5, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)       # noqa: E731
    good = dict(table=t, n=n, m=m, given=k["given"], src=src, depth=0.1, piv=1e-9, gap=1e-3, rk=0.0, fb=0, fe=n, sph=sph, rad=rad, dec=dec)

    def call(**over):
        a = dict(good, **over)
        held = (C.c_double * 4)(*a["given"]) if a["given"] is not None else None
        return L.lib().vbs_sphere_series(dev.index, p(a["table"]), a["n"], a["m"], C.cast(held, C.c_void_p) if held is not None
                                         else C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), p(a["src"]), a["depth"], a["piv"], a["gap"],
                                         a["rk"], a["fb"], a["fe"], p(a["sph"]), p(a["rad"]), p(a["dec"]), C.c_void_p(0))

    inf, nan = float("inf"), float("nan")
    c = k["given"]
    for over in (dict(table=None), dict(sph=None, rad=None, dec=None), dict(n=0), dict(m=0), dict(depth=0.0), dict(depth=-0.1),
                 dict(depth=nan), dict(depth=inf), dict(piv=-1e-12), dict(piv=nan), dict(gap=-1e-9), dict(gap=inf), dict(rk=-1.0),
                 dict(rk=nan), dict(fb=-1), dict(fe=n + 1), dict(fb=2, fe=1), dict(src=None), dict(given=c[:3] + (0.0,)),
                 dict(given=c[:3] + (-27.0,)), dict(given=c[:3] + (inf,)), dict(given=(nan,) + c[1:]), dict(given=c[:2] + (inf, 27.0))):
        assert call(**over) == L.VBS_EINVAL, over
    torch.cuda.synchronize()
    assert (sph == -7.5).all() and (rad == -7.5).all() and (dec == -7.5).all()
    assert call(fb=1, fe=1) == L.VBS_OK                           # an empty range emits nothing
    torch.cuda.synchronize()
    assert (sph == -7.5).all() and (rad == -7.5).all() and (dec == -7.5).all()
    assert call() == L.VBS_OK
    torch.cuda.synchronize()
    O.check((sph.cpu().numpy(), rad.cpu().numpy(), dec.cpu().numpy()), k["want"]["given"], "the direct call")
    assert call(src=None, dec=None) == L.VBS_OK                   # without a source: the other two outputs
    for bad in (dict(contact_depth=0.0), dict(sphere=HELD[:3] + (0.0,)), dict(frame_range=(0, n + 1)), dict(source=None, want=("decomp",)),
                dict(source=k["source"][:, :3]), dict(reject_k=-1.0)):
        with pytest.raises(ValueError):
            _run(k, "given", **bad)


def test_bonnet_analysis_on_the_synthetic_press_equals_the_pipeline_over_the_restatement(eng, tmp_path):
    """8 unloaded frames, then the 65-marker cap cut at 0 -> 2.8 mm while leaning 0 -> 15 degrees towards 35 over 24 frames, noise
    0.02 mm, 3 % gaps.  The pipeline - a fit per still frame, the median sphere, the whole recording against it - equals the same
    steps over the restatement in bits, so the held sphere is the same.  One still frame leaves R to some 0.05 mm
    (`tests/test_sphere_host.py` measures it), the median of eight to 0.05 x 1.25 / sqrt(8) = 0.02 mm, and the offset R - dist carries
    that: the bound on |offset - delta| is 0.1 mm, five times it (the plane's own share is below 0.03 mm there)."""
    import pandas as pd
    from vbs_amd import fields, pipeline as P, rigid as RG, sphere as SP
    from vbs_amd.filters import half_taps
    k = SC.press_recording(24, still=8, seed=1)
    tab, F = k["table"], 32
    lay = k["layout"]
    grid_xy = np.stack([g.ravel() for g in np.meshgrid(np.linspace(-12, 12, 5), np.linspace(-12, 12, 5))], axis=1)
    W = fields.gaussian_weights(lay[:, :2], grid_xy, 4.0)
    wsum = fields.row_sums(W)
    taps = np.array([0.25, 0.5, 0.25])
    res = P.bonnet_analysis(eng, torch.from_numpy(tab).cuda(), still=(0, 8), taps=taps, grid=(W, wsum, grid_xy))
    # the same pipeline over the restatement
    margins = []
    fits, _, _ = O.sphere_series(tab, None, reject_k=3.0, frame_range=(0, 8), margins=margins)
    held = SP.combine(fits)
    src = RG.source_from_table(tab, 0)
    want = O.sphere_series(tab, held["sphere"], source=src, margins=margins)
    O.assert_margins(margins, "the synthetic press")
    assert held["frames"] == 8 and np.array_equal(res["held"], held["sphere"]) and np.array_equal(res["source"], src)
    assert np.array_equal(res["still"]["scatter"], held["scatter"]) and np.abs(held["sphere"] - HELD).max() < 0.1
    O.check((res["sphere"].cpu().numpy(), res["radial"].cpu().numpy(), res["decomp"].cpu().numpy()), want, "the synthetic press")
    rows = res["sphere"].cpu().numpy()                           # (the device's own, just held to the restatement)
    s = SP.summary(want[0])
    for name in ("first_contact", "max_offset_frame", "max_tilt_frame", "share"):
        assert res[name] == s[name], name
    assert np.array_equal(res["kind"], s["kind"]) and np.array_equal(res["offset"], s["offset"], equal_nan=True)
    flat = rows[:, O.FLAG] == 3.0
    assert np.array_equal(res["tilt_deg"], np.where(flat, rows[:, O.TILT_DEG], np.nan), equal_nan=True)   # (an arc tangent: the device's own)
    assert (rows[:8, O.FLAG] == 1.0).all() and flat[-20:].all() and 8 < res["first_contact"] <= 12 and res["max_offset_frame"] == F - 1
    assert np.abs(rows[flat, O.OFFSET] - k["delta"][flat]).max() < 0.1
    assert np.abs(rows[-8:, O.TILT_DEG] - k["tilt"][-8:]).max() < 0.5 and np.abs(rows[-8:, O.AZIMUTH_DEG] - 35.0).max() < 2.0
    # the trend: filtered components, renormalised
    got = res["trend_filtered"].cpu().numpy()
    FI.check_fir(got, SP.trend_record(rows), half_taps(taps), 7, what="the trend record through the filter")
    tr = res["trend"]
    ok = tr[:, 0] == 1.0
    assert tr.shape == (F, 10) and ok[-10:-1].all() and np.abs((tr[ok, 5:8] ** 2).sum(axis=1) - 1.0).max() < 1e-14
    assert np.abs(tr[-10:-1, 8] - k["tilt"][-10:-1]).max() < 0.5
    # the radial record through the field map, as it is; the depth map is its negative
    mp = E.field_map_f64(res["radial"], W, wsum, 0.5, 1).cpu().numpy()
    _, _, d = FO.exact_map(want[1], W, 1)
    assert FO.coverage_margin(d, wsum, 0.5) > FO.Fraction(1, 10 ** 9)
    FO.check_within_bound(mp, want[1], W, wsum, 0.5, 1, what="radial through the field map")
    dm = res["depth_map"].cpu().numpy()
    assert dm.shape == (F, 25, 2) and (mp[..., 0] == 1.0).any() and np.array_equal(dm[..., 0], mp[..., 0])
    assert np.allclose(dm[..., 1], -mp[..., 1], rtol=0, atol=1e-12) and res["depth_patch"].shape == (F, 8)
    assert (res["depth_patch"].cpu().numpy()[-8:, 0] == 2.0).all()
    # d_n of the pressed slots is the push: negative (towards the centre) and as deep as the cut at the apex
    # (the leaning plane moves the apex by R cos t - (R - delta) along its normal, of which the apex's own normal sees cos t; D is the
    # difference of two positions with 0.02 mm of noise each: 5 x 0.028 mm)
    dec = want[2]
    f = int(np.flatnonzero(~k["dead"][:, 0])[-1])
    ct = np.cos(np.deg2rad(k["tilt"][f]))
    assert f >= F - 4 and dec[f, 0, 0] == 1.0 and abs(dec[f, 0, 1] + (SC.R0 * ct - (SC.R0 - k["delta"][f])) * ct) < 0.15
    # a still stretch of two frames cannot give the three fits a held sphere needs; a sphere given by the caller is held as it is
    with pytest.raises(ValueError):
        P.bonnet_analysis(eng, tab, still=(0, 2))
    own = P.bonnet_analysis(eng, tab, still=(0, 8), sphere=held["sphere"], source=None)
    assert "still" not in own and "decomp" not in own and np.array_equal(own["sphere"].cpu().numpy().view(np.uint64), rows.view(np.uint64))
    df = P.to_bonnet_frame(res, frame_offset=100, path=tmp_path / "bonnet.csv")
    assert tuple(df.columns) == P.BONNET_FRAME_COLUMNS + P.BONNET_TREND_COLUMNS and len(df) == F
    assert df["frameno"].tolist() == list(range(100, 100 + F)) and df["kind"].tolist()[0] == "free" and df["kind"].tolist()[-1] == "flat"
    for name in ("flag", "n_used", "n_contact", "deepest"):
        assert df[name].dtype == np.int64, name
    assert np.array_equal(df["offset"].to_numpy()[flat], rows[flat, O.OFFSET]) and df["offset"].isna().to_numpy()[:8].all()
    back = pd.read_csv(tmp_path / "bonnet.csv", float_precision="round_trip")
    assert tuple(back.columns) == tuple(df.columns)
    for name in df.columns:
        if name != "kind":
            assert np.array_equal(back[name].to_numpy(), df[name].to_numpy(), equal_nan=True), name
