"""GPU tests of the uncertainty of the 3-D solve (`vbs_uncert_points`, `vbs_uncert_cov`, `vbs_uncert_total`, `vbs_pixel_noise`;
DESIGN 4.22) against the NumPy restatement `tests/helpers/uncert_oracle.py`: EVERY output bit for bit, nothing masked.  Shapes
are the smallest at which the kernels can go wrong - around a wave (64 slots), around the 256 threads of a row block and around
the frames a workgroup of the total takes (VBS_UNCERT_GROUP) - not the workload's; the tables hold untracked rows, rows below the
size gate, a row on the principal point, cleared XYZ flags, a reference frame with missing rows, and NaN / 1e30 in every cell
that must not be read."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import vbs_amd._lib as L                                       # noqa: E402
from vbs_amd import engine as E, uncertainty as UN             # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import uncert_cases as UC                                      # noqa: E402
import uncert_oracle as U                                      # noqa: E402

pytestmark = pytest.mark.gpu
G = L.UNCERT_GROUP


def _cam(cam):
    return L.make_camera(*cam[:4], cam[4])


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same(got, want, what):
    """Bit for bit (a NaN equals a NaN; +0 is not -0)."""
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float64:
        same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ, first at {np.argwhere(~same)[0]}: " \
                       f"{got[~same][0]!r} against {want[~same][0]!r}"


def _obs(form, m, seed=0):
    if form == "one":
        return np.array([0.0025, 0.0004, -0.0003, 0.0036, 0.0002, 0.0064])
    rng = np.random.default_rng(50 + seed)
    A = rng.normal(size=(m, 3, 3)) * 0.05
    S = A @ A.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def _move(n, m, seed):
    rng = np.random.default_rng(200 + seed)
    return np.cumsum(rng.normal(size=(n, m, 3)) * np.array([0.3, 0.3, 0.15]), axis=0)


@pytest.mark.parametrize("size,distorted,exact", [((640, 480), True, False), ((640, 480), False, False), ((1920, 1200), True, True),
                                                  ((1920, 1200), False, True)])
def test_points_equal_the_restatement_and_the_solve(size, distorted, exact):
    cam = UC.camera(size, distorted, exact)
    c = U.Cam(*cam)
    uvd = UC.points(cam, size)
    rng = np.random.default_rng(3)
    more = np.stack([rng.uniform(0, size[0], 300), rng.uniform(0, size[1], 300), rng.uniform(5, 40, 300)], axis=1)
    edge = np.array([[c.cx, c.cy, 12.0], [10.0, 10.0, 0.0], [np.nan, 5.0, 9.0], [30.0, 40.0, np.inf], [1e30, 1.0, 8.0]])
    uvd = np.concatenate([uvd, more, edge])                       # 337 points: more than one block, the last one ragged
    xyz, jo, jc, ok = E.solve3d_jacobian(uvd, _cam(cam))
    X, Jo, Jc, okw = U.jacobians(c, uvd)
    _same(ok, okw, "ok")
    _same(xyz, X, "xyz")
    _same(jo, Jo, "J_obs")
    _same(jc, Jc, "J_cam")
    assert okw[:-5].all() and okw[-5:-1].tolist() == [0, 0, 0, 1]   # (an infinite diameter is a point at h = 0: a solve)
    und = E.undistort_points(uvd[:, :2].copy(), _cam(cam))
    xyz2, ok2 = E.calculate_3d(torch.cat([und, torch.as_tensor(uvd[:, 2:3], device=und.device)], dim=1), _cam(cam))
    assert torch.equal(ok, ok2)
    _same(xyz, _np(xyz2), "xyz against calculate_3d(undistort_points)")
    again = E.solve3d_jacobian(uvd, _cam(cam))
    assert all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() for a, b in zip((xyz, jo, jc, ok), again))
    one = E.solve3d_jacobian(uvd[:1], _cam(cam))
    _same(one[2], Jc[:1], "J_cam of one point")
    none = E.solve3d_jacobian(np.zeros((0, 3)), _cam(cam))
    assert none[0].shape == (0, 3) and none[2].shape == (0, 3, 16)


#        n,       m,  q, obs,   distorted
TABLES = [(1,      1,  0, "one",  True),
          (2,      2,  1, "slot", False),
          (G - 1,  63, 5, "one",  True),
          (G,      64, 16, "slot", True),
          (G + 1,  65, 5, "slot", False),
          (2 * G + 3, 255, 1, "one", True),
          (2,      256, 16, "one", False),
          (G + 1,  257, 0, "slot", True),
          (2 * G + 3, 441, 16, "slot", True)]


@pytest.fixture(scope="module")
def table_cases():
    cases = {}
    for i, (n, m, q, form, distorted) in enumerate(TABLES):
        cam = UC.camera((640, 480) if i % 2 == 0 else (1920, 1200), distorted, exact=False)
        size = (640, 480) if i % 2 == 0 else (1920, 1200)
        tab = UC.table(cam, n, m, size, seed=i, move=_move(n, m, i))
        ref = n // 3
        cases[(n, m)] = dict(cam=cam, tab=tab, obs=_obs(form, m, i), L=UC.factor(q, i), ref=ref, n=n, m=m, q=q)
    return cases


@pytest.mark.parametrize("n,m", [(t[0], t[1]) for t in TABLES])
def test_table_entries_equal_the_restatement(table_cases, n, m):
    k = table_cases[(n, m)]
    c, cam = U.Cam(*k["cam"]), _cam(k["cam"])
    out = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=k["ref"])
    cov, dcov = U.solve3d_cov(k["tab"], c, k["obs"], k["L"], ref_frame=k["ref"])
    _same(out["cov"], cov, "cov")
    _same(out["dcov"], dcov, "dcov")
    _same(out["total"], U.solve3d_total(k["tab"], c, k["obs"], k["L"], ref_frame=k["ref"]), "total")
    _same(E.pixel_noise(k["tab"]), U.pixel_noise(k["tab"]), "pixel_noise")
    plain = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"])        # no reference frame: Sigma_X alone, the same bits
    assert plain["dcov"] is None and plain["total"] is None and torch.equal(plain["cov"], out["cov"])
    again = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=k["ref"])
    assert all(torch.equal(out[w], again[w]) for w in out)
    if n * m >= 8:                                                # the content is there: every kind of row
        flags = k["tab"][..., 0].astype(int)
        assert (flags == 0).any() and (cov[..., 0] == 0)[flags == 3].any() and (dcov[..., 0] == 3).any()
        assert np.isfinite(cov).all() and np.isfinite(dcov).all()


@pytest.mark.parametrize("n,m", [(G + 1, 65), (2 * G + 3, 441)])
def test_table_path_equals_the_point_path(table_cases, n, m):
    """Sigma_X of a usable row from the Jacobians of the point interface: the identity as the camera factor makes g_c the
    columns of J_cam, and the products are the restatement's."""
    k = table_cases[(n, m)]
    cam = _cam(k["cam"])
    out = _np(E.solve3d_cov(k["tab"], cam, k["obs"], np.eye(16))["cov"]).reshape(-1, 7)
    rows = k["tab"].reshape(-1, 10)
    use = out[:, 0] == 1
    assert use.sum() > n * m // 2
    uvd = rows[use][:, 1:4].astype(np.float64)
    xyz, jo, jc, ok = (_np(t) for t in E.solve3d_jacobian(uvd, cam))
    assert ok.all()
    obs = np.tile(U._obs(k["obs"], m), (n, 1))[use]
    want = U.obs_product(jo, obs)
    for col in range(16):
        U._outer_add(want, jc[:, :, col])
    _same(out[use][:, 1:], want, "Sigma_X from the point path")
    assert np.array_equal(xyz.astype(np.float32), rows[use][:, 6:9])


def test_frame_ranges_reference_frames_and_slots(table_cases):
    k = table_cases[(2 * G + 3, 255)]
    n, m = k["n"], k["m"]
    c, cam = U.Cam(*k["cam"]), _cam(k["cam"])
    for ref in (0, 5, n - 1):
        whole = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=ref)
        for a, b in ((0, G), (G, G + 1), (G + 1, n), (3, 3), (1, n - 1)):      # ref inside and outside the range
            part = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=ref, frame_range=(a, b))
            for w in ("cov", "dcov", "total"):
                assert torch.equal(part[w], whole[w][a:b]), (ref, a, b, w)
        _same(whole["total"], U.solve3d_total(k["tab"], c, k["obs"], k["L"], ref_frame=ref), f"total, ref {ref}")
    _same(E.pixel_noise(k["tab"], (2, 9)), U.pixel_noise(k["tab"], (2, 9)), "pixel_noise of a range")
    _same(E.pixel_noise(k["tab"], (4, 4)), np.zeros((m, 10)), "pixel_noise of no frames")
    ref = k["ref"]
    usable0 = _np(E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=ref)["dcov"])[ref, :, 0] >= 1
    good = np.nonzero(usable0)[0]
    for slots in ([], good[:1], good[:2], good[::3], np.arange(m)):
        mask = np.zeros(m, dtype=bool)
        mask[np.asarray(slots, dtype=int)] = True
        got = E.solve3d_cov(k["tab"], cam, k["obs"], k["L"], ref_frame=ref, slots=slots)["total"]
        want = U.solve3d_total(k["tab"], c, k["obs"], k["L"], ref_frame=ref, slots=mask)
        _same(got, want, f"total over {len(slots)} slots")
        assert want[:, 0].max() <= len(slots)
    assert {0.0, 1.0, 2.0} <= set(np.concatenate([U.solve3d_total(k["tab"], c, k["obs"], k["L"], ref_frame=ref, slots=np.isin(
        np.arange(m), good[:j]))[:, 0] for j in (0, 1, 2)]))


def test_refusals_leave_the_outputs_untouched():
    cam = UC.camera()
    tab = UC.table(cam, 4, 6)
    import ctypes as C
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.as_tensor(tab, device=dev)
    work = torch.full((6 * L.UNCERT_WORK_COLS,), 7.0, dtype=torch.float64, device=dev)
    cov = torch.full((4, 6, 7), 7.0, dtype=torch.float64, device=dev)
    dcov = torch.full((4, 6, 8), 7.0, dtype=torch.float64, device=dev)
    total = torch.full((4, 8), 7.0, dtype=torch.float64, device=dev)
    obs, fac = np.array([[0.01, 0.0, 0.0, 0.01, 0.0, 0.02]]), np.zeros((16, 17))
    ccam = _cam(cam)

    def p(x):
        return C.c_void_p(x.data_ptr())

    def hp(a):
        return a.ctypes.data_as(C.c_void_p)

    def call(obs=obs, rows=1, q=16, ref=0):
        a = L.lib().vbs_uncert_cov(dev.index, p(t), 4, 6, C.byref(ccam), hp(obs), rows, hp(fac), q, ref, 5.0, 1e-12, 0, 4, p(work),
                                   p(cov), p(dcov), None)
        b = L.lib().vbs_uncert_total(dev.index, p(t), 4, 6, C.byref(ccam), hp(obs), rows, hp(fac), q, ref, None, 5.0, 0, 4, p(work),
                                     p(total), None)
        return a, b
    bad = obs.copy()
    bad[0, 3] = np.nan
    for kw in (dict(q=17), dict(ref=4), dict(ref=-1), dict(obs=bad), dict(rows=3)):
        assert call(**kw) == (L.VBS_EINVAL, L.VBS_EINVAL), kw
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in (work, cov, dcov, total))
    with pytest.raises(ValueError):
        E.solve3d_cov(tab, ccam, obs, np.zeros((16, 17)))
    with pytest.raises(ValueError):
        E.solve3d_cov(tab[0], ccam, obs)
    with pytest.raises(ValueError):
        E.solve3d_cov(tab[..., :9], ccam, obs)
    with pytest.raises(ValueError):
        E.solve3d_jacobian(np.zeros((3, 2)), ccam)
    with pytest.raises(ValueError):
        E.pixel_noise(tab, (0, 5))


def _synth_table(spec, cam, n, move=None):
    """The table of a `synth` recording from its ground truth: frames 1 .. n (frame 0 carries no jitter), every dot tracked."""
    from vbs_amd import synth
    o = synth.dot_truth(spec, 5, range(1, n + 1))
    if move is not None:
        o = o + move
    t = np.zeros((n, spec.n_markers, 10), dtype=np.float32)
    t[..., 1:4] = o
    _, X, ok = U.primal(U.Cam(*cam), *(t[..., k].ravel().astype(np.float64) for k in (1, 2, 3)))
    assert ok.all()
    t[..., 6:9], t[..., 0] = X.reshape(n, -1, 3), 3.0
    return t


def test_uncertainty_analysis_of_a_synthetic_recording(tmp_path):
    """`pipeline.uncertainty_analysis` and its sheet on a small recording of `synth.py`, with the noise it was generated with: the
    centre of a dot is uniform over 5 levels of 1/16 px (sigma = sqrt(2) / 16), its diameter takes (-1, -1, 0, 0, 1) / 8 px
    (sigma = sqrt(0.56) / 8).  Two frames differ by at most 2.83 sigma in any one of the three, so a displacement - a combination
    of three of them - by at most 2.83 / sqrt(2) * sqrt(3) = 3.47 of its own sigma_D: at k = 3.5 no marker of the still recording
    is significant, whatever the seed.  A marker moved by 10 sigma_D is, in every frame after the move."""
    from vbs_amd import pipeline as P, synth
    spec = synth.grid_spec(640, 480, 6, 60, 20, jitter16=2, djitter16=2)
    K, _, R, T = synth.default_camera(spec)
    cam = (K, UC.DIST, R, T, 2.0)
    n, m, k = 24, spec.n_markers, 3.5
    obs = UN.obs_cov(np.sqrt(2.0) / 16, np.sqrt(0.56) / 8)
    fac = UN.camera_factor(std_intrinsics=[0.5, 0.5, 0.3, 0.3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-3], t_std=[0.02, 0.02, 0.05], diameter_std=0.01)
    still = _synth_table(spec, cam, n)
    noise = _np(E.pixel_noise(still))
    # a variance from n samples of a distribution of kurtosis <= 1.8 (uniform) has the relative standard error
    # sqrt((1.8 - 1) / n + 2 / (n (n - 1))) = 0.19 at n = 24: four of them over the 108 variances here
    assert (noise[:, 0] == n).all() and (np.abs(noise[:, [4, 7]] / obs[0] - 1) < 0.76).all() and (np.abs(noise[:, 9] / obs[5] - 1) < 0.76).all()
    res = P.uncertainty_analysis(None, still, _cam(cam), obs, fac, ref_frame=0, k=k)
    assert res["significant"].shape == (n, m, 3) and not res["significant"].any()
    assert res["usable_d"].all() and (res["sigma_d"][1:] > 0).all() and res["limit"].shape == (m, 3) and (res["limit"] > 0).all()
    # markers 3 and 7 move from frame 12 on by 10 sigma_D: 3 along Z (through the diameter), 7 along X (through Cx)
    _, Jo, _, _ = U.jacobians(U.Cam(*cam), still[0, [3, 7], 1:4].astype(np.float64))
    sd = res["sigma_d"][12, [3, 7]]
    move = np.zeros((n, m, 3))
    move[12:, 3, 2] = 10 * sd[0, 2] / abs(Jo[0, 2, 2])
    move[12:, 7, 0] = 10 * sd[1, 0] / abs(Jo[1, 0, 0])
    res = P.uncertainty_analysis(None, _synth_table(spec, cam, n, move), _cam(cam), obs, fac, ref_frame=0, k=k)
    sig = res["significant"]
    assert sig[12:, 3, 2].all() and sig[12:, 7, 0].all() and not sig[:12].any()
    others = np.ones(m, dtype=bool)
    others[[3, 7]] = False
    assert not sig[:, others].any()
    assert res["t2_valid"][1:].all() and (res["t2"][12:, [3, 7]] > k * k).all()
    assert res["sigma_total"].shape == (n, 3) and res["complete"].all() and (res["count"] == m).all()
    assert ((res["camera_share"] >= 0) & (res["camera_share"] <= 1)).all() and (res["camera_share"][1:] > 0).all()
    # the sigma_Z map through the contact-map smoother, and the DataFrame-facing form
    from vbs_amd import fields
    from vbs_amd.reconstruction3d import Config, MarkerAnalysis
    nodes = still[0, :, 1:3].astype(np.float64)
    grid_xy, _ = fields.grid_over(nodes, (8, 8))
    W = fields.gaussian_weights(nodes, grid_xy, fields.default_bandwidth(nodes))
    mapped = P.uncertainty_analysis(None, still, _cam(cam), obs, fac, ref_frame=0, k=k, grid=(W, fields.row_sums(W)))
    zmap = _np(mapped["sigma_z_map"])
    assert zmap.shape == (n, 64, 2) and (zmap[..., 0] == 1).all()
    assert (zmap[..., 1] >= np.nanmin(mapped["sigma_x"][..., 2]) * (1 - 1e-12)).all()
    assert (zmap[..., 1] <= np.nanmax(mapped["sigma_x"][..., 2]) * (1 + 1e-12)).all()
    ma = MarkerAnalysis(Config(data_dir=tmp_path / "data", output_dir=tmp_path / "out", plots_dir=tmp_path / "plots"))
    ma.set_camera(*cam[:4])
    ma.config.marker_diameter_mm = cam[4]
    frame = ma.uncertainty(still, obs, fac, ref_frame=0, k=k)
    assert np.array_equal(frame["sigma_Z"].to_numpy(), mapped["sigma_x"][..., 2].reshape(-1))
    sheet = P.to_uncertainty_frame(res)
    assert len(sheet) == n * m and tuple(sheet.columns) == P.UNCERTAINTY_FRAME_COLUMNS
    assert sheet["significant_Z"].sum() == sig[..., 2].sum() and sheet["frameno"].iloc[-1] == n
