"""CPU tests of the modal analysis' host side (no GPU): the four new C symbols and their constants, what the entries refuse before
a device is touched, the wrappers' argument checks, `vbs_amd.modes`, and the restatements the GPU tests hold the device to
(`tests/helpers/modes_oracle.py`): the moments' against exact rational arithmetic, the covariance's against `np.cov`, the eigen
part's against `np.linalg.eigh` (EIG_MEASURED / EIG_TOL), the scores' against a masked einsum, and the thresholds of
the end-to-end GPU test on the restatement alone."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from vbs_amd import _build
from vbs_amd import modes as MD

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import modes_oracle as O                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbs_cross_moments_f64", "vbs_covariance_f64", "vbs_leading_modes_f64", "vbs_mode_scores_f64")


def test_header_symbols_constants_and_source_agree():
    hdr = open(os.path.join(ROOT, "include", "vbs.h")).read()
    declared = set(re.findall(r"\b(vbs_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in L.SYMBOLS and hasattr(L.lib(), name)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(VBS_[A-Z0-9_]+)\s+(-?\d+)", hdr)}
    for name in ("MOM_CHUNK", "MOM_WG_SLOTS", "MOM_MAX_SLOTS", "MODES_MAX", "MODES_MAX_DIM", "MODES_SWEEPS", "MODES_MAX_ITERS", "SCORE_GROUP"):
        assert getattr(L, name) == defs["VBS_" + name], name
    assert L.MODES_MAX == 16 == O.MR and L.MODES_SWEEPS == O.SWEEPS and L.MODES_MAX_DIM == 3 * L.MOM_MAX_SLOTS == 3072
    assert L.MOM_CHUNK % 16 == 0 and L.MOM_WG_SLOTS == 16 and L.SCORE_GROUP == 8
    assert (L.PROJ_MAX_FRAMES + 7) * 2.0 ** -53 < 1e-9            # gamma_(n+6) is far from its pole at every admitted n
    assert "k_modes.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "k_modes.hip"))
    lib = L.lib()
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [9, 11, 12, 15]


def test_refusals_without_a_gpu():
    """Every C entry decides every refusal before the device is touched: with device pointers that are never followed, on a machine
    without a GPU, they answer VBS_EINVAL / VBS_ECAPACITY, a bad argument before a capacity."""
    lib = L.lib()
    p, nul = C.c_void_p(8), None

    def cm(rec=p, n=10, s=5, cols=4, nv=3, shift=p, mom=p):
        return lib.vbs_cross_moments_f64(0, rec, n, s, cols, nv, shift, mom, None)
    for bad in (dict(rec=nul), dict(mom=nul), dict(n=0), dict(s=0), dict(n=-1), dict(cols=1), dict(cols=9), dict(nv=0), dict(nv=4, cols=8),
                dict(nv=3, cols=3)):
        assert cm(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.MOM_MAX_SLOTS + 1)):
        assert cm(**big) == L.VBS_ECAPACITY, big
        assert cm(**dict(big, shift=nul)) == L.VBS_ECAPACITY      # no shift is no error
        assert cm(**dict(big, rec=nul)) == L.VBS_EINVAL and cm(**dict(big, nv=0)) == L.VBS_EINVAL

    def cv(mom=p, s=5, nv=3, mode=1, mc=2, denom=9.0, mask=nul, cov=p, ok=nul):
        return lib.vbs_covariance_f64(0, mom, s, nv, mode, mc, denom, mask, cov, ok, None)
    for bad in (dict(mom=nul), dict(cov=nul), dict(s=0), dict(nv=0), dict(nv=4), dict(mode=2), dict(mode=-1), dict(mc=1), dict(denom=0.0),
                dict(denom=-1.0), dict(denom=math.nan), dict(denom=math.inf)):
        assert cv(**bad) == L.VBS_EINVAL, bad
    assert cv(s=L.MOM_MAX_SLOTS + 1) == L.VBS_ECAPACITY and cv(s=L.MOM_MAX_SLOTS + 1, mode=0, denom=math.nan) == L.VBS_ECAPACITY
    assert cv(s=L.MOM_MAX_SLOTS + 1, mc=1) == L.VBS_EINVAL

    def lm(A=p, Cn=20, r=6, iters=48, tiny=1e-24, work=p, values=p, modes=p, resid=p, info=p):
        return lib.vbs_leading_modes_f64(0, A, Cn, r, iters, tiny, work, values, modes, resid, info, None)
    for bad in (dict(A=nul), dict(work=nul), dict(values=nul), dict(modes=nul), dict(resid=nul), dict(info=nul), dict(Cn=0), dict(r=0),
                dict(r=17), dict(r=6, Cn=5), dict(iters=-1), dict(iters=L.MODES_MAX_ITERS + 1), dict(tiny=-1e-30), dict(tiny=1.0),
                dict(tiny=math.nan)):
        assert lm(**bad) == L.VBS_EINVAL, bad
    assert lm(Cn=L.MODES_MAX_DIM + 1) == L.VBS_ECAPACITY and lm(Cn=L.MODES_MAX_DIM + 1, r=17) == L.VBS_EINVAL

    def ms(rec=p, n=10, s=5, cols=4, nv=3, center=p, modes=p, r=6, mc=0.5, fb=0, fe=10, scores=p, energy=nul):
        return lib.vbs_mode_scores_f64(0, rec, n, s, cols, nv, center, modes, r, mc, fb, fe, scores, energy, None)
    for bad in (dict(rec=nul), dict(center=nul), dict(modes=nul), dict(scores=nul), dict(n=0, fe=0), dict(s=0), dict(cols=1), dict(cols=9),
                dict(nv=0), dict(nv=4, cols=8), dict(nv=3, cols=3), dict(r=0), dict(r=17), dict(mc=0.0), dict(mc=1.0000001), dict(mc=math.nan),
                dict(fb=-1), dict(fe=11), dict(fb=6, fe=5)):
        assert ms(**bad) == L.VBS_EINVAL, bad
    for big in (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.MOM_MAX_SLOTS + 1)):
        assert ms(**big) == L.VBS_ECAPACITY, big
        assert ms(**dict(big, mc=0.0)) == L.VBS_EINVAL


def test_wrapper_argument_checks():
    from vbs_amd.engine import _covariance_args, _modes_args, _moments_args, _scores_args
    assert _moments_args(10, 5, 4, (5, 3), None) == 3 and _moments_args(10, 5, 8, None, 2) == 2 and _moments_args(1, 1, 2, (1, 1), None) == 1
    for bad in (dict(n=0), dict(s=0), dict(cols=1), dict(cols=9), dict(n_values=4, cols=8), dict(n_values=0), dict(shift_shape=(5, 2)),
                dict(shift_shape=(15,))):
        with pytest.raises(ValueError):
            _moments_args(**dict(dict(n=10, s=5, cols=4, shift_shape=(5, 3), n_values=None), **bad))
    with pytest.raises(L.VbsError, match=f"VBS_MOM_MAX_SLOTS = {L.MOM_MAX_SLOTS}"):
        _moments_args(10, L.MOM_MAX_SLOTS + 1, 4, None, None)
    with pytest.raises(L.VbsError, match="VBS_PROJ_MAX_FRAMES"):
        _moments_args(L.PROJ_MAX_FRAMES + 1, 5, 4, None, None)
    good = dict(mom_shape=(5, 5, 4, 4), n_values=3, mode="filled", min_count=2, denom=9.0, mask_shape=None)
    assert _covariance_args(**good) == (5, 3, 1, 2, 9.0) and _covariance_args(**dict(good, mode="pairwise", denom=None))[2] == 0
    for bad in (dict(mom_shape=(5, 4, 4, 4)), dict(mom_shape=(5, 5, 4)), dict(n_values=0), dict(n_values=4), dict(mode="both"), dict(min_count=1),
                dict(denom=None), dict(denom=0.0), dict(denom=math.nan), dict(mask_shape=(4,))):
        with pytest.raises(ValueError):
            _covariance_args(**dict(good, **bad))
    assert _modes_args((20, 20), 6, 48, 1e-24) == (20, 6, 48, 1e-24) and _modes_args((3, 3), 3, 0, 0.0) == (3, 3, 0, 0.0)
    for bad in (((20, 19), 6, 48, 1e-24), ((20,), 6, 48, 1e-24), ((20, 20), 0, 48, 1e-24), ((20, 20), 17, 48, 1e-24), ((5, 5), 6, 48, 1e-24),
                ((20, 20), 6, -1, 1e-24), ((20, 20), 6, 48, 1.0), ((20, 20), 6, 48, math.nan)):
        with pytest.raises(ValueError):
            _modes_args(*bad)
    with pytest.raises(L.VbsError, match=f"VBS_MODES_MAX_DIM = {L.MODES_MAX_DIM}"):
        _modes_args((L.MODES_MAX_DIM + 1,) * 2, 6, 48, 1e-24)
    sg = dict(n=10, s=5, cols=4, center_shape=(15,), modes_shape=(6, 15), n_values=None, min_coverage=0.5, frame_range=None)
    assert _scores_args(**sg) == (3, 6, 0.5, 0, 10) and _scores_args(**dict(sg, frame_range=(4, 4)))[3:] == (4, 4)
    for bad in (dict(center_shape=(14,)), dict(modes_shape=(6, 14)), dict(modes_shape=(17, 15)), dict(modes_shape=(15,)), dict(min_coverage=0.0),
                dict(min_coverage=1.5), dict(frame_range=(0, 11)), dict(frame_range=(6, 5)), dict(n_values=4)):
        with pytest.raises(ValueError):
            _scores_args(**dict(sg, **bad))
    from vbs_amd.pipeline import _modal_args
    assert _modal_args(200, 169, 6, 48, "filled", 0, None, 0.5) == (6, 48, None)
    assert _modal_args(200, 4, 6, 48, "pairwise", 0, [1, 0, 1, 1], 0.5)[2].tolist() == [0, 2, 3]
    for bad in ((1, 9, 6, 48, "filled", 0, None, 0.5), (200, 1, 6, 48, "filled", 0, None, 0.5), (200, 9, 17, 48, "filled", 0, None, 0.5),
                (200, 9, 6, -1, "filled", 0, None, 0.5), (200, 9, 6, 48, "full", 0, None, 0.5), (200, 9, 6, 48, "filled", 200, None, 0.5),
                (200, 9, 6, 48, "filled", 0, [1, 1], 0.5), (200, 9, 6, 48, "filled", 0, None, 0.0)):
        with pytest.raises(ValueError):
            _modal_args(*bad)
    with pytest.raises(L.VbsError, match=f"VBS_MOM_MAX_SLOTS = {L.MOM_MAX_SLOTS}"):    # a capacity, as the engine's wrappers report it
        _modal_args(200, L.MOM_MAX_SLOTS + 1, 6, 48, "filled", 0, None, 0.5)
    with pytest.raises(L.VbsError, match="VBS_PROJ_MAX_FRAMES"):
        _modal_args(L.PROJ_MAX_FRAMES + 1, 9, 6, 48, "filled", 0, None, 0.5)
    with pytest.raises(ValueError):                               # a bad argument comes before a capacity
        _modal_args(200, L.MOM_MAX_SLOTS + 1, 17, 48, "filled", 0, None, 0.5)


@pytest.mark.parametrize("n,s,nv", ((1, 2, 3), (17, 5, 2), (40, 3, 1), (70, 4, 3)))
def test_restated_moments_are_exact_on_dyadic_cases_and_within_the_bound_on_random_ones(n, s, nv):
    rec, shift = O.dyadic_case(n, s, nv + 2, nv, seed=n)
    rec[:, -1, 0] = 0.0
    got = O.moments(rec, nv, shift)
    value, _ = O.exact_moments(rec, nv, shift)
    assert all(O.Fraction(float(got[i])) == value[i] for i in np.ndindex(*got.shape))
    assert not got[-1].any() and not got[:, -1].any()
    O.assert_bits(got, got.transpose(1, 0, 3, 2), "mirror")
    assert np.array_equal(got[..., 3, 3], np.rint(got[..., 3, 3]))
    valid = rec[..., 0] != 0
    assert np.array_equal(got[..., 3, 3], (valid[:, :, None] & valid[:, None, :]).sum(axis=0))
    rec, shift = O.random_case(n, s, nv + 1, nv, seed=n + 1)
    worst = O.check_within_bound(O.moments(rec, nv, shift), rec, nv, shift, what=f"n {n} s {s}")
    print(f"n {n} s {s} nv {nv}: the restatement's largest error / bound = {worst:.3g}")


def test_restated_covariance_against_numpy():
    r = np.random.default_rng(3)
    n, s, nv = 60, 7, 3
    rec = np.ones((n, s, 4))
    rec[..., 1:] = r.standard_normal((n, s, 3)) * np.array([1.0, 10.0, 0.1]) + 5.0 + r.standard_normal((n, 1, 3))
    X = rec[..., 1:].reshape(n, -1)
    want = np.cov(X, rowvar=False)
    shift = rec[..., 1:].mean(axis=0)
    for mode in (0, 1):                                           # complete data: both estimators are np.cov
        cov, ok = O.covariance(O.moments(rec, nv, shift), nv, mode, 2, n - 1)
        assert ok.all() and np.abs(cov - want).max() <= 1e-13 * np.abs(want).max()
        O.assert_bits(cov, cov.T, "symmetric")
    # without the shift the centring cancels: the same figures are worse by orders of magnitude (why the shift is in the interface)
    cov0, _ = O.covariance(O.moments(rec, nv, None), nv, 0, 2, n - 1)
    print(f"largest |cov - np.cov| / max|cov| without a shift: {np.abs(cov0 - want).max() / np.abs(want).max():.3g}")
    # pairwise deletion: every pair over the frames both have
    rec[..., 0] = r.random((n, s)) >= 0.25
    rec[:, 5, 0] = 0.0
    rec[3:, 6, 0] = 0.0                                           # three frames: below min_count 4 against most partners
    mom = O.moments(O.poison(rec, nv), nv, shift)
    cov, ok = O.covariance(mom, nv, 0, 4, None)
    for i in range(s):
        for j in range(s):
            both = (rec[:, i, 0] != 0) & (rec[:, j, 0] != 0)
            assert ok[i, j] == (both.sum() >= 4)
            blk = cov[3 * i:3 * i + 3, 3 * j:3 * j + 3]
            if not ok[i, j]:
                assert not blk.any()
                continue
            ref = np.cov(np.concatenate([rec[both, i, 1:], rec[both, j, 1:]], axis=1), rowvar=False)[:3, 3:]
            assert np.abs(blk - ref).max() <= 1e-12 * np.abs(want).max(), (i, j)
    assert not ok[5].any() and not ok[:, 5].any()
    # filled: the Gram matrix of the mean-filled data
    filled = np.where((rec[..., :1] != 0), rec[..., 1:], 0.0)
    cnt = (rec[..., 0] != 0).sum(axis=0)
    mean = filled.sum(axis=0) / np.maximum(cnt, 1)[:, None]
    Z = np.where(rec[..., :1] != 0, rec[..., 1:] - mean[None], 0.0).reshape(n, -1)
    cov, ok = O.covariance(mom, nv, 1, 2, n - 1)
    live = np.repeat(cnt >= 2, 3)
    ref = Z.T @ Z / (n - 1)
    assert np.abs(cov - ref)[np.ix_(live, live)].max() <= 1e-12 * np.abs(want).max()
    assert np.linalg.eigvalsh(cov).min() >= -1e-12 * np.abs(want).max()
    mask = np.ones(s, np.uint8)
    mask[2] = 0
    covm, okm = O.covariance(mom, nv, 1, 2, n - 1, mask)
    assert not okm[2].any() and not okm[:, 2].any() and not covm[6:9].any() and not covm[:, 6:9].any()
    keep = np.delete(np.arange(3 * s), [6, 7, 8])
    O.assert_bits(covm[np.ix_(keep, keep)], cov[np.ix_(keep, keep)], "a mask changes nothing else")


def test_restated_modes_against_eigh():
    """Adjacent eigenvalue ratio 0.25 (and a tail at most 0.25 of the last mode asked for): 48 iterations contract every wanted
    direction by 0.25^48 < 1e-28, so what is left is rounding.  The largest figure seen is what EIG_MEASURED records."""
    worst = np.zeros(3)
    for C_, r, k in O.EIG_CASES:
        A = O.eig_case(C_, r, k)
        values, modes, resid, info = O.leading_modes(A, r)
        assert info.tolist() == [r, 0] and np.all(np.diff(values) <= 0)
        assert np.abs(modes @ modes.T - np.eye(r)).max() < 1e-14
        at = np.argmax(np.abs(modes), axis=1)
        assert (modes[np.arange(r), at] > 0).all()
        e = O.eig_errors(A, values, modes, resid)
        print(f"C {C_} r {r}: errors {e}")
        worst = np.maximum(worst, e)
    # a repeated eigenvalue inside the block: only the subspace is compared
    for C_, lams, groups in O.EIG_REPEATED:
        A = O.spectrum_matrix(C_, lams, seed=C_)
        values, modes, resid, info = O.leading_modes(A, len(lams))
        e = O.eig_errors(A, values, modes, resid, groups)
        print(f"C {C_} repeated: errors {e}")
        worst = np.maximum(worst, e)
    # an indefinite matrix: the largest magnitudes, descending by value
    A = O.spectrum_matrix(40, [-4.0, 1.0, -0.25, 0.0625], seed=2)
    values, modes, resid, info = O.leading_modes(A, 4)
    assert np.allclose(values, [1.0, 0.0625, -0.25, -4.0], rtol=0, atol=1e-13)
    worst = np.maximum(worst, O.eig_errors(A, values, modes, resid))
    print(f"EIG_MEASURED: largest errors seen {worst}, recorded {O.EIG_MEASURED}")
    assert (worst <= np.array(O.EIG_MEASURED)).all() and O.EIG_TOL == tuple(10 * e for e in O.EIG_MEASURED)


def test_restated_modes_rank_deficient_and_the_tie_rule_of_the_sign():
    A = O.spectrum_matrix(20, [2.0, 0.5, 0.125], seed=1)
    values, modes, resid, info = O.leading_modes(A, 6)
    assert info.tolist() == [3, 3] and not modes[3:].any() and not values[3:].any() and not resid[3:].any()
    assert O.within_eig_tol(O.eig_errors(A, values[:3], modes[:3], resid[:3]))
    # an EXACT tie of the largest entry, with opposite signs, where the unflipped mode is negative at the smaller index: the
    # smaller index decides the sign
    q0 = O.start_block(600, 1)[:, 0]
    cases = O.tied_cases()
    assert [k for k, _, _ in cases] == ["one thread", "two lanes of a wave", "two waves", "second rows, two waves"]
    for kind, a_, b_ in cases + [("the first two", 0, 1)]:
        ta, tb = a_ % 256, b_ % 256
        if kind == "one thread":
            assert ta == tb
        elif kind == "two lanes of a wave":
            assert ta != tb and ta // 64 == tb // 64
        elif kind != "the first two":
            assert ta // 64 != tb // 64
        for r in (1, 2):                                          # r = 2: a second column that is dropped behind the mode
            values, modes, resid, info = O.leading_modes(O.tied_matrix(600, a_, b_), r, iters=3)
            assert values[0] == pytest.approx(2.0, abs=1e-15) and info.tolist() == [1, r - 1]
            assert modes[0, a_] == -modes[0, b_] and abs(modes[0, a_]) == np.abs(modes[0]).max()      # the tie is exact
            assert modes[0, a_] > 0, kind
            assert np.count_nonzero(modes[0]) == 2 and not modes[1:].any()
        if kind != "the first two":
            assert q0[a_] < q0[b_]                                # unflipped, the mode is negative at a: the rule had to act
    assert O.start_block(5, 3).shape == (5, 3) and np.abs(O.start_block(3072, 16)).max() < 1.0


def test_restated_scores_against_a_masked_einsum():
    r = np.random.default_rng(9)
    n, s, nv = 23, 70, 3
    rec = np.zeros((n, s, 5))
    rec[..., 0] = r.random((n, s)) >= 0.2
    rec[5, :, 0] = 0.0
    rec[..., 1:] = r.standard_normal((n, s, 4))
    B, _ = np.linalg.qr(r.standard_normal((s * nv, 6)))
    modes, center = np.ascontiguousarray(B.T), r.standard_normal(s * nv)
    sc, en = O.scores(O.poison(rec, nv), nv, center, modes, 0.5)
    num, den, e, mag, cnt = O.masked_scores(rec, nv, center, modes)
    g = float(2 * O.gamma(s * nv + 2))
    assert np.array_equal(en[:, 0], cnt) and np.abs(en[:, 1] - e).max() <= g * e.max()
    assert np.abs(sc[..., 2] - den).max() <= g
    seen = sc[..., 0] != 0
    assert np.array_equal(seen, sc[..., 2] >= 0.5) and not sc[5].any() and en[5].tolist() == [0.0, 0.0]
    assert np.abs(sc[..., 1] * sc[..., 2] - num)[seen].max() <= 2 * g * mag.max()
    assert not sc[..., 1][~seen].any()
    one, _ = O.scores(rec, nv, center, modes, 0.5, (7, 8))
    O.assert_bits(one[0], sc[7], "a frame alone")


def test_modes_helpers():
    cov = np.diag([4.0, 3.0, 2.0, 1.0, 0.0, 0.0])
    share, cum = MD.explained([4.0, 3.0], cov)
    assert share.tolist() == [0.4, 0.3] and cum.tolist() == [0.4, 0.7]
    assert np.isnan(MD.explained([1.0], np.zeros((2, 2)))[0]).all()
    modes = np.eye(6)[:2]
    rec = MD.mode_record(modes, 2, 3)
    assert rec.shape == (2, 2, 4) and rec[..., 0].all() and rec[0, 0, 1] == 1.0 and rec[1, 0, 2] == 1.0 and not rec[:, 1, 1:].any()
    assert MD.mode_record(modes, 2, 3, [1, 0])[..., 0].tolist() == [[1.0, 0.0], [1.0, 0.0]]
    lone, order = MD.loner_slots(cov, modes, [4.0, 3.0], 3)
    assert lone[0] == pytest.approx(2.0 / 9.0) and lone[1] == 1.0 and order.tolist() == [1, 0]
    for bad in (lambda: MD.mode_record(modes, 2, 2), lambda: MD.loner_slots(cov, modes, [1.0], 3), lambda: MD.explained([1.0], np.zeros(3))):
        with pytest.raises(ValueError):
            bad()


def test_the_end_to_end_thresholds_hold_on_the_restatement():
    """The thresholds tests/test_gpu_modes.py asserts on the device, on the restatement alone for the chosen seed."""
    sc = O.planted_scene()
    e = O.end_to_end(sc)
    print({k: (float(np.min(v)) if np.ndim(v) else v) for k, v in e.items() if k in ("cosines", "correlations", "share3", "planted_share")})
    assert (e["cosines"] >= 0.99).all() and (e["correlations"] >= 0.99).all()
    assert e["share3"] > e["planted_share"] and e["loner_top"] == sc["loner"]
