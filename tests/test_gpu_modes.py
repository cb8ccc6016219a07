"""GPU tests of the modal analysis (k_modes.hip; run on the MI355X box: `pytest -m gpu`): `engine.cross_moments_f64`,
`engine.covariance_f64`, `engine.leading_modes_f64`, `engine.mode_scores_f64`, `pipeline.modal_analysis` and the sheet.

The moments' order of summation is not part of their interface (the order inside the float64 matrix instruction is not
documented), so they are held three ways (`tests/helpers/modes_oracle.py`): BIT FOR BIT to the loop restatement where every order
is exact (dyadic inputs) - which is what catches a wrong lane map, tile pair or mirror -, within the DERIVED bound gamma_(n+6) *
sum |col col| of exact rational arithmetic on float content, and bit for bit to THEMSELVES under every change of batching.  The
covariance, the eigen part and the scores have a stated order and are held bit for bit to their restatements; the eigen part also
to `np.linalg.eigh` within EIG_TOL.  No entry is skipped or masked.  Shapes are the smallest at which a kernel can go
wrong: around the 16-frame step, the VBS_MOM_CHUNK frames of a chunk and its double buffer, the 4 slots of a column tile and the
VBS_MOM_WG_SLOTS of a tile pair, the 64 lanes and 256 threads of the sums; not the workload's."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import filter_oracle as FO                                    # noqa: E402
import modes_oracle as O                                      # noqa: E402

FRAMES = (1, 15, 16, 17, 63, 64, 65, 129, 200)
SLOTS = (1, 3, 4, 5, 15, 16, 17, 33, 130)
BUDGET = 300000                                               # frames x s^2 x 16 of the exact side (rational arithmetic)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mom(rec, nv=None, shift=None):
    from vbs_amd.engine import cross_moments_f64
    return cross_moments_f64(dev(rec), None if shift is None else dev(shift), nv).cpu().numpy()


def shape_of(n, k=0, budget=None):
    """The k-th shape for a frame count: s, cols, n_values rotate through their lists; with `budget`, s shrinks until the exact
    side's work stays below it."""
    i = FRAMES.index(n)
    s = SLOTS[(2 * i + 4 * k + 1) % len(SLOTS)]
    nv = 1 + (i + k) % 3
    cols = nv + 1 + (i + 2 * k) % (8 - nv)
    if budget:
        while n * s * s * 16 > budget and s > 1:
            s = SLOTS[SLOTS.index(s) - 1]
    return s, cols, nv


_met = [shape_of(n, k) for n in FRAMES for k in range(3)]
assert {m[0] for m in _met} == set(SLOTS) and {m[2] for m in _met} == {1, 2, 3} and {m[1] for m in _met} == set(range(2, 9))


@pytest.mark.parametrize("n", FRAMES)
def test_dyadic_moments_equal_the_loops_bit_for_bit(n):
    for k in range(3):
        s, cols, nv = shape_of(n, k)
        rec, shift = O.dyadic_case(n, s, cols, nv, seed=100 * n + k)
        if s > 1:
            rec[:, -1, 0] = 0.0                                  # a slot that is never valid
        if n > 1:
            rec[1, :, 0] = 0.0                                   # an all-invalid frame
        sh = shift if k != 1 else None
        want = O.moments(rec, nv, sh)
        got = mom(rec, nv, sh)
        O.assert_bits(got, want, f"n {n} s {s} cols {cols} nv {nv}")
        O.assert_bits(got, got.transpose(1, 0, 3, 2), "mom[i, j, v, w] and mom[j, i, w, v] are the same bits")
        valid = rec[..., 0] != 0
        assert np.array_equal(got[..., 3, 3], (valid[:, :, None] & valid[:, None, :]).sum(axis=0))     # the pair counts, exact
        if s > 1:
            assert not got[-1].any() and not got[:, -1].any()
        assert not got[:, :, nv:3, :].any() and not got[:, :, :, nv:3].any()


@pytest.mark.parametrize("n", (17, 65))
def test_dyadic_moments_on_every_slot_count(n):
    for j, s in enumerate(SLOTS):
        nv = 1 + j % 3
        rec, shift = O.dyadic_case(n, s, 4, nv, seed=1000 + s)
        O.assert_bits(mom(rec, nv, shift), O.moments(rec, nv, shift), f"n {n} s {s} nv {nv}")


@pytest.mark.parametrize("n", FRAMES)
def test_random_moments_lie_within_the_derived_bound(n):
    s, cols, nv = shape_of(n, 1, budget=BUDGET)
    rec, shift = O.random_case(n, s, cols, nv, seed=7000 + n, kind=None)
    if s > 1:
        rec[:, -1, 0] = 0.0
    got = mom(O.poison(rec, nv, np.nan), nv, shift)
    worst = O.check_within_bound(got, rec, nv, shift, what=f"n {n} s {s} nv {nv}")
    print(f"n {n} s {s} cols {cols} nv {nv}: largest error / bound = {worst:.3g}")
    O.assert_bits(got, got.transpose(1, 0, 3, 2), "mirror bits")
    assert np.array_equal(got[..., 3, 3], np.rint(got[..., 3, 3]))
    for kind in (1e300, -np.inf):                                # NaN and 1e300 in every cell that must not be read change no bit
        O.assert_bits(mom(O.poison(rec, nv, kind), nv, shift), got, f"n {n}: poison {kind}")
    O.assert_bits(mom(rec, nv, shift), got, f"n {n}: ordinary numbers in the cells that are not read")


@pytest.mark.parametrize("kind", ("all", "none", "one"))
def test_validity_kinds(kind):
    for n, s, nv in ((65, 5, 3), (129, 33, 2), (40, 1, 1)):
        rec, shift = O.dyadic_case(n, s, nv + 2, nv, seed=n + s, kind=None)
        rec[..., 0] = {"all": 1.0, "none": 0.0}.get(kind, rec[..., 0])
        if kind == "one":
            rec[:, s // 2, 0] = 0.0
        rec = O.poison(rec, nv, np.nan)
        got = mom(rec, nv, shift)
        O.assert_bits(got, O.moments(rec, nv, shift), f"{kind}: n {n} s {s}")
        if kind == "all":
            assert (got[..., 3, 3] == n).all()
        if kind == "none":
            assert not got.any()
        if kind == "one":
            assert not got[s // 2].any() and not got[:, s // 2].any()


def test_moments_are_bit_identical_under_every_change_of_batching():
    n, s, nv = 200, 130, 3
    rec, shift = O.random_case(n, s, 5, nv, seed=11)
    full = mom(rec, nv, shift)
    O.assert_bits(mom(rec, nv, shift), full, "run to run")
    from vbs_amd.engine import cross_moments_f64
    O.assert_bits(cross_moments_f64(rec, shift, nv).cpu().numpy(), full, "array against tensor input")
    for a, b in ((0, 1), (3, 129), (17, 16), (64, 65), (100, 100)):                 # a pair alone against the same pair among 130
        pick = [a, b] if a != b else [a]
        alone = mom(rec[:, pick], nv, shift[pick])
        O.assert_bits(alone, full[np.ix_(pick, pick)], f"slots {pick} alone")
    dead = np.concatenate([rec, np.full((n, 7, 5), np.nan)], axis=1)
    dead[:, s:, 0] = 0.0
    got = mom(dead, nv, np.concatenate([shift, np.full((7, nv), 1e300)]))
    O.assert_bits(got[:s, :s], full, "dead slots appended")
    assert not got[s:].any() and not got[:, s:].any()
    for extra in (1, 31, 32, 70):                                                    # into the chunk, to its end, past two more
        tail = np.full((extra, s, 5), np.nan)
        tail[..., 0] = 0.0
        O.assert_bits(mom(np.concatenate([rec, tail]), nv, shift), full, f"{extra} dead frames appended")


def cov_of(m, nv, mode, min_count=2, denom=None, mask=None):
    from vbs_amd.engine import covariance_f64
    cov, ok = covariance_f64(dev(m), nv, mode, min_count, denom, None if mask is None else dev(mask), want_ok=True)
    return cov.cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("n,s,nv", ((65, 17, 3), (200, 130, 2), (16, 1, 1), (40, 33, 3)))
def test_covariance_equals_the_expressions_bit_for_bit_on_the_device_moments(n, s, nv):
    rec, shift = O.random_case(n, s, nv + 1, nv, seed=n + s, drop=0.3)
    if s > 2:
        rec[:, 1, 0] = 0.0
        rec[3:, 2, 0] = 0.0                                      # three frames
    m = mom(rec, nv, shift)
    mask = (np.arange(s) % 5 != 3).astype(np.uint8)
    for mode, mc, denom, mk in ((0, 2, None, None), (0, 4, None, mask), (1, 2, float(n - 1), None), (1, 5, 7.5, mask)):
        cov, ok = cov_of(m, nv, mode, mc, denom, mk)
        wc, wok = O.covariance(m, nv, mode, mc, denom, mk)
        O.assert_bits(cov, wc, f"mode {mode} min_count {mc}")
        assert np.array_equal(ok, wok)
        O.assert_bits(cov, cov.T, "symmetric bits")


def test_covariance_rules_on_hand_built_moments():
    s, nv = 4, 2
    m = np.zeros((s, s, 4, 4))
    r = np.random.default_rng(0)
    for i in range(s):
        for j in range(i, s):
            blk = r.integers(-64, 65, (4, 4)) / 8.0
            if i == j:
                blk = blk + blk.T
            m[i, j], m[j, i] = blk, blk.T
    N = np.array([[9.0, 5.0, 4.0, 1.0], [5.0, 8.0, 5.0, 6.0], [4.0, 5.0, 7.0, 0.0], [1.0, 6.0, 0.0, 6.0]])
    m[..., 3, 3] = N
    for mode, denom in ((0, None), (1, 8.0)):
        cov, ok = cov_of(m, nv, mode, 5, denom)                   # N at min_count (5), one below (4), N = 1, N = 0
        O.assert_bits(cov, O.covariance(m, nv, mode, 5, denom)[0], f"hand-built, mode {mode}")
        assert np.array_equal(ok, (N >= 5).astype(np.uint8))
        for i in range(s):
            for j in range(s):
                blk = cov[2 * i:2 * i + 2, 2 * j:2 * j + 2]
                assert (not blk.any()) if N[i, j] < 5 else np.isfinite(blk).all()
        cov2, ok2 = cov_of(m, nv, mode, 2, denom)                 # N = 1 in mode 0: not ok, so N - 1 = 0 never divides
        assert ok2[0, 3] == 0 and not cov2[0:2, 6:8].any() and np.isfinite(cov2).all()
        mask = np.array([1, 0, 1, 1], np.uint8)
        covm, okm = cov_of(m, nv, mode, 2, denom, mask)
        O.assert_bits(covm, O.covariance(m, nv, mode, 2, denom, mask)[0], "masked")
        assert not okm[1].any() and not okm[:, 1].any() and not covm[2:4].any() and not covm[:, 2:4].any()


def lead(A, r, iters=48, tiny=1e-24):
    from vbs_amd.engine import leading_modes_f64
    return tuple(t.cpu().numpy() for t in leading_modes_f64(dev(A), r, iters, tiny))


def check_modes(A, r, what, groups=None, iters=48):
    """The device against the restatement on the same A: every bit of values, modes and resid, and `info` (the builder found every
    bit equal on every case here, so that is what is asserted); and both within EIG_TOL of np.linalg.eigh."""
    values, modes, resid, info = lead(A, r, iters)
    wv, wm, wr, wi = O.leading_modes(A, r, iters)
    assert info.tolist() == wi.tolist(), what
    O.assert_bits(values, wv, f"{what}: values")
    O.assert_bits(modes, wm, f"{what}: modes")
    O.assert_bits(resid, wr, f"{what}: resid")
    live = modes.any(axis=1)                                       # (a dropped column's zero row sorts in by its value 0: not always last)
    assert int(live.sum()) == int(info[0]) and not values[~live].any() and not resid[~live].any(), what
    e = O.eig_errors(A, values[live], modes[live], resid[live], groups)
    print(f"{what}: errors against eigh {e}, EIG_TOL {O.EIG_TOL}")
    assert O.within_eig_tol(e), what
    return values, modes, resid, info


@pytest.mark.parametrize("case", O.EIG_CASES, ids=lambda c: f"C{c[0]}-r{c[1]}")
def test_modes_equal_the_restatement_and_eigh(case):
    C_, r, k = case
    values, modes, resid, info = check_modes(O.eig_case(C_, r, k), r, f"C {C_} r {r}")
    assert info.tolist() == [r, 0] and np.all(np.diff(values) <= 0)
    at = np.argmax(np.abs(modes), axis=1)
    assert (modes[np.arange(r), at] > 0).all()                    # the sign rule


def test_modes_repeated_rank_deficient_indefinite_tied_and_run_to_run():
    # (the tie cases are modes_oracle.tied_cases, checked on the restatement in tests/test_modes_host.py)
    for C_, lams, groups in O.EIG_REPEATED:                       # a repeated eigenvalue inside the block: the subspace
        check_modes(O.spectrum_matrix(C_, lams, seed=C_), len(lams), f"C {C_} repeated", groups)
    A = O.spectrum_matrix(20, [2.0, 0.5, 0.125], seed=1)          # rank 3, r = 6: three dropped columns, zeros behind
    values, modes, resid, info = check_modes(A, 6, "rank 3")
    assert info.tolist() == [3, 3] and not modes[3:].any() and not values[3:].any() and not resid[3:].any()
    A = O.spectrum_matrix(40, [-4.0, 1.0, -0.25, 0.0625], seed=2)  # indefinite: the largest magnitudes, descending by value
    values = check_modes(A, 4, "indefinite")[0]
    assert np.allclose(values, [1.0, 0.0625, -0.25, -4.0], rtol=0, atol=1e-13)
    A = O.spectrum_matrix(20, [1.0, -2.0], seed=3)                # indefinite AND rank-deficient: the dropped column's value 0 and
    values, modes, resid, info = check_modes(A, 3, "indefinite, rank 2")    # zero mode sort BETWEEN the positive and the negative one
    assert info.tolist() == [2, 1] and values[0] > 0 and values[1] == 0 and values[2] < 0 and not modes[1].any() and resid[1] == 0
    # an EXACT tie of the largest entry with opposite signs, unflipped negative at the smaller index: both rows in one thread, in
    # two lanes of a wave, in two waves - the strict > of a thread, the fold's tie test, the same test across the wave results
    q0 = O.start_block(600, 1)[:, 0]
    for kind, a_, b_ in O.tied_cases() + [("the first two", 0, 1)]:
        for r in (1, 2):
            A = O.tied_matrix(600, a_, b_)
            values, modes, resid, info = lead(A, r, 3)
            wv, wm, wr, wi = O.leading_modes(A, r, 3)
            O.assert_bits(modes, wm, f"tied, {kind}: modes")
            O.assert_bits(values, wv, f"tied, {kind}: values")
            O.assert_bits(resid, wr, f"tied, {kind}: resid")
            assert info.tolist() == wi.tolist() == [1, r - 1]
            assert modes[0, a_] == -modes[0, b_] and abs(modes[0, a_]) == np.abs(modes[0]).max(), kind       # the tie is exact
            assert modes[0, a_] > 0, f"{kind}: the smaller index of the tied entries must be the positive one"
        assert kind == "the first two" or q0[a_] < q0[b_]         # unflipped, the mode is negative at a: the rule had to act
    B = np.zeros((3, 3))
    B[0, 0], B[1, 1], B[2, 2] = 1.0, 1.0, 0.5                     # modes e0, e1 exactly? whatever comes: device == restatement
    O.assert_bits(lead(B, 2, 8)[1], O.leading_modes(B, 2, 8)[1], "a diagonal matrix with a repeated value")
    A = O.eig_case(390, 16, 20)
    first, again = lead(A, 16), lead(A, 16)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    from vbs_amd.engine import leading_modes_f64
    work = torch.full((2 * 390 * 16 + 5,), float("nan"), dtype=torch.float64, device="cuda")
    O.assert_bits(leading_modes_f64(A, 16, work=work)[1].cpu().numpy(), first[1], "array input, a caller's workspace full of NaN")


def sco(rec, center, modes, nv, mc=0.5, rng=None, energy=True):
    from vbs_amd.engine import mode_scores_f64
    s, e = mode_scores_f64(dev(rec), dev(center), dev(modes), nv, mc, rng, energy)
    return s.cpu().numpy(), (e.cpu().numpy() if energy else None)


@pytest.mark.parametrize("n,s,nv,r", ((23, 70, 3, 6), (9, 1, 1, 1), (17, 22, 2, 16), (8, 130, 3, 3), (1, 21, 3, 2)))
def test_scores_equal_the_restatement_bit_for_bit(n, s, nv, r):
    rg = np.random.default_rng(n + s)
    rec = np.zeros((n, s, nv + 2))
    rec[..., 0] = rg.random((n, s)) >= 0.2
    if n > 5:
        rec[5, :, 0] = 0.0                                       # a frame with nothing valid
    rec[..., 1:] = rg.standard_normal((n, s, nv + 1))
    rec = O.poison(rec, nv, np.nan)
    B, _ = np.linalg.qr(rg.standard_normal((s * nv, r)))
    modes, center = np.ascontiguousarray(B.T), rg.standard_normal(s * nv)
    got, en = sco(rec, center, modes, nv)
    want, wen = O.scores(rec, nv, center, modes, 0.5)
    O.assert_bits(got, want, "scores")
    O.assert_bits(en, wen, "energy")
    if n > 5:
        assert not got[5].any() and not en[5].any()
    for a, b in ((0, n), (n // 2, n // 2 + 1), (n - 1, n), (2, 2)):  # a frame alone against a range
        part, pen = sco(rec, center, modes, nv, rng=(min(a, n), min(b, n)))
        O.assert_bits(part, got[min(a, n):min(b, n)], f"range {a}, {b}")
        O.assert_bits(pen, en[min(a, n):min(b, n)], f"range {a}, {b}: energy")
    O.assert_bits(sco(rec, center, modes, nv, energy=False)[0], got, "without the energy")


def test_scores_coverage_at_its_edge():
    s, nv = 6, 1
    modes = np.zeros((2, 6))
    modes[0, :4] = 0.5                                            # den = 0.25 per seen column: exact
    modes[1, 4:] = np.sqrt(0.5)
    rec = np.ones((3, s, 2))
    rec[..., 1] = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] * 3
    rec[1, 2:4, 0] = 0.0                                          # frame 1: half of mode 0 is seen, den == 0.5 exactly
    rec[2, :, 0] = 0.0
    center = np.zeros(6)
    for mc, flag in ((0.5, 1.0), (np.nextafter(0.5, 0.0), 1.0), (np.nextafter(0.5, 1.0), 0.0)):
        got, _ = sco(rec, center, modes, nv, float(mc))
        O.assert_bits(got, O.scores(rec, nv, center, modes, mc)[0], f"min_coverage {mc!r}")
        assert got[1, 0].tolist() == ([1.0, 3.0, 0.5] if flag else [0.0, 0.0, 0.5]) and got[0, 0].tolist() == [1.0, 5.0, 1.0]
        assert not got[2].any()


def test_the_scores_are_a_record_the_filter_takes():
    from vbs_amd.engine import fir_series_f64
    rg = np.random.default_rng(4)
    n, s, nv, r = 60, 9, 3, 4
    rec = np.zeros((n, s, 4))
    rec[..., 0] = rg.random((n, s)) >= 0.4
    rec[..., 1:] = rg.standard_normal((n, s, 3))
    B, _ = np.linalg.qr(rg.standard_normal((s * nv, r)))
    modes, center = np.ascontiguousarray(B.T), np.zeros(s * nv)
    want, _ = O.scores(rec, nv, center, modes, 0.5)
    assert 0 < (want[..., 0] == 0).sum() < want[..., 0].size     # some scores are gaps
    half = np.array([1.0, 0.75, 0.5, 0.25])
    from vbs_amd.engine import mode_scores_f64
    got = fir_series_f64(mode_scores_f64(dev(rec), dev(center), dev(modes), nv)[0], FO.full_taps(half), 1).cpu().numpy()
    O.assert_bits(got, FO.fir(want, half, 1), "fir_series_f64 of the scores record")


def test_wrappers_refuse_what_the_entries_refuse():
    from vbs_amd.engine import covariance_f64, cross_moments_f64, leading_modes_f64, mode_scores_f64
    rec, shift = O.dyadic_case(12, 3, 4, 3, seed=1)
    assert cross_moments_f64(rec).shape == (3, 3, 4, 4) and cross_moments_f64(rec, shift[:, :1], n_values=1).shape == (3, 3, 4, 4)
    for bad in (dict(n_values=4), dict(n_values=0), dict(shift=shift[:2]), dict(shift=shift, n_values=2)):
        with pytest.raises(ValueError):
            cross_moments_f64(rec, **bad)
    with pytest.raises(L.VbsError, match=f"VBS_MOM_MAX_SLOTS = {L.MOM_MAX_SLOTS}"):
        cross_moments_f64(np.zeros((2, L.MOM_MAX_SLOTS + 1, 2)))
    m = cross_moments_f64(rec, shift)
    assert covariance_f64(m, 3, denom=11.0).shape == (9, 9) and covariance_f64(m, 2, "pairwise").shape == (6, 6)
    for bad in (dict(mode="filled"), dict(mode="x", denom=1.0), dict(denom=1.0, min_count=1), dict(denom=1.0, slot_mask=[1, 1])):
        with pytest.raises(ValueError):
            covariance_f64(m, 3, **bad)
    A = covariance_f64(m, 3, denom=11.0)
    for bad in (dict(n_modes=0), dict(n_modes=10), dict(n_modes=17), dict(n_modes=3, iters=-1), dict(n_modes=3, tiny=1.0),
                dict(n_modes=3, work=torch.zeros(10, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError):
            leading_modes_f64(A, **bad)
    values, md, resid, info = leading_modes_f64(A, 3)
    assert mode_scores_f64(rec, np.zeros(9), md)[0].shape == (12, 3, 3) and mode_scores_f64(rec, np.zeros(9), md, frame_range=(3, 7))[1].shape == (4, 2)
    for bad in (dict(min_coverage=0.0), dict(frame_range=(0, 13)), dict(n_values=2)):
        with pytest.raises(ValueError):
            mode_scores_f64(rec, np.zeros(9), md, **bad)


def test_modal_analysis_finds_the_planted_modes():
    """13 x 13 markers, 200 frames, 3 % missing: a press, a drag and a torsion, 16 : 4 : 1 in variance, noise, and one marker on a
    random walk.  The thresholds were checked on the restatement alone (tests/test_modes_host.py) before they were fixed."""
    from vbs_amd import fields
    from vbs_amd import pipeline as PL
    from vbs_amd.engine import Engine, patch_stats_f64
    sc = O.planted_scene()
    t = O.table_from(sc)
    n, m = t.shape[:2]
    nodes = sc["pos"]
    grid_xy, _ = fields.grid_over(nodes, (25, 25), 0.0)          # a grid point every half marker spacing
    W = fields.gaussian_weights(nodes, grid_xy, 0.75)
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        taps = FO.full_taps(np.array([1.0, 0.75, 0.5, 0.25]))
        res = PL.modal_analysis(eng, torch.from_numpy(t).cuda(), n_modes=3, taps=taps, grid=(W, fields.row_sums(W)))
        values, modes, scores = res["values"], res["modes"].reshape(3, -1), res["scores"].cpu().numpy()
        cov = res["cov"].cpu().numpy()
        assert res["modes"].shape == (3, m, 3) and scores.shape == (n, 3, 3) and res["energy"].shape == (n, 2) and cov.shape == (3 * m, 3 * m)
        assert res["info"].tolist() == [3, 0] and (res["resid"] <= 1e-9 * values[0]).all()
        e = O.judge(sc, values, modes, scores, cov)
        print({k: v for k, v in e.items()}, "explained", res["explained"], "resid", res["resid"])
        assert (e["cosines"] >= 0.99).all() and sorted(e["best"].tolist()) == [0, 1, 2]
        assert (e["correlations"] >= 0.99).all()
        assert e["share3"] > e["planted_share"] and res["cumulative"][2] == pytest.approx(e["share3"])
        assert e["loner_top"] == sc["loner"] == int(res["loner_order"][0])
        # the device against the whole restatement on the same series
        series = res["series"].cpu().numpy()
        ref = O.end_to_end(sc)
        O.assert_bits(series, ref["rec"], "the series is the axis displacement")
        rc = res["reconstructed"]
        # (under gaps the seen parts of two modes are not orthogonal: the sum may pass one by about the share of gaps)
        assert rc.shape == (n,) and np.nanmin(rc) > 0.9 and np.nanmax(rc) < 1.05
        # the press mode's map centres on the dimple
        press = int(e["best"][0])
        maps = res["mode_maps"]
        assert tuple(maps.shape) == (3, 625, 4)
        sign = -1.0 if modes[press].reshape(m, 3)[np.argmax(np.abs(modes[press].reshape(m, 3)[:, 2])), 2] < 0 else 1.0
        patch = patch_stats_f64(maps, grid_xy, 2, sign, 0.5 * float(np.abs(maps[press, :, 3].cpu().numpy()).max())).cpu().numpy()
        centre = patch[press, 4:6]
        print(f"press mode {press}: patch centre {centre}, the dimple at {sc['dimple_at']}")
        assert patch[press, 0] == 2.0 and np.abs(centre - sc["dimple_at"]).max() <= 0.5 + 1e-9      # within one grid cell
        assert tuple(res["scores_trend"].shape) == (n, 3, 3)
        df = PL.to_mode_frame(res, frame_offset=10)
        assert tuple(df.columns) == PL.MODE_FRAME_COLUMNS and len(df) == 3 * n and df["frameno"].iloc[0] == 11 and df["mode"].iloc[2] == 3
        assert np.array_equal(df["score"].to_numpy().reshape(n, 3), np.where(scores[..., 0] != 0, scores[..., 1], np.nan), equal_nan=True)
        with pytest.raises(ValueError):
            PL.modal_analysis(eng, torch.from_numpy(t).cuda(), n_modes=17)
        pw = PL.modal_analysis(eng, torch.from_numpy(t).cuda(), n_modes=3, mode="pairwise", slot_mask=(np.arange(m) != sc["loner"]))
        assert not pw["modes"][:, sc["loner"]].any() and pw["cumulative"][2] > 0.999      # unbiased pair by pair: the gaps cost nothing
    finally:
        eng.close()
