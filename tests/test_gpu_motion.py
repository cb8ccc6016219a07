"""GPU tests of the strain entries (k_motion.hip; run on the MI355X box: `pytest -m gpu`): `engine.motion_series_f64`,
`engine.local_strain_f64`, their composition with the contact-map entries, `pipeline.motion_analysis` and the sheet.

`grad`, `residual` and the `strain` columns flag .. e2 and worst are held BIT FOR BIT to the NumPy restatement
(`tests/helpers/motion_oracle.py`: the same IEEE operations in the same order); the columns that pass through sqrt / atan / atan2
last (max_shear .. rms_z) to 4 ulp, the two rms also within 4 ulp of the root of the restated quotient.  The local fit: everything
bit for bit but max_shear (4 ulp).  No entry is skipped or masked.  Shapes are the smallest at which the kernels can go wrong:
around the wave (64 slots), the workgroup and the frames a workgroup takes, not the workload's.
K = 1 admits no min_count (3 <= min_count <= K + 1), so it is held as a refusal; the smallest K that runs is 2."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from vbs_amd import _lib as L                                 # noqa: E402
from vbs_amd import engine as E                               # noqa: E402
from vbs_amd import fields as FL                              # noqa: E402
from vbs_amd import filters as F                              # noqa: E402
from vbs_amd import strain as ST                              # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import motion_oracle as O                                     # noqa: E402

G, GL = L.MOTION_GROUP, L.LSTRAIN_GROUP
SLOTS = (1, 2, 3, 4, 63, 64, 65, 128, 130, 441, 1024)


def frames_of(g):
    return sorted({1, 2, g - 1, g, g + 1, 2 * g + 3} - {0})


def motion(rec, pos, **kw):
    """`engine.motion_series_f64` -> a dict of host arrays."""
    return {k: v.cpu().numpy() for k, v in E.motion_series_f64(rec, pos, **kw).items()}


def local(rec, pos, nbr, **kw):
    return E.local_strain_f64(rec, pos, nbr, **kw).cpu().numpy()


def global_case(n, m, i):
    """The i-th content for a shape: 20 % dropouts, the last four frames with 3, 2, 1, 0 used slots, NaN / 1e30 in every cell that
    must not be read (dead entries, columns >= 4, the pos of unselected slots); cols, mask and reject_k rotate."""
    cols = (4, 5, 8)[i % 3]
    rec, pos = O.random_case(n, m, cols, 1000 * m + 10 * n + i, drop=0.2 if m > 4 or i % 2 else 0.0)
    mask = None
    if i % 4 == 3 and m > 1:
        mask = np.random.default_rng(i).random(m) < 0.7
        pos = pos.copy()
        pos[~mask] = (np.nan, 1e300)
    return rec, pos, mask, (0.0, 3.0, 1.0)[(i // 3) % 3]


@pytest.mark.parametrize("m", SLOTS)
def test_motion_series_equals_the_restatement_on_every_edge_shape(m):
    seen = set()
    for j, n in enumerate(frames_of(G)):
        i = SLOTS.index(m) + 5 * j                           # (content rotates through the shapes)
        rec, pos, mask, k = global_case(n, m, i)
        kw = {} if mask is None else {"slots": np.flatnonzero(mask)}
        got = motion(rec, pos, reject_k=k, **kw)
        what = f"m {m} n {n} cols {rec.shape[2]} k {k} mask {mask is not None}"
        O.check_motion(got, O.motion_series(rec, pos, mask, k), what)
        st = got["strain"]
        seen |= set(st[:, 0].tolist())
        assert set(st[:, 0].tolist()) <= {0.0, 1.0, 2.0} and (st[:, 2] <= st[:, 1]).all(), what
        if k == 0.0:
            assert (st[:, 0] != 2.0).all()                   # no rejection asked, none made
        if n >= 4:                                           # the last four frames: at most 3, 2, 1, 0 used slots
            assert (st[-4:, 1] <= [3, 2, 1, 0]).all() and (st[-3:, 3:15] == 0).all() and (st[-3:, 15] == -1).all(), what
            assert (got["grad"][-3:] == 0).all() and (got["residual"][-3:] == 0).all(), what
    print(f"m = {m}: flags seen {sorted(seen)}")
    assert 0.0 in seen and (m < 65 or {1.0, 2.0} <= seen)


def test_degenerate_positions_a_tie_and_null_outputs():
    """Exactly collinear and exactly coincident pos with integer data: det is exactly 0, no fit.  An exactly affine dyadic field:
    every q is 0, so `worst` is the first used slot.  Each output alone equals itself among the three."""
    rng = np.random.default_rng(5)
    m, n = 70, G + 1
    rec = O.record(rng.integers(-3, 4, (n, m, 3)).astype(np.float64))
    line = np.stack([np.arange(70.0), 2.0 * np.arange(70.0)], axis=1)
    for pts in (line, np.full((m, 2), 5.0)):
        for k in (0.0, 3.0):
            got = motion(rec, pts, reject_k=k)
            O.check_motion(got, O.motion_series(rec, pts, None, k), "degenerate")
            assert (got["strain"][:, 0] == 0).all() and (got["strain"][:, 1] == m).all() and (got["strain"][:, 15] == -1).all()
    pos = O.grid_pos(130, 2.0)
    Gm = np.array([[0.25, -0.5], [0.125, 0.0625], [-0.03125, 0.5]])
    d = np.broadcast_to((pos @ Gm.T + np.array([1.5, -0.75, 0.25]))[None], (3, 130, 3)).copy()
    rec = O.record(d, 5)
    rec[:, [0, 129], 0] = 0.0                                 # 128 used slots (exact means), of which the first is slot 1
    for k in (0.0, 2.0):
        got = motion(rec, pos, reject_k=k)
        O.check_motion(got, O.motion_series(rec, pos, None, k), "tie")
        assert (got["strain"][:, 0] == 1).all() and (got["strain"][:, 15] == 1).all()
    rec, pos = O.random_case(G + 2, 130, 4, 77)
    full = motion(rec, pos, reject_k=2.0)
    for w in ("grad", "strain", "residual"):
        one = motion(rec, pos, reject_k=2.0, want=(w,))
        assert list(one) == [w]
        O.assert_bits(one[w], full[w], f"{w} alone")


def corrupt(nbr, s, rng):
    """What a caller may hand in: -1 in the middle of a row, the entries s, -7 and 2^31 - 1, duplicates, and slot 0 and slot s - 1
    as each other's neighbours (across every wave and the whole workgroup)."""
    nb = nbr.astype(np.int64).copy()
    K = nb.shape[1]
    for r in range(s):
        c = int(rng.integers(0, K))
        kind = (r + int(rng.integers(0, 2))) % 6
        if kind < 4:
            nb[r, c] = (-1, s, -7, 2 ** 31 - 1)[kind]
        elif kind == 4 and K > 1:
            nb[r, c] = nb[r, (c + 1) % K]
    nb[0, K - 1], nb[s - 1, K - 1] = s - 1, 0
    return nb.astype(np.int32)


@pytest.mark.parametrize("m", SLOTS)
def test_local_strain_equals_the_restatement_on_every_edge_shape(m):
    results = 0
    for j, n in enumerate(frames_of(GL)):
        i = SLOTS.index(m) + 5 * j
        K = (2, 3, 6, 12)[i % 4]
        cols = (4, 5, 8)[i % 3]
        rec, pos = O.random_case(n, m, cols, 2000 * m + 10 * n + i, drop=0.2 if m > 4 else 0.0, thin=i % 2 == 0)
        rng = np.random.default_rng(i)
        nbr = corrupt(ST.neighbour_lists(pos, K), m, rng)
        mc, dr = (3, min(4, K + 1), K + 1)[i % 3], (0.01, 0.0, 0.3)[(i // 2) % 3]
        got = local(rec, pos, nbr, min_count=mc, det_rel=dr)
        want = O.local_strain(rec, pos, nbr, mc, dr)
        O.check_local(got, want, f"m {m} n {n} cols {cols} K {K} min_count {mc} det_rel {dr}")
        assert (got[rec[..., 0] == 0] == 0).all()            # self dead: no result
        results += int((got[..., 0] != 0).sum())
    print(f"m = {m}: {results} results")
    assert m < 4 or results > 0


def test_local_strain_edges_of_its_rules():
    """cnt exactly at min_count and one below; exactly collinear neighbourhoods with det_rel = 0; a dyadic neighbourhood whose
    det / (xx yy) sits exactly on det_rel (0.75: refused, the test is strict) and just above it; K = 1 admits no min_count."""
    pos = O.grid_pos(49, 1.0)
    rng = np.random.default_rng(2)
    rec = O.record(rng.normal(0.0, 0.1, (GL + 1, 49, 3)))
    nbr = ST.neighbour_lists(pos, 6)
    rec[1, nbr[24, :2], 0] = 0.0                              # slot 24 keeps 5 of its 7 members in frame 1, 4 in frame 2
    rec[2, nbr[24, :3], 0] = 0.0
    got = local(rec, pos, nbr, min_count=5, det_rel=0.01)
    O.check_local(got, O.local_strain(rec, pos, nbr, 5, 0.01), "min_count")
    assert got[0, 24, 0] == 7 and got[1, 24, 0] == 5 and (got[2, 24] == 0).all()
    line = np.stack([np.arange(49.0), 3.0 * np.arange(49.0)], axis=1)
    rec = O.record(rng.integers(-3, 4, (2, 49, 3)).astype(np.float64))
    nbl = ST.neighbour_lists(line, 4)
    got = local(rec, line, nbl, min_count=3, det_rel=0.0)
    O.check_local(got, O.local_strain(rec, line, nbl, 3, 0.0), "collinear")
    assert (got == 0).all()                                   # det is exactly 0: not > 0
    pts = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0]])
    nb8 = np.full((8, 7), -1, dtype=np.int32)
    nb8[0] = [1, 2, 3, 4, 5, 6, 7]                            # xx = yy = 8, xy = 4: det / (xx yy) = 48 / 64
    rec = O.record(rng.integers(-3, 4, (2, 8, 3)).astype(np.float64))
    for dr, has in ((0.75, False), (0.75 - 2.0 ** -53, True), (0.5, True)):
        got = local(rec, pts, nb8, min_count=8, det_rel=dr)
        O.check_local(got, O.local_strain(rec, pts, nb8, 8, dr), f"det_rel {dr!r}")
        assert (got[:, 0, 0] == (8 if has else 0)).all() and (got[:, 1:] == 0).all()
    with pytest.raises(ValueError):
        local(rec, pts, nb8[:, :1], min_count=3)
    with pytest.raises(ValueError):
        local(rec, pts, nb8[:, :1], min_count=2)


def test_bit_identical_under_every_change_of_batching():
    """Run to run, range by range against the whole, a frame alone against the same frame in a batch, dead slots appended, NumPy
    against tensor input, and s = 130 against the same 130 among 441 under a mask."""
    n, m = 2 * G + 3, 130
    rec, pos = O.random_case(n, m, 4, 31)
    nbr = ST.neighbour_lists(pos, 6)
    whole, lwhole = motion(rec, pos, reject_k=2.0), local(rec, pos, nbr)
    again, lagain = motion(torch.from_numpy(rec).cuda(), torch.from_numpy(pos).cuda(), reject_k=2.0), local(
        torch.from_numpy(rec).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(nbr).cuda())
    for w in whole:
        O.assert_bits(again[w], whole[w], f"run to run / tensor input: {w}")
    O.assert_bits(lagain, lwhole, "run to run / tensor input: local")
    assert {0.0, 1.0, 2.0} <= set(whole["strain"][:, 0].tolist())
    for a, b in ((0, 3), (3, G + 2), (G + 2, n), (5, 6), (n - 1, n), (4, 4)):
        part = motion(rec, pos, reject_k=2.0, frame_range=(a, b))
        for w in whole:
            O.assert_bits(part[w], whole[w][a:b], f"range {a}:{b}: {w}")
        O.assert_bits(local(rec, pos, nbr, frame_range=(a, b)), lwhole[a:b], f"range {a}:{b}: local")
    alone = motion(rec[5:6], pos, reject_k=2.0)
    for w in whole:
        O.assert_bits(alone[w], whole[w][5:6], f"a frame alone: {w}")
    O.assert_bits(local(rec[5:6], pos, nbr), lwhole[5:6], "a frame alone: local")
    big = np.zeros((n, 441, 4))
    big[:, :m] = rec
    big[:, m:, 1:] = np.nan                                   # dead slots appended: flag 0, never read
    bpos = np.concatenate([pos, np.full((441 - m, 2), 1e300)])
    bnbr = np.concatenate([nbr, np.full((441 - m, 6), -1, dtype=np.int32)])
    dead = motion(big, bpos, reject_k=2.0)
    O.assert_bits(dead["grad"], whole["grad"], "dead slots appended: grad")
    O.assert_bits(dead["strain"], whole["strain"], "dead slots appended: strain")
    O.assert_bits(dead["residual"][:, :m], whole["residual"], "dead slots appended: residual")
    assert (dead["residual"][:, m:] == 0).all()
    ldead = local(big, bpos, bnbr)
    O.assert_bits(ldead[:, :m], lwhole, "dead slots appended: local")
    assert (ldead[:, m:] == 0).all()
    big[:, m:] = O.random_case(n, 441 - m, 4, 32, thin=False)[0]          # live slots a mask leaves out
    masked = motion(big, bpos, reject_k=2.0, slots=np.arange(m))
    O.assert_bits(masked["grad"], whole["grad"], "130 among 441 under a mask: grad")
    O.assert_bits(masked["strain"], whole["strain"], "130 among 441 under a mask: strain")
    O.assert_bits(masked["residual"][:, :m], whole["residual"], "130 among 441 under a mask: residual")


def test_local_strain_composes_with_the_contact_map_entries():
    """A disc of 5 mm radius rotated by 5 degrees in a still 13 x 13 grid of markers: local strain -> `field_map_f64` with three
    values -> `patch_stats_f64` on max_shear.  The shear zone is the disc's rim: its centre lies within one cell of the map's
    grid of the disc's centre; the global fit's worst slot lies on the rim; with rejection the run stays deterministic."""
    centre = np.array([1.5, -1.5])
    rec, pos, inside = O.rotated_disc(13, 1.5, centre, 5.0, 5.0)
    nbr = ST.neighbour_lists(pos, 6)
    out = E.local_strain_f64(rec, pos, nbr)
    O.check_local(out.cpu().numpy(), O.local_strain(rec, pos, nbr), "disc")
    grid, _ = FL.grid_over(pos, (32, 32))
    W = FL.gaussian_weights(pos, grid, 1.5)
    mp = E.field_map_f64(out, W, n_values=3)
    patch = E.patch_stats_f64(mp, grid, component=2, threshold=1e-6).cpu().numpy()
    cell = float(grid[1, 0] - grid[0, 0])
    assert (patch[:, 0] == 2).all() and (np.abs(patch[:, 4:6] - centre) <= cell).all(), (patch[0], cell)
    assert (patch[1:] == patch[0]).all()
    sh = out.cpu().numpy()[0, :, 3]
    r = np.hypot(*(pos - centre).T)
    assert (sh[r > 5.0 + 3.1] == 0).all() and sh[(r > 3.5) & (r < 6.5)].max() > 0.01 and sh[r < 1.6].max() < 1e-12
    got = motion(rec, pos)
    O.check_motion(got, O.motion_series(rec, pos), "disc, global")
    worst = got["strain"][:, 15].astype(int)
    assert (worst == worst[0]).all() and inside[worst[0]] and r[worst[0]] > 5.0 - 1.5
    a, b = motion(rec, pos, reject_k=1.5), motion(rec, pos, reject_k=1.5)
    O.check_motion(a, O.motion_series(rec, pos, None, 1.5), "disc, rejection")
    for w in a:
        O.assert_bits(a[w], b[w], f"rejection, run to run: {w}")
    assert (a["strain"][:, 0] == 2).all()


def test_motion_analysis_end_to_end(tmp_path):
    """A float32 table in which the tool drags (t_X 0 -> 0.5 mm) and twists (0 -> 3 degrees): the trend follows both ramps within
    10 x what the restatement meets on the CPU (`motion_oracle.TREND_TOL_*`), every piece equals its restatement, and the sheet
    round-trips."""
    pytest.importorskip("pandas")
    from vbs_amd import pipeline as P
    from vbs_amd.engine import Engine
    t, pos, tx, th = O.drag_twist_table()
    taps = F.lowpass_taps(15, 0.2)
    eng = Engine(480, 640, max_markers=256, max_batch=2)
    try:
        res = P.motion_analysis(eng, torch.from_numpy(t).cuda(), taps=taps)
    finally:
        eng.close()
    host = {k: v.cpu().numpy() for k, v in res.items()}
    assert set(host) == {"axis", "total", "pos", "nbr", "grad", "strain", "residual", "local", "grad_filtered", "trend"}
    assert np.array_equal(host["pos"], pos) and np.array_equal(host["nbr"], ST.neighbour_lists(pos, 6))
    grad, strain, gf, trend = O.motion_analysis_cpu(t, taps)
    O.check_motion(host, O.motion_series(host["axis"], pos), "pipeline")
    O.check_local(host["local"], O.local_strain(host["axis"], pos, host["nbr"]), "pipeline, local")
    ok = host["trend"][:, 0] != 0
    assert ok.sum() >= 40 and np.array_equal(ok, trend[:, 0] != 0)
    assert np.array_equal(host["trend"][:, 1:], ST.invariants(np.where(ok[:, None, None], np.concatenate(
        [np.ones((48, 3, 1)), host["grad_filtered"][..., 1:4]], axis=2), 0.0)))
    rot, t_f = np.abs(host["trend"][ok, 7] - th[ok]).max(), np.abs(host["grad_filtered"][ok, 0, 1] - tx[ok]).max()
    print(f"trend: rot_deg off the ramp by {rot:.4f} deg, t_X by {t_f:.4f} mm")
    assert rot <= O.TREND_TOL_DEG and t_f <= O.TREND_TOL_MM
    df = P.to_motion_frame(res["strain"], res["grad"], res["trend"], path=str(tmp_path / "motion.xlsx"))
    assert tuple(df.columns) == P.MOTION_FRAME_COLUMNS + P.MOTION_TREND_COLUMNS and len(df) == 48
    assert np.array_equal(df["rot_deg"].to_numpy(), host["strain"][:, 9]) and np.array_equal(df["tX"].to_numpy(), host["grad"][:, 0, 1])
    assert np.array_equal(df["rot_deg_f"].to_numpy()[ok], host["trend"][ok, 7]) and os.path.getsize(tmp_path / "motion.xlsx") > 0
