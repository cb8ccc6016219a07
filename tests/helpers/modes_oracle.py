"""Restatements of the modal analysis (include/vbs.h), NumPy and exact rational arithmetic only:
  - `moments`: the cross moments as loops over the frames in ascending order (an order, not THE order: the device's is not part of
    its interface), `exact_moments` the same sums of the ROUNDED z as rationals with the sums of magnitudes the bound is made of;
  - `covariance`: the two expressions as written;
  - `leading_modes`, `scores`: the same operations in the same order as the kernels (their order IS the interface).
EIG_MEASURED is what the restatement of the eigen part was seen to reach against `np.linalg.eigh` on the cases of
tests/test_modes_host.py; EIG_TOL = 10 x that by the project's standing rule."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
MR, THREADS, SWEEPS = 16, 256, 10
# the largest seen of: |value - eigh| / lambda_1; the sine of the subspace angle in units of u lambda_1 / gap (`eig_errors`);
# resid / lambda_1
EIG_MEASURED = (8.9e-16, 9.3, 3.5e-16)
EIG_TOL = tuple(10 * e for e in EIG_MEASURED)


def gamma(k):
    return k * U / (1 - k * U)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {got[i]!r} != {want[i]!r}")


def poison(rec, n_values, kind=np.nan):
    """A copy of rec with `kind` in every cell that must not be read: the values of invalid entries, every column beyond n_values."""
    out = np.array(rec, dtype=np.float64, copy=True)
    dead = out[..., 0] == 0.0
    out[..., 1:][dead] = kind
    out[..., 1 + n_values:] = kind
    return out


def dyadic_case(n, s, cols, n_values, seed, drop=0.2, kind=1e300):
    """rec [n, s, cols] and shift [s, n_values]: multiples of 2^-8 below 2^8 with a dyadic shift: every z, product and partial sum
    of up to 2^20 frames is representable, so every order of summation is exact."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.integers(-2 ** 16 + 1, 2 ** 16, (n, s, cols - 1)) / 256.0
    shift = r.integers(-2 ** 10, 2 ** 10, (s, n_values)) / 256.0
    return (rec if kind is None else poison(rec, n_values, kind)), shift


def random_case(n, s, cols, n_values, seed, drop=0.2, kind=np.nan):
    """The same shapes with float content: values of mixed sign over six decades, the means as the shift."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, s, cols))
    rec[..., 0] = (r.random((n, s)) >= drop).astype(np.float64)
    rec[..., 1:] = r.standard_normal((n, s, cols - 1)) * 10.0 ** r.uniform(-3, 3, (n, s, cols - 1))
    shift = r.standard_normal((s, n_values))
    return (rec if kind is None else poison(rec, n_values, kind)), shift


# ---- 1. cross moments -----------------------------------------------------------------------------------------------------------
def staged(rec, n_values, shift=None):
    """-> col [n, s, 4]: (z1, z2, z3, flag as 1.0 / 0.0) per frame and slot, z = x - shift rounded once, SELECTED: an invalid entry
    and a column beyond n_values are 0.0 whatever the record holds there."""
    rec = np.asarray(rec, dtype=np.float64)
    n, s, _ = rec.shape
    valid = rec[..., 0] != 0.0
    col = np.zeros((n, s, 4))
    for v in range(n_values):
        x = np.where(valid, rec[..., 1 + v], 0.0)
        z = x - (0.0 if shift is None else np.asarray(shift, np.float64)[None, :, v])
        col[..., v] = np.where(valid, z, 0.0)
    col[..., 3] = valid.astype(np.float64)
    return col


def moments(rec, n_values, shift=None):
    """mom [s, s, 4, 4]: for every frame in ascending order, mom[i, j, v, w] += col_v(i) * col_w(j), the product rounded, then
    the sum - the loops, with the cells of a frame taken at once."""
    col = staged(rec, n_values, shift)
    n, s, _ = col.shape
    mom = np.zeros((s, s, 4, 4))
    for f in range(n):
        mom = mom + col[f][:, None, :, None] * col[f][None, :, None, :]
    return mom


def exact_moments(rec, n_values, shift=None):
    """-> (value, mag) [s, s, 4, 4] of Fractions: the exact sums of col_v(i) col_w(j) of the ROUNDED z, and of their magnitudes."""
    col = staged(rec, n_values, shift)
    n, s, _ = col.shape
    F = [[[Fraction(float(col[f, i, v])) for v in range(4)] for i in range(s)] for f in range(n)]
    value = np.empty((s, s, 4, 4), dtype=object)
    mag = np.empty((s, s, 4, 4), dtype=object)
    for i in range(s):
        for j in range(s):
            for v in range(4):
                for w in range(4):
                    tv, tm = Fraction(0), Fraction(0)
                    for f in range(n):
                        p = F[f][i][v] * F[f][j][w]
                        tv += p
                        tm += abs(p)
                    value[i, j, v, w], mag[i, j, v, w] = tv, tm
    return value, mag


def check_within_bound(got, rec, n_values, shift=None, what=""):
    """Every entry of `got` against `exact_moments` within gamma_(n+6) * (sum of magnitudes); where the bound is zero the entry
    is an exact zero.  No entry is skipped.  Returns the largest error / bound ratio seen (a float, to print)."""
    value, mag = exact_moments(rec, n_values, shift)
    g_ = gamma(np.asarray(rec).shape[0] + 6)
    got = np.asarray(got)
    assert got.shape == value.shape, f"{what}: shape {got.shape} != {value.shape}"
    worst = 0.0
    for idx in np.ndindex(*value.shape):
        g = got[idx]
        assert np.isfinite(g), f"{what}: entry {idx} is {g}"
        err, lim = abs(Fraction(float(g)) - value[idx]), g_ * mag[idx]
        assert err <= lim, f"{what}: entry {idx}: error {float(err):.3e} above the bound {float(lim):.3e}"
        if lim > 0:
            worst = max(worst, float(err / lim))
    return worst


# ---- 2. covariance --------------------------------------------------------------------------------------------------------------
def covariance(mom, n_values, mode, min_count=2, denom=None, slot_mask=None):
    """-> (cov [C, C], ok uint8 [s, s]): the expressions of include/vbs.h as written, for (i, v) <= (j, w), mirrored."""
    mom = np.asarray(mom, dtype=np.float64)
    s, nv = mom.shape[0], n_values
    C = s * nv
    cov = np.zeros((C, C))
    ok = np.zeros((s, s), dtype=np.uint8)
    need = np.float64(min_count)
    den = None if denom is None else np.float64(denom)
    with np.errstate(all="ignore"):
        for i in range(s):
            for j in range(i, s):
                P = mom[i, j]
                N = P[3, 3]
                good = bool(N >= need) and (slot_mask is None or (slot_mask[i] != 0 and slot_mask[j] != 0))
                ok[i, j] = ok[j, i] = 1 if good else 0
                for v in range(nv):
                    for w in range(nv):
                        if i == j and v > w:
                            continue
                        c = np.float64(0.0)
                        if good:
                            S, a, b = P[v, w], P[v, 3], P[3, w]
                            if mode == 0:
                                c = (S - (a * b) / N) / (N - np.float64(1.0))
                            else:
                                mi = mom[i, i, v, 3] / mom[i, i, 3, 3]
                                mj = mom[j, j, w, 3] / mom[j, j, 3, 3]
                                c = (S - mi * b - mj * a + N * (mi * mj)) / den
                        cov[i * nv + v, j * nv + w] = c
                        cov[j * nv + w, i * nv + v] = c
    return cov, ok


# ---- 3. leading modes -----------------------------------------------------------------------------------------------------------
def _fold64(a):
    """a [64, ...] -> the fold a[i] + a[i + 32], then + 16, 8, 4, 2, 1."""
    for off in (32, 16, 8, 4, 2, 1):
        a = a[:off] + a[off:2 * off]
    return a[0]


def lane_sums(terms):
    """terms [C, ...] -> the sum over C by the wave rule: lane l adds terms l, l + 64, .. ascending from 0.0, then the fold."""
    C = terms.shape[0]
    acc = np.zeros((64,) + terms.shape[1:])
    for base in range(0, C, 64):
        blk = terms[base:base + 64]
        acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk
    return _fold64(acc)


def block_sums(terms):
    """terms [C, ...] -> the sum over C by the workgroup rule: thread t of 256 adds terms t, t + 256, .. ascending from 0.0, every
    wave folds its 64 sums, the wave sums are added ((W0 + W1) + W2) + W3."""
    C = terms.shape[0]
    acc = np.zeros((THREADS,) + terms.shape[1:])
    for base in range(0, C, THREADS):
        blk = terms[base:base + THREADS]
        acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk
    W = [_fold64(acc[64 * w:64 * w + 64]) for w in range(4)]
    return ((W[0] + W[1]) + W[2]) + W[3]


def start_block(C, r):
    x = (np.arange(C, dtype=np.uint64)[:, None] * MR + np.arange(r, dtype=np.uint64)[None, :] + 1).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x.view(np.int32).astype(np.float64) * 2.0 ** -31


def apply(A, Q):
    return lane_sums(A.T[:, :, None] * Q[:, None, :])              # terms[c, row, k] = A[row, c] * Q[c, k]


def orth(X, tiny):
    """-> (the block orthonormalised, columns dropped): twice modified Gram-Schmidt, row-oriented, as include/vbs.h states it."""
    X = X.copy()
    r = X.shape[1]
    big = np.float64(0.0)
    for j in range(r):
        nn = block_sums(X[:, j] * X[:, j])
        big = nn if nn > big else big
    dropped = 0
    for rnd in range(2):
        for j in range(r):
            S = block_sums(X[:, j, None] * X[:, j:])
            nn = S[0]
            keep = bool(nn > tiny * big) if rnd == 0 else bool(nn > 0.0)
            if not keep:
                dropped += rnd == 0
                X[:, j] = 0.0
                continue
            nrm = np.sqrt(nn)
            X[:, j] = X[:, j] / nrm
            for k in range(j + 1, r):
                X[:, k] = X[:, k] - (S[k - j] / nrm) * X[:, j]
    return X, dropped


def jacobi(T):
    """Cyclic Jacobi on the symmetric T [r, r]: -> (diagonal, V), in the fixed pair order for SWEEPS sweeps."""
    T = T.copy()
    r = T.shape[0]
    V = np.eye(r)
    one = np.float64(1.0)
    with np.errstate(over="ignore"):
        for _ in range(SWEEPS):
            for p in range(r - 1):
                for q in range(p + 1, r):
                    apq = T[p, q]
                    if apq == 0.0:
                        continue
                    theta = (T[q, q] - T[p, p]) / (np.float64(2.0) * apq)
                    t = (-one if theta < 0.0 else one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    x, y = T[:, p].copy(), T[:, q].copy()
                    T[:, p], T[:, q] = c * x - s * y, s * x + c * y
                    x, y = T[p, :].copy(), T[q, :].copy()
                    T[p, :], T[q, :] = c * x - s * y, s * x + c * y
                    x, y = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * x - s * y, s * x + c * y
                    T[p, q] = T[q, p] = 0.0
    return np.diag(T).copy(), V


def leading_modes(A, r, iters=48, tiny=1e-24):
    """-> (values [r], modes [r, C], resid [r], info [2]) by the operations of vbs_leading_modes_f64 in their order."""
    A = np.asarray(A, dtype=np.float64)
    C = A.shape[0]
    Q, dropped = orth(start_block(C, r), tiny)
    for _ in range(iters):
        Q, dropped = orth(apply(A, Q), tiny)
    Y = apply(A, Q)
    T = np.zeros((r, r))
    for k in range(r):
        S = block_sums(Q[:, k, None] * Y[:, k:])
        T[k, k:] = S
        T[k:, k] = S
    d, V = jacobi(T)
    perm = np.argsort(-d, kind="stable")
    lam = d[perm]
    Uu, AU = np.zeros((C, r)), np.zeros((C, r))
    for l in range(r):
        Uu = Uu + Q[:, l, None] * V[l, perm][None, :]
        AU = AU + Y[:, l, None] * V[l, perm][None, :]
    D = AU - lam[None, :] * Uu
    resid = np.sqrt(block_sums(D * D))
    at = np.argmax(np.abs(Uu), axis=0)                             # the first of equal maxima
    neg = Uu[at, np.arange(r)] < 0.0
    modes = np.where(neg[:, None], -Uu.T, Uu.T)
    return lam, np.ascontiguousarray(modes), resid, np.array([r - dropped, dropped], dtype=np.int32)


# C, r, the number of nonzero eigenvalues 3 * 0.25^k: every C around the 64 lanes and the 256 threads' first row, r = 1, 2, 16, C
EIG_CASES = ((1, 1, 1), (2, 2, 2), (2, 1, 2), (16, 16, 16), (16, 2, 6), (17, 16, 17), (63, 16, 20), (63, 1, 5), (65, 2, 11), (65, 16, 18),
             (390, 16, 20), (390, 6, 9))
EIG_REPEATED = ((30, (4.0, 1.0, 1.0, 0.25), ((0,), (1, 2), (3,))), (65, (8.0, 2.0, 0.5, 0.5, 0.5, 0.125), ((0,), (1,), (2, 3, 4), (5,))))


def eig_case(C, r, k):
    return spectrum_matrix(C, 3.0 * 0.25 ** np.arange(k), seed=1000 * C + r)


def spectrum_matrix(C, lams, seed, return_basis=False):
    """A symmetric [C, C] with the eigenvalues `lams` (the rest 0) on known orthonormal modes (QR of a seeded Gaussian block)."""
    r = np.random.default_rng(seed)
    B, _ = np.linalg.qr(r.standard_normal((C, C)))
    lam = np.zeros(C)
    lam[:len(lams)] = lams
    A = (B * lam[None, :]) @ B.T
    A = 0.5 * (A + A.T)
    return (A, B) if return_basis else A


def subspace_sine(Ua, Ub):
    """The sine of the largest principal angle between the row spaces of Ua and Ub (orthonormal rows, the same count)."""
    return float(np.linalg.svd(Ua - (Ua @ Ub.T) @ Ub, compute_uv=False).max())     # what of Ua lies outside the span of Ub


def eig_errors(A, values, modes, resid, groups=None):
    """The three figures EIG_TOL bounds, against np.linalg.eigh of A taken by largest magnitude: |value - eigh| / lambda_1; the
    sine of the subspace angle (per group of equal eigenvalues in `groups` = lists of mode indices; default every mode alone)
    IN UNITS OF u lambda_1 / gap, gap the distance of the group's eigenvalues to the nearest eigenvalue outside it - a vector is
    only determined to about that, by eigh as by the iteration, so the figure is of order one at r = 1 and at r = 16 alike and one
    tolerance holds every case as tightly as its own conditioning allows; and resid / lambda_1.  -> the three of them."""
    w, Vv = np.linalg.eigh(A)
    order = np.argsort(-np.abs(w), kind="stable")[:len(values)]
    order = order[np.argsort(-w[order], kind="stable")]
    l1 = np.abs(w[order]).max()
    sine = 0.0
    for g in ([list(g) for g in groups] if groups else [[k] for k in range(len(values))]):
        inside = order[g]
        outside = np.setdiff1d(np.arange(w.size), inside)
        if outside.size == 0:                                     # the group is the whole space: nothing to be turned towards
            continue
        gap = float(np.abs(w[inside][:, None] - w[outside][None, :]).min())
        sine = max(sine, subspace_sine(modes[g], Vv[:, inside].T) / (float(U) * l1 / gap))
    return np.array([float(np.abs(values - w[order]).max() / l1), sine, float(np.abs(resid).max() / l1)])


def tied_matrix(C, a, b):
    """A[a][a] = A[b][b] = 1, A[a][b] = A[b][a] = -1, the rest 0: row b is the exact negation of row a, so after the first apply
    u[b] == -u[a] bit for bit - the one mode (value 2) has an EXACT tie of its two largest entries, with opposite signs."""
    A = np.zeros((C, C))
    A[a, a] = A[b, b] = 1.0
    A[a, b] = A[b, a] = -1.0
    return A


def tied_cases(C=600):
    """(kind, a, b), a < b, for the tie rule of the sign: both rows of ONE thread (b = a + 256: the strict > inside a thread), two
    lanes of one wave (the fold's tie test), two waves (the same test across the wave results) and two waves of different threads'
    second rows; each pair chosen so that the start block has Q0[a] < Q0[b], i.e. the UNFLIPPED mode is negative at the smaller
    index (y[a] = Q0[a] - Q0[b], and the value 2 > 0 keeps that sign): a rule that took the larger index would leave it negative."""
    q0 = start_block(C, 1)[:, 0]
    out = []
    for kind, base, step in (("one thread", 5, 256), ("two lanes of a wave", 70, 1), ("two waves", 20, 130), ("second rows, two waves", 300, 150)):
        a = base
        while not q0[a] < q0[a + step]:
            a += 1
        out.append((kind, a, a + step))
    return out


def within_eig_tol(errors):
    return bool((np.asarray(errors) <= np.asarray(EIG_TOL)).all())


# ---- 4. scores ------------------------------------------------------------------------------------------------------------------
def scores(rec, n_values, center, modes, min_coverage=0.5, frame_range=None):
    """-> (scores [b-a, r, 3], energy [b-a, 2]) as vbs_mode_scores_f64 states them: the lane sums over the valid columns."""
    rec = np.asarray(rec, dtype=np.float64)
    modes = np.asarray(modes, dtype=np.float64)
    n, s, _ = rec.shape
    nv, r = n_values, modes.shape[0]
    a, b = (0, n) if frame_range is None else frame_range
    sc, en = np.zeros((b - a, r, 3)), np.zeros((b - a, 2))
    mc = np.float64(min_coverage)
    for f in range(a, b):
        valid = np.repeat(rec[f, :, 0] != 0.0, nv)
        x = np.where(valid, rec[f, :, 1:1 + nv].reshape(-1), 0.0)
        d = np.where(valid, x - center, 0.0)
        u = np.where(valid[None, :], modes, 0.0)
        num, den = lane_sums((d[None, :] * u).T), lane_sums((u * u).T)
        en[f - a] = lane_sums(valid.astype(np.float64)), lane_sums(d * d)
        with np.errstate(divide="ignore", invalid="ignore"):
            seen = den >= mc
            sc[f - a, :, 0] = seen
            sc[f - a, :, 1] = np.where(seen, num / den, 0.0)
            sc[f - a, :, 2] = den
    return sc, en


def masked_scores(rec, n_values, center, modes):
    """The independent side of 4: a masked einsum, with the sums of magnitudes its summation bound is made of.
    -> (num, den, e, |num| terms, count) per frame."""
    rec = np.asarray(rec, dtype=np.float64)
    n, s, _ = rec.shape
    valid = np.repeat(rec[..., 0] != 0.0, n_values, axis=1)
    x = np.where(valid, np.where(valid, rec[..., 1:1 + n_values].reshape(n, -1), 0.0) - center[None, :], 0.0)
    num = np.einsum("fc,kc->fk", x, modes)
    den = np.einsum("fc,kc->fk", valid.astype(np.float64), modes * modes)
    mag = np.einsum("fc,kc->fk", np.abs(x), np.abs(modes))
    return num, den, np.einsum("fc,fc->f", x, x), mag, valid.sum(axis=1)


# ---- the end-to-end scene -------------------------------------------------------------------------------------------------------
def planted_scene(seed=5, side=13, n=200, missing=0.03, noise=0.002):
    """The end-to-end scene as a float64 displacement [n, M = side^2, 3] with its parts (`table_from` makes the tracked table of
    it): a press (a Gaussian dimple in Z), a drag in X and a torsion about the centre, each with its own time course, amplitudes
    4 : 2 : 1 in standard deviation (16 : 4 : 1 in variance), plus noise; one marker with an independent random walk on top;
    `missing` of the entries not seen.  -> dict."""
    r = np.random.default_rng(seed)
    g = np.arange(side, dtype=np.float64) - (side - 1) / 2
    gx, gy = np.meshgrid(g, g, indexing="xy")
    pos = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)
    M = side * side
    dimple_at = np.array([2.0, -1.0])
    press = np.zeros((M, 3))
    press[:, 2] = -np.exp(-((pos[:, 0] - dimple_at[0]) ** 2 + (pos[:, 1] - dimple_at[1]) ** 2) / (2 * 2.5 ** 2))
    drag = np.zeros((M, 3))
    drag[:, 0] = 1.0
    tors = np.zeros((M, 3))
    tors[:, 0], tors[:, 1] = -pos[:, 1], pos[:, 0]
    pats = [p / np.linalg.norm(p) for p in (press, drag, tors)]
    t = np.arange(n, dtype=np.float64)
    courses = [np.sin(2 * np.pi * t / 97.0), np.sign(np.sin(2 * np.pi * t / 41.0 + 0.3)) * 1.0, np.cos(2 * np.pi * t / 23.0 + 1.0)]
    courses = [c - c.mean() for c in courses]
    courses = [c / c.std() for c in courses]
    amps = (4.0, 2.0, 1.0)
    disp = sum(a * c[:, None, None] * p[None] for a, c, p in zip(amps, courses, pats))
    signal_var = float((disp ** 2).sum() / n)
    disp = disp + noise * r.standard_normal(disp.shape)
    loner = 17
    disp[:, loner, :] += np.cumsum(0.03 * r.standard_normal((n, 3)), axis=0)
    valid = r.random((n, M)) >= missing
    valid[0] = True                                               # the reference frame
    return {"disp": disp, "valid": valid, "pos": pos, "patterns": pats, "courses": courses, "amps": amps, "loner": loner,
            "dimple_at": dimple_at, "noise_var": 3 * M * noise ** 2, "signal_var": signal_var, "side": side}


def table_from(scene):
    """The scene as a tracked table float32 [n, M, 10]: flag 3 (tracked, with XYZ) where the marker is seen, X, Y, Z in cols 6 .. 8."""
    disp, valid, pos = scene["disp"], scene["valid"], scene["pos"]
    n, M = valid.shape
    t = np.zeros((n, M, 10), dtype=np.float32)
    t[..., 0] = np.where(valid, 3.0, 0.0)
    t[..., 6:8] = (pos[None] + disp[..., :2]).astype(np.float32)
    t[..., 8] = disp[..., 2].astype(np.float32)
    return t


def judge(scene, values, modes, sc, cov):
    """What the end-to-end test asserts, from the values [r], modes [r, 3 M], scores [n, r, 3] and cov of a run (r >= 3): the
    |cosine| of every planted pattern with its best mode among the three leading ones, the |correlation| of that mode's score with
    the planted time course over the flagged frames, the explained share of three modes against the planted signal's minus the
    noise's, and the slot on top of `loner_slots`.  The planted share is the variance `cov` itself holds along the three planted
    patterns (orthonormal by construction) over its trace: no three orthonormal directions hold more than the three leading
    eigenvectors (Ky Fan), so a solver that has converged exceeds it, and one that has not found the subspace does not."""
    from vbs_amd import modes as MD
    pats = np.stack([p.reshape(-1) for p in scene["patterns"]])
    cos = np.abs(pats @ modes[:3].T)                               # [pattern, mode]
    best = cos.argmax(axis=1)
    corr = []
    for k, b in enumerate(best):
        ok = sc[:, b, 0] != 0
        corr.append(abs(np.corrcoef(sc[ok, b, 1], scene["courses"][k][ok])[0, 1]))
    tr = float(np.trace(cov))
    share, cum = MD.explained(values, cov)
    _, order = MD.loner_slots(cov, modes[:3], values[:3], 3)
    return {"cosines": cos.max(axis=1), "best": best, "correlations": np.array(corr), "share3": float(cum[2]),
            "planted_share": (float(np.einsum("kc,cd,kd->", pats, cov, pats)) - scene["noise_var"]) / tr, "loner_top": int(order[0])}


def end_to_end(scene, r=3, iters=48):
    """The whole analysis on the restatements: -> `judge`'s dict, with the values, modes, scores and cov it was made of."""
    t = table_from(scene)
    valid = ((t[..., 0].astype(np.int64) & 2) != 0)
    valid = valid & valid[0][None]
    d = np.where(valid[..., None], t[..., 6:9].astype(np.float64) - t[0, :, 6:9].astype(np.float64)[None], 0.0)
    rec = np.concatenate([valid.astype(np.float64)[..., None], d], axis=2)
    n = rec.shape[0]
    cnt = valid.sum(axis=0)
    shift = d.sum(axis=0) / np.maximum(cnt, 1)[:, None]
    mom = moments(rec, 3, shift)
    cov, _ = covariance(mom, 3, 1, 2, n - 1)
    values, modes, resid, info = leading_modes(cov, r, iters)
    dg = mom[np.arange(mom.shape[0]), np.arange(mom.shape[0])]
    center = shift + dg[:, :3, 3] / np.maximum(dg[:, 3, 3:4], 1.0)
    sc, en = scores(rec, 3, center.reshape(-1), modes, 0.5)
    out = judge(scene, values, modes, sc, cov)
    out.update(values=values, modes=modes, scores=sc, cov=cov, resid=resid, rec=rec)
    return out
