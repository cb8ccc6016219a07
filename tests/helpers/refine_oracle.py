"""The rule of `vbs_refine_markers` restated from include/vbs.h in NumPy and Python integers (never from the kernel): `refine_row`
is the restatement the GPU tests hold the kernel to, `refine_row_brute` a second form of the same rule - quartiles from `np.sort`,
sums from Python integers over an explicit pixel list - that the host tests hold the first one to."""
import math

import numpy as np

COLS, SUM_COLS, TABLE_COLS, MAX_R = 12, 8, 10, 63
DEFAULTS = {"core_f": 0.5, "disc_f": 1.5, "ring_f": 2.0, "min_contrast": 16.0, "max_shift_f": 1.0, "polarity": 0,
            "keep_unrefined": 0}
PI = 3.14159265358979323846
ROOTED = (3, 4, 5, 6, 10, 11)          # rec columns that end in a root or an arc tangent: held to 4 ulp, the others bit for bit


def geometry(Cx, Cy, major, h, w, core_f=0.5, disc_f=1.5, ring_f=2.0):
    """-> (status, x0, y0, R, c2, g2) of a TRACKED row (status 0, 2, 3 or 4), every step in float64 as the header states it."""
    Cx, Cy, major = float(np.float32(Cx)), float(np.float32(Cy)), float(np.float32(major))
    if not (math.isfinite(Cx) and math.isfinite(Cy) and math.isfinite(major)) or major < 2.0 or abs(Cx) >= 2.0 ** 30 \
            or abs(Cy) >= 2.0 ** 30:
        return 2, 0, 0, 0, 0, 0
    r = 0.5 * major
    if math.ceil(ring_f * r) + 1.0 > MAX_R:
        return 3, 0, 0, 0, 0, 0
    x0, y0 = int(math.floor(Cx + 0.5)), int(math.floor(Cy + 0.5))
    R = int(math.ceil(ring_f * r)) + 1
    cr, gr = core_f * r, disc_f * r
    c2, g2 = int(math.floor(cr * cr)), int(math.floor(gr * gr))
    if x0 - R < 0 or x0 + R > w - 1 or y0 - R < 0 or y0 + R > h - 1:
        return 4, x0, y0, R, c2, g2
    return 0, x0, y0, R, c2, g2


def trimmed8(levels):
    """T8 of a set of levels (a 1-D integer array, not empty) through its histogram."""
    H = np.bincount(np.asarray(levels, dtype=np.int64), minlength=256)
    cum, total = np.cumsum(H), int(H.sum())
    q1 = int(np.argmax(cum * 4 >= total))
    q3 = int(np.argmax(cum * 4 >= total * 3))
    v = np.arange(q1, q3 + 1)
    return int(8 * int((v * H[q1:q3 + 1]).sum()) // int(H[q1:q3 + 1].sum()))


def trimmed8_sorted(levels):
    """The same T8 from the sorted list: q(num) is the element at 0-based index ceil(total num / 4) - 1."""
    s = np.sort(np.asarray(levels, dtype=np.int64))
    n = len(s)
    q1, q3 = int(s[-(-n // 4) - 1]), int(s[-(-3 * n // 4) - 1])
    kept = [int(x) for x in s if q1 <= x <= q3]
    return (8 * sum(kept)) // len(kept)


def tail(S, C8, B8, D8, x0, y0, Cx, Cy, r, max_shift_f):
    """Step 5: the float64 tail from the integer sums -> (status, rec row)."""
    o = [0.0] * COLS
    o[8], o[9] = B8 / 8.0, D8 / 8.0
    S0, Sx, Sy, Sxx, Sxy, Syy = (int(v) for v in S)
    A = float(S0) / float(C8)
    d_area = 2.0 * math.sqrt(A / PI)
    o[6], o[7] = d_area, A
    if S0 <= 0:
        return 6, o
    s0 = float(S0)
    cx, cy = float(x0) + float(Sx) / s0, float(y0) + float(Sy) / s0
    shift = math.hypot(cx - Cx, cy - Cy)
    o[1], o[2], o[11] = cx, cy, shift
    den = s0 * s0
    mxx = float(Sxx * S0 - Sx * Sx) / den
    mxy = float(Sxy * S0 - Sx * Sy) / den
    myy = float(Syy * S0 - Sy * Sy) / den
    t, hd = 0.5 * (mxx + myy), 0.5 * (mxx - myy)
    q = math.sqrt(hd * hd + mxy * mxy)
    l1, l2 = t + q, t - q
    if not l2 > 0.0:
        return 6, o
    k = math.sqrt(math.sqrt(l1 / l2))
    o[3], o[4] = d_area * k, d_area / k
    o[5] = (0.5 * math.atan2(2.0 * mxy, mxx - myy)) * 180.0 / PI + 180.0
    o[10] = math.sqrt(l1 * l2) - A / (4.0 * PI)
    return (7 if shift > max_shift_f * r else 0), o


def refine_row(gray, row, **params):
    """One table row on one gray frame [h, w] -> (rec [COLS] float64, sums [SUM_COLS] Python ints, table_out [TABLE_COLS] float32)."""
    p = {**DEFAULTS, **params}
    row = np.asarray(row, dtype=np.float32)
    h, w = gray.shape
    rec, sums = [0.0] * COLS, [0] * SUM_COLS
    f0 = float(row[0])
    flags = int(f0) if 0.0 <= f0 < 2.0 ** 24 else 0
    if not flags & 1:
        status = 1
    else:
        status, x0, y0, R, c2, g2 = geometry(row[1], row[2], row[3], h, w, p["core_f"], p["disc_f"], p["ring_f"])
    if status == 0:
        Cx, Cy, r = float(row[1]), float(row[2]), 0.5 * float(row[3])
        win = gray[y0 - R:y0 + R + 1, x0 - R:x0 + R + 1].astype(np.int64)
        if p["polarity"]:
            win = 255 - win
        d = np.arange(-R, R + 1, dtype=np.int64)
        dx, dy = np.meshgrid(d, d)
        d2 = dx * dx + dy * dy
        B8, D8 = trimmed8(win[(d2 > g2) & (d2 <= R * R)]), trimmed8(win[d2 <= c2])
        C8 = B8 - D8
        sums[0], sums[1] = B8, D8
        if float(C8) < 8.0 * p["min_contrast"]:
            status = 5
            rec[8], rec[9] = B8 / 8.0, D8 / 8.0
        else:
            disc = d2 <= g2
            wgt = np.minimum(np.maximum(B8 - 8 * win, 0), C8)[disc]
            x, y = dx[disc], dy[disc]
            S = [int(wgt.sum()), int((wgt * x).sum()), int((wgt * y).sum()), int((wgt * x * x).sum()), int((wgt * x * y).sum()),
                 int((wgt * y * y).sum())]
            sums[2:] = S
            status, rec = tail(S, C8, B8, D8, x0, y0, Cx, Cy, r, p["max_shift_f"])
    rec[0] = float(status)
    out = np.zeros(TABLE_COLS, dtype=np.float32)
    out[9] = row[9]
    if status == 0:
        out[0] = 1.0
        out[1:6] = np.asarray(rec[1:6], dtype=np.float64).astype(np.float32)
    elif p["keep_unrefined"] and status >= 2:
        out[0] = np.float32(flags & ~2)
        out[1:6] = row[1:6]
    return np.asarray(rec, dtype=np.float64), sums, out


def refine_row_brute(gray, row, **params):
    """The second form: an explicit pixel list, `np.sort` quartiles, Python-integer sums.  Tracked rows only -> (status, sums)."""
    p = {**DEFAULTS, **params}
    row = np.asarray(row, dtype=np.float32)
    h, w = gray.shape
    status, x0, y0, R, c2, g2 = geometry(row[1], row[2], row[3], h, w, p["core_f"], p["disc_f"], p["ring_f"])
    if status:
        return status, [0] * SUM_COLS
    px = []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            v = int(gray[y0 + dy, x0 + dx])
            px.append((dx, dy, dx * dx + dy * dy, 255 - v if p["polarity"] else v))
    B8 = trimmed8_sorted([v for _, _, d2, v in px if g2 < d2 <= R * R])
    D8 = trimmed8_sorted([v for _, _, d2, v in px if d2 <= c2])
    C8 = B8 - D8
    if C8 < 8 * p["min_contrast"]:
        return 5, [B8, D8, 0, 0, 0, 0, 0, 0]
    S = [0] * 6
    for dx, dy, d2, v in px:
        if d2 <= g2:
            wgt = min(max(B8 - 8 * v, 0), C8)
            for i, f in enumerate((1, dx, dy, dx * dx, dx * dy, dy * dy)):
                S[i] += wgt * f
    status, _ = tail(S, C8, B8, D8, x0, y0, float(row[1]), float(row[2]), 0.5 * float(row[3]), p["max_shift_f"])
    return status, [B8, D8] + S


def refine(gray, table, **params):
    """Frames [n, h, w] and a table [n, m, TABLE_COLS] -> rec float64 [n, m, COLS], sums int64 [n, m, SUM_COLS], table_out."""
    gray, table = np.asarray(gray), np.asarray(table, dtype=np.float32)
    n, m = table.shape[:2]
    rec = np.zeros((n, m, COLS), dtype=np.float64)
    sums = np.zeros((n, m, SUM_COLS), dtype=np.int64)
    out = np.zeros((n, m, TABLE_COLS), dtype=np.float32)
    for f in range(n):
        for s in range(m):
            rec[f, s], sm, out[f, s] = refine_row(gray[f], table[f, s], **params)
            sums[f, s] = sm
    return rec, sums, out


def ulp_diff(a, b):
    """The distance of two float64 arrays in units in the last place (equal signs assumed; both zero: 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def check(got_rec, got_sums, got_table, want, what=""):
    """Hold a device result to the restatement: sums and status exactly, the rooted rec columns to 4 ulp, the others bit for bit,
    table_out bit for bit GIVEN the device's own rec (each column cast to float32 once)."""
    rec, sums, table = want
    assert np.array_equal(got_sums, sums), f"{what}: sums differ at {np.argwhere(got_sums != sums)[:4].tolist()}"
    assert np.array_equal(got_rec[..., 0], rec[..., 0]), f"{what}: status {got_rec[..., 0].tolist()} != {rec[..., 0].tolist()}"
    for c in range(1, COLS):
        if c in ROOTED:
            d = ulp_diff(got_rec[..., c], rec[..., c])
            assert d.max(initial=0) <= 4, f"{what}: rec column {c} off by {int(d.max())} ulp"
        else:
            assert np.array_equal(got_rec[..., c].view(np.int64), rec[..., c].view(np.int64)), f"{what}: rec column {c}"
    expect = table.copy()
    ok = got_rec[..., 0] == 0
    expect[ok, 1:6] = got_rec[ok, 1:6].astype(np.float32)
    assert np.array_equal(got_table.view(np.int32), expect.view(np.int32)), f"{what}: table_out"
