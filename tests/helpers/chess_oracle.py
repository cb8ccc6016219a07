"""Sequential NumPy statement of the chessboard corner stage (csrc/k_chess.hip), one function per kernel: the yardstick of
tests/test_chess_host.py and tests/test_gpu_chess.py.  cv2 cannot be installed here, so `find_chessboard_corners` is a
restatement (a ChESS response, a lattice search) and `corner_subpix` is cv2.cornerSubPix restated from its published source.

Every decision of the response, the candidates and the ordering is integer arithmetic, so the device must agree EXACTLY; the
sub-pixel step is float64 and differs from the device only in the order of its five sums."""
import numpy as np

MAX_CANDIDATES = 256
MAX_PATTERN = 256
MAX_WIN = 15
STRENGTH_RATIO = 8
RING = ((0, 5), (2, 5), (3, 3), (5, 2), (5, 0), (5, -2), (3, -3), (2, -5), (0, -5), (-2, -5), (-3, -3), (-5, -2), (-5, 0),
        (-5, 2), (-3, 3), (-2, 5))
NEG = np.iinfo(np.int32).min                 # "minus infinity": pixels nearer than 5 to an edge, and everything outside
FINDER_SUBPIX = dict(win=(2, 2), zero_zone=(-1, -1), max_iter=15, eps=0.1)


def response(gray):
    """int32 [H,W]: R = 5 (SR - DR) - |5 sum(ring) - 16 L| where it is defined, NEG elsewhere."""
    g = np.asarray(gray).astype(np.int32)
    h, w = g.shape
    out = np.full((h, w), NEG, dtype=np.int32)
    if h < 11 or w < 11:
        return out
    ring = [g[5 + dy:h - 5 + dy, 5 + dx:w - 5 + dx] for dx, dy in RING]
    sr = sum(np.abs((ring[n] + ring[n + 8]) - (ring[n + 4] + ring[n + 12])) for n in range(4))
    dr = sum(np.abs(ring[n] - ring[n + 8]) for n in range(8))
    tot = sum(ring)
    loc = g[5:h - 5, 5:w - 5] + g[4:h - 6, 5:w - 5] + g[6:h - 4, 5:w - 5] + g[5:h - 5, 4:w - 6] + g[5:h - 5, 6:w - 4]
    out[5:h - 5, 5:w - 5] = 5 * (sr - dr) - np.abs(5 * tot - 16 * loc)
    return out


def candidates(resp):
    """(x, y, R) int64 [M,3] in row-major order: R > 0, >= all of its 9x9 neighbourhood, > those before it in row-major order."""
    r = np.asarray(resp, dtype=np.int64)
    h, w = r.shape
    pad = np.full((h + 8, w + 8), NEG, dtype=np.int64)
    pad[4:-4, 4:-4] = r
    ok = r > 0
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = pad[4 + dy:4 + dy + h, 4 + dx:4 + dx + w]
            ok &= (r > nb) if (dy < 0 or (dy == 0 and dx < 0)) else (r >= nb)
    ys, xs = np.nonzero(ok)
    return np.stack([xs, ys, r[ys, xs]], axis=1).astype(np.int64).reshape(-1, 3)


def strongest(cand, cap=MAX_CANDIDATES):
    """The `cap` strongest candidates by (R desc, y asc, x asc)."""
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 3)
    order = np.lexsort((c[:, 0], c[:, 1], -c[:, 2]))
    return c[order[:cap]]


class _Walk:
    """The lattice search of one seed over the kept candidates (k_chess_order's per-thread code, statement for statement)."""

    def __init__(self, xy, pw, ph):
        self.x, self.y = xy[:, 0].copy(), xy[:, 1].copy()
        self.m, self.pw, self.ph = len(xy), pw, ph
        # walk decisions that were not clear-cut: an accepted nearest candidate with an equal-distance rival, or an acceptance
        # exactly on its threshold (the case generator wants 0 over every seed tried)
        self.ties = 0
        # seeds whose first two steps had an equal-distance rival: inherent on an axis-aligned board of integer peaks (the four
        # neighbours of a corner are equidistant), settled by the lowest index here and on the device; reported, not asserted
        self.step_ties = 0

    def find(self, qx, qy, lim2):
        """Nearest candidate to q (lowest index on ties), accepted when 16 d^2 <= lim2; -1 otherwise."""
        d2 = (self.x - qx) ** 2 + (self.y - qy) ** 2
        i = int(np.argmin(d2))
        best = int(d2[i])
        self.ties += int(16 * best == lim2) + int(16 * best <= lim2 and int((d2 == best).sum()) > 1)
        return i if 16 * best <= lim2 else -1

    def chain(self, start, sx, sy, limit):
        """Walk from `start` by the step (sx, sy), re-estimated at every corner: the indices met, None beyond `limit`."""
        out, p = [], start
        while True:
            c = self.find(int(self.x[p]) + sx, int(self.y[p]) + sy, sx * sx + sy * sy)
            if c < 0:
                return out
            if len(out) == limit:
                return None
            out.append(c)
            sx, sy = int(self.x[c] - self.x[p]), int(self.y[c] - self.y[p])
            p = c

    def next_row(self, row, c0, vx, vy):
        """The row one step (vx, vy) from `row`, grown from column c0 outwards: list, [] at the lattice's end, None = incomplete."""
        n = len(row)
        new = [-1] * n
        new[c0] = self.find(int(self.x[row[c0]]) + vx, int(self.y[row[c0]]) + vy, vx * vx + vy * vy)
        if new[c0] < 0:
            return []
        for rng, back in ((range(c0 + 1, n), -1), (range(c0 - 1, -1, -1), 1)):
            for c in rng:
                p = c + back
                sx, sy = int(self.x[new[p]] - self.x[row[p]]), int(self.y[new[p]] - self.y[row[p]])
                new[c] = self.find(int(self.x[row[c]]) + sx, int(self.y[row[c]]) + sy, sx * sx + sy * sy)
                if new[c] < 0:
                    return None
        return new

    def seed(self, s):
        """Grid [nv][nu] of candidate indices (cross(column step, row step) > 0) when the maximal lattice through candidate s
        is pw x ph or ph x pw; None otherwise."""
        pw, ph, x, y = self.pw, self.ph, self.x, self.y
        if self.m < pw * ph:
            return None
        d2 = (x - x[s]) ** 2 + (y - y[s]) ** 2
        d2[s] = np.iinfo(np.int64).max
        a = int(np.argmin(d2))
        ux, uy = int(x[a] - x[s]), int(y[a] - y[s])
        uu = ux * ux + uy * uy
        self.step_ties += int((d2 == d2[a]).sum() > 1)
        b, bd, rivals = -1, 0, 0
        for k in range(self.m):              # nearest neighbour between 60 and 120 degrees of u, at most twice as long
            if k == s:
                continue
            wx, wy = int(x[k] - x[s]), int(y[k] - y[s])
            ww, dot = wx * wx + wy * wy, ux * wx + uy * wy
            if 4 * dot * dot <= uu * ww and ww <= 4 * uu:
                if b < 0 or ww < bd:
                    b, bd, rivals = k, ww, 0
                elif ww == bd:
                    rivals += 1
        if b < 0:
            return None
        self.step_ties += int(rivals > 0)
        vx, vy = int(x[b] - x[s]), int(y[b] - y[s])
        if ux * vy - uy * vx < 0:
            ux, uy, vx, vy = vx, vy, ux, uy
        big = max(pw, ph)
        neg = self.chain(s, -ux, -uy, big)
        pos = self.chain(s, ux, uy, big)
        if neg is None or pos is None:
            return None
        row = neg[::-1] + [s] + pos
        nu, c0 = len(row), len(neg)
        if nu != pw and nu != ph:
            return None
        max_rows = (pw * ph) // nu
        rows_pos, rows_neg = [], []
        for rows, sgn in ((rows_pos, 1), (rows_neg, -1)):
            cur, sx, sy = row, sgn * vx, sgn * vy
            while True:
                new = self.next_row(cur, c0, sx, sy)
                if new is None:
                    return None
                if not new:
                    break
                if 1 + len(rows_pos) + len(rows_neg) == max_rows:
                    return None              # larger than the pattern
                rows.append(new)
                sx, sy = int(x[new[c0]] - x[cur[c0]]), int(y[new[c0]] - y[cur[c0]])
                cur = new
        grid = rows_neg[::-1] + [row] + rows_pos
        nv = len(grid)
        if not ((nu == pw and nv == ph) or (nu == ph and nv == pw)):
            return None
        return grid


def labelled(grid, x, y, pw, ph):
    """The labelling of `grid` whose rows have pw corners, whose column step x row step is positive and whose corner 0 has the
    smallest (y, x): candidate indices [ph*pw], corner (r, c) at r * pw + c."""
    g = np.asarray(grid)
    best = None
    for k in range(4):                        # np.rot90 keeps the handedness of the two steps
        q = np.rot90(g, -k)
        if q.shape != (ph, pw):
            continue
        key = (int(y[q[0, 0]]), int(x[q[0, 0]]))
        if best is None or key < best[0]:
            best = (key, q.reshape(-1))
    return best[1]


def order(cand, pw, ph, want_ties=False):
    """(found, peaks int32 [pw*ph,2]) from ALL candidates of a frame: the strongest MAX_CANDIDATES, seeds in strength order, the
    first seed whose maximal lattice is exactly pw x ph.  peaks are -1 when nothing is found.  With `want_ties` also (ties,
    step_ties) summed over every seed tried (see _Walk)."""
    if pw < 2 or ph < 2 or pw * ph > MAX_PATTERN:
        raise ValueError("pattern outside 2 <= pw, ph and pw * ph <= 256")
    top = strongest(cand)
    peaks = np.full((pw * ph, 2), -1, dtype=np.int32)
    found, ties, step_ties = 0, 0, 0
    for s in range(len(top)):
        # a seed walks only over candidates at least an eighth as strong as itself (a prefix of the sorted list): the weak
        # maxima of texture that sit between the corners of a real shot take no part
        walk = _Walk(top[:int((STRENGTH_RATIO * top[:, 2] >= top[s, 2]).sum()), :2], pw, ph)
        grid = walk.seed(s)
        ties, step_ties = ties + walk.ties, step_ties + walk.step_ties
        if grid is not None:
            peaks[:] = top[labelled(grid, walk.x, walk.y, pw, ph), :2]
            found = 1
            break
    return (found, peaks, ties, step_ties) if want_ties else (found, peaks)


def _window(wx, wy, zx, zy):
    """cv2's Gaussian window, float32 as cv2 keeps it, zeroed inside the zero zone."""
    i = (np.arange(-wy, wy + 1, dtype=np.float64) / wy)[:, None]
    j = (np.arange(-wx, wx + 1, dtype=np.float64) / wx)[None, :]
    m = (np.exp(-i * i).astype(np.float32) * np.exp(-j * j).astype(np.float32)).astype(np.float32)
    if zx >= 0 and zy >= 0 and 2 * zx + 1 < 2 * wx + 1 and 2 * zy + 1 < 2 * wy + 1:
        m[wy - zy:wy + zy + 1, wx - zx:wx + zx + 1] = 0
    return m


def _patch(g, cx, cy, pw_, ph_):
    """cv2.getRectSubPix: bilinear ph_ x pw_ patch centred on (cx, cy), replicated border, rounded to float32."""
    h, w = g.shape
    xs = cx - (pw_ - 1) * 0.5 + np.arange(pw_, dtype=np.float64)
    ys = cy - (ph_ - 1) * 0.5 + np.arange(ph_, dtype=np.float64)
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = (xs - x0)[None, :], (ys - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    top = g[ya][:, xa] * (1.0 - fx) + g[ya][:, xb] * fx
    bot = g[yb][:, xa] * (1.0 - fx) + g[yb][:, xb] * fx
    return (top * (1.0 - fy) + bot * fy).astype(np.float32)


def corner_subpix(gray, corners, win=(11, 11), zero_zone=(-1, -1), max_iter=30, eps=1e-3, reverse=False):
    """cv2.cornerSubPix on one gray image: (refined float64 [k,2], iterations int32 [k]).  Positions are float64 throughout
    (cv2: float32); the patch and the window are float32, the five sums float64.  `reverse` sums in the opposite order."""
    g = np.asarray(gray).astype(np.float64)
    h, w = g.shape
    wx, wy = int(win[0]), int(win[1])
    mask = _window(wx, wy, int(zero_zone[0]), int(zero_zone[1])).astype(np.float64)
    px = np.arange(-wx, wx + 1, dtype=np.float64)[None, :]
    py = np.arange(-wy, wy + 1, dtype=np.float64)[:, None]
    pts = np.array(corners, dtype=np.float64).reshape(-1, 2)
    out, iters = pts.copy(), np.zeros(len(pts), dtype=np.int32)

    def total(a):
        a = a.reshape(-1)
        return float(np.sum(a[::-1] if reverse else a))

    for k, (sx, sy) in enumerate(pts):
        cx, cy, it = float(sx), float(sy), 0
        while True:
            p = _patch(g, cx, cy, 2 * wx + 3, 2 * wy + 3).astype(np.float64)
            gx = p[1:-1, 2:] - p[1:-1, :-2]
            gy = p[2:, 1:-1] - p[:-2, 1:-1]
            gxx, gxy, gyy = gx * gx * mask, gx * gy * mask, gy * gy * mask
            a, b, c = total(gxx), total(gxy), total(gyy)
            bb1, bb2 = total(gxx * px + gxy * py), total(gxy * px + gyy * py)
            it += 1
            det = a * c - b * b
            if abs(det) <= np.finfo(np.float64).eps ** 2:
                break
            scale = 1.0 / det
            nx = cx + c * scale * bb1 - b * scale * bb2
            ny = cy - b * scale * bb1 + a * scale * bb2
            err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy)
            cx, cy = nx, ny
            if cx < 0 or cx >= w or cy < 0 or cy >= h:
                break
            if it >= max_iter or err <= eps * eps:
                break
        if abs(cx - sx) > wx or abs(cy - sy) > wy:
            cx, cy = float(sx), float(sy)
        out[k], iters[k] = (cx, cy), it
    return out, iters


def find_chessboard_corners(gray, pattern_size, want=False):
    """(found, corners float64 [pw*ph,2]) as vbs_chess_corners: ordered peaks through the finder's own cornerSubPix.  With
    `want`: a dict with response, candidates, n_candidates, peaks, iters, ties and step_ties as well."""
    pw, ph = int(pattern_size[0]), int(pattern_size[1])
    resp = response(gray)
    cand = candidates(resp)
    found, peaks, ties, step_ties = order(cand, pw, ph, want_ties=True)
    corners = np.full((pw * ph, 2), np.nan)
    iters = np.zeros(pw * ph, dtype=np.int32)
    if found:
        corners, iters = corner_subpix(gray, peaks.astype(np.float64), **FINDER_SUBPIX)
    if want:
        return dict(found=found, corners=corners, response=resp, candidates=cand, n_candidates=len(cand), peaks=peaks,
                    iters=iters, ties=ties, step_ties=step_ties)
    return found, corners
