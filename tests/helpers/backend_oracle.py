"""CPU restatement (NumPy float64, no torch) of the 3-D back end on the package's dense tables - what
`tests/test_gpu_backend_edges.py` holds `k_solve3d` / the fused solve of `k_track` and `k_finalize_track`, `k_displacement`
and `k_plane_fit` to.  Where `oracle/stages.py` has the operation it is called; `tests/test_backend_host.py` pins this file
to `tests/golden/solve3d.json` (outputs of the reference's own function bodies) without a GPU.

  solve_table    load_marker_data's size filter (3d_reconstruction.py:172-176) + _undistort_points + _calculate_3d_position
                 (:185-238) on every tracked row of a table, from the table's OWN columns 1-3
  displacement   MarkerAnalysis._track_markers (:263-314) as one sequential loop per slot
  plane          fit_plane_least_squares (ForceDistribution.py:138-162) over the rows with a 3-D point

Tables are [..., 10] = flags, Cx, Cy, major, minor, angle, X, Y, Z, det index (float32 as the device writes them, or float64);
everything is promoted to float64 first, which is exact.
"""
import numpy as np

from oracle import stages as O

FLAG_TRACKED, FLAG_XYZ = 1, 2


def solve_table(table, K, dist, R, T, dmm=2.0, min_size=5.0):
    """(flags int64 [...], xyz float64 [..., 3]) a solve of `table` has to leave: a tracked row with major >= min_size goes
    through `O.undistort_points` and `O.calculate_3d_position`; a `ValueError` there (principal point, non-finite) or a row
    that is filtered or untracked keeps its TRACKED bit only, loses FLAG_XYZ and has zeros for X, Y, Z.  K, dist, R, T are
    taken as the float32 arrays `load_parameters` hands over (that decides which products NumPy keeps in float32)."""
    t = np.asarray(table, dtype=np.float64)
    K = np.asarray(K, dtype=np.float32).reshape(3, 3)
    dist = np.asarray(dist, dtype=np.float32).ravel()
    R = np.asarray(R, dtype=np.float32).reshape(3, 3)
    T = np.asarray(T, dtype=np.float32).reshape(3, 1)
    rows = t.reshape(-1, t.shape[-1])
    flags = rows[:, 0].astype(np.int64) & ~FLAG_XYZ
    xyz = np.zeros((rows.shape[0], 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i, row in enumerate(rows):
            if not (flags[i] & FLAG_TRACKED) or not row[3] >= min_size:
                continue
            u, v = O.undistort_points(row[1:3], K, dist)[0]
            try:
                xyz[i] = O.calculate_3d_position(np.float64(u), np.float64(v), np.float64(row[3]), K, R, T, dmm)
                flags[i] |= FLAG_XYZ
            except ValueError:
                pass
    return flags.reshape(t.shape[:-1]), xyz.reshape(t.shape[:-1] + (3,))


def displacement(table, warmup, min_size, limit):
    """disp float64 [n, m, 5] = (flag, dX, dY, dZ, |d|) of a table [n, m, 10]: rows that are untracked or below `min_size`
    do not exist; frames before (first frame holding any row) + max(warmup, 0) are skipped; a slot's row is compared with
    the row in which the slot was LAST SEEN, which must hold a 3-D point as well; |d| > limit drops the row but still
    becomes the last-seen one.  Differences and norm are written in the order the kernel uses, sqrt(dx*dx + dy*dy + dz*dz),
    so a float64 table gives the same bits."""
    t = np.asarray(table, dtype=np.float64)
    n, m = t.shape[:2]
    out = np.zeros((n, m, 5), dtype=np.float64)
    flags = t[..., 0].astype(np.int64)
    seen = ((flags & FLAG_TRACKED) != 0) & (t[..., 3] >= min_size)
    if not seen.any():
        return out
    first = int(np.nonzero(seen.any(axis=1))[0][0]) + max(int(warmup), 0)
    for r in range(m):
        last = None
        for f in range(first, n):
            if not seen[f, r]:
                continue
            good = bool(flags[f, r] & FLAG_XYZ)
            cur = t[f, r, 6:9]
            if last is not None and last[0] and good:
                dx, dy, dz = cur[0] - last[1][0], cur[1] - last[1][1], cur[2] - last[1][2]
                mm = np.sqrt(dx * dx + dy * dy + dz * dz)
                if not mm > limit:
                    out[f, r] = [1.0, dx, dy, dz, mm]
            last = (good, cur)
    return out


def plane(table_frame):
    """(count, (a, b, c, tilt_deg), s_min / s_max) of one frame's rows [m, 10]: `O.fit_plane` (np.linalg.lstsq) over the rows
    with FLAG_XYZ, and the ratio of the extreme singular values of their [X Y 1] - how well conditioned the fit is (rounding
    noise, about 1e-17, when the points are exactly collinear or coincident; 0 for fewer than 3).  count 0: zeros."""
    t = np.asarray(table_frame, dtype=np.float64)
    v = (t[:, 0].astype(np.int64) & FLAG_XYZ) != 0
    cnt = int(v.sum())
    if cnt == 0:
        return 0, (0.0, 0.0, 0.0, 0.0), 0.0
    X, Y, Z = t[v, 6], t[v, 7], t[v, 8]
    s = np.linalg.svd(np.column_stack([X, Y, np.ones(cnt)]), compute_uv=False)
    ratio = float(s[-1] / s[0]) if cnt >= 3 else 0.0
    return cnt, O.fit_plane(X, Y, Z), ratio
