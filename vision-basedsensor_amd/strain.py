"""Host side of the strain analysis (`vbs_motion_series_f64`, `vbs_local_strain_f64`): the neighbour lists the
local fit takes, and the invariants of a gradient, which is what a trend is computed from.  NumPy only."""
import numpy as np

DEG = 57.29577951308232
INVARIANT_COLUMNS = ("dilation", "omega", "e1", "e2", "max_shear", "shear_deg", "rot_deg", "lambda1", "lambda2", "tilt_deg")


def neighbour_lists(pos, K, radius=None, valid=None):
    """int32 [s, K] for `local_strain_f64`: row i holds the K slots nearest to slot i by squared distance (dx dx + dy dy in
    float64), nearest first, the lower index first among equal distances, i itself left out.  Slots farther than `radius` and
    slots not `valid` ([s] bool; default all) are left out, and the row of an invalid slot is empty; a row with fewer than K
    entries is padded with -1 ("no neighbour")."""
    p = np.asarray(pos, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("pos must be [s >= 1, 2]")
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    s = p.shape[0]
    ok = np.ones(s, dtype=bool) if valid is None else np.asarray(valid).astype(bool).reshape(-1)
    if ok.shape != (s,):
        raise ValueError(f"valid must be [{s}]")
    if radius is not None and not (float(radius) >= 0.0):
        raise ValueError("radius must be >= 0")
    out = np.full((s, K), -1, dtype=np.int32)
    cand = np.flatnonzero(ok)
    for i in cand:
        others = cand[cand != i]
        with np.errstate(all="ignore"):
            dx, dy = p[others, 0] - p[i, 0], p[others, 1] - p[i, 1]
            d2 = dx * dx + dy * dy
        keep = ~np.isnan(d2)
        if radius is not None:
            keep &= d2 <= float(radius) * float(radius)
        others, d2 = others[keep], d2[keep]
        order = np.argsort(d2, kind="stable")[:K]            # `others` ascends: a stable sort leaves the lower index first
        out[i, :order.size] = others[order]
    return out


def invariants(grad):
    """[N, 3, 4] (flag, t_k, g_kx, g_ky for k = X, Y, Z: `motion_series_f64`'s `grad`, or the filtered part of its FIR output) ->
    [N, 10] = `INVARIANT_COLUMNS`, the columns 3 .. 12 of `strain`, by the expressions `include/vbs.h` states in their order;
    zeros where the flag is 0."""
    g = np.asarray(grad, dtype=np.float64)
    if g.ndim != 3 or g.shape[1] != 3 or g.shape[2] < 4:
        raise ValueError("grad must be [N, 3, >= 4]")
    gxx, gxy, gyx, gyy, gzx, gzy = g[:, 0, 2], g[:, 0, 3], g[:, 1, 2], g[:, 1, 3], g[:, 2, 2], g[:, 2, 3]
    with np.errstate(all="ignore"):
        dilation = gxx + gyy
        omega = 0.5 * (gyx - gxy)
        e1, e2 = 0.5 * (gxx - gyy), 0.5 * (gxy + gyx)
        max_shear = np.sqrt(e1 * e1 + e2 * e2)
        shear_deg = 0.5 * np.arctan2(e2, e1) * DEG
        f11, f12, f21, f22 = 1.0 + gxx, gxy, gyx, 1.0 + gyy
        p, q = f11 + f22, f21 - f12
        a, b = f11 - f22, f12 + f21
        h, w = np.sqrt(p * p + q * q), np.sqrt(a * a + b * b)
        rot_deg = np.arctan2(q, p) * DEG
        lam1, lam2 = 0.5 * (h + w), 0.5 * (h - w)
        tilt_deg = np.arctan(np.sqrt(gzx * gzx + gzy * gzy)) * DEG
    out = np.stack([dilation, omega, e1, e2, max_shear, shear_deg, rot_deg, lam1, lam2, tilt_deg], axis=1)
    return np.where((g[:, 0, 0] != 0)[:, None], out, 0.0)
