"""Host-side companions of `analysis.sphere_series`: the held sphere of a still stretch, the slots of the rim, the kind
of contact a row of `sphere` describes, the spot radius of an offset and the offset per dwell.  NumPy only; nothing here touches a
device."""
import numpy as np

SPHERE_COLS, SPHERE_SWEEPS = 31, 6
(FLAG, N_FIT, N_FIT_USED, REJECTED, CX, CY, CZ, RADIUS, RMS_FIT, N_USED, N_CONTACT, CMX, CMY, CMZ, DEPTH_SUM, DEPTH_MEAN, DEPTH_MAX,
 DEEPEST, NX, NY, NZ, DIST, OFFSET, SPOT_RADIUS, TILT_DEG, AZIMUTH_DEG, SX, SY, SZ, PLANE_RMS, GAP) = range(SPHERE_COLS)
SPHERE_COLUMNS = ("flag", "n_fit", "n_fit_used", "rejected", "cx", "cy", "cz", "radius", "rms_fit", "n_used", "n_contact", "cmx", "cmy",
                  "cmz", "depth_sum", "depth_mean", "depth_max", "deepest", "nx", "ny", "nz", "dist", "offset", "spot_radius", "tilt_deg",
                  "azimuth_deg", "spot_x", "spot_y", "spot_z", "plane_rms", "gap")
KIND_NONE, KIND_FREE, KIND_TOUCH, KIND_FLAT = range(4)           # the flag of a row: no sphere, no contact slot, contact, contact plane
KIND_NAMES = ("none", "free", "touch", "flat")
_DEG = 57.29577951308232


def _rows(rows):
    r = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != SPHERE_COLS:
        raise ValueError(f"sphere rows must be [N, {SPHERE_COLS}]")
    return r


def combine(sphere_rows):
    """The sphere to HOLD from the rows of a per-frame fit over an unloaded stretch: the median of Cx, Cy, Cz and R over the frames
    with a fit, and their scatter (1.4826 times the median absolute deviation, per entry).  -> dict(sphere [4], scatter [4], frames
    (how many had a fit), rms (the median rms_fit)).  ValueError where no frame has a fit."""
    r = _rows(sphere_rows)
    ok = r[:, FLAG] != 0.0
    if not ok.any():
        raise ValueError("no frame has a sphere fit")
    v = r[ok][:, [CX, CY, CZ, RADIUS]]
    med = np.median(v, axis=0)
    return dict(sphere=med, scatter=1.4826 * np.median(np.abs(v - med), axis=0), frames=int(ok.sum()),
                rms=float(np.median(r[ok, RMS_FIT])))


def rim_slots(source, fraction=0.4):
    """The slots of the rim: the share `fraction` (at least four slots) of the valid rows of `source` [m, 4] = (flag, X, Y, Z) that
    lie farthest from the axis through the centroid of the valid rows along z, the farther first, the smaller slot among equals.
    These are the slots that touch last: what a held sphere is checked against, or a per-frame fit under load is confined to."""
    s = np.asarray(source, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("source must be [m, 4] = (flag, X, Y, Z)")
    if not 0.0 < float(fraction) <= 1.0:
        raise ValueError("fraction must lie in (0, 1]")
    ok = np.flatnonzero(s[:, 0] != 0)
    if ok.size < 4:
        raise ValueError("fewer than four valid source slots")
    xy = s[ok, 1:3] - s[ok, 1:3].mean(axis=0)
    order = np.argsort(-(xy * xy).sum(axis=1), kind="stable")
    k = min(ok.size, max(4, int(np.ceil(float(fraction) * ok.size))))
    return np.sort(ok[order[:k]]).astype(np.int64)


def kind(rows):
    """int64 [N]: KIND_NONE / KIND_FREE / KIND_TOUCH / KIND_FLAT, the flag of every row under its name."""
    return _rows(rows)[:, FLAG].astype(np.int64)


def spot(R, offset):
    """The radius of the contact spot of a sphere of radius R cut at the depth `offset`: sqrt(R^2 - (R - offset)^2), 0 where the
    plane does not cut (offset <= 0) and R at offset >= R."""
    R, d = np.asarray(R, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    dist = np.clip(R - d, 0.0, R)
    return np.sqrt(np.maximum(R * R - dist * dist, 0.0))


def normal_angles(n):
    """(tilt_deg, azimuth_deg) of normals n [..., 3] by the expressions of the columns (the components need not be normalised)."""
    n = np.asarray(n, dtype=np.float64)
    return (np.arctan2(np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]), n[..., 2]) * _DEG,
            np.arctan2(n[..., 1], n[..., 0]) * _DEG)


def summary(rows):
    """What `pipeline.bonnet_analysis` reads off the rows of a whole recording, on the host (NaN where a frame has no contact
    plane): dict(kind [N], offset, tilt_deg, azimuth_deg, spot_radius, plane_rms [N], normal, spot_centre [N, 3], depth_max [N] (NaN
    without a contact slot), first_contact (the first frame with a contact slot, -1: none), max_offset_frame, max_tilt_frame (-1: no
    frame has a plane), share (the share of frames per kind, by name))."""
    r = _rows(rows)
    flat, touch = r[:, FLAG] == 3.0, r[:, FLAG] >= 2.0
    nan = lambda v, ok=flat: np.where(ok.reshape((-1,) + (1,) * (v.ndim - 1)), v, np.nan)           # noqa: E731
    out = dict(kind=kind(r))
    for name, col in (("offset", OFFSET), ("tilt_deg", TILT_DEG), ("azimuth_deg", AZIMUTH_DEG), ("spot_radius", SPOT_RADIUS),
                      ("plane_rms", PLANE_RMS)):
        out[name] = nan(r[:, col])
    out["normal"], out["spot_centre"] = nan(r[:, NX:NZ + 1]), nan(r[:, SX:SZ + 1])
    out["depth_max"] = nan(r[:, DEPTH_MAX], touch)
    out["first_contact"] = int(np.argmax(touch)) if touch.any() else -1
    out["max_offset_frame"] = int(np.argmax(np.where(flat, r[:, OFFSET], -np.inf))) if flat.any() else -1
    out["max_tilt_frame"] = int(np.argmax(np.where(flat, r[:, TILT_DEG], -np.inf))) if flat.any() else -1
    out["share"] = {name: float((out["kind"] == k).mean()) if r.shape[0] else 0.0 for k, name in enumerate(KIND_NAMES)}
    return out


def trend_record(rows):
    """The FIR record [N, 1, 8] = (flag, offset, spot centre [3], n [3]) of the rows, flag 1 where the frame has a contact plane: what
    `pipeline.bonnet_analysis` filters (COMPONENTS of n, never angles), with n_values 7."""
    r = _rows(rows)
    rec = np.zeros((r.shape[0], 1, 8))
    flat = r[:, FLAG] == 3.0
    rec[:, 0, 0] = flat
    rec[:, 0, 1:] = np.where(flat[:, None], r[:, [OFFSET, SX, SY, SZ, NX, NY, NZ]], 0.0)
    return rec


def trend(filtered):
    """`fir_series_f64` of `trend_record` [N, 1, 15] -> [N, 10] = flag (1 where filtered), offset, spot centre [3], n [3] RENORMALISED,
    tilt_deg and azimuth_deg recomputed from the renormalised components (zeros where the filter has no value or n vanished)."""
    f = filtered.detach().cpu().numpy() if hasattr(filtered, "detach") else np.asarray(filtered, dtype=np.float64)
    if f.ndim != 3 or f.shape[1:] != (1, 15):
        raise ValueError("filtered must be [N, 1, 15]")
    v = f[:, 0, 1:8]
    nn = np.sqrt((v[:, 4:7] * v[:, 4:7]).sum(axis=1))
    ok = (f[:, 0, 0] == 3.0) & (nn > 0.0)
    n = v[:, 4:7] / np.where(ok, nn, 1.0)[:, None]
    tilt, az = normal_angles(n)
    out = np.concatenate([ok[:, None].astype(np.float64), v[:, 0:4], n, tilt[:, None], az[:, None]], axis=1)
    return np.where(ok[:, None], out, 0.0)


def offset_steps(rows, begin, end):
    """The offset per dwell: `begin`, `end` int [k + 1] are the dwells [begin, end) of `pipeline.indentation_analysis` (its `begin`
    and `end`, guards already left out) -> dict(count [k + 1] (the frames of the dwell with a contact plane), offset [k + 1] (their
    mean offset, NaN where none), std [k + 1] (ddof 1, NaN below two), delta [k] (the step of the offset from dwell to dwell))."""
    r = _rows(rows)
    begin, end = np.asarray(begin, dtype=np.int64).reshape(-1), np.asarray(end, dtype=np.int64).reshape(-1)
    if begin.shape != end.shape or (begin < 0).any() or (end > r.shape[0]).any() or (begin > end).any():
        raise ValueError("dwells must be frames 0 <= begin <= end <= N, one end per begin")
    k1 = begin.shape[0]
    count, mean, std = np.zeros(k1, dtype=np.int64), np.full(k1, np.nan), np.full(k1, np.nan)
    for j in range(k1):
        seg = r[begin[j]:end[j]]
        v = seg[seg[:, FLAG] == 3.0, OFFSET]
        count[j] = v.size
        if v.size >= 1:
            mean[j] = v.mean()
        if v.size >= 2:
            std[j] = v.std(ddof=1)
    return dict(count=count, offset=mean, std=std, delta=np.diff(mean))
