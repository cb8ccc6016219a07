"""Batch driver: frames resident on the device -> fixed-slot tables -> (all-gather) -> displacement
-> plane-fit pose.  This is what `bench.py` times and what the multi-GPU path runs per rank."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import dist as D
from . import ids as _ids
from .engine import Engine
from .marker_detection import _det_to_markers


@dataclass
class TrackResult:
    ids: np.ndarray            # [M,2] (row, col) per slot
    ref_xy: np.ndarray         # [M,2]
    table: torch.Tensor        # [N,M,10] float32 (gathered when distributed)
    disp: Optional[torch.Tensor]     # [n_local,M,5]  this rank's frames [frame_begin, frame_end)
    plane: Optional[torch.Tensor]    # [n_local,5]
    frame_begin: int = 0
    frame_end: int = 0
    counts: Optional[torch.Tensor] = None   # [n_local] int32 detections per frame of this rank (never negative here)


ID_CHECK = {}                  # what the last reference_from_frame0 found (bench.py reports it)


def reference_from_frame0(eng: Engine, frame0: torch.Tensor, num_layers=5, id_mode="full", kmeans="optimal",
                          ids_on_device=True):
    """Detect frame 0 on the device and assign the identities (once per video, `marker_detection.py:275-347`).
    `ids_on_device` (default) runs the assignment on the GPU (`vbs_assign_ids`, deterministic clustering only) and the host
    restatement (`ids.assign_ids`, pinned to the reference body's golden) on the same detections as its checker:
      * the two tables agree bit for bit (every benchmark frame 0, the reference's real frame) -> the DEVICE table is what is
        returned and used (`ID_CHECK["used"] == "device"`);
      * they hold the same IDs but order markers at mathematically equal angles differently (collinear with the centre:
        np.arctan2's last bit decides on the host, the device's atan2 on the GPU) -> the host table, the reference's own
        order (`"host"`, `slots_in_another_order` says how many slots);
      * anything else raises.
    The device kernel covers `num_layers <= L.IDS_MAX_LAYERS` (16, VBS_IDS_MAX_LAYERS) and `kmeans == "optimal"`; other configurations run
    on the host alone (`"host"`, `on_device: False`) as they always did."""
    _, det, counts = eng.track_to_3d(frame0[:1], None, want_det=True)
    dev = None
    if ids_on_device and kmeans == "optimal" and int(num_layers) <= L.IDS_MAX_LAYERS:
        ids_d, xy_d = eng.assign_ids(det, counts, num_layers, id_mode)      # raises the reference's ValueError on no markers
        dev = (ids_d.cpu().numpy().astype("int64"), xy_d.cpu().numpy())
    n0 = int(counts[0].item())
    if n0 < 0:
        raise L.VbsError(f"device status {n0} in frame 0: {L.status_text(n0, eng.max_markers)}")
    table = _ids.assign_ids(_det_to_markers(det[0].cpu().numpy(), n0), num_layers, id_mode, kmeans)
    ids, xy = _ids.reference_arrays(table)
    ID_CHECK.clear()
    ID_CHECK.update({"on_device": dev is not None, "used": "host"})
    if dev is not None:
        same_ids = dev[0].shape == np.asarray(ids).shape and bool(np.array_equal(dev[0], ids))
        if not same_ids:
            raise L.VbsError("vbs_assign_ids disagrees with the host assignment on the marker IDs (not only on the order of "
                             "markers at equal angles): the device path must not be trusted on this frame 0")
        differ = int((dev[1] != np.asarray(xy)).any(axis=1).sum())
        # a slot may only differ by holding ANOTHER marker of the same layer (a swap among equal angles)
        if differ and sorted(map(tuple, dev[1].tolist())) != sorted(map(tuple, np.asarray(xy).tolist())):
            raise L.VbsError("vbs_assign_ids returned reference coordinates the host assignment does not have")
        ID_CHECK.update({"equal_to_host": differ == 0, "slots_in_another_order": differ, "markers": int(len(ids))})
        if differ == 0:
            ID_CHECK["used"] = "device"
            return dev[0], dev[1]
    return ids, xy


def track_and_gather(eng: Engine, frames_local: torch.Tensor, n_total: int, xy, min_dist=20.0, cam=None,
                     min_marker_size_px=5.0, pipelined=True):
    """This rank's frames through the fused path, `eng.pass_streams` internal passes (`eng.max_batch` frames each) at a time,
    the all-gather of their rows issued as soon as they are enqueued (`dist.TableGather`): the exchange overlaps the next ones.
    `pipelined=False`: all passes first, then the single `dist.gather_tables` collective (SURVEY 8e as written).
    Returns (local table [n_local, M, 10], counts [n_local], gathered table [n_total, M, 10])."""
    rank, ws = D.world()
    m = int(np.asarray(xy).reshape(-1, 2).shape[0])
    n_local = int(frames_local.shape[0])
    if ws == 1 or not pipelined:
        local, _, counts = eng.track_to_3d(frames_local, xy, min_dist, cam, min_marker_size_px)
        return local, counts, (local if ws == 1 else D.gather_tables(local, n_total))
    # one call and one collective per `pass_streams` internal passes: with two, the library runs the second pass of a call
    # on its second workspace and stream (VBS_OPT_PASS_STREAMS), as it does for a single process
    chunk = eng.max_batch * max(1, int(getattr(eng, "pass_streams", 1)))
    g = D.TableGather(n_total, m, L.TABLE_COLS, eng.device, chunk)
    a, _ = D.shard_bounds(n_total, ws, rank)
    counts = torch.zeros((n_local,), dtype=torch.int32, device=eng.device)
    for off in range(0, g.n_max, chunk):
        part = frames_local[off:off + chunk]
        if part.shape[0]:
            t, _, c = eng.track_to_3d(part, xy, min_dist, cam, min_marker_size_px)
            counts[off:off + part.shape[0]] = c
        else:                                           # a shorter shard has run out of frames: still joins the collective
            t = torch.zeros((0, m, L.TABLE_COLS), dtype=torch.float32, device=eng.device)
        g.push(off, t)
    table = g.finish()
    return table[a:a + n_local], counts, table


def track_shard(eng: Engine, frames_local: torch.Tensor, n_total: int, ref=None, cam: L.Camera = None,
                min_dist=20.0, min_marker_size_px=5.0, warmup_frames=0, max_displacement=50.0,
                num_layers=5, id_mode="full", kmeans="optimal", with_plane=True, pipelined=True) -> TrackResult:
    """One rank's part of a sequence of `n_total` frames (`frames_local` = this rank's contiguous block).
    `ref` = (ids, ref_xy) if already known; otherwise the rank holding frame 0 computes and broadcasts it."""
    rank, ws = D.world()
    if ref is None:
        ids = xy = None
        if rank == 0:
            ids, xy = reference_from_frame0(eng, frames_local, num_layers, id_mode, kmeans)
        ids, xy = D.broadcast_reference(ids, xy, eng.device)
    else:
        ids, xy = ref
    local, counts, table = track_and_gather(eng, frames_local, n_total, xy, min_dist, cam, min_marker_size_px, pipelined)
    bad = torch.nonzero(counts < 0)            # (after the collective, so a failing rank cannot leave the others waiting in it)
    if bad.numel():
        f = int(bad[0].item())
        raise L.VbsError(f"device status {int(counts[f].item())} in frame {D.shard_bounds(n_total, ws, rank)[0] + f} "
                         f"({L.status_text(int(counts[f].item()), eng.max_markers)}): the reference would have emitted rows "
                         f"for it")
    a, b = D.shard_bounds(n_total, ws, rank)
    disp = plane = None
    if cam is not None:
        # every rank scans only its own frames of the gathered table (the look-back may cross into the previous
        # rank's block), so the per-rank work does not grow with the number of GPUs
        disp = eng.displacement(table, warmup_frames, min_marker_size_px, max_displacement, frame_range=(a, b))
        if with_plane:
            plane = eng.plane_fit(local)
    return TrackResult(ids, xy, table, disp, plane, a, b, counts)


def deviation_pose(eng: Engine, table_vert: torch.Tensor, table_tilt: torch.Tensor, ref_xyz, mode="plane", scale=1.0,
                   start=0, end=-1):
    """Pose misalignment from two tracked loadings (`ForceDistribution.py:168-208,218-243`): the displacement of every
    marker between frames `start` and `end` of the vertical session's table and of the tilted session's, their difference
    (the deviation field), the plane through reference position + scale * deviation and its tilt.  Both tables must use
    the same slot order (the same frame-0 identities).  Returns a dict with `deviation` [M,4] (device tensor: common,
    dX, dY, dZ), `n`, `a`, `b`, `c`, `tilt_deg`, `mean_vector` (scaled, as the reference plots it) and `mean_magnitude`."""
    dev, out = eng.deviation_plane(table_vert[start], table_vert[end], table_tilt[start], table_tilt[end], ref_xyz, mode, scale)
    o = out.cpu().numpy().astype(np.float64)
    return {"deviation": dev, "n": int(o[0]), "a": o[1], "b": o[2], "c": o[3], "tilt_deg": o[4],
            "mean_vector": o[5:8].copy(), "mean_magnitude": o[8]}


# ---- the time axis (k_series.hip): what the reference's analysis layer computes from its result sheet ------------------------
def series_stats_shard(eng: Engine, res: TrackResult, n_total: int) -> torch.Tensor:
    """`Engine.series_stats` of a sequence whose `disp` is spread over the ranks (`track_shard`): every rank reduces its own
    frames to per-chunk records (chunks aligned to global frame 0, so `frame_begin = res.frame_begin`), ONE all-gather of
    those records (padded to the largest per-rank count), then the same merge in frame order on every rank -> stats [M, 5],
    bit-identical on all ranks.  A chunk cut by a shard edge arrives as two records, merged in frame order like any others."""
    rank, ws = D.world()
    m = int(res.table.shape[1])
    spans = [D.shard_bounds(n_total, ws, r) for r in range(ws)]
    a, b = spans[rank]
    if (a, b) != (res.frame_begin, res.frame_end):
        raise ValueError(f"res holds frames [{res.frame_begin}, {res.frame_end}), rank {rank} of {ws} owns [{a}, {b})")
    k_max = max((eng.lib.vbs_series_chunks(rb - ra, ra) if rb > ra else 0) for ra, rb in spans)
    if k_max < 1:
        raise ValueError("series_stats_shard: no frames")
    if b > a:
        rec = eng.series_partial(res.disp, frame_begin=a)
    else:                                               # a rank without frames still joins the collective
        rec = torch.zeros((0, m, L.SERIES_REC_COLS), dtype=torch.float64, device=eng.device)
    return eng.series_merge(D.gather_records(rec, k_max))


def window_displacement(eng: Engine, table: torch.Tensor, start=(1, 30), end=(120, 150), slots=None):
    """`LocalAnalysis.py`'s flow (:53-60, :77-94) on a table [N, M, 10]: the mean X, Y, Z of every slot over two inclusive
    frame windows, the inner join of the slots seen in both (:81), their difference vector, its norm and the mean norm.
    `slots` (indices) selects markers as TARGET_MARKERS does (:11, :47).  Returns a dict of device tensors: `slots` [K],
    `start_xyz` / `end_xyz` [K,3], `d` [K,4] = dX, dY, dZ, |d|, and `mean` (0-d; NaN when no slot is common)."""
    means = eng.window_means(table, [start, end])
    common = (means[0, :, 0] > 0) & (means[1, :, 0] > 0)
    if slots is not None:
        pick = torch.zeros_like(common)
        pick[torch.as_tensor(np.asarray(slots, dtype=np.int64).reshape(-1), device=common.device)] = True
        common &= pick
    idx = torch.nonzero(common).reshape(-1)
    s_xyz, e_xyz = means[0, idx, 1:4], means[1, idx, 1:4]
    d = e_xyz - s_xyz
    mag = torch.sqrt((d * d).sum(dim=1))
    return {"slots": idx, "start_xyz": s_xyz, "end_xyz": e_xyz, "d": torch.cat([d, mag[:, None]], dim=1), "mean": mag.mean()}


# ---- the dynamic polishing process (k_filter.hip): the reference's Figure 11 from a tracked table ------------------------------
def polishing_analysis(eng: Engine, table: torch.Tensor, taps, ref_frame=0, slots=None, min_coverage=0.5):
    """Figure 11 of the reference (it ships no code for it) from a table [N, M, 10]: (a) the total marker
    displacement per frame and its trend, (b) per marker the amplitude left when the marker's own trend is removed.  `taps`: a
    full odd-length symmetric FIR (`filters.lowpass_taps`).  Returns a dict of device tensors (float64):
      `axis` [N, M, 4] flag, dX, dY, dZ against frame `ref_frame`;  `total` [N, 5] complete, sum dX, dY, dZ, count;
      `total_filtered` [N, 7] flag, trend, residual: the FIR of the TOTAL series over its complete frames (not the sum of the
      per-marker trends: a frame with a dropout is a gap of the total, whichever marker it was);
      `marker_filtered` [N, M, 7] the same per marker over the frames it was seen in;
      `amplitude` [M, 3, 3]: per marker and axis the count, std (ddof = 1) and max |.| of its residual (NaN as `series_stats`)."""
    from .engine import fir_series_f64, series_stats_f64
    axis, total = eng.axis_displacement(table, ref_frame, slots)
    dev = eng.device.index
    total_f = fir_series_f64(total[:, None, :], taps, 3, min_coverage, device=dev)[:, 0]
    marker_f = fir_series_f64(axis, taps, 3, min_coverage, device=dev)
    n, m = marker_f.shape[0], marker_f.shape[1]
    amplitude = torch.empty((m, 3, 3), dtype=torch.float64, device=eng.device)
    packed = torch.zeros((n, m, L.DISP_COLS), dtype=torch.float64, device=eng.device)     # the layout series_stats_f64 reads
    packed[..., 0] = (marker_f[..., 0] == 3.0).to(torch.float64)
    for a in range(3):
        packed[..., 4] = marker_f[..., 4 + a]
        st = series_stats_f64(packed, device=dev)
        packed[..., 4] = marker_f[..., 4 + a].abs()
        amplitude[:, a, 0], amplitude[:, a, 1] = st[:, 0], st[:, 2]
        amplitude[:, a, 2] = series_stats_f64(packed, device=dev)[:, 3]
    return {"axis": axis, "total": total, "total_filtered": total_f, "marker_filtered": marker_f, "amplitude": amplitude}


def to_total_frame(total, total_filtered, frame_offset=0, path=None):
    """The sheet behind Figure 11 (a): one row `frameno, count, complete, dX, dY, dZ, dX_f, dY_f, dZ_f` per frame from
    `polishing_analysis`'s `total` [N, 5] and `total_filtered` [N, 7]; the filtered columns are NaN (empty cells) where the
    frame has no trend (flag != 3).  `path`: also written as .xlsx (`xlsx_io.dataframe_to_xlsx`)."""
    import pandas as pd
    t = total.detach().cpu().numpy() if isinstance(total, torch.Tensor) else np.asarray(total)
    f = total_filtered.detach().cpu().numpy() if isinstance(total_filtered, torch.Tensor) else np.asarray(total_filtered)
    if t.ndim != 2 or t.shape[1] != L.TOTAL_COLS or f.shape != (t.shape[0], 7):
        raise ValueError(f"total must be [N, {L.TOTAL_COLS}] and total_filtered [N, 7]")
    trend = np.where((f[:, 0] == 3.0)[:, None], f[:, 1:4], np.nan)
    df = pd.DataFrame({"frameno": np.arange(t.shape[0], dtype=np.int64) + int(frame_offset), "count": t[:, 4].astype(np.int64),
                       "complete": t[:, 0].astype(np.int64), "dX": t[:, 1].astype(np.float64), "dY": t[:, 2].astype(np.float64),
                       "dZ": t[:, 3].astype(np.float64), "dX_f": trend[:, 0], "dY_f": trend[:, 1], "dZ_f": trend[:, 2]})
    if path is not None:
        from .xlsx_io import dataframe_to_xlsx
        dataframe_to_xlsx(df, path)
    return df


# ---- despiking a tracked table (k_robust.hip): the Hampel rule along time, spikes turned into gaps ----------------------------------
_SPIKE_SOURCES = {"xyz": (L.FLAG_XYZ, L.FLAG_XYZ, (6, 7, 8), ("Xw", "Yw", "Zw")),
                  "pixel": (L.FLAG_TRACKED, L.FLAG_TRACKED | L.FLAG_XYZ, (1, 2), ("Cx", "Cy"))}


def despike_table(eng: Engine, table: torch.Tensor, half_window=7, k_sigma=3.0, *, min_scale, source="xyz", slots=None):
    """The rows of a table [N, M, 10] that are isolated jumps of one marker's series along time - a neighbour taken during a
    dropout, a merged blob, a bad ellipse - found by `engine.hampel_series_f64` and turned into gaps, which every
    `*_analysis` of this module handles.  `source` "xyz": the rows with VBS_FLAG_XYZ, values X, Y, Z (cols 6-8); "pixel": the rows
    with VBS_FLAG_TRACKED, values Cx, Cy.  A row is a spike when ANY of its values is.  `min_scale` (required: millimetres and
    pixels share no default) is the absolute floor below which a deviation is never a spike; `slots` (indices) restricts the
    test to those markers.  Returns (clean_table, report): clean_table is a copy of the table in which the spike rows have
    VBS_FLAG_XYZ cleared ("xyz") or both flag bits ("pixel": the 3-D row derives from the 2-D one), every other bit and column
    untouched.  report, a dict of tensors on the table's device: `spike` bool [N, M]; `per_marker` [M] and `per_frame` [N] int64
    counts; `median`, `mad` float64 [N, M, nv] (0 where not judged); `fill` bool [N, M]: the marker is missing and `median` is
    the value to fill the gap with; `ref_spikes` int64: the slots whose row in frame 0 is a spike - such a slot drops out of
    every analysis that takes frame 0 as its reference, so the caller may want another `ref_frame`; nothing is chosen for them
    here; `source`, which `to_spike_frame` reads."""
    from . import engine as _engine
    if source not in _SPIKE_SOURCES:
        raise ValueError(f"source must be one of {sorted(_SPIKE_SOURCES)}")
    bit, clear, cols, _ = _SPIKE_SOURCES[source]
    t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.asarray(table), device=eng.device)
    if t.dim() != 3 or t.shape[2] != L.TABLE_COLS:
        raise ValueError(f"table must be [N, M, {L.TABLE_COLS}]")
    flags = t[..., 0].to(torch.int64)
    valid = (flags & bit) != 0
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= t.shape[1]):
            raise ValueError(f"slots outside the table's {t.shape[1]} slots")
        pick = torch.zeros(t.shape[1], dtype=torch.bool, device=t.device)
        pick[torch.as_tensor(idx, device=t.device)] = True
        valid = valid & pick[None, :]
    rec = torch.cat([valid.to(torch.float64)[..., None], t[..., list(cols)].to(torch.float64)], dim=2).contiguous()
    out, _ = _engine.hampel_series_f64(rec, half_window, k_sigma, min_scale, want_clean=False, device=eng.device.index)
    out = torch.as_tensor(out, device=t.device)
    nv = len(cols)
    spike, fill = out[..., 0] == 7.0, out[..., 0] == 2.0
    clean = t.clone()
    clean[..., 0] = torch.where(spike, (flags & ~clear).to(t.dtype), t[..., 0])
    report = {"spike": spike, "per_marker": spike.sum(dim=0), "per_frame": spike.sum(dim=1),
              "median": out[..., 2:2 + nv], "mad": out[..., 2 + nv:2 + 2 * nv], "fill": fill,
              "ref_spikes": torch.nonzero(spike[0]).reshape(-1), "source": source}
    return clean, report


def to_spike_frame(report, table, ids=None, frame_offset=0, path=None):
    """The sheet of `despike_table`: one row per spike, frame-major, from its `report` and the table it was given: `frameno,
    marker_id`, the values (`Xw, Yw, Zw` or `Cx, Cy` by the report's source), their medians (`*_med`) and MADs (`*_mad`);
    `marker_id` = `ids.marker_ids` (slot number + 1 without `ids`).  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    t, spike, med, mad = host(table), host(report["spike"]), host(report["median"]), host(report["mad"])
    _, _, cols, names = _SPIKE_SOURCES[report["source"]]
    if t.ndim != 3 or t.shape[2] != L.TABLE_COLS or spike.shape != t.shape[:2] or med.shape != t.shape[:2] + (len(cols),):
        raise ValueError(f"table must be the [N, M, {L.TABLE_COLS}] table the report was made from")
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, t.shape[1] + 1, dtype=np.int64)
    if len(mid) != t.shape[1]:
        raise ValueError(f"table has {t.shape[1]} slots, ids {len(mid)}")
    f, s = np.nonzero(spike)
    data = {"frameno": (f + int(frame_offset)).astype(np.int64), "marker_id": np.asarray(mid)[s]}
    for k, name in enumerate(names):
        data[name] = t[f, s, cols[k]].astype(np.float64)
    for k, name in enumerate(names):
        data[name + "_med"] = med[f, s, k].astype(np.float64)
    for k, name in enumerate(names):
        data[name + "_mad"] = mad[f, s, k].astype(np.float64)
    df = pd.DataFrame(data)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- pose misalignment along a recording (k_pose.hip): `deviation_pose` for every frame, with its trend ----------------------------
_DEG = 57.29577951308232


def misalignment_analysis(eng: Engine, table: torch.Tensor, table_ref: torch.Tensor, ref_xyz, taps=None, start=0, ref_start=0,
                          ref_end=-1, mode="plane", scale=1.0, slots=None, reject_k=0.0, min_coverage=0.5):
    """`deviation_pose` for every frame of a recording: `table_ref` [Nr, M, 10] is the reference state's session
    (the vertical loading), whose displacement between its frames `ref_start` and `ref_end` is the field every frame of `table`
    [N, M, 10] is compared with - frame f of `table` against its frame `start`.  Both tables use the same slot order.  Returns a
    dict of device tensors (float64): `ref_disp` [M, 4], `deviation` [N, M, 4], `field` [N, 6], `pose` [N, 8]
    (`Engine.pose_series`) and, with `taps` (a full odd-length symmetric FIR, `filters.lowpass_taps`): `pose_filtered` [N, 7] =
    flag, trend and residual of the plane's a, b, c over the frames that have a plane (`fir_series_f64`), and `trend` [N, 3] =
    flag (1 where the frame has a trend), tilt_deg and azimuth_deg OF THE FILTERED a and b - angles themselves are never
    filtered (an azimuth wraps, a tilt is not linear in the plane)."""
    from .engine import fir_series_f64
    n_ref = int(table_ref.shape[0])
    end = int(ref_end) + n_ref if int(ref_end) < 0 else int(ref_end)
    if not (0 <= end < n_ref):
        raise ValueError(f"ref_end {ref_end} outside the reference table's {n_ref} frames")
    ref_disp = eng.axis_displacement(table_ref, ref_start, slots, frame_range=(end, end + 1))[0][0]
    deviation, field, pose = eng.pose_series(table, ref_disp, ref_xyz, start, mode, scale, slots, reject_k)
    out = {"ref_disp": ref_disp, "deviation": deviation, "field": field, "pose": pose}
    if taps is not None:
        pf = fir_series_f64(pose[:, None, :], taps, 3, min_coverage, device=eng.device.index)[:, 0]
        ok = pf[:, 0] == 3.0
        a, b = pf[:, 1], pf[:, 2]
        zero = torch.zeros_like(a)
        out["pose_filtered"] = pf
        out["trend"] = torch.stack([ok.to(torch.float64), torch.where(ok, torch.atan(torch.sqrt(a * a + b * b)) * _DEG, zero),
                                    torch.where(ok, torch.atan2(b, a) * _DEG, zero)], dim=1)
    return out


POSE_FRAME_COLUMNS = ("frameno", "count", "complete", "n_used", "flag", "a", "b", "c", "tilt_deg", "azimuth_deg", "rms", "mean_dX",
                      "mean_dY", "mean_dZ", "mean_mag")
POSE_TREND_COLUMNS = ("a_f", "b_f", "c_f", "tilt_f", "azimuth_f")


def to_pose_frame(field, pose, pose_filtered=None, frame_offset=0, path=None):
    """The sheet of `misalignment_analysis`: one row per frame with `POSE_FRAME_COLUMNS` from `field` [N, 6] and `pose` [N, 8],
    and with `pose_filtered` [N, 7] also `POSE_TREND_COLUMNS` (the angles computed from the filtered a and b).  a .. rms are NaN
    (empty cells) where the frame has no plane (flag 0), the trend columns where it has no trend (flag != 3).  `path`: also
    written as .xlsx (`xlsx_io.dataframe_to_xlsx`)."""
    import pandas as pd
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    fl, po = host(field), host(pose)
    if fl.ndim != 2 or fl.shape[1] != L.POSEFIELD_COLS or po.shape != (fl.shape[0], L.POSE_COLS):
        raise ValueError(f"field must be [N, {L.POSEFIELD_COLS}] and pose [N, {L.POSE_COLS}]")
    plane = np.where((po[:, 0] != 0)[:, None], po[:, 1:7], np.nan)
    cols = {"frameno": np.arange(fl.shape[0], dtype=np.int64) + int(frame_offset), "count": fl[:, 1].astype(np.int64),
            "complete": fl[:, 0].astype(np.int64), "n_used": po[:, 7].astype(np.int64), "flag": po[:, 0].astype(np.int64)}
    for k, name in enumerate(("a", "b", "c", "tilt_deg", "azimuth_deg", "rms")):
        cols[name] = plane[:, k]
    for k, name in enumerate(("mean_dX", "mean_dY", "mean_dZ", "mean_mag")):
        cols[name] = fl[:, 2 + k].astype(np.float64)
    if pose_filtered is not None:
        pf = host(pose_filtered)
        if pf.shape != (fl.shape[0], 7):
            raise ValueError("pose_filtered must be [N, 7]")
        t = np.where((pf[:, 0] == 3.0)[:, None], pf[:, 1:4], np.nan)
        cols["a_f"], cols["b_f"], cols["c_f"] = t[:, 0], t[:, 1], t[:, 2]
        cols["tilt_f"] = np.arctan(np.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1])) * _DEG
        cols["azimuth_f"] = np.arctan2(t[:, 1], t[:, 0]) * _DEG
    df = pd.DataFrame(cols)
    if path is not None:
        from .xlsx_io import dataframe_to_xlsx
        dataframe_to_xlsx(df, path)
    return df


# ---- uncertainty of the pose misalignment (k_posecov.hip): is the tilt a misalignment or the noise of the markers? -----------------
def _misalignment_uncertainty_args(n_ref, ref_start, ref_end, k):
    """`misalignment_uncertainty`'s own argument checks (no device needed); the entry's are `engine._posecov_args`.  -> (ref_start,
    ref_end counted from the front, k)."""
    end = int(ref_end) + n_ref if int(ref_end) < 0 else int(ref_end)
    if not (0 <= end < n_ref):
        raise ValueError(f"ref_end {ref_end} outside the reference table's {n_ref} frames")
    if int(ref_start) != ref_start or not (0 <= int(ref_start) < n_ref):
        raise ValueError(f"ref_start {ref_start} outside the reference table's {n_ref} frames")
    if not (np.isfinite(float(k)) and float(k) > 0.0):
        raise ValueError("k must be finite and > 0")
    return int(ref_start), end, float(k)


def misalignment_uncertainty(eng: Engine, table, table_ref, ref_xyz, cam: L.Camera, obs_cov, cam_factor=None, start=0, ref_start=0,
                             ref_end=-1, mode="plane", scale=1.0, slots=None, reject_k=0.0, k=3.0, min_marker_size_px=5.0,
                             exact_reference=False):
    """How good the plane of `misalignment_analysis` is, to first order: `pose_cov` on the same inputs, with the
    observation covariance `obs_cov` and the camera's factor `cam_factor` of `uncertainty_analysis`.  `ref_disp` is formed as
    `misalignment_analysis` forms it; the reference session's rows at `ref_start` and `ref_end` carry their own pixel noise and
    camera directions into every frame unless `exact_reference`.  Returns a dict of host arrays over the N frames: `pose` [N, 8],
    `pcov` [N, 17], `flag`; `sigma_abc` [N, 3] the standard deviations of a, b, c (NaN where flag bit 1 is clear: no plane, or a
    used slot whose rows are not usable - `n_unusable` counts them); `sigma_tilt_deg`, `sigma_azimuth_deg` (NaN where bit 4 is
    clear: a = b = 0); `camera_share` the camera's share of var_tilt - coherent over the markers, it does not average out; `t2` =
    (a, b) Sigma_ab^-1 (a, b)' (NaN where bit 2 is clear) and `significant` = t2 > k^2; `tilt_limit_deg` = atan(k
    sqrt(lambda_max(Sigma_ab))) in degrees, the tilt a frame could not tell from zero in its worst direction.
    `significant` is a test with TWO degrees of freedom: for an untilted plane t2 is chi-squared with 2, so its false-alarm rate
    is exp(-k^2 / 2) - 1.1 % at k = 3, not the 0.27 % of a one-dimensional 3 sigma.  A tilt is >= 0 and not Gaussian near 0, which
    is why t2 and not tilt / sigma_tilt decides."""
    from .engine import pose_cov
    table_ref = eng._table32(table_ref)
    rs, end, kk = _misalignment_uncertainty_args(int(table_ref.shape[0]), ref_start, ref_end, k)
    ref_disp = eng.axis_displacement(table_ref, rs, slots, frame_range=(end, end + 1))[0][0]
    ref_rows = None if exact_reference else torch.stack([table_ref[rs], table_ref[end]]).contiguous()
    pose, pcov = pose_cov(table, ref_disp, ref_xyz, cam, obs_cov, cam_factor, ref_rows, start, mode, scale, slots, reject_k,
                          min_marker_size_px, device=eng.device.index)
    po, pc = pose.cpu().numpy(), pcov.cpu().numpy()
    flag = pc[:, 0].astype(np.int64)
    ok, t2ok, angok = (flag & 1) != 0, (flag & 2) != 0, (flag & 4) != 0
    a, b = po[:, 1], po[:, 2]
    S, Cm = pc[:, 2:8], pc[:, 8:14]
    with np.errstate(all="ignore"):
        sig = np.where(ok[:, None], np.sqrt(S[:, [0, 3, 5]]), np.nan)
        quad = lambda M: a * a * M[:, 0] + 2.0 * a * b * M[:, 1] + b * b * M[:, 3]      # noqa: E731
        qs, qc = quad(S), quad(Cm)
        share = np.where(angok & (qs > 0.0), qc / np.where(qs > 0.0, qs, 1.0), np.where(angok, 0.0, np.nan))
        lam = 0.5 * (S[:, 0] + S[:, 3]) + np.sqrt(0.25 * (S[:, 0] - S[:, 3]) ** 2 + S[:, 1] * S[:, 1])
        t2 = np.where(t2ok, pc[:, 16], np.nan)
        res = dict(pose=po, pcov=pc, flag=flag, n_unusable=pc[:, 1].astype(np.int64), sigma_abc=sig,
                   sigma_tilt_deg=np.where(angok, np.sqrt(pc[:, 14]), np.nan),
                   sigma_azimuth_deg=np.where(angok, np.sqrt(pc[:, 15]), np.nan), camera_share=share, t2=t2, significant=t2ok & (pc[:, 16] > kk * kk),
                   tilt_limit_deg=np.where(ok, np.arctan(kk * np.sqrt(lam)) * _DEG, np.nan), k=kk)
    return res


POSE_UNCERTAINTY_COLUMNS = ("frameno", "flag", "n_used", "n_unusable", "a", "b", "c", "sigma_a", "sigma_b", "sigma_c", "tilt_deg",
                            "sigma_tilt_deg", "azimuth_deg", "sigma_azimuth_deg", "camera_share", "t2", "significant", "tilt_limit_deg")


def to_pose_uncertainty_frame(result, frame_offset=0, path=None):
    """The sheet of `misalignment_uncertainty`: one row `POSE_UNCERTAINTY_COLUMNS` per frame; `flag` is the entry's bit set, a .. c
    and the angles are empty (NaN) where the frame has no plane, every sigma where its flag bit is clear.  `path`: also written,
    as .csv or as .xlsx."""
    import pandas as pd
    po, pc = np.asarray(result["pose"], dtype=np.float64), np.asarray(result["pcov"], dtype=np.float64)
    if po.ndim != 2 or po.shape[1] != L.POSE_COLS or pc.shape != (po.shape[0], L.POSECOV_COLS):
        raise ValueError(f"pose must be [N, {L.POSE_COLS}] and pcov [N, {L.POSECOV_COLS}]")
    N = po.shape[0]
    plane = np.where((po[:, 0] != 0)[:, None], po[:, 1:6], np.nan)
    sig = np.asarray(result["sigma_abc"], dtype=np.float64)
    cols = {"frameno": np.arange(N, dtype=np.int64) + int(frame_offset), "flag": pc[:, 0].astype(np.int64),
            "n_used": po[:, 7].astype(np.int64), "n_unusable": pc[:, 1].astype(np.int64),
            "a": plane[:, 0], "b": plane[:, 1], "c": plane[:, 2], "sigma_a": sig[:, 0], "sigma_b": sig[:, 1], "sigma_c": sig[:, 2],
            "tilt_deg": plane[:, 3], "sigma_tilt_deg": np.asarray(result["sigma_tilt_deg"], dtype=np.float64),
            "azimuth_deg": plane[:, 4], "sigma_azimuth_deg": np.asarray(result["sigma_azimuth_deg"], dtype=np.float64),
            "camera_share": np.asarray(result["camera_share"], dtype=np.float64), "t2": np.asarray(result["t2"], dtype=np.float64),
            "significant": np.asarray(result["significant"]).astype(bool),
            "tilt_limit_deg": np.asarray(result["tilt_limit_deg"], dtype=np.float64)}
    df = pd.DataFrame(cols, columns=list(POSE_UNCERTAINTY_COLUMNS))
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- indentation shape along a recording (k_shape.hip): what the plane leaves behind - the bowl, its apex, depth and curvatures ------
def _hessian_columns(p, q, r):
    """H, K, k1, k2, dir_deg of a Hessian (p, q, r), the expressions of `vbs_shape_series` on torch tensors."""
    H, K = (p + r) / 2.0, p * r - q * q
    hd = (p - r) / 2.0
    s = torch.sqrt(hd * hd + q * q)
    return H, K, H + s, H - s, (0.5 * torch.atan2(2.0 * q, p - r)) * _DEG


def shape_analysis(eng: Engine, table: torch.Tensor, table_ref: torch.Tensor, ref_xyz, taps=None, start=0, ref_start=0, ref_end=-1,
                   mode="plane", scale=1.0, slots=None, reject_k=0.0, min_coverage=0.5, length=None, min_count=9, piv_rel=1e-10,
                   apex_rel=1e-6, max_apex=2.0, grid=None):
    """`shape_series` for every frame of a recording, on the inputs of `misalignment_analysis` and with `ref_disp`
    formed as that function forms it.  Returns a dict: the device tensors `ref_disp` [M, 4], `shape` [N, 24], `coef` [N, 2, 4] and
    `residual` [N, M, 2]; with `taps` (a full odd-length symmetric FIR) `coef_filtered` [N, 2, 7] (`fir_series_f64` of `coef`: row 0
    over the frames with a fit, row 1 over those of degree 2) and `trend` [N, 6] = flag (1 where the frame has a filtered Hessian),
    H, K, k1, k2, dir_deg RECOMPUTED from the filtered p, q, r - curvatures and angles themselves are never filtered; with `grid` =
    (W [P, M], wsum [P]) of `fields` the `residual_map` [N, P, 2] (`field_map_f64`): what no smooth surface explains, smoothed.  Per
    recording, on the host: `kind` [N] (`shapes.kind`), `kind_share` (name -> share of the frames), `apex_track` [N, 4] = valid,
    apex_x, apex_y, apex_z (NaN where not valid) and `deepest_frame`, the frame of largest |depth| among those with an apex
    (-1: none)."""
    from . import shapes
    from .engine import field_map_f64, fir_series_f64, shape_series
    n_ref = int(table_ref.shape[0])
    end = int(ref_end) + n_ref if int(ref_end) < 0 else int(ref_end)
    if not (0 <= end < n_ref):
        raise ValueError(f"ref_end {ref_end} outside the reference table's {n_ref} frames")
    ref_disp = eng.axis_displacement(table_ref, ref_start, slots, frame_range=(end, end + 1))[0][0]
    out = shape_series(table, ref_disp, ref_xyz, start, mode, scale, length, slots, reject_k, min_count, piv_rel, apex_rel, max_apex,
                       device=eng.device.index)
    out["ref_disp"] = ref_disp
    if taps is not None:
        cf = fir_series_f64(out["coef"], taps, 3, min_coverage, device=eng.device.index)
        ok = cf[:, 1, 0] == 3.0
        zero = torch.zeros_like(cf[:, 1, 1])
        cols = _hessian_columns(cf[:, 1, 1], cf[:, 1, 2], cf[:, 1, 3])
        out["coef_filtered"] = cf
        out["trend"] = torch.stack([ok.to(torch.float64)] + [torch.where(ok, c, zero) for c in cols], dim=1)
    if grid is not None:
        W, wsum = grid
        out["residual_map"] = field_map_f64(out["residual"], W, wsum, min_coverage, 1, device=eng.device.index)
    sh = out["shape"].cpu().numpy()
    kinds = shapes.kind(sh, apex_rel)
    valid = sh[:, shapes.APEX] == 1.0
    out["kind"] = kinds
    out["kind_share"] = {name: float((kinds == k).mean()) if kinds.size else 0.0 for k, name in enumerate(shapes.KIND_NAMES)}
    out["apex_track"] = np.concatenate([valid[:, None].astype(np.float64),
                                        np.where(valid[:, None], sh[:, shapes.APEX_X:shapes.APEX_Z + 1], np.nan)], axis=1)
    out["deepest_frame"] = int(np.argmax(np.where(valid, np.abs(sh[:, shapes.DEPTH]), -1.0))) if valid.any() else -1
    return out


SHAPE_FRAME_COLUMNS = ("frameno", "kind", "degree", "count", "n_used", "mx", "my", "mz", "c0", "a", "b", "p", "q", "r", "rms_plane",
                       "rms", "H", "K", "k1", "k2", "dir_deg", "apex", "apex_x", "apex_y", "apex_z", "depth")
SHAPE_TREND_COLUMNS = ("c0_f", "a_f", "b_f", "p_f", "q_f", "r_f", "H_f", "K_f", "k1_f", "k2_f", "dir_deg_f")


def to_shape_frame(result, frame_offset=0, path=None):
    """The sheet of `shape_analysis`: one row `SHAPE_FRAME_COLUMNS` per frame - `kind` as its name, degree, count, n_used and apex
    as integers, c0 .. rms_plane empty (NaN) below degree 1, p .. dir_deg below degree 2, the apex and the depth where there is no
    valid apex - and with a trend also `SHAPE_TREND_COLUMNS` (empty where the filter has no value).  `path`: also written, as .csv
    or as .xlsx."""
    import pandas as pd
    from . import shapes
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    sh = host(result["shape"]).astype(np.float64)
    if sh.ndim != 2 or sh.shape[1] != L.SHAPE_COLS:
        raise ValueError(f"shape must be [N, {L.SHAPE_COLS}]")
    N = sh.shape[0]
    deg, apex = sh[:, shapes.DEGREE], sh[:, shapes.APEX] == 1.0
    kinds = np.asarray(result["kind"]) if "kind" in result else shapes.kind(sh)
    cols = {"frameno": np.arange(N, dtype=np.int64) + int(frame_offset), "kind": [shapes.KIND_NAMES[int(k)] for k in kinds]}
    for c, name in enumerate(shapes.SHAPE_COLUMNS):
        if name in ("degree", "count", "n_used", "apex"):
            cols[name] = sh[:, c].astype(np.int64)
        elif c <= shapes.MZ:
            cols[name] = np.where(sh[:, shapes.COUNT] >= 1.0, sh[:, c], np.nan)
        elif c in (shapes.C0, shapes.A, shapes.B, shapes.RMS_PLANE):
            cols[name] = np.where(deg >= 1.0, sh[:, c], np.nan)
        elif c >= shapes.APEX_X:
            cols[name] = np.where(apex, sh[:, c], np.nan)
        else:
            cols[name] = np.where(deg == 2.0, sh[:, c], np.nan)
    names = list(SHAPE_FRAME_COLUMNS)
    if "coef_filtered" in result:
        cf, tr = host(result["coef_filtered"]), host(result["trend"])
        if cf.shape != (N, 2, 7) or tr.shape != (N, 6):
            raise ValueError("coef_filtered must be [N, 2, 7] and trend [N, 6]")
        for k, name in enumerate(("c0_f", "a_f", "b_f")):
            cols[name] = np.where(cf[:, 0, 0] == 3.0, cf[:, 0, 1 + k], np.nan)
        for k, name in enumerate(("p_f", "q_f", "r_f")):
            cols[name] = np.where(cf[:, 1, 0] == 3.0, cf[:, 1, 1 + k], np.nan)
        for k, name in enumerate(("H_f", "K_f", "k1_f", "k2_f", "dir_deg_f")):
            cols[name] = np.where(tr[:, 0] == 1.0, tr[:, 1 + k], np.nan)
        names += list(SHAPE_TREND_COLUMNS)
    df = pd.DataFrame(cols, columns=names)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- rigid motion along a recording (k_rigid.hip): how the markers moved as a body, and what is left once that is removed -----------
def rigid_analysis(eng: Engine, table: torch.Tensor, source="start", start_frame=0, layout=None, with_scale=False, reject_k=3.0,
                   taps=None, grid=None, slots=None, gap_rel=1e-6, min_coverage=0.5, worst=5):
    """`rigid_series` for every frame of a recording.  `source`: "start" registers every frame against frame
    `start_frame` of the table itself (`rigid.source_from_table`), "layout" against `layout` [M, 3] (`rigid.source_from_layout`:
    the sensor's pose against its design), or a ready [M, 4] array.  Returns a dict: the device tensors `rigid` [N, 33], `coef`
    [N, 4, 4] and `residual` [N, M, 4] and the host array `source` [M, 4]; per frame, on the host (NaN where the frame has no fit):
    `rotvec` [N, 3] (the axis times the angle in degrees), `tilt_deg`, `azimuth_deg`, `twist_deg`, `shift` [N, 3] = pm - qm (the
    shift of the centroid), `scale`, `rms`, `share` = 1 - SSR / SS0 (`rigid.rigid_share`) and `kind` (`rigid.kind`, default
    thresholds); with `taps` (a full odd-length symmetric FIR) `coef_filtered` [N, 4, 7] (`fir_series_f64` of `coef`) and `trend`
    [N, 8] = flag, angle_deg, tilt_deg, azimuth_deg, twist_deg of the rotation NEAREST to the filtered matrix
    (`rigid.nearest_rotation`; angles and quaternions themselves are never filtered) and the filtered t; with `grid` = (W [P, M],
    wsum [P]) of `fields` the `residual_map` [N, P, 2] (`field_map_f64` of the record (flag, |e|)) and, where the grid's positions are
    given as a third element grid_xy [P, 2], its `residual_patch` [N, 8] (`patch_stats_f64`); `max_tilt_frame` and
    `max_twist_frame` (-1: no frame has a fit); `slot_rms` [M] (the rms of |e| along the recording, NaN for a slot that was never
    used) and `worst_slots`, the `worst` slots of largest `slot_rms`, descending."""
    from . import rigid as RG
    from .engine import field_map_f64, fir_series_f64, patch_stats_f64, rigid_series
    if isinstance(source, str):
        if source == "start":
            src = RG.source_from_table(table, start_frame)
        elif source == "layout":
            if layout is None:
                raise ValueError("source='layout' needs `layout` [M, 3]")
            src = RG.source_from_layout(layout)
        else:
            raise ValueError("source must be 'start', 'layout' or an [M, 4] array")
    else:
        src = np.asarray(source, dtype=np.float64)
    out = rigid_series(table, src, slots, with_scale, reject_k, gap_rel, device=eng.device.index)
    out["source"] = src
    rg = out["rigid"].cpu().numpy()
    fit = rg[:, RG.FLAG] != 0.0
    nan = lambda v: np.where(fit.reshape((-1,) + (1,) * (v.ndim - 1)), v, np.nan)                   # noqa: E731
    v = rg[:, RG.QX:RG.QZ + 1]
    vn = np.sqrt((v * v).sum(axis=1))
    out["rotvec"] = nan(np.where(vn[:, None] > 0.0, v / np.where(vn > 0.0, vn, 1.0)[:, None], 0.0) * rg[:, RG.ANGLE_DEG, None])
    for name, col in (("tilt_deg", RG.TILT_DEG), ("azimuth_deg", RG.AZIMUTH_DEG), ("twist_deg", RG.TWIST_DEG), ("scale", RG.SCALE),
                      ("rms", RG.RMS)):
        out[name] = nan(rg[:, col])
    out["shift"] = nan(rg[:, RG.PMX:RG.PMZ + 1] - rg[:, RG.QMX:RG.QMZ + 1])
    out["share"] = nan(RG.rigid_share(rg[:, RG.RMS], rg[:, RG.RMS0]))
    out["kind"] = RG.kind(rg)
    if taps is not None:
        cf = fir_series_f64(out["coef"], taps, 3, min_coverage, device=eng.device.index)
        ch = cf.cpu().numpy()
        ok = (ch[:, :, 0] == 3.0).all(axis=1)
        Rf = RG.nearest_rotation(np.where(ok[:, None, None], ch[:, :3, 1:4], np.eye(3)[None]))
        out["coef_filtered"] = cf
        out["trend"] = np.concatenate([ok[:, None].astype(np.float64), np.where(ok[:, None], RG.angles(Rf), 0.0),
                                       np.where(ok[:, None], ch[:, 3, 1:4], 0.0)], axis=1)
    res = out["residual"]
    if grid is not None:
        W, wsum = grid[0], grid[1]
        mag = torch.sqrt((res[..., 1] * res[..., 1] + res[..., 2] * res[..., 2]) + res[..., 3] * res[..., 3])
        out["residual_map"] = field_map_f64(torch.stack([res[..., 0], mag], dim=-1), W, wsum, min_coverage, 1, device=eng.device.index)
        if len(grid) > 2:
            out["residual_patch"] = patch_stats_f64(out["residual_map"], grid[2], 0, 1.0, 0.0, device=eng.device.index)
    tilt, twist = np.where(fit, rg[:, RG.TILT_DEG], -1.0), np.where(fit, np.abs(rg[:, RG.TWIST_DEG]), -1.0)
    out["max_tilt_frame"] = int(np.argmax(tilt)) if fit.any() else -1
    out["max_twist_frame"] = int(np.argmax(twist)) if fit.any() else -1
    rh = res.cpu().numpy()
    used = rh[..., 0].sum(axis=0)
    ee = (rh[..., 1:] * rh[..., 1:]).sum(axis=2).sum(axis=0)
    out["slot_rms"] = np.where(used > 0.0, np.sqrt(ee / np.where(used > 0.0, used, 1.0)), np.nan)
    order = np.argsort(-np.where(used > 0.0, out["slot_rms"], -1.0), kind="stable")
    out["worst_slots"] = order[:min(int(worst), int((used > 0.0).sum()))].astype(np.int64)
    return out


RIGID_FRAME_COLUMNS = ("frameno", "kind", "flag", "count", "n_used", "shift_x", "shift_y", "shift_z", "rot_x", "rot_y", "rot_z",
                       "angle_deg", "tilt_deg", "azimuth_deg", "twist_deg", "tx", "ty", "tz", "scale", "rms", "rms0", "share", "gap")
RIGID_TREND_COLUMNS = ("angle_f", "tilt_f", "azimuth_f", "twist_f", "tx_f", "ty_f", "tz_f")


def to_rigid_frame(result, frame_offset=0, path=None):
    """The sheet of `rigid_analysis`: one row `RIGID_FRAME_COLUMNS` per frame - `kind` as its name, flag, count and n_used as
    integers, everything from shift_x to share empty (NaN) where the frame has no fit - and with a trend also
    `RIGID_TREND_COLUMNS` (empty where the filter has no value).  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    from . import rigid as RG
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    rg = host(result["rigid"]).astype(np.float64)
    if rg.ndim != 2 or rg.shape[1] != L.RIGID_COLS:
        raise ValueError(f"rigid must be [N, {L.RIGID_COLS}]")
    N = rg.shape[0]
    fit = rg[:, RG.FLAG] != 0.0
    nan = lambda v: np.where(fit, v, np.nan)                                                        # noqa: E731
    kinds = np.asarray(result["kind"]) if "kind" in result else RG.kind(rg)
    v = rg[:, RG.QX:RG.QZ + 1]
    vn = np.sqrt((v * v).sum(axis=1))
    rot = np.where(vn[:, None] > 0.0, v / np.where(vn > 0.0, vn, 1.0)[:, None], 0.0) * rg[:, RG.ANGLE_DEG, None]
    cols = {"frameno": np.arange(N, dtype=np.int64) + int(frame_offset), "kind": [RG.KIND_NAMES[int(k)] for k in kinds],
            "flag": rg[:, RG.FLAG].astype(np.int64), "count": rg[:, RG.COUNT].astype(np.int64), "n_used": rg[:, RG.N_USED].astype(np.int64)}
    for k, name in enumerate(("shift_x", "shift_y", "shift_z")):
        cols[name] = nan(rg[:, RG.PMX + k] - rg[:, RG.QMX + k])
    for k, name in enumerate(("rot_x", "rot_y", "rot_z")):
        cols[name] = nan(rot[:, k])
    for name, c in (("angle_deg", RG.ANGLE_DEG), ("tilt_deg", RG.TILT_DEG), ("azimuth_deg", RG.AZIMUTH_DEG), ("twist_deg", RG.TWIST_DEG),
                    ("tx", RG.TX), ("ty", RG.TY), ("tz", RG.TZ), ("scale", RG.SCALE), ("rms", RG.RMS), ("rms0", RG.RMS0)):
        cols[name] = nan(rg[:, c])
    cols["share"] = nan(RG.rigid_share(rg[:, RG.RMS], rg[:, RG.RMS0]))
    cols["gap"] = rg[:, RG.GAP]
    names = list(RIGID_FRAME_COLUMNS)
    if "trend" in result:
        tr = host(result["trend"])
        if tr.shape != (N, 8):
            raise ValueError("trend must be [N, 8]")
        for k, name in enumerate(RIGID_TREND_COLUMNS):
            cols[name] = np.where(tr[:, 0] == 1.0, tr[:, 1 + k], np.nan)
        names += list(RIGID_TREND_COLUMNS)
    df = pd.DataFrame(cols, columns=names)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- noise-weighted rigid motion (k_rigid_ml.hip): the pose under the noise of every point, its covariance, chi^2, the distances ------
def _rigid_uncertainty_args(n, source, reject_k, iters, k, worst):
    """`rigid_uncertainty`'s own argument checks (no device needed), reject_k and iters included so that nothing it can refuse by
    value waits for the device; the entries' shape checks are `engine._rigid_args` and `engine._rigid_ml_args`.  -> (source frame or
    None, k, worst)."""
    frame = None
    if isinstance(source, str):
        if source not in ("start", "layout"):
            raise ValueError("source must be 'start', 'layout' or a frame of the table")
        frame = 0 if source == "start" else None
    else:
        if isinstance(source, (bool, np.bool_)) or int(source) != source or not (0 <= int(source) < n):
            raise ValueError(f"source frame {source} outside the table's {n} frames")
        frame = int(source)
    if not (np.isfinite(float(reject_k)) and float(reject_k) >= 0.0):
        raise ValueError(f"reject_k {reject_k} must be finite and >= 0")
    if isinstance(iters, (bool, np.bool_)) or int(iters) != iters or not (1 <= int(iters) <= L.RIGID_ML_MAX_ITERS):
        raise ValueError(f"iters {iters} must be an integer in [1, {L.RIGID_ML_MAX_ITERS}]")
    if not (np.isfinite(float(k)) and float(k) > 0.0):
        raise ValueError("k must be finite and > 0")
    if int(worst) != worst or int(worst) < 0:
        raise ValueError("worst must be an integer >= 0")
    return frame, float(k), int(worst)


def rigid_uncertainty_columns(ml, pc, mh, kk=3.0, worst=5):
    """The per-frame columns `rigid_uncertainty` derives from the host copies of `ml` [N, 40], `pcov` [N, 22] and `mahal` [N, M, 3]
    (no device needed) -> a dict: tilt_deg, azimuth_deg, twist_deg, t2_tilt, centre, sigma_rot_deg, sigma_centre, significant,
    twist_z, chi2_dof, tilt_limit_deg, consistent, worst_frames, slot_mahal, worst_slots (NaN where the frame has no weighted fit)."""
    from . import rigid as RG
    ml, pc, mh = np.asarray(ml, dtype=np.float64), np.asarray(pc, dtype=np.float64), np.asarray(mh, dtype=np.float64)
    out = {}
    fit = ml[:, RG.ML_FLAG] == 2.0
    nan = lambda v: np.where(fit.reshape((-1,) + (1,) * (v.ndim - 1)), v, np.nan)                   # noqa: E731
    for name, col in (("tilt_deg", RG.ML_TILT_DEG), ("azimuth_deg", RG.ML_AZIMUTH_DEG), ("twist_deg", RG.ML_TWIST_DEG),
                      ("t2_tilt", RG.ML_T2_TILT)):
        out[name] = nan(ml[:, col])
    out["centre"] = nan(ml[:, RG.ML_CX:RG.ML_CX + 3])
    out["sigma_rot_deg"], out["sigma_centre"] = RG.pose_sigma(ml, pc)
    with np.errstate(all="ignore"):
        out["significant"] = fit & (ml[:, RG.ML_T2_TILT] > kk * kk)
        out["twist_z"] = nan(ml[:, RG.ML_TWIST_DEG] / (np.sqrt(ml[:, RG.ML_VAR_TWIST]) * _DEG))
        out["chi2_dof"] = np.where(fit & (ml[:, RG.ML_DOF] >= 1.0), ml[:, RG.ML_CHI2] / np.where(ml[:, RG.ML_DOF] >= 1.0, ml[:, RG.ML_DOF], 1.0), np.nan)
        nxx, nxy, nyy = ml[:, RG.ML_NXX], ml[:, RG.ML_NXY], ml[:, RG.ML_NYY]
        lam = 0.5 * (nxx + nyy) + np.sqrt(0.25 * (nxx - nyy) ** 2 + nxy * nxy)
        out["tilt_limit_deg"] = nan(np.arcsin(np.minimum(kk * np.sqrt(lam), 1.0)) * _DEG)
    out["consistent"] = RG.consistent(ml, kk)
    ratio = np.where(np.isnan(out["chi2_dof"]), -1.0, out["chi2_dof"])
    out["worst_frames"] = np.argsort(-ratio, kind="stable")[:min(worst, int((ratio >= 0.0).sum()))].astype(np.int64)
    used = mh[..., 0].sum(axis=0)
    out["slot_mahal"] = np.where(used > 0.0, mh[..., 1].sum(axis=0) / np.where(used > 0.0, used, 1.0), np.nan)
    order = np.argsort(-np.where(used > 0.0, out["slot_mahal"], -1.0), kind="stable")
    out["worst_slots"] = order[:min(worst, int((used > 0.0).sum()))].astype(np.int64)
    return out


def rigid_uncertainty(eng: Engine, table, cam: L.Camera, obs_cov, source="start", reject_k=0.0, iters=8, k=3.0, taps=None,
                      layout=None, slots=None, min_marker_size_px=5.0, piv_rel=1e-12, min_coverage=0.5, worst=5):
    """The rigid motion of every frame under the noise of its 3-D points, and how good it is: `rigid_series`
    (with_scale off) for the start, `solve3d_cov` with an exact camera for the covariance of every point - the weights are the pixel
    noise `obs_cov`: a camera error moves all markers together and is no independent noise -, the source row's covariance as
    `source_cov` where the source is a frame of the table ("start" = frame 0, or a frame number; "layout" registers against `layout`
    [M, 3], an exact source), then `rigid_ml_series`.  Returns a dict: the device tensors `ml`, `pcov`, `coef`, `mahal`, `rigid`,
    `residual`, `cov` and the host array `source`; per frame on the host (NaN where the frame has no weighted fit) `tilt_deg`,
    `azimuth_deg`, `twist_deg`, `centre` [N, 3], `sigma_rot_deg` [N, 3], `sigma_centre` [N, 3] (`rigid.pose_sigma`), `t2_tilt` and
    `significant` = t2_tilt > k^2 (two degrees of freedom: a false-alarm rate of exp(-k^2 / 2), as `misalignment_uncertainty`),
    `twist_z` = twist / sigma_twist, `chi2_dof`, `consistent` (`rigid.consistent`), `tilt_limit_deg` = the smallest tilt the frame
    could tell from zero in its worst direction, k sqrt(lambda_max(Sigma_n)) in degrees; `worst_frames` (largest chi2 / dof,
    descending) and `worst_slots` (largest mean Mahalanobis distance^2 along the recording), `worst` of each; with `taps` the
    `coef_filtered` and `trend` [N, 8] of `rigid_analysis`, from filtered matrices through `rigid.nearest_rotation`."""
    from . import rigid as RG
    from .engine import fir_series_f64, rigid_ml_series, rigid_series, solve3d_cov
    table = eng._table32(table)
    n = int(table.shape[0])
    frame, kk, worst = _rigid_uncertainty_args(n, source, reject_k, iters, k, worst)
    if frame is None:
        if layout is None:
            raise ValueError("source='layout' needs `layout` [M, 3]")
        src = RG.source_from_layout(layout)
    else:
        src = RG.source_from_table(table, frame)
    dev = eng.device.index
    start = rigid_series(table, src, slots, False, reject_k, want=("rigid", "residual"), device=dev)
    cov = solve3d_cov(table, cam, obs_cov, None, None, None, min_marker_size_px, piv_rel, device=dev)["cov"]
    source_cov = None if frame is None else cov[frame].contiguous()
    out = rigid_ml_series(table, src, cov, start["rigid"], start["residual"], source_cov, iters, piv_rel, device=dev)
    out.update(rigid=start["rigid"], residual=start["residual"], cov=cov, source=src, k=kk)
    out.update(rigid_uncertainty_columns(out["ml"].cpu().numpy(), out["pcov"].cpu().numpy(), out["mahal"].cpu().numpy(), kk, worst))
    if taps is not None:
        cf = fir_series_f64(out["coef"], taps, 3, min_coverage, device=dev)
        ch = cf.cpu().numpy()
        ok = (ch[:, :, 0] == 3.0).all(axis=1)
        Rf = RG.nearest_rotation(np.where(ok[:, None, None], ch[:, :3, 1:4], np.eye(3)[None]))
        out["coef_filtered"] = cf
        out["trend"] = np.concatenate([ok[:, None].astype(np.float64), np.where(ok[:, None], RG.angles(Rf), 0.0),
                                       np.where(ok[:, None], ch[:, 3, 1:4], 0.0)], axis=1)
    return out


RIGID_UNCERTAINTY_COLUMNS = ("frameno", "flag", "n_start", "n_used", "steps", "tilt_deg", "azimuth_deg", "twist_deg", "cx", "cy", "cz",
                             "sigma_rot_x_deg", "sigma_rot_y_deg", "sigma_rot_z_deg", "sigma_cx", "sigma_cy", "sigma_cz", "t2_tilt",
                             "significant", "tilt_limit_deg", "twist_z", "chi2", "dof", "chi2_dof", "chi2_start", "consistent",
                             "step_rot", "step_c")


def to_rigid_uncertainty_frame(result, frame_offset=0, path=None):
    """The sheet of `rigid_uncertainty`: one row `RIGID_UNCERTAINTY_COLUMNS` per frame - the counts as integers, everything that
    needs the weighted fit empty (NaN) where the frame has none - and with a trend also `RIGID_TREND_COLUMNS`.  `path`: also
    written, as .csv or as .xlsx."""
    import pandas as pd
    from . import rigid as RG
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    ml = host(result["ml"]).astype(np.float64)
    if ml.ndim != 2 or ml.shape[1] != L.RIGID_ML_COLS:
        raise ValueError(f"ml must be [N, {L.RIGID_ML_COLS}]")
    N = ml.shape[0]
    f64 = lambda name: np.asarray(result[name], dtype=np.float64)                                   # noqa: E731
    cols = {"frameno": np.arange(N, dtype=np.int64) + int(frame_offset), "flag": ml[:, RG.ML_FLAG].astype(np.int64),
            "n_start": ml[:, RG.ML_N_START].astype(np.int64), "n_used": ml[:, RG.ML_N_USED].astype(np.int64),
            "steps": ml[:, RG.ML_STEPS].astype(np.int64), "tilt_deg": f64("tilt_deg"), "azimuth_deg": f64("azimuth_deg"),
            "twist_deg": f64("twist_deg")}
    for i, name in enumerate(("cx", "cy", "cz")):
        cols[name] = f64("centre")[:, i]
    for i, name in enumerate(("sigma_rot_x_deg", "sigma_rot_y_deg", "sigma_rot_z_deg")):
        cols[name] = f64("sigma_rot_deg")[:, i]
    for i, name in enumerate(("sigma_cx", "sigma_cy", "sigma_cz")):
        cols[name] = f64("sigma_centre")[:, i]
    have = ml[:, RG.ML_FLAG] != 0.0
    cols.update({"t2_tilt": f64("t2_tilt"), "significant": np.asarray(result["significant"]).astype(bool),
                 "tilt_limit_deg": f64("tilt_limit_deg"), "twist_z": f64("twist_z"), "chi2": np.where(have, ml[:, RG.ML_CHI2], np.nan),
                 "dof": ml[:, RG.ML_DOF].astype(np.int64), "chi2_dof": f64("chi2_dof"),
                 "chi2_start": np.where(have, ml[:, RG.ML_CHI2_START], np.nan), "consistent": np.asarray(result["consistent"]).astype(bool),
                 "step_rot": ml[:, RG.ML_STEP_ROT], "step_c": ml[:, RG.ML_STEP_C]})
    names = list(RIGID_UNCERTAINTY_COLUMNS)
    if "trend" in result:
        tr = host(result["trend"])
        if tr.shape != (N, 8):
            raise ValueError("trend must be [N, 8]")
        for i, name in enumerate(RIGID_TREND_COLUMNS):
            cols[name] = np.where(tr[:, 0] == 1.0, tr[:, 1 + i], np.nan)
        names += list(RIGID_TREND_COLUMNS)
    df = pd.DataFrame(cols, columns=names)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- bonnet contact geometry along a recording (k_sphere.hip): the held sphere, the contact plane, offset, spot and normal ----------
def bonnet_analysis(eng: Engine, table: torch.Tensor, still=(0, 8), sphere=None, contact_depth=0.1, source="start", fit_slots=None,
                    taps=None, grid=None, slots=None, piv_rel=1e-9, gap_rel=1e-3, reject_k=3.0, min_coverage=0.5):
    """`sphere_series` for every frame of a recording of a bonnet pressed against a workpiece.  The camera sits inside
    the tool, so the unloaded sphere is a constant of the sensor in the table's coordinates: unless `sphere` = (Cx, Cy, Cz, R) is
    given it is fitted per frame over the UNLOADED frames `still` = (a, b) (over `fit_slots`, one round of rejection at `reject_k`)
    and combined by `sphere.combine` (refused unless three frames fit); the whole recording then runs against that HELD sphere - a
    per-frame fit over a pressed cap is wrong by millimetres.  `source`: "start" resolves the displacement against frame still[0] of
    the table itself (`rigid.source_from_table`), an [M, 4] array against that, None leaves `decomp` out.  Returns a dict: the
    device tensors `sphere` [N, 31], `radial` [N, M, 2] and, with a source, `decomp` [N, M, 4]; the host arrays `held` [4], `source`
    and, where the sphere was fitted here, `still` (what `sphere.combine` returns); everything `sphere.summary` reads off the rows
    (kind, offset, tilt_deg, azimuth_deg, spot_radius, plane_rms, normal, spot_centre, depth_max, first_contact, max_offset_frame,
    max_tilt_frame, share); with `taps` (a full odd-length symmetric FIR) `trend_filtered` [N, 1, 15] (`fir_series_f64` of
    `sphere.trend_record`) and `trend` [N, 10] = flag, offset, spot centre, the RENORMALISED filtered normal and the angles
    recomputed from it (`sphere.trend`; angles are never filtered); with `grid` = (W [P, M], wsum [P]) of `fields` the `depth_map`
    [N, P, 2] (`field_map_f64` of the record (flag, -rho): how far inside the held sphere the shell lies) and, where the grid's
    positions are given as a third element grid_xy [P, 2], its `depth_patch` [N, 8] (`patch_stats_f64` at `contact_depth`)."""
    from . import rigid as RG
    from . import sphere as SP
    from .engine import field_map_f64, fir_series_f64, patch_stats_f64, sphere_series
    dev = eng.device.index
    a, b = int(still[0]), int(still[1])
    if isinstance(source, str):
        if source != "start":
            raise ValueError("source must be 'start', None or an [M, 4] array")
        src = RG.source_from_table(table, a)
    else:
        src = None if source is None else np.asarray(source, dtype=np.float64)
    out = {}
    if sphere is None:
        fit = sphere_series(table, None, fit_slots, slots, None, contact_depth, piv_rel, gap_rel, reject_k, (a, b), ("sphere",), dev)
        held = SP.combine(fit["sphere"])
        if held["frames"] < 3:
            raise ValueError(f"only {held['frames']} of the still frames [{a}, {b}) give a sphere: three are needed")
        out["still"] = held
        sphere = held["sphere"]
    sphere = np.asarray(sphere, dtype=np.float64).reshape(-1)
    out.update(sphere_series(table, sphere, fit_slots, slots, src, contact_depth, piv_rel, gap_rel, 0.0, device=dev))
    out["held"], out["source"] = sphere, src
    rows = out["sphere"].cpu().numpy()
    out.update(SP.summary(rows))
    if taps is not None:
        out["trend_filtered"] = fir_series_f64(SP.trend_record(rows), taps, 7, min_coverage, device=dev)
        out["trend"] = SP.trend(out["trend_filtered"])
    if grid is not None:
        rad = out["radial"]
        out["depth_map"] = field_map_f64(torch.stack([rad[..., 0], -rad[..., 1]], dim=-1), grid[0], grid[1], min_coverage, 1, device=dev)
        if len(grid) > 2:
            out["depth_patch"] = patch_stats_f64(out["depth_map"], grid[2], 0, 1.0, float(contact_depth), device=dev)
    return out


BONNET_FRAME_COLUMNS = ("frameno", "kind", "flag", "n_used", "n_contact", "deepest", "rms_fit", "depth_mean", "depth_max", "offset",
                        "spot_radius", "tilt_deg", "azimuth_deg", "nx", "ny", "nz", "spot_x", "spot_y", "spot_z", "plane_rms", "gap")
BONNET_TREND_COLUMNS = ("offset_f", "spot_x_f", "spot_y_f", "spot_z_f", "nx_f", "ny_f", "nz_f", "tilt_f", "azimuth_f")


def to_bonnet_frame(result, frame_offset=0, path=None):
    """The sheet of `bonnet_analysis`: one row `BONNET_FRAME_COLUMNS` per frame - `kind` as its name, flag, n_used, n_contact and
    deepest as integers, depth_mean and depth_max empty (NaN) without a contact slot, everything from offset to plane_rms empty
    without a contact plane - and with a trend also `BONNET_TREND_COLUMNS` (empty where the filter has no value).  `path`: also
    written, as .csv or as .xlsx."""
    import pandas as pd
    from . import sphere as SP
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    r = host(result["sphere"]).astype(np.float64)
    if r.ndim != 2 or r.shape[1] != L.SPHERE_COLS:
        raise ValueError(f"sphere must be [N, {L.SPHERE_COLS}]")
    N = r.shape[0]
    flat, touch = r[:, SP.FLAG] == 3.0, r[:, SP.FLAG] >= 2.0
    cols = {"frameno": np.arange(N, dtype=np.int64) + int(frame_offset), "kind": [SP.KIND_NAMES[int(k)] for k in SP.kind(r)]}
    for name, c in (("flag", SP.FLAG), ("n_used", SP.N_USED), ("n_contact", SP.N_CONTACT), ("deepest", SP.DEEPEST)):
        cols[name] = r[:, c].astype(np.int64)
    cols["rms_fit"] = np.where(r[:, SP.FLAG] != 0.0, r[:, SP.RMS_FIT], np.nan)
    for name, c in (("depth_mean", SP.DEPTH_MEAN), ("depth_max", SP.DEPTH_MAX)):
        cols[name] = np.where(touch, r[:, c], np.nan)
    for name, c in (("offset", SP.OFFSET), ("spot_radius", SP.SPOT_RADIUS), ("tilt_deg", SP.TILT_DEG), ("azimuth_deg", SP.AZIMUTH_DEG),
                    ("nx", SP.NX), ("ny", SP.NY), ("nz", SP.NZ), ("spot_x", SP.SX), ("spot_y", SP.SY), ("spot_z", SP.SZ),
                    ("plane_rms", SP.PLANE_RMS)):
        cols[name] = np.where(flat, r[:, c], np.nan)
    cols["gap"] = r[:, SP.GAP]
    names = list(BONNET_FRAME_COLUMNS)
    if "trend" in result:
        tr = host(result["trend"])
        if tr.shape != (N, 10):
            raise ValueError("trend must be [N, 10]")
        for k, name in enumerate(BONNET_TREND_COLUMNS):
            cols[name] = np.where(tr[:, 0] == 1.0, tr[:, 1 + k], np.nan)
        names += list(BONNET_TREND_COLUMNS)
    df = pd.DataFrame(cols, columns=names)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- shear, torsion and strain along a recording (k_motion.hip): the affine part of the field, globally and around every marker ----
def motion_analysis(eng: Engine, table: torch.Tensor, ref_frame=0, slots=None, reject_k=0.0, neighbours=6, radius=None, min_count=4,
                    det_rel=0.01, taps=None, min_coverage=0.5):
    """The decomposition of the displacement field of every frame of a table [N, M, 10]: drag, twist about the
    normal, dilation and shear, what is left once that smooth motion is removed, and the same around every marker.  The rest
    positions are the X, Y of frame `ref_frame`; of the selected slots (`slots`, as `Engine.axis_displacement`) those without a
    3-D point there are masked out.  Returns a dict of device tensors (float64 unless said): `axis` [N, M, 4], `total` [N, 5]
    (`Engine.axis_displacement`); `pos` [M, 2] (zeros where masked out) and `nbr` int32 [M, neighbours]
    (`strain.neighbour_lists` within `radius`); `grad` [N, 3, 4], `strain` [N, 16], `residual` [N, M, 4]
    (`engine.motion_series_f64` with `reject_k`); `local` [N, M, 8] (`engine.local_strain_f64` with `min_count`, `det_rel`); and
    with `taps` (a full odd-length symmetric FIR, `filters.lowpass_taps`): `grad_filtered` [N, 3, 7] = flag, trend and residual
    of t_k, g_kx, g_ky over the frames that have a fit (`fir_series_f64`), and `trend` [N, 11] = flag (1 where the frame has a
    trend), then `strain.invariants` OF THE FILTERED gradient - angles and roots are never filtered themselves.
    The call SYNCHRONISES its stream twice: the reference frame's row is copied to the host for `pos` and the neighbour lists, and
    with `taps` the filtered gradient is, for the trend (NumPy).  It is an analysis off the timed path, as `misalignment_analysis`."""
    from .engine import fir_series_f64, local_strain_f64, motion_series_f64
    from .strain import invariants, neighbour_lists
    axis, total = eng.axis_displacement(table, ref_frame, slots)
    m = int(axis.shape[1])
    row = table[int(ref_frame)].detach().to(torch.float64).cpu().numpy()
    valid = (row[:, 0].astype(np.int64) & L.FLAG_XYZ) != 0
    if slots is not None:
        chosen = np.zeros(m, dtype=bool)
        chosen[np.asarray(slots, dtype=np.int64).reshape(-1)] = True
        valid &= chosen
    pos = np.where(valid[:, None], row[:, 6:8], 0.0)
    nbr = neighbour_lists(pos, neighbours, radius, valid)
    dev = eng.device.index
    pos_d = torch.as_tensor(pos, dtype=torch.float64, device=eng.device)
    nbr_d = torch.as_tensor(nbr, dtype=torch.int32, device=eng.device)
    out = {"axis": axis, "total": total, "pos": pos_d, "nbr": nbr_d}
    out.update(motion_series_f64(axis, pos_d, np.flatnonzero(valid), reject_k, device=dev))
    out["local"] = local_strain_f64(axis, pos_d, nbr_d, min_count, det_rel, device=dev)
    if taps is not None:
        gf = fir_series_f64(out["grad"], taps, 3, min_coverage, device=dev)
        g = gf[..., :4].detach().cpu().numpy().copy()
        ok = (g[..., 0] == 3.0).all(axis=1)
        g[..., 0] = ok[:, None]
        out["grad_filtered"] = gf
        out["trend"] = torch.as_tensor(np.concatenate([ok[:, None].astype(np.float64), invariants(g)], axis=1), device=eng.device)
    return out


MOTION_FRAME_COLUMNS = ("frameno", "flag", "count", "n_used", "tX", "tY", "tZ", "gXx", "gXy", "gYx", "gYy", "gZx", "gZy", "dilation",
                        "omega", "e1", "e2", "max_shear", "shear_deg", "rot_deg", "lambda1", "lambda2", "tilt_deg", "rms_inplane",
                        "rms_z", "worst")
MOTION_TREND_COLUMNS = ("dilation_f", "omega_f", "e1_f", "e2_f", "max_shear_f", "shear_deg_f", "rot_deg_f", "lambda1_f", "lambda2_f",
                        "tilt_deg_f")


def to_motion_frame(strain, grad, trend=None, frame_offset=0, path=None):
    """The sheet of `motion_analysis`: one row per frame with `MOTION_FRAME_COLUMNS` from `strain` [N, 16] and `grad` [N, 3, 4], and
    with `trend` [N, 11] also `MOTION_TREND_COLUMNS`.  tX .. rms_z are NaN (empty cells) where the frame has no fit (flag 0; worst
    is -1 there), the trend columns where it has no trend.  `path`: also written as .xlsx (`xlsx_io.dataframe_to_xlsx`)."""
    import pandas as pd
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    st, gr = host(strain), host(grad)
    if st.ndim != 2 or st.shape[1] != L.STRAIN_COLS or gr.shape != (st.shape[0], 3, 4):
        raise ValueError(f"strain must be [N, {L.STRAIN_COLS}] and grad [N, 3, 4]")
    fit = (st[:, 0] != 0)[:, None]
    cols = {"frameno": np.arange(st.shape[0], dtype=np.int64) + int(frame_offset), "flag": st[:, 0].astype(np.int64),
            "count": st[:, 1].astype(np.int64), "n_used": st[:, 2].astype(np.int64)}
    g = np.where(fit, np.concatenate([gr[:, :, 1], gr[:, :, 2:4].reshape(-1, 6)], axis=1), np.nan)
    for k, name in enumerate(MOTION_FRAME_COLUMNS[4:13]):
        cols[name] = g[:, k]
    v = np.where(fit, st[:, 3:15], np.nan)
    for k, name in enumerate(MOTION_FRAME_COLUMNS[13:25]):
        cols[name] = v[:, k]
    cols["worst"] = st[:, 15].astype(np.int64)
    if trend is not None:
        tr = host(trend)
        if tr.shape != (st.shape[0], 11):
            raise ValueError("trend must be [N, 11]")
        t = np.where((tr[:, 0] != 0)[:, None], tr[:, 1:], np.nan)
        for k, name in enumerate(MOTION_TREND_COLUMNS):
            cols[name] = t[:, k]
    df = pd.DataFrame(cols)
    if path is not None:
        from .xlsx_io import dataframe_to_xlsx
        dataframe_to_xlsx(df, path)
    return df


# ---- contact maps along a recording (k_field.hip): field on a grid, contact patch, centre, with their trend ----------------------
_CONTACT_COMPONENT = {"x": 0, "y": 1, "z": 2, "xyz": -1}
CONTACT_FRAME_COLUMNS = ("frameno", "flag", "covered", "count", "area_mm2", "sum", "cx", "cy", "peak", "peak_x", "peak_y")
CONTACT_TREND_COLUMNS = ("sum_f", "cx_f", "cy_f")


def _contact_args(n, m, grid_shape, bandwidth, component, sign, threshold, ref_frame, min_coverage, keep_maps, max_map_bytes):
    """`contact_analysis`'s argument checks (no device needed): -> (P, frames per range, sorted kept frames) or ValueError."""
    if len(tuple(grid_shape)) != 2 or int(grid_shape[0]) < 1 or int(grid_shape[1]) < 1:
        raise ValueError("grid_shape must be (rows >= 1, columns >= 1)")
    P = int(grid_shape[0]) * int(grid_shape[1])
    if P > L.FIELD_MAX_POINTS:
        raise ValueError(f"grid_shape {tuple(grid_shape)} has more than VBS_FIELD_MAX_POINTS = {L.FIELD_MAX_POINTS} points")
    if m > L.FIELD_MAX_SLOTS:
        raise ValueError(f"the table's {m} slots exceed VBS_FIELD_MAX_SLOTS = {L.FIELD_MAX_SLOTS}")
    if component not in _CONTACT_COMPONENT:
        raise ValueError(f"component must be one of {sorted(_CONTACT_COMPONENT)}")
    if float(sign) not in (1.0, -1.0):
        raise ValueError("sign must be +1 or -1")
    if not (float(threshold) >= 0.0):
        raise ValueError("threshold must be >= 0")
    if bandwidth is not None and not (np.isfinite(float(bandwidth)) and float(bandwidth) > 0.0):
        raise ValueError("bandwidth must be finite and > 0")
    if not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    if not (0.0 < float(min_coverage) <= 1.0):
        raise ValueError("min_coverage must lie in (0, 1]")
    keep = sorted({int(f) for f in keep_maps})
    if keep and (keep[0] < 0 or keep[-1] >= n):
        raise ValueError(f"keep_maps outside the table's {n} frames")
    per_frame = P * 4 * 8
    if int(max_map_bytes) < per_frame:
        raise ValueError(f"max_map_bytes {max_map_bytes} holds no frame of the map ({per_frame} bytes)")
    return P, int(max_map_bytes) // per_frame, keep


def contact_analysis(eng: Engine, table: torch.Tensor, grid_shape=(64, 64), bandwidth=None, component="z", sign=1.0, threshold=0.1,
                     ref_frame=0, slots=None, taps=None, min_coverage=0.5, keep_maps=(), max_map_bytes=256 << 20):
    """The contact along a recording (the reference draws arrows on the markers only) from a table [N, M, 10]:
    the displacement of every slot against `ref_frame` (`Engine.axis_displacement`) spread over a regular grid by a gap-aware
    Gaussian smoother (`field_map_f64`; nodes = the X, Y of the selected slots valid in `ref_frame`, other slots get zero weight;
    `bandwidth` default `fields.default_bandwidth`), and per frame the contact patch of that map (`patch_stats_f64`): the grid
    points where `sign` * `component` ("x", "y", "z", or "xyz" = the norm) reaches `threshold` (in the table's units).  The maps
    are computed in frame ranges of at most `max_map_bytes` and dropped again, except the frames listed in `keep_maps`; no
    result depends on the ranges.  Returns a dict: `grid_xy` [P, 2], `cell_area`, `bandwidth`, `total` [N, 5], `patch` [N, 8],
    `maps` {frame: [P, 4]} and, with `taps` (a full odd-length symmetric FIR), `patch_filtered` [N, 7] = flag, trend and
    residual of S, cx, cy over the frames that have a patch with a centre (flag 2)."""
    from . import fields
    from .engine import field_map_f64, fir_series_f64, patch_stats_f64
    n, m = int(table.shape[0]), int(table.shape[1])
    P, per_range, keep = _contact_args(n, m, grid_shape, bandwidth, component, sign, threshold, ref_frame, min_coverage, keep_maps,
                                       max_map_bytes)
    dev = eng.device.index
    axis, total = eng.axis_displacement(table, ref_frame, slots)
    ref = table[int(ref_frame)].detach().cpu().numpy()
    valid = (ref[:, 0].astype(np.int64) & L.FLAG_XYZ) != 0
    if slots is not None:
        pick = np.zeros(m, dtype=bool)
        pick[np.asarray(slots, dtype=np.int64).reshape(-1)] = True
        valid &= pick
    if not valid.any():
        raise ValueError(f"no selected slot has a 3-D point in ref_frame {ref_frame}")
    nodes = np.where(valid[:, None], ref[:, 6:8].astype(np.float64), np.nan)
    h = fields.default_bandwidth(nodes) if bandwidth is None else float(bandwidth)
    grid_xy, cell_area = fields.grid_over(nodes, grid_shape, 0.0)
    W = fields.gaussian_weights(nodes, grid_xy, h)
    Wd = torch.from_numpy(W).to(eng.device)
    wsum = torch.from_numpy(fields.row_sums(W)).to(eng.device)
    grid_d = torch.from_numpy(grid_xy).to(eng.device)
    patch = torch.empty((n, L.PATCH_COLS), dtype=torch.float64, device=eng.device)
    maps = {}
    for a in range(0, n, per_range):
        b = min(n, a + per_range)
        mp = field_map_f64(axis, Wd, wsum, min_coverage, 3, (a, b), device=dev)
        patch[a:b] = patch_stats_f64(mp, grid_d, _CONTACT_COMPONENT[component], sign, threshold, device=dev)
        for f in keep:
            if a <= f < b:
                maps[f] = mp[f - a].clone()
    out = {"grid_xy": grid_d, "cell_area": cell_area, "bandwidth": h, "total": total, "patch": patch, "maps": maps}
    if taps is not None:
        rec = torch.stack([(patch[:, 0] == 2.0).to(torch.float64), patch[:, 3], patch[:, 4], patch[:, 5]], dim=1)
        out["patch_filtered"] = fir_series_f64(rec[:, None, :], taps, 3, min_coverage, device=dev)[:, 0]
    return out


def to_contact_frame(patch, cell_area, grid_xy, patch_filtered=None, frame_offset=0, path=None):
    """The sheet of `contact_analysis`: one row per frame with `CONTACT_FRAME_COLUMNS` from `patch` [N, 8] - area_mm2 = count *
    `cell_area`, peak_x / peak_y the grid point of the peak - and with `patch_filtered` [N, 7] also `CONTACT_TREND_COLUMNS`.
    cx .. peak_y are NaN (empty cells) where the frame has no patch with a centre (flag != 2), the trend columns where it has no
    trend (flag != 3).  `path`: also written, as .csv (`DataFrame.to_csv(index=False)`, the form the drop-in's CSV has) or as
    .xlsx (`xlsx_io.dataframe_to_xlsx`)."""
    import pandas as pd
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    pa, g = host(patch), host(grid_xy)
    if pa.ndim != 2 or pa.shape[1] != L.PATCH_COLS or g.ndim != 2 or g.shape[1] != 2:
        raise ValueError(f"patch must be [N, {L.PATCH_COLS}] and grid_xy [P, 2]")
    has = pa[:, 0] == 2.0
    idx = np.where(has, pa[:, 7], 0).astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= g.shape[0]):
        raise ValueError("a peak index lies outside grid_xy")
    nan = lambda v: np.where(has, v, np.nan).astype(np.float64)                                    # noqa: E731
    cols = {"frameno": np.arange(pa.shape[0], dtype=np.int64) + int(frame_offset), "flag": pa[:, 0].astype(np.int64),
            "covered": pa[:, 1].astype(np.int64), "count": pa[:, 2].astype(np.int64),
            "area_mm2": pa[:, 2].astype(np.float64) * float(cell_area), "sum": pa[:, 3].astype(np.float64),
            "cx": nan(pa[:, 4]), "cy": nan(pa[:, 5]), "peak": nan(pa[:, 6]), "peak_x": nan(g[idx, 0]), "peak_y": nan(g[idx, 1])}
    if patch_filtered is not None:
        pf = host(patch_filtered)
        if pf.shape != (pa.shape[0], 7):
            raise ValueError("patch_filtered must be [N, 7]")
        t = np.where((pf[:, 0] == 3.0)[:, None], pf[:, 1:4], np.nan)
        cols["sum_f"], cols["cx_f"], cols["cy_f"] = t[:, 0], t[:, 1], t[:, 2]
    df = pd.DataFrame(cols)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- displacement spectra along a recording (k_spectrum.hip): fit, peak and phase of every marker in a band -------------------------
_SPECTRUM_AXES = ("x", "y", "z")
SPECTRUM_FRAME_COLUMNS = ("marker_id", "axis", "freq", "amplitude", "phase_deg", "power", "explained", "count")
SPECTRUM_COLS = 6              # freq, amplitude, phase_deg, power, explained, count of `spectral_analysis`'s `marker` and `total`


def _oscillation_series(rec, taps, dev):
    """The record [N, k, 4] = flag, x, y, z that `spectral_analysis` and `envelope_analysis` analyse: the first three values of
    `rec` as they are, or with `taps` their FIR residual over the entries that have a trend (flag 3)."""
    from .engine import fir_series_f64
    if taps is None:
        return rec[..., :4].contiguous()
    f = fir_series_f64(rec, taps, 3, device=dev)
    return torch.cat([(f[..., :1] == 3.0).to(torch.float64), f[..., 4:7]], dim=2)


def _spectrum_args(n, m, freqs, ref_frame, slot_mask, min_count, det_min, axis="z"):
    """`spectral_analysis`'s argument checks (no device needed): -> (freqs [Q], min_count, slot indices or None, axis index)."""
    from . import spectra
    nu = spectra._freqs(freqs)
    if 1 + 4 * nu.size > L.PROJ_MAX_ROWS:
        raise ValueError(f"{nu.size} frequencies need {1 + 4 * nu.size} basis rows, above VBS_PROJ_MAX_ROWS = {L.PROJ_MAX_ROWS}")
    if n > L.PROJ_MAX_FRAMES or m > L.PROJ_MAX_SLOTS:
        raise ValueError(f"the table's {n} frames x {m} slots exceed VBS_PROJ_MAX_FRAMES = {L.PROJ_MAX_FRAMES} or "
                         f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}")
    if not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    mc = max(8, n // 4) if min_count is None else int(min_count)
    if mc < 3:
        raise ValueError("min_count must be >= 3")
    if not (0.0 <= float(det_min) < 0.25):
        raise ValueError("det_min must lie in [0, 0.25)")
    if axis not in _SPECTRUM_AXES:
        raise ValueError(f"axis must be one of {_SPECTRUM_AXES}")
    slots = None
    if slot_mask is not None:
        k = np.asarray(slot_mask)
        if k.shape != (m,):
            raise ValueError(f"slot_mask must be [{m}]: nonzero = the slot takes part")
        slots = np.nonzero(k)[0]
    return nu, mc, slots, _SPECTRUM_AXES.index(axis)


def _peak_rows(peak, M2, nu):
    """peak [s, 3, 7] and M2 [s, 3] (host) -> [s, 3, SPECTRUM_COLS] = freq, amplitude, phase_deg, power, explained, count; the
    first five are NaN where the series has no peak (flag != 2)."""
    from . import spectra
    has = peak[..., 0] == 2.0
    amp, ph = spectra.amplitude_phase(peak[..., 4], peak[..., 5])
    with np.errstate(divide="ignore", invalid="ignore"):
        expl = peak[..., 6] / M2
    nan = lambda v: np.where(has, v, np.nan)                                                      # noqa: E731
    return np.stack([nan(nu[np.where(has, peak[..., 3], 0).astype(np.int64)]), nan(amp), nan(ph), nan(peak[..., 6]), nan(expl),
                     peak[..., 1]], axis=-1)


def spectral_analysis(eng: Engine, table: torch.Tensor, freqs, ref_frame=0, taps=None, slot_mask=None, min_count=None, det_min=1e-3,
                      fps=None, axis="z"):
    """How the displacement oscillates (the reference's Figure 11(b) shows the oscillation and ships no code for
    it) from a table [N, M, 10]: the displacement of every slot against `ref_frame` (`Engine.axis_displacement`; `slot_mask` [M],
    nonzero = the slot takes part) - with `taps` (a full odd-length symmetric FIR) its FIR residual over the entries that have a
    trend (flag 3), so that the trend does not leak into the low bins - projected onto `spectra.harmonic_basis(N, freqs)`
    (`project_series_f64`) and fitted at every frequency (`harmonic_fit_f64`; `min_count` default max(8, N // 4)), and the same
    pair for the per-frame `total` over its complete frames, a record of one series.  `freqs`: cycles per frame, each in
    (0, 0.25] (`spectra.zoom_grid`).  Returns a dict.  Device tensors (float64): `series` [N, M, 4] and `total_series` [N, 1, 4]
    (what was projected), `proj`, `fit` [M, Q, 10], `peak` [M, 3, 7], `total_fit` [1, Q, 10], `total_peak` [1, 3, 7].  Host arrays:
    `freqs` [Q]; `marker` [M, 3, 6] and `total` [3, 6] = per series and axis the peak's freq, amplitude, phase_deg
    (x ~ A cos(theta - phi)), power (the drop in the sum of squares), explained (power / the series' sum of squared deviations,
    from `series_stats_f64`) and count, the first five NaN where there is no peak; the COMMON LINE of `axis`: `common_power` [Q] =
    the sum over the slots, ascending, of the power of every ok bin, `common_bin` its largest (the smallest of equal ones, -1
    without an ok bin), `common_freq`; and the PHASE MAP `phase_map` [M, 3] = ok, amplitude, phase_deg of every slot at that bin.
    With `fps`: `freqs_hz`, `common_freq_hz`."""
    from . import spectra
    from .engine import harmonic_fit_f64, project_series_f64, series_stats_f64
    n, m = int(table.shape[0]), int(table.shape[1])
    nu, mc, slots, ax = _spectrum_args(n, m, freqs, ref_frame, slot_mask, min_count, det_min, axis)
    dev = eng.device.index
    ax_rec, tot = eng.axis_displacement(table, ref_frame, slots)
    Q = int(nu.size)
    basis = torch.from_numpy(spectra.harmonic_basis(n, nu)).to(eng.device)
    out = {"freqs": nu}
    for name, rec in (("", ax_rec), ("total_", tot[:, None, :])):
        series = _oscillation_series(rec, taps, dev)
        proj = project_series_f64(series, basis, 3, device=dev)
        fit, peak = harmonic_fit_f64(proj, Q, mc, det_min, device=dev)
        k = series.shape[1]
        packed = torch.zeros((n, k, L.DISP_COLS), dtype=torch.float64, device=eng.device)     # the layout series_stats_f64 reads
        packed[..., 0] = (series[..., 0] != 0).to(torch.float64)
        M2 = np.empty((k, 3))
        for a in range(3):
            packed[..., 4] = series[..., 1 + a]
            st = series_stats_f64(packed, device=dev).cpu().numpy()
            M2[:, a] = st[:, 2] * st[:, 2] * (st[:, 0] - 1.0)
        out.update({name + "series": series, name + "proj": proj, name + "fit": fit, name + "peak": peak})
        rows = _peak_rows(peak.cpu().numpy(), M2, nu)
        out["marker" if not name else "total"] = rows if not name else rows[0]
    fh = out["fit"].cpu().numpy()
    ok, a, b, p = fh[..., 0] != 0, fh[..., 1 + 3 * ax], fh[..., 2 + 3 * ax], fh[..., 3 + 3 * ax]
    common = np.zeros(Q)
    for i in range(m):                                                   # ascending slots; a bin that is not ok, or a NaN, adds nothing
        common = common + np.where(ok[i] & ~np.isnan(p[i]), p[i], 0.0)
    cb = int(np.argmax(common)) if ok.any() else -1                     # (argmax: the smallest of equal ones)
    out.update({"common_power": common, "common_bin": cb, "common_freq": float(nu[cb]) if cb >= 0 else float("nan")})
    pm = np.zeros((m, 3))
    if cb >= 0:
        amp, ph = spectra.amplitude_phase(a[:, cb], b[:, cb])
        pm = np.stack([ok[:, cb].astype(np.float64), np.where(ok[:, cb], amp, 0.0), np.where(ok[:, cb], ph, 0.0)], axis=1)
    out["phase_map"] = pm
    if fps is not None:
        out["freqs_hz"] = spectra.to_hz(nu, fps)
        out["common_freq_hz"] = float(spectra.to_hz(out["common_freq"], fps))
    return out


def to_spectrum_frame(marker, ids=None, fps=None, path=None):
    """The sheet of `spectral_analysis`: one row `SPECTRUM_FRAME_COLUMNS` per slot and axis (slot-major; axis "x", "y", "z") from
    its `marker` [M, 3, 6]; `marker_id` = `ids.marker_ids` (slot number + 1 without `ids`); with `fps` also `freq_hz`.  freq ..
    explained are NaN (empty cells) where the series has no peak.  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    mk = marker.detach().cpu().numpy() if isinstance(marker, torch.Tensor) else np.asarray(marker, dtype=np.float64)
    if mk.ndim != 3 or mk.shape[1:] != (3, SPECTRUM_COLS):
        raise ValueError(f"marker must be [M, 3, {SPECTRUM_COLS}]")
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, mk.shape[0] + 1, dtype=np.int64)
    if len(mid) != mk.shape[0]:
        raise ValueError(f"marker has {mk.shape[0]} slots, ids {len(mid)}")
    flat = mk.reshape(-1, SPECTRUM_COLS)
    cols = {"marker_id": np.repeat(np.asarray(mid), 3), "axis": np.tile(np.array(_SPECTRUM_AXES, dtype=object), mk.shape[0])}
    for k, name in enumerate(SPECTRUM_FRAME_COLUMNS[2:7]):
        cols[name] = flat[:, k].astype(np.float64)
    cols["count"] = flat[:, 5].astype(np.int64)
    if fps is not None:
        from . import spectra
        cols["freq_hz"] = spectra.to_hz(flat[:, 0], fps)
    df = pd.DataFrame(cols)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- time-resolved amplitude and phase (k_envelope.hip): the fit of every marker in a sliding window at one frequency -------------
ENVELOPE_FRAME_COLUMNS = ("frameno", "marker_id", "axis", "amplitude", "phase_deg", "explained")
ENVELOPE_SUMMARY_COLS = 5      # peak amplitude, its frame, level, onset, count of ok frames


def _envelope_analysis_args(n, m, nu, half_window, window, ref_frame, slot_mask, min_coverage, det_min, onset_frac, axis="z"):
    """`envelope_analysis`'s argument checks (no device needed): -> (nu, the window's full taps, slot indices or None, axis index)."""
    from . import spectra
    if isinstance(nu, dict):
        nu = nu["common_freq"]
    nu = float(spectra._freqs([nu])[0])
    w = spectra.window_taps(half_window, window)
    if w.size > 2 * L.ENV_MAX_HALF + 1:
        raise ValueError(f"half_window {half_window} above VBS_ENV_MAX_HALF = {L.ENV_MAX_HALF}")
    if n > L.PROJ_MAX_FRAMES or m > L.PROJ_MAX_SLOTS:
        raise ValueError(f"the table's {n} frames x {m} slots exceed VBS_PROJ_MAX_FRAMES = {L.PROJ_MAX_FRAMES} or "
                         f"VBS_PROJ_MAX_SLOTS = {L.PROJ_MAX_SLOTS}")
    if not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    if not (0.0 < float(min_coverage) <= 1.0):
        raise ValueError("min_coverage must lie in (0, 1]")
    if not (0.0 <= float(det_min) < 0.25):
        raise ValueError("det_min must lie in [0, 0.25)")
    if not (0.0 < float(onset_frac) <= 1.0):
        raise ValueError("onset_frac must lie in (0, 1]")
    if axis not in _SPECTRUM_AXES:
        raise ValueError(f"axis must be one of {_SPECTRUM_AXES}")
    slots = None
    if slot_mask is not None:
        k = np.asarray(slot_mask)
        if k.shape != (m,):
            raise ValueError(f"slot_mask must be [{m}]: nonzero = the slot takes part")
        slots = np.nonzero(k)[0]
    return nu, w, slots, _SPECTRUM_AXES.index(axis)


def _envelope_rows(fit, onset_frac=0.5):
    """The host arithmetic of `envelope_analysis`: fit [F, k, 16] (host, as `window_fit_f64` writes it for 3 values) -> a dict of
    `amplitude`, `phase_deg`, `explained` = p / M2 [F, k, 3], NaN where the window is not ok; `freq_dev` [k, 3] = minus the
    least-squares slope of the unwrapped phase over the longest run of consecutive ok frames (the first of equal ones; at least 3
    frames, else NaN), in cycles per frame: how far the line lies above the carrier; `summary` [k, 3, 5] = the peak amplitude
    (NaN without an ok frame), its frame (the first of equal ones, -1), `level` = the median amplitude over the ok frames, `onset`
    = the first ok frame whose amplitude reaches `onset_frac` x peak (-1 without one), and the count of ok frames."""
    from . import spectra
    fit = np.asarray(fit, dtype=np.float64)
    F, k = fit.shape[0], fit.shape[1]
    ok = fit[..., 0] != 0.0
    a, b, p, M2 = fit[..., 1::5], fit[..., 2::5], fit[..., 3::5], fit[..., 5::5]
    amp, ph = spectra.amplitude_phase(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        expl = p / M2
    nan = lambda v: np.where(ok[..., None], v, np.nan)                                           # noqa: E731
    out = {"amplitude": nan(amp), "phase_deg": nan(ph), "explained": nan(expl)}
    summary = np.zeros((k, 3, ENVELOPE_SUMMARY_COLS))
    freq_dev = np.full((k, 3), np.nan)
    for i in range(k):
        fr = np.nonzero(ok[:, i])[0]
        if fr.size == 0:
            summary[i] = (np.nan, -1.0, np.nan, -1.0, 0.0)
            continue
        # the longest run of consecutive ok frames, the first of equal ones
        cut = np.nonzero(np.diff(fr) != 1)[0] + 1
        runs = np.split(fr, cut)
        run = runs[int(np.argmax([r.size for r in runs]))]
        for v in range(3):
            av = amp[fr, i, v]
            if np.isnan(av).all():
                summary[i, v] = (np.nan, -1.0, np.nan, -1.0, fr.size)
                continue
            j = int(np.nanargmax(av))
            reach = np.nonzero(av >= onset_frac * av[j])[0]
            summary[i, v] = (av[j], fr[j], np.nanmedian(av), fr[reach[0]] if reach.size else -1.0, fr.size)
            if run.size >= 3 and np.isfinite(ph[run, i, v]).all():
                un = np.unwrap(np.radians(ph[run, i, v]))
                freq_dev[i, v] = -np.polyfit(run.astype(np.float64) - run[0], un, 1)[0] / (2.0 * np.pi)
    out["freq_dev"], out["summary"] = freq_dev, summary
    return out


def envelope_analysis(eng: Engine, table: torch.Tensor, nu, half_window=32, window="hann", ref_frame=0, taps=None, slot_mask=None,
                      min_coverage=0.5, det_min=1e-3, onset_frac=0.5, fps=None, grid=None, axis="z"):
    """How the oscillation at the known frequency `nu` changes along the recording (the reference's Figure 11(b)
    shows it set in, burst and settle, and ships no code for it) from a table [N, M, 10]: the series `spectral_analysis` analyses
    (`Engine.axis_displacement` against `ref_frame`, `slot_mask` [M]; with `taps` its FIR residual over flag 3) fitted by
    c0 + a cos + b sin in a sliding window of 2 `half_window` + 1 frames weighted by `spectra.window_taps(half_window, window)`:
    `window_moments_f64` then `window_fit_f64` for the markers, and the same pair for the per-frame `total` as a record of one
    series.  `nu`: cycles per frame in (0, 0.25], or the dict `spectral_analysis` returned (its `common_freq`).  Returns a dict.
    Device tensors (float64): `series` [N, M, 4], `fit` [N, M, 16], `total_series` [N, 1, 4], `total_fit` [N, 1, 16].  Host arrays
    (`_envelope_rows`): `amplitude`, `phase_deg`, `explained` [N, M, 3], NaN where the window is not ok; `freq_dev` [M, 3];
    `summary` [M, 3, 5] = peak amplitude, its frame, level (the median amplitude over the ok frames), onset (the first ok frame
    whose amplitude reaches `onset_frac` x peak, -1 without one), count of ok frames; and `total_amplitude`, `total_phase_deg`,
    `total_explained` [N, 3], `total_freq_dev` [3], `total_summary` [3, 5]; `nu`, `taps_sum`.  With `grid` = (weights [P, M], wsum
    [P]) from `fields.gaussian_weights` / `fields.row_sums`: `amplitude_map` [N, P, 2] = `field_map_f64` of the record (ok,
    amplitude of `axis`): where on the bonnet the oscillation is strongest, frame by frame.  With `fps`: `nu_hz`, `freq_dev_hz`,
    `total_freq_dev_hz`."""
    from . import spectra
    from .engine import field_map_f64, taps_sum, window_fit_f64, window_moments_f64
    from .filters import half_taps
    n, m = int(table.shape[0]), int(table.shape[1])
    nu, w, slots, ax = _envelope_analysis_args(n, m, nu, half_window, window, ref_frame, slot_mask, min_coverage, det_min, onset_frac,
                                               axis)
    dev = eng.device.index
    ax_rec, tot = eng.axis_displacement(table, ref_frame, slots)
    car = torch.from_numpy(spectra.carrier(n, nu)).to(eng.device)
    sw = taps_sum(half_taps(w))
    out = {"nu": nu, "taps_sum": sw}
    for name, rec in (("", ax_rec), ("total_", tot[:, None, :])):
        series = _oscillation_series(rec, taps, dev)
        mom = window_moments_f64(series, car, w, 3, device=dev)
        fit = window_fit_f64(mom, sw, min_coverage, det_min, device=dev)
        out.update({name + "series": series, name + "fit": fit})
        rows = _envelope_rows(fit.cpu().numpy(), onset_frac)
        for key, val in rows.items():
            out[name + key] = val if not name else (val[0] if key in ("freq_dev", "summary") else val[:, 0])
    if grid is not None:
        Wg, wsum = grid
        amp = out["amplitude"][..., ax]
        rec = torch.from_numpy(np.stack([(~np.isnan(amp)).astype(np.float64), np.nan_to_num(amp, nan=0.0)], axis=2)).to(eng.device)
        out["amplitude_map"] = field_map_f64(rec, torch.as_tensor(Wg, dtype=torch.float64, device=eng.device),
                                             torch.as_tensor(wsum, dtype=torch.float64, device=eng.device), min_coverage, 1, device=dev)
    if fps is not None:
        out["nu_hz"] = float(spectra.to_hz(nu, fps))
        out["freq_dev_hz"] = spectra.to_hz(out["freq_dev"], fps)
        out["total_freq_dev_hz"] = spectra.to_hz(out["total_freq_dev"], fps)
    return out


def to_envelope_frame(result, ids=None, fps=None, path=None):
    """The long sheet of `envelope_analysis`: one row `ENVELOPE_FRAME_COLUMNS` per frame, slot and axis (frame-major, then slot,
    then axis "x", "y", "z") from its `amplitude`, `phase_deg`, `explained` [N, M, 3]; `frameno` counts from 1, `marker_id` =
    `ids.marker_ids` (slot number + 1 without `ids`); with `fps` also `time_s` = (frameno - 1) / fps.  amplitude .. explained are
    NaN (empty cells) where the window is not ok.  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    amp, ph, ex = (np.asarray(result[k], dtype=np.float64) for k in ("amplitude", "phase_deg", "explained"))
    if amp.ndim != 3 or amp.shape[2] != 3 or ph.shape != amp.shape or ex.shape != amp.shape:
        raise ValueError("amplitude, phase_deg and explained must be [N, M, 3]")
    N, M = amp.shape[:2]
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, M + 1, dtype=np.int64)
    if len(mid) != M:
        raise ValueError(f"the result has {M} slots, ids {len(mid)}")
    cols = {"frameno": np.repeat(np.arange(1, N + 1, dtype=np.int64), 3 * M),
            "marker_id": np.tile(np.repeat(np.asarray(mid), 3), N),
            "axis": np.tile(np.array(_SPECTRUM_AXES, dtype=object), N * M),
            "amplitude": amp.reshape(-1), "phase_deg": ph.reshape(-1), "explained": ex.reshape(-1)}
    if fps is not None:
        fps = float(fps)
        if not (np.isfinite(fps) and fps > 0.0):
            raise ValueError("fps must be finite and > 0")
        cols["time_s"] = (cols["frameno"] - 1) / fps
    df = pd.DataFrame(cols)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- principal modes of the displacement field (k_modes.hip): which patterns a recording consists of ----------------------------
MODE_FRAME_COLUMNS = ("frameno", "mode", "flag", "score", "coverage", "value", "explained")


def _modal_args(n, m, n_modes, iters, mode, ref_frame, slot_mask, min_coverage):
    """`modal_analysis`'s argument checks (no device needed): -> (n_modes, iters, slot indices or None)."""
    from .analysis import _COV_MODES
    r, it = int(n_modes), int(iters)
    if n < 2:
        raise ValueError("a covariance needs at least 2 frames")
    if not (1 <= r <= min(3 * m, L.MODES_MAX)):
        raise ValueError(f"n_modes must lie in 1 .. min(3 M, VBS_MODES_MAX = {L.MODES_MAX})")
    if not (0 <= it <= L.MODES_MAX_ITERS):
        raise ValueError(f"iters must lie in 0 .. {L.MODES_MAX_ITERS}")
    if mode not in _COV_MODES:
        raise ValueError("mode must be 'filled' or 'pairwise'")
    if not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    if not (0.0 < float(min_coverage) <= 1.0):
        raise ValueError("min_coverage must lie in (0, 1]")
    slots = None
    if slot_mask is not None:
        k = np.asarray(slot_mask)
        if k.shape != (m,):
            raise ValueError(f"slot_mask must be [{m}]: nonzero = the slot takes part")
        slots = np.nonzero(k)[0]
    for what, got, name, cap in (("frames", n, "VBS_PROJ_MAX_FRAMES", L.PROJ_MAX_FRAMES), ("slots", m, "VBS_MOM_MAX_SLOTS", L.MOM_MAX_SLOTS)):
        if got > cap:                                             # after the arguments, as the entries decide it
            raise L.VbsError(f"modal_analysis: the table's {got} {what} exceed {name} = {cap} (status {L.VBS_ECAPACITY})")
    return r, it, slots


def modal_analysis(eng: Engine, table: torch.Tensor, n_modes=6, iters=48, mode="filled", ref_frame=0, slot_mask=None,
                   min_coverage=0.5, taps=None, grid=None):
    """Which spatial patterns of marker displacement a recording consists of, how much of the variance each carries and how each
    evolves along time (PCA with gaps; the reference ships no code for it) from a table [N, M, 10]:
    `Engine.axis_displacement` against `ref_frame` (`slot_mask` [M]: nonzero = the slot takes part), the means of every series as
    the shift, then `cross_moments_f64`, `covariance_f64` (`mode` 'filled': positive semidefinite, biased by the share of gaps;
    'pairwise': unbiased pair by pair, possibly indefinite), `leading_modes_f64` (`n_modes` <= 16, a fixed `iters`) and
    `mode_scores_f64`.  Returns a dict.  Device tensors (float64): `series` [N, M, 4], `cov` [3 M, 3 M], `scores` [N, r, 3] = flag,
    score, coverage (a record of r series: the entries for filtering, despiking, spectra and steps take it), `energy` [N, 2].
    Host arrays: `values` [r], `explained`, `cumulative` [r] (shares of the trace), `modes` [r, M, 3] (unit norm, the largest
    entry positive), `resid` [r] = |A u - lambda u| (the convergence reached: compare with `values`), `info` = rank found, columns
    dropped, `center` [M, 3], `reconstructed` [N] = the share of the frame's energy the flagged modes carry (NaN for an empty
    frame), `loners` [M] = the share of every slot's variance outside the leading subspace and `loner_order`.  With `taps`:
    `scores_trend` = `fir_series_f64` of the scores.  With `grid` = (weights [P, M], wsum [P]): `mode_maps` [r, P, 4] =
    `field_map_f64` of `modes.mode_record`."""
    from . import modes as MD
    from .engine import covariance_f64, cross_moments_f64, field_map_f64, fir_series_f64, leading_modes_f64, mode_scores_f64
    n, m = int(table.shape[0]), int(table.shape[1])
    r, it, slots = _modal_args(n, m, n_modes, iters, mode, ref_frame, slot_mask, min_coverage)
    dev = eng.device.index
    ax_rec, _ = eng.axis_displacement(table, ref_frame, slots)
    rec = ax_rec[..., :4].contiguous()
    valid = rec[..., :1] != 0.0
    cnt = valid.sum(dim=0).to(torch.float64)                                                   # [M, 1]
    tot = torch.where(valid, rec[..., 1:], torch.zeros((), dtype=torch.float64, device=rec.device)).sum(dim=0)
    shift = torch.where(cnt > 0, tot / cnt.clamp(min=1.0), torch.zeros_like(tot))              # [M, 3]
    mom = cross_moments_f64(rec, shift, 3, device=dev)
    mask = None if slots is None else torch.as_tensor(np.asarray(slot_mask) != 0, device=eng.device).to(torch.uint8)
    cov = covariance_f64(mom, 3, mode, 2, float(n - 1), mask, device=dev)
    values, md, resid, info = leading_modes_f64(cov, r, it, device=dev)
    diag = torch.diagonal(mom, dim1=0, dim2=1).permute(2, 0, 1)                                # [M, 4, 4]
    nn = diag[:, 3, 3:4]
    center = shift + torch.where(nn > 0, diag[:, :3, 3] / nn.clamp(min=1.0), torch.zeros_like(shift))
    scores, energy = mode_scores_f64(rec, center.reshape(-1), md, 3, min_coverage, device=dev)
    cov_h, md_h, val_h = cov.cpu().numpy(), md.cpu().numpy(), values.cpu().numpy()
    share, cum = MD.explained(val_h, cov_h)
    sc_h, en_h = scores.cpu().numpy(), energy.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        recon = np.where(en_h[:, 1] > 0.0, (sc_h[..., 0] * sc_h[..., 1] ** 2 * sc_h[..., 2]).sum(axis=1) / en_h[:, 1], np.nan)
    loners, order = MD.loner_slots(cov_h, md_h, val_h, 3)
    out = {"series": rec, "cov": cov, "scores": scores, "energy": energy, "values": val_h, "explained": share, "cumulative": cum,
           "modes": md_h.reshape(r, m, 3), "resid": resid.cpu().numpy(), "info": info.cpu().numpy(), "center": center.cpu().numpy(),
           "reconstructed": recon, "loners": loners, "loner_order": order}
    if taps is not None:
        out["scores_trend"] = fir_series_f64(scores, taps, 1, device=dev)
    if grid is not None:
        Wg, wsum = grid
        mrec = torch.from_numpy(MD.mode_record(md_h, m, 3, None if slot_mask is None else np.asarray(slot_mask))).to(eng.device)
        out["mode_maps"] = field_map_f64(mrec, torch.as_tensor(Wg, dtype=torch.float64, device=eng.device),
                                         torch.as_tensor(wsum, dtype=torch.float64, device=eng.device), min_coverage, 3, device=dev)
    return out


def to_mode_frame(result, frame_offset=0, path=None):
    """The long sheet of `modal_analysis`: one row `MODE_FRAME_COLUMNS` per frame and mode (frame-major) from its `scores`
    [N, r, 3]; `frameno` counts from 1 + `frame_offset`, `mode` from 1; `value` and `explained` repeat the mode's eigenvalue and
    share; score is NaN (an empty cell) where the mode was not seen enough.  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    sc = result["scores"]
    sc = np.asarray(sc.cpu().numpy() if hasattr(sc, "cpu") else sc, dtype=np.float64)
    val, ex = np.asarray(result["values"], dtype=np.float64), np.asarray(result["explained"], dtype=np.float64)
    if sc.ndim != 3 or sc.shape[2] != 3 or val.shape != (sc.shape[1],) or ex.shape != val.shape:
        raise ValueError("scores must be [N, r, 3], values and explained [r]")
    N, r = sc.shape[:2]
    flag = sc[..., 0] != 0.0
    df = pd.DataFrame({"frameno": np.repeat(np.arange(1, N + 1, dtype=np.int64) + int(frame_offset), r),
                       "mode": np.tile(np.arange(1, r + 1, dtype=np.int64), N), "flag": flag.reshape(-1).astype(np.int64),
                       "score": np.where(flag, sc[..., 1], np.nan).reshape(-1), "coverage": sc[..., 2].reshape(-1),
                       "value": np.tile(val, N), "explained": np.tile(ex, N)})
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- marker velocity, acceleration and gap filling (k_kinematics.hip): a gap-aware local polynomial fit along time -----------------
KINEMATIC_FRAME_COLUMNS = ("frameno", "marker_id", "axis", "displacement", "velocity", "acceleration", "noise", "degree")


def _kinematic_args(n, m, half_window, degree, window, ref_frame, min_coverage, piv_rel, onset_frac, axis="z"):
    """`kinematic_analysis`'s argument checks (no device needed): -> (h, d, axis index) or ValueError."""
    from .analysis import _kin_args
    h, d, _, _, _ = _kin_args(max(n, 1), max(m, 1), 4, half_window, degree, window, 3, None)
    if n < 1 or m < 1:
        raise ValueError("the table must have at least one frame and one slot")
    if not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} outside the table's {n} frames")
    if not (0.0 < float(min_coverage) <= 1.0):
        raise ValueError("min_coverage must lie in (0, 1]")
    if not (0.0 <= float(piv_rel) < 1.0):
        raise ValueError("piv_rel must lie in [0, 1)")
    if not (0.0 < float(onset_frac) <= 1.0):
        raise ValueError("onset_frac must lie in (0, 1]")
    if axis not in _SPECTRUM_AXES:
        raise ValueError(f"axis must be one of {_SPECTRUM_AXES}")
    return h, d, _SPECTRUM_AXES.index(axis)


def _kinematic_rows(fit, mom, degree, fps=None, onset_frac=0.1):
    """The host arithmetic of `kinematic_analysis`: fit [F, k, 2 + 3 (d + 2)] and mom [F, k, M] (host, three values) -> a dict of
    `displacement`, `velocity`, `acceleration` [F, k, 3] (the derivatives y_0, y_1, y_2 of the fit, times fps and fps^2 with `fps`;
    NaN where no degree was reached, velocity NaN below degree 1 of the request, acceleration below 2), `speed` [F, k] = |v|,
    `noise` [F, k, 3] = sqrt(max(rss, 0) / S_0), `degree` int64 [F, k] (the degree used, -1 without one); per frame `mean_speed`,
    `max_speed` [F] over the slots that have a speed (NaN without one) and `fastest` int64 [F], the slot that has the largest speed,
    ties to the smaller slot, -1 without one; per slot `peak_speed` [k] and `peak_frame` int64 [k] (the first of equal ones, NaN / -1
    without a speed); `onset`: the first frame whose mean speed exceeds `onset_frac` x the largest mean speed (-1 without one)."""
    fit, mom = np.asarray(fit, dtype=np.float64), np.asarray(mom, dtype=np.float64)
    d = int(degree)
    F, k = fit.shape[:2]
    q = fit[..., 1].astype(np.int64)
    have = q >= 0
    per = fit[..., 2:].reshape(F, k, 3, d + 2)
    nan = lambda v: np.where(have[..., None], v, np.nan)                                          # noqa: E731
    scale = 1.0 if fps is None else float(fps)
    out = {"degree": q, "displacement": nan(per[..., 0])}
    out["velocity"] = nan(per[..., 1] * scale) if d >= 1 else np.full((F, k, 3), np.nan)
    out["acceleration"] = nan(per[..., 2] * (scale * scale)) if d >= 2 else np.full((F, k, 3), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["noise"] = nan(np.sqrt(np.maximum(per[..., d + 1], 0.0) / mom[..., :1]))
    speed = np.sqrt((out["velocity"] ** 2).sum(axis=2))
    out["speed"] = speed
    seen = ~np.isnan(speed)
    cnt = seen.sum(axis=1)
    filled = np.where(seen, speed, -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["mean_speed"] = np.where(cnt > 0, np.where(seen, speed, 0.0).sum(axis=1) / cnt, np.nan)
    out["max_speed"] = np.where(cnt > 0, filled.max(axis=1, initial=-np.inf), np.nan)
    out["fastest"] = np.where(cnt > 0, np.argmax(filled, axis=1), -1).astype(np.int64)               # argmax: the first of equal ones
    any_f = seen.any(axis=0)
    out["peak_speed"] = np.where(any_f, filled.max(axis=0, initial=-np.inf), np.nan)
    out["peak_frame"] = np.where(any_f, np.argmax(filled, axis=0), -1).astype(np.int64)
    ms = out["mean_speed"]
    onset = -1
    if np.isfinite(ms).any() and np.nanmax(ms) > 0.0:
        over = np.nonzero(np.nan_to_num(ms, nan=0.0) > float(onset_frac) * np.nanmax(ms))[0]
        onset = int(over[0]) if over.size else -1
    out["onset"] = onset
    return out


def kinematic_analysis(eng: Engine, table: torch.Tensor, half_window=7, degree=2, window="hann", ref_frame=0, slots=None, fps=None,
                       min_coverage=0.5, piv_rel=None, grid=None, onset_frac=0.1, axis="z"):
    """Smoothed displacement, velocity and acceleration of every marker along a recording (slip, approach speed,
    first contact and the direction reversal of the reference's Figure 11(b) are statements about rates, and it ships no code for
    them) from a table [N, M, 10]: `Engine.axis_displacement` against `ref_frame` (`slots`: indices), fitted by a polynomial of
    `degree` <= 3 in a sliding window of 2 `half_window` + 1 frames weighted by `window`, gaps selected out, one-sided at the ends:
    `poly_moments_f64` then `poly_fit_f64` for the markers, and the same pair for the per-frame `total` as a record of one series.
    A window that a gap or an end leaves badly determined falls back in degree (`piv_rel`, default `engine.KIN_PIV_REL`).  Returns
    a dict.  Device tensors (float64): `series` [N, M, 4], `moments`, `fit` [N, M, 2 + 3 (d + 2)], `total_series` [N, 1, 5],
    `total_fit`.  Host arrays (`_kinematic_rows`): `displacement`, `velocity`, `acceleration`, `noise` [N, M, 3] (per frame, times
    `fps` and `fps`^2 when given; NaN where the window reached no degree), `speed` [N, M], `degree` [N, M], `mean_speed`,
    `max_speed`, `fastest` [N], `peak_speed`, `peak_frame` [M], `onset`, and `total_displacement`, `total_velocity`,
    `total_acceleration` [N, 3].  With `grid` = (weights [P, M], wsum [P]) from `fields.gaussian_weights` / `fields.row_sums`:
    `speed_map` [N, P, 2] = `field_map_f64` of the record (has a speed, speed): where on the bonnet the skin moves fastest, frame
    by frame; with a third element grid_xy [P, 2] also `speed_patch` [N, 8] = `patch_stats_f64` of that map."""
    from .engine import KIN_PIV_REL, field_map_f64, patch_stats_f64, poly_fit_f64, poly_moments_f64
    n, m = int(table.shape[0]), int(table.shape[1])
    pr = KIN_PIV_REL if piv_rel is None else piv_rel
    h, d, ax = _kinematic_args(n, m, half_window, degree, window, ref_frame, min_coverage, pr, onset_frac, axis)
    dev = eng.device.index
    ax_rec, tot = eng.axis_displacement(table, ref_frame, slots)
    out = {"half_window": h, "degree_asked": d, "fps": fps}
    for name, rec in (("", ax_rec), ("total_", tot[:, None, :].contiguous())):
        mom = poly_moments_f64(rec, h, d, window, 3, device=dev)
        fit = poly_fit_f64(mom, rec, h, d, window, 3, min_coverage, pr, device=dev)
        out.update({name + "series": rec, name + "moments": mom, name + "fit": fit})
        rows = _kinematic_rows(fit.cpu().numpy(), mom.cpu().numpy(), d, fps, onset_frac)
        if not name:
            out.update(rows)
        else:
            for key in ("displacement", "velocity", "acceleration"):
                out[name + key] = rows[key][:, 0]
    if grid is not None:
        Wg, wsum = grid[0], grid[1]
        sp = out["speed"]
        rec = torch.from_numpy(np.stack([(~np.isnan(sp)).astype(np.float64), np.nan_to_num(sp, nan=0.0)], axis=2)).to(eng.device)
        out["speed_map"] = field_map_f64(rec, torch.as_tensor(Wg, dtype=torch.float64, device=eng.device),
                                         torch.as_tensor(wsum, dtype=torch.float64, device=eng.device), min_coverage, 1, device=dev)
        if len(grid) > 2:
            out["speed_patch"] = patch_stats_f64(out["speed_map"], grid[2], component=0, device=dev)
    return out


def to_kinematic_frame(result, ids=None, fps=None, path=None):
    """The long sheet of `kinematic_analysis`: one row `KINEMATIC_FRAME_COLUMNS` per frame, slot and axis (frame-major, then slot,
    then axis "x", "y", "z"); `frameno` counts from 1, `marker_id` = `ids.marker_ids` (slot number + 1 without `ids`); with `fps` also
    `time_s` = (frameno - 1) / fps.  displacement .. noise are NaN (empty cells) where the window reached no degree.  `path`: also
    written, as .csv or as .xlsx."""
    import pandas as pd
    dis, vel, acc, noi = (np.asarray(result[k], dtype=np.float64) for k in ("displacement", "velocity", "acceleration", "noise"))
    deg = np.asarray(result["degree"])
    if dis.ndim != 3 or dis.shape[2] != 3 or any(v.shape != dis.shape for v in (vel, acc, noi)) or deg.shape != dis.shape[:2]:
        raise ValueError("displacement, velocity, acceleration and noise must be [N, M, 3], degree [N, M]")
    N, M = dis.shape[:2]
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, M + 1, dtype=np.int64)
    if len(mid) != M:
        raise ValueError(f"the result has {M} slots, ids {len(mid)}")
    cols = {"frameno": np.repeat(np.arange(1, N + 1, dtype=np.int64), 3 * M),
            "marker_id": np.tile(np.repeat(np.asarray(mid), 3), N),
            "axis": np.tile(np.array(_SPECTRUM_AXES, dtype=object), N * M),
            "displacement": dis.reshape(-1), "velocity": vel.reshape(-1), "acceleration": acc.reshape(-1), "noise": noi.reshape(-1),
            "degree": np.repeat(deg.reshape(-1).astype(np.int64), 3)}
    if fps is not None:
        fps = float(fps)
        if not (np.isfinite(fps) and fps > 0.0):
            raise ValueError("fps must be finite and > 0")
        cols["time_s"] = (cols["frameno"] - 1) / fps
    df = pd.DataFrame(cols)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


def _uncertainty_args(n, m, ref_frame, k, grid):
    """`uncertainty_analysis`'s own argument checks (no device needed); the entries' are `engine._uncert_args`."""
    if ref_frame is None or int(ref_frame) != ref_frame or not (0 <= int(ref_frame) < n):
        raise ValueError(f"ref_frame {ref_frame} must be a frame of the table's {n}")
    if not (np.isfinite(float(k)) and float(k) > 0.0):
        raise ValueError("k must be finite and > 0")
    if grid is not None and (len(grid) < 2 or tuple(np.shape(grid[0]))[1:] != (m,)):
        raise ValueError(f"grid must be (weights [P, {m}], wsum [P])")
    return int(ref_frame), float(k)


def uncertainty_analysis(eng, table, cam: L.Camera, obs_cov, cam_factor=None, ref_frame=0, k=3.0, grid=None, slots=None,
                         min_marker_size_px=5.0):
    """How good every 3-D point and displacement of a table [N, M, 10] is, to first order: `solve3d_cov` with
    the observation covariance `obs_cov` (`uncertainty.obs_cov`, or columns 4 .. 9 of `pixel_noise` over a still segment) and the
    camera's factor `cam_factor` (`uncertainty.camera_factor`), displacements against `ref_frame`.  `eng` may be None (the entries
    take no handle; with an engine its device is used).  Returns a dict of host arrays: `usable`, `usable_d` [N, M]; `sigma_x`,
    `sigma_d` [N, M, 3] the standard deviations of X, Y, Z and of dX, dY, dZ (NaN where not usable); `displacement` [N, M, 3];
    `significant` [N, M, 3] = |D_axis| > k sigma_axis; `t2` [N, M] (NaN where its flag is not set) and `t2_valid`; `limit` [M, 3]
    the detection limit of a marker, k times the median sigma_D per axis over its usable frames; `count`, `complete` [N],
    `sigma_total` [N, 3] of `axis_displacement`'s total and `camera_share` [N, 3], the share of its variance that is the
    camera's - coherent over the markers, it does not average out.  The device tensors are under `cov`, `dcov`, `total`.  With
    `grid` = (weights [P, M], wsum [P]): `sigma_z_map` [N, P, 2] = `field_map_f64` of (usable, sigma_Z)."""
    from .engine import field_map_f64, solve3d_cov
    n, m = int(table.shape[0]), int(table.shape[1])
    rf, kk = _uncertainty_args(n, m, ref_frame, k, grid)
    dev = None if eng is None else eng.device.index
    out = solve3d_cov(table, cam, obs_cov, cam_factor, ref_frame=rf, slots=slots, min_marker_size_px=min_marker_size_px, device=dev)
    cov, dcov, tot = (out[w].cpu().numpy() for w in ("cov", "dcov", "total"))
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    usable, usable_d = cov[..., 0] == 1.0, dcov[..., 0] >= 1.0
    with np.errstate(invalid="ignore"):
        sx = np.where(usable[..., None], np.sqrt(cov[..., [1, 4, 6]]), np.nan)
        sd = np.where(usable_d[..., None], np.sqrt(dcov[..., [1, 4, 6]]), np.nan)
        D = np.where(usable_d[..., None], np.where(usable_d[..., None], t[..., 6:9], 0).astype(np.float64) -
                     np.where(usable_d[..., None], t[rf][None, :, 6:9], 0).astype(np.float64), np.nan)
        sig = usable_d[..., None] & (np.abs(D) > kk * sd)
        limit = np.full((m, 3), np.nan)
        for i in range(m):
            if usable_d[:, i].any():
                limit[i] = kk * np.median(sd[usable_d[:, i], i], axis=0)
        var, camv = tot[:, 2:5], tot[:, 5:8]
        share = np.where(var > 0.0, camv / np.where(var > 0.0, var, 1.0), 0.0)
    res = dict(out, usable=usable, usable_d=usable_d, sigma_x=sx, sigma_d=sd, displacement=D, significant=sig,
               t2=np.where(dcov[..., 0] == 3.0, dcov[..., 7], np.nan), t2_valid=dcov[..., 0] == 3.0, limit=limit, k=kk,
               ref_frame=rf, count=tot[:, 0], complete=tot[:, 1] == 1.0, sigma_total=np.sqrt(var), camera_share=share)
    if grid is not None:
        d = out["cov"].device
        rec = torch.stack([out["cov"][..., 0], torch.sqrt(out["cov"][..., 6])], dim=2).contiguous()
        res["sigma_z_map"] = field_map_f64(rec, torch.as_tensor(grid[0], dtype=torch.float64, device=d),
                                           torch.as_tensor(grid[1], dtype=torch.float64, device=d), 0.5, 1, device=d.index)
    return res


UNCERTAINTY_FRAME_COLUMNS = ("frameno", "slot", "usable", "sigma_X", "sigma_Y", "sigma_Z", "dX", "dY", "dZ", "sigma_dX", "sigma_dY",
                             "sigma_dZ", "significant_X", "significant_Y", "significant_Z", "t2")


def to_uncertainty_frame(result, ids=None, frame_offset=0, path=None):
    """The long sheet of `uncertainty_analysis`: one row `UNCERTAINTY_FRAME_COLUMNS` per frame and slot (frame-major); `frameno`
    counts from 1 + `frame_offset`, `slot` = `ids.marker_ids` (slot number + 1 without `ids`); cells are empty (NaN) where the row
    or its reference row is not usable.  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    sx, sd, D = (np.asarray(result[w], dtype=np.float64) for w in ("sigma_x", "sigma_d", "displacement"))
    sig, t2 = np.asarray(result["significant"]), np.asarray(result["t2"], dtype=np.float64)
    if sx.ndim != 3 or sx.shape[2] != 3 or sd.shape != sx.shape or D.shape != sx.shape or sig.shape != sx.shape or t2.shape != sx.shape[:2]:
        raise ValueError("sigma_x, sigma_d, displacement and significant must be [N, M, 3], t2 [N, M]")
    N, M = sx.shape[:2]
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, M + 1, dtype=np.int64)
    if len(mid) != M:
        raise ValueError(f"the result has {M} slots, ids {len(mid)}")
    cols = {"frameno": np.repeat(np.arange(1, N + 1, dtype=np.int64) + int(frame_offset), M), "slot": np.tile(np.asarray(mid), N),
            "usable": np.asarray(result["usable"]).reshape(-1)}
    for j, a in enumerate("XYZ"):
        cols["sigma_" + a] = sx[..., j].reshape(-1)
    for j, a in enumerate("XYZ"):
        cols["d" + a] = D[..., j].reshape(-1)
    for j, a in enumerate("XYZ"):
        cols["sigma_d" + a] = sd[..., j].reshape(-1)
    for j, a in enumerate("XYZ"):
        cols["significant_" + a] = sig[..., j].reshape(-1)
    cols["t2"] = t2.reshape(-1)
    df = pd.DataFrame(cols, columns=list(UNCERTAINTY_FRAME_COLUMNS))
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


def fill_table(eng: Engine, table: torch.Tensor, half_window=7, degree=2, *, source="xyz", fill_degree=1, slots=None, window="hann",
               min_coverage=0.5, piv_rel=None):
    """The gaps of a table [N, M, 10] filled along time by the constant term of the gap-aware local polynomial fit
    (`engine.poly_moments_f64`, `engine.poly_fit_f64`), in `despike_table`'s conventions.  `source` "xyz": the rows
    with VBS_FLAG_XYZ, values X, Y, Z (cols 6-8); "pixel": the rows with VBS_FLAG_TRACKED, values Cx, Cy.  `slots` (indices)
    restricts the filling to those markers.  Returns (filled_table, report): filled_table is a copy of the table in which a MISSING
    row whose window reaches `fill_degree` has its values replaced by y_0, rounded to the table's dtype once; its flag bits are
    untouched - whether to set VBS_FLAG_XYZ (or VBS_FLAG_TRACKED) on an interpolated row is the caller's decision, and
    `report["filled"]` bool [N, M] is what they would OR in.  report, a dict of tensors on the table's device: `filled`; `degree`
    int64 [N, M] (the degree used, -1 without one); `per_marker` [M] and `per_frame` [N] int64 counts of filled rows; `values`
    float64 [N, M, nv] (y_0 where filled, else 0); `source`."""
    from . import engine as _engine
    if source not in _SPIKE_SOURCES:
        raise ValueError(f"source must be one of {sorted(_SPIKE_SOURCES)}")
    bit, _, cols, _ = _SPIKE_SOURCES[source]
    t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.asarray(table), device=eng.device)
    if t.dim() != 3 or t.shape[2] != L.TABLE_COLS:
        raise ValueError(f"table must be [N, M, {L.TABLE_COLS}]")
    flags = t[..., 0].to(torch.int64)
    valid = (flags & bit) != 0
    pick = torch.ones(t.shape[1], dtype=torch.bool, device=t.device)
    if slots is not None:
        idx = np.asarray(slots, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= t.shape[1]):
            raise ValueError(f"slots outside the table's {t.shape[1]} slots")
        pick = torch.zeros(t.shape[1], dtype=torch.bool, device=t.device)
        pick[torch.as_tensor(idx, device=t.device)] = True
    nv = len(cols)
    rec = torch.cat([valid.to(torch.float64)[..., None], t[..., list(cols)].to(torch.float64)], dim=2).contiguous()
    pr = _engine.KIN_PIV_REL if piv_rel is None else piv_rel
    dev = eng.device.index
    mom = _engine.poly_moments_f64(rec, half_window, degree, window, nv, device=dev)
    fit, filled_rec = _engine.poly_fit_f64(mom, rec, half_window, degree, window, nv, min_coverage, pr, fill_degree, want_filled=True,
                                           device=dev)
    fit, filled_rec = torch.as_tensor(fit, device=t.device), torch.as_tensor(filled_rec, device=t.device)
    did = (filled_rec[..., 0] == 2.0) & pick[None, :]
    out = t.clone()
    vals = filled_rec[..., 1:1 + nv]
    for k, c in enumerate(cols):
        out[..., c] = torch.where(did, vals[..., k].to(t.dtype), t[..., c])
    report = {"filled": did, "degree": fit[..., 1].to(torch.int64), "per_marker": did.sum(dim=0), "per_frame": did.sum(dim=1),
              "values": torch.where(did[..., None], vals, torch.zeros_like(vals)), "source": source}
    return out, report


# ---- the probe-indentation validation (k_steps.hip): the reference's Figure 6(b) from a tracked table -------------------------
@dataclass
class IndentationResult:
    """What `indentation_analysis` returns (host arrays; k = the number of steps kept, so k + 1 dwells)."""
    step_mm: float
    component: str
    step_frames: np.ndarray         # int64 [k]
    begin: np.ndarray               # int64 [k + 1]: dwell j is the frames [begin, end) ...
    end: np.ndarray                 # int64 [k + 1]
    count: np.ndarray               # int64 [k + 1]: ... of which this many are complete
    cumulative: np.ndarray          # float64 [k + 1]: the dwell mean (for "xyz" the norm of the dwell-mean vector)
    std: np.ndarray                 # float64 [k + 1], ddof = 1; NaN below two frames
    delta: np.ndarray               # float64 [k]: cumulative[j + 1] - cumulative[j]
    abs_error: np.ndarray           # float64 [k]: |delta - step_mm|
    marker_means: np.ndarray        # float64 [m, k + 1, 3]: per marker the dwell means of dX, dY, dZ (NaN where never seen)
    overflow: bool                  # more steps were found than `VBS_STEP_MAX_STEPS`: the last dwell runs over the rest


_COMPONENT_COLS = {"x": (1,), "y": (2,), "z": (3,), "xyz": (1, 2, 3)}


def indentation_analysis(eng: Engine, table: torch.Tensor, step_mm=0.7, window=8, threshold=None, guard=None, ref_frame=0,
                         slots=None, component="z"):
    """Figure 6(b) of the reference (it ships no code for it) from a table [N, M, 10] of a tool pressed in steps
    of `step_mm`: the displacement of the selected slots against `ref_frame`, averaged over the slots in every COMPLETE frame
    (`Engine.axis_displacement`; a frame where a marker dropped out is a gap), the steps of that one series (`step_response_f64`,
    `find_steps_f64` on `component`: "x", "y", "z" or "xyz"; `threshold` in mm, default step_mm / 2), the statistics of the dwells
    between them (`dwell_stats_f64`, `guard` frames left out on either side of a step, default `window`) and, with the same step
    list, the dwell means of every marker.  The displacement is signed: a tool that lowers the component gives negative steps,
    which "xyz" (a norm) does not see."""
    from .engine import dwell_stats_f64, find_steps_f64, step_response_f64
    if component not in _COMPONENT_COLS:
        raise ValueError(f"component must be one of {sorted(_COMPONENT_COLS)}")
    threshold = step_mm / 2 if threshold is None else threshold
    guard = window if guard is None else guard
    axis, total = eng.axis_displacement(table, ref_frame, slots)
    dev = eng.device.index
    cols = list(_COMPONENT_COLS[component])
    series = torch.cat([total[:, 0:1], total[:, cols] / total[:, 4:5]], dim=1)[:, None, :].contiguous()   # [N, 1, 1 + nv]
    resp = step_response_f64(series, window, device=dev)
    steps = find_steps_f64(resp, window, threshold, device=dev)
    own = dwell_stats_f64(series, steps, guard, device=dev)[0].cpu().numpy()
    per_marker = dwell_stats_f64(axis, steps, guard, 3, device=dev).cpu().numpy()
    st = steps[0].cpu().numpy()
    found = int(st[0])
    k = min(found, L.STEP_MAX_STEPS)
    nv = len(cols)
    own = own[:k + 1]
    count = own[:, 2]
    with np.errstate(all="ignore"):
        cumulative = own[:, 3] if nv == 1 else np.sqrt((own[:, 3:3 + nv] ** 2).sum(axis=1))
        std = np.where(count >= 2, np.sqrt(own[:, 3 + nv:].sum(axis=1) / (count - 1)), np.nan)
    delta = np.diff(cumulative)
    return IndentationResult(step_mm=float(step_mm), component=component, step_frames=st[1:1 + k].astype(np.int64),
                             begin=own[:, 0].astype(np.int64), end=own[:, 1].astype(np.int64), count=count.astype(np.int64),
                             cumulative=cumulative, std=std, delta=delta, abs_error=np.abs(delta - float(step_mm)),
                             marker_means=per_marker[:, :k + 1, 3:6], overflow=found > L.STEP_MAX_STEPS)


def to_step_frame(result: IndentationResult, path=None):
    """The sheet behind Figure 6(b): one row `step, frame_first, frame_last, count, cumulative_mm, std_mm, step_mm,
    abs_error_mm` per dwell of an `IndentationResult` (frame_last inclusive; `step_mm` here is the MEASURED step from the dwell
    before); row 0 has no step before it: NaN (empty cells) there.  `path`: also written as .xlsx."""
    import pandas as pd
    k1 = len(result.cumulative)
    nan = np.full(1, np.nan)
    df = pd.DataFrame({"step": np.arange(k1, dtype=np.int64), "frame_first": np.asarray(result.begin, dtype=np.int64),
                       "frame_last": np.asarray(result.end, dtype=np.int64) - 1, "count": np.asarray(result.count, dtype=np.int64),
                       "cumulative_mm": np.asarray(result.cumulative, dtype=np.float64),
                       "std_mm": np.asarray(result.std, dtype=np.float64),
                       "step_mm": np.concatenate([nan, result.delta]), "abs_error_mm": np.concatenate([nan, result.abs_error])})
    if path is not None:
        from .xlsx_io import dataframe_to_xlsx
        dataframe_to_xlsx(df, path)
    return df


# ---- re-tracking a recording along time (k_retrack.hip) ---------------------------------------------------------------------------
def retrack_table(eng: Engine, det, counts, ref_xy, cam=None, min_dist=20.0, min_marker_size_px=5.0, **params):
    """The table of a recording re-tracked ALONG TIME (`engine.retrack`) from the detections
    `eng.track_to_3d(..., want_det=True)` returned: every slot predicts where its marker is, takes only a detection inside
    `gate` px of the prediction, and a detection goes to at most one slot - so a marker that drops out hands its ID to nobody,
    and one dragged far from its first-frame position is followed.  `params`: gate, max_travel, vel_gain, max_coast, state.
    Returns (table, report).  table float32 [n, m, 10] is `eng.track`'s format (with `cam`, `eng.solve3d` has run on it), so
    `despike_table`, `fill_table` and every `*_analysis` take it as it is.  report: `info` int32 [n, 4] (used, matched,
    with_candidate, contested) and `dist2` float64 [n, m] as `engine.retrack` returns them, `state` to continue from,
    `comparison` = `retrack.compare_tables(table, eng.track(det, counts, ref_xy, min_dist))` - what changed against the
    per-frame rule (a = this table, b = the per-frame one) - and `lost`, the slots never matched."""
    from . import engine as _engine
    from .retrack import compare_tables
    out = _engine.retrack(det, counts, ref_xy, want=("table", "dist2", "info"), device=eng.device.index, **params)
    table = out["table"]
    d = torch.as_tensor(det, dtype=torch.float64, device=eng.device).contiguous()
    c = torch.as_tensor(counts, device=eng.device).to(torch.int32).contiguous().reshape(-1)
    legacy = eng.track(d, c, ref_xy, min_dist)
    comparison = compare_tables(table, legacy)
    if cam is not None:
        eng.solve3d(table, cam, min_marker_size_px)
    lost = torch.nonzero(~(out["dist2"] >= 0).any(dim=0)).reshape(-1) if table.shape[0] else torch.arange(table.shape[1], device=eng.device)
    return table, {"info": out["info"], "dist2": out["dist2"], "state": out["state"], "comparison": comparison, "lost": lost}


def to_retrack_frame(report, frame_offset=0, path=None):
    """The sheet of `retrack_table`: one row per frame - `frameno, used, matched, with_candidate, contested` from the report's
    `info`, then `same, only_retrack, only_per_frame, differ` from its comparison with the per-frame rule.  `path`: also written,
    as .csv or as .xlsx."""
    import pandas as pd
    info = report["info"].detach().cpu().numpy() if isinstance(report["info"], torch.Tensor) else np.asarray(report["info"])
    cmp_ = report["comparison"]
    if info.ndim != 2 or info.shape[1] != L.RETRACK_INFO_COLS or len(cmp_["same"]) != info.shape[0]:
        raise ValueError(f"report must hold info [n, {L.RETRACK_INFO_COLS}] and the comparison of the same n frames")
    data = {"frameno": np.arange(info.shape[0], dtype=np.int64) + int(frame_offset)}
    for k, name in enumerate(("used", "matched", "with_candidate", "contested")):
        data[name] = info[:, k].astype(np.int64)
    for key, name in (("same", "same"), ("only_a", "only_retrack"), ("only_b", "only_per_frame"), ("differ", "differ")):
        data[name] = np.asarray(cmp_[key], dtype=np.int64)
    df = pd.DataFrame(data)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


# ---- grey-level refinement of the tracked markers (k_refine.hip) --------------------------------------------------------------------
def refine_table(eng: Engine, frames, table, cam=None, min_marker_size_px=5.0, **params):
    """The table with centre, diameter, axes and angle of every tracked marker re-measured from the grey levels
    (`Engine.refine_markers`): the size from the integral of the contrast-normalised darkness - which blur and
    contrast leave alone - instead of from the contour of a threshold.  `frames` are the frames the detector saw (see
    `Engine.refine_markers`), `table` what `eng.track` / `eng.track_to_3d` / `retrack_table` returned for them; `params`:
    `refine.DEFAULTS`.  Returns (table, report).  table float32 [n, m, 10] is `eng.track`'s format - a row that could not be
    refined is a gap unless `keep_unrefined` - and with `cam`, `eng.solve3d` has run on it, so `despike_table`, `fill_table`
    and every `*_analysis` take it as it is.  report: `refine.report` of the run (status counts per frame and per slot, per slot
    mean and standard deviation of major' - major and of the shift, the slots never refined, the median edge_var, and
    `uncovered`: rows with status 0 whose disc did not cover the marker - a start far too small; they are still short and want
    `passes` > 1) plus `rec` and `sums` as the engine returned them."""
    from .refine import report as _report
    rec, sums, out = eng.refine_markers(frames, table, **params)
    if cam is not None:
        eng.solve3d(out, cam, min_marker_size_px)
    rep = _report(rec, table, params.get("disc_f", 1.5))
    if params.get("passes", 1) > 1:
        # `uncovered` is about the LAST pass's start, which is not `table`: a table refined again is its own start to within the
        # rule's accuracy, so judge the disc of one more pass from the result
        rep["uncovered"] = _report(rec, out, params.get("disc_f", 1.5))["uncovered"]
        rep["uncovered_per_slot"] = rep["uncovered"].sum(axis=0).astype(np.int64)
    rep["rec"], rep["sums"] = rec, sums
    return out, rep


def to_refine_frame(report, ids=None, path=None):
    """The sheet of `refine_table`: one row per slot - `slot` (and `marker_id` with `ids`), the count of every status under its
    name, `dmajor_mean`, `dmajor_std`, `shift_mean`, `shift_std`, `uncovered`.  `path`: also written, as .csv or as .xlsx."""
    import pandas as pd
    from .refine import STATUS_NAMES
    per_slot = np.asarray(report["status_per_slot"])
    if per_slot.ndim != 2 or per_slot.shape[1] != 8:
        raise ValueError("report must hold status_per_slot [m, 8] as refine_table returns it")
    data = {"slot": np.arange(per_slot.shape[0], dtype=np.int64)}
    if ids is not None:
        mid = _ids.marker_ids(ids)
        if len(mid) != per_slot.shape[0]:
            raise ValueError(f"{len(mid)} ids for {per_slot.shape[0]} slots")
        data["marker_id"] = mid
    for s in range(8):
        data[STATUS_NAMES[s]] = per_slot[:, s].astype(np.int64)
    for k in ("dmajor_mean", "dmajor_std", "shift_mean", "shift_std"):
        data[k] = np.asarray(report[k], dtype=np.float64)
    data["uncovered"] = np.asarray(report["uncovered_per_slot"], dtype=np.int64)
    df = pd.DataFrame(data)
    if path is not None:
        if str(path).lower().endswith(".csv"):
            df.to_csv(path, index=False)
        else:
            from .xlsx_io import dataframe_to_xlsx
            dataframe_to_xlsx(df, path)
    return df


def to_marker_frame(table, ids, frame_offset=0, path=None):
    """The sheet the reference's L4 scripts read (`LocalAnalysis.py:47,58`, `MarkerDisplacement.py:72,80`): one row
    `frameno, marker_id, Xw, Yw, Zw` per table entry with a 3-D point, frame-major; `marker_id` = `ids.marker_ids`.
    `path`: also written as .xlsx (`xlsx_io.dataframe_to_xlsx`), so a recorded session can be fed to those scripts."""
    import pandas as pd
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    mid = _ids.marker_ids(ids)
    if t.ndim != 3 or t.shape[2] != L.TABLE_COLS or t.shape[1] != len(mid):
        raise ValueError(f"table must be [N, {len(mid)}, {L.TABLE_COLS}] for these ids")
    f, s = np.nonzero((t[..., 0].astype(np.int64) & L.FLAG_XYZ) != 0)
    df = pd.DataFrame({"frameno": (f + int(frame_offset)).astype(np.int64), "marker_id": mid[s],
                       "Xw": t[f, s, 6].astype(np.float64), "Yw": t[f, s, 7].astype(np.float64),
                       "Zw": t[f, s, 8].astype(np.float64)})
    if path is not None:
        from .xlsx_io import dataframe_to_xlsx
        dataframe_to_xlsx(df, path)
    return df


def to_pixel_markers(table, ids=None, frame=0, path=None):
    """The `pixel_marker.csv` sheet `extrinsic_calibration.py`'s main reads (`:266,277`): one row `marker_id, u, v` per slot
    tracked in `frame` (Cx, Cy of the table), `marker_id` = `ids.marker_ids` (slot number + 1 without `ids`).  `path`: also
    written as .csv."""
    import pandas as pd
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim != 3 or t.shape[2] != L.TABLE_COLS:
        raise ValueError(f"table must be [N, M, {L.TABLE_COLS}]")
    mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, t.shape[1] + 1, dtype=np.int64)
    if len(mid) != t.shape[1]:
        raise ValueError(f"table has {t.shape[1]} slots, ids {len(mid)}")
    row = t[int(frame)]
    s = np.nonzero((row[:, 0].astype(np.int64) & L.FLAG_TRACKED) != 0)[0]
    df = pd.DataFrame({"marker_id": mid[s], "u": row[s, 1].astype(np.float64), "v": row[s, 2].astype(np.float64)})
    if path is not None:
        df.to_csv(path, index=False)
    return df
