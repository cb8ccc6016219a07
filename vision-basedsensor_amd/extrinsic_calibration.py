"""Drop-in for the reference's `code/Marker_Calibration/extrinsic_calibration.py`: the same public names (`CameraParameters`,
`MARKER_DIAMETER_MM`, `load_intrinsics_from_excel`, `calibrate_camera_extrinsics`, `save_extrinsics_to_excel`, `main`), the same
sheet layout and the same console messages, with the PnP RANSAC running on the MI355X (`vbs_pnp_ransac`).  New here:
`calibrate_recording`, one pose per frame of a tracked recording, which the reference's single call cannot give.

Published inconsistencies, resolved as DESIGN.md §7 records:
 * the reference's intrinsic loader (`:47-79`) indexes the sheet by `Parameter` while the intrinsic writer writes `Param`, and
   lines the coefficients up as `[k1..k5, p1, p2]`, which OpenCV reads as `(k1, k2, p1, p2, k3, ...)`: here the sheet goes
   through `reconstruction3d._read_params` (both spellings) and the coefficients are `(k1, k2, p1, p2, k3)`, the order of
   `MarkerAnalysis.load_parameters`;
 * `cv2.solvePnPRansac` shortens its iteration count by `confidence` and draws EPnP hypotheses from 5 points; here all
   `iterations` hypotheses run with the minimal solver of `csrc/pnp_math.h` on 6 points: equal up to the optimiser, not bit
   for bit - and a problem needs 6 correspondences where cv2 needs 4.
The 3-D plot (`:166-254`) is out of scope."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import pandas as pd

from . import _lib as L

MARKER_DIAMETER_MM = 2.0
RANSAC_ITERATIONS = 1000           # iterationsCount of the reference's call (`:105`)
REPROJECTION_ERROR_PX = 8.0        # its reprojectionError (`:104`)
MIN_POINTS = 4                     # below this the reference does not call the solver (`:89`)

DIST_KEYS = ("k1", "k2", "p1", "p2", "k3")
SHEET_COLUMNS = ("Parameter", "Value", "Description")
PREPROCESS_DIR = Path("Results") / "data" / "PreprocessPara"
SHEETS = {"intrinsic": "IntrinsicParameters.xlsx", "extrinsic": "ExtrinsicParameters.xlsx",
          "world_points": "world_marker_CMM.csv", "image_points": "pixel_marker.csv"}


@dataclass
class CameraParameters:
    """What the reference's container of the same name holds: intrinsics, extrinsics and the error of their fit."""
    matrix: Optional[np.ndarray] = None
    distortion: Optional[np.ndarray] = None
    R_world_to_cam: Optional[np.ndarray] = None
    T_world_to_cam: Optional[np.ndarray] = None
    reprojection_error: Optional[float] = None


def load_intrinsics_from_excel(filepath: str) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """(camera_matrix float32 [3,3], dist_coeffs float32 [5] = k1 k2 p1 p2 k3) from the intrinsic sheet, or (None, None) with
    the reference's message on the console when the file or one of fx, fy, cx, cy is missing."""
    from .reconstruction3d import _read_params
    if not Path(filepath).exists():
        print(f"Error: Intrinsic parameters file not found at '{filepath}'")
        return None, None
    try:
        sheet = _read_params(filepath)
    except Exception as exc:
        print(f"Unexpected error loading intrinsics: {exc}")
        return None, None
    absent = [k for k in ("fx", "fy", "cx", "cy") if k not in sheet.index]
    if absent:
        print(f"Error: Missing required parameter in Excel file: {absent[0]!r}")
        return None, None
    K = np.eye(3, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = sheet["fx"], sheet["fy"], sheet["cx"], sheet["cy"]
    K[0, 1] = sheet.get("skew", 0.0)
    dist = np.array([sheet.get(k, 0.0) for k in DIST_KEYS], dtype=np.float32)
    print("Successfully loaded intrinsic parameters")
    return K, dist


def _camera(camera_matrix, dist_coeffs) -> L.Camera:
    return L.make_camera(camera_matrix, np.zeros(5) if dist_coeffs is None else dist_coeffs, np.eye(3), np.zeros(3),
                         MARKER_DIAMETER_MM)


def calibrate_camera_extrinsics(object_points: np.ndarray, image_points: np.ndarray, camera_matrix: np.ndarray,
                                dist_coeffs: np.ndarray, seed: int = 0
                                ) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Optional[float]]:
    """(R [3,3], T [3,1], mean reprojection error in pixels over ALL points) by PnP RANSAC on the device, 1000 hypotheses at
    8 px as the reference asks of cv2.  (None, None, None): under 4 points (the reference's own check), and when no pose is
    found - which includes 4 and 5 points, since every hypothesis here is drawn from 6 (cv2 solves those)."""
    from .engine import pnp_ransac
    world = np.asarray(object_points, dtype=np.float32).reshape(-1, 3)      # both sides pass through float32, as in the reference
    pixels = np.asarray(image_points, dtype=np.float32).reshape(-1, 2)
    if len(world) < MIN_POINTS:
        print("Need at least 4 points for PnP")
        return None, None, None
    res = pnp_ransac(world.astype(np.float64), pixels.astype(np.float64)[None], _camera(camera_matrix, dist_coeffs),
                     iterations=RANSAC_ITERATIONS, reproj_px=REPROJECTION_ERROR_PX, seed=seed)
    if int(res["status"][0]) != L.VBS_OK:
        print("PnP failed to find solution")
        return None, None, None
    error = float(res["mean_error"][0])
    print(f"PnP solved with {int(res['inlier_count'][0])} inliers")
    print(f"Mean reprojection error: {error:.3f} pixels")
    return res["R"][0].cpu().numpy(), res["T"][0].cpu().numpy().reshape(3, 1), error


def calibrate_recording(table, world_by_id, K, dist, frames=slice(None), ids=None, iterations: int = RANSAC_ITERATIONS,
                        reproj_px: float = REPROJECTION_ERROR_PX, seed: int = 0):
    """One pose per frame of a tracked recording (a still one: the warm-up frames), all frames in one call.
    table: [N,M,10] as `Engine.track_to_3d` returns it (device tensor or array); world_by_id: the world position of every slot -
    an array [M,3] in slot order, or a mapping marker_id -> (Xw, Yw, Zw) with `ids` [M,2] (`ids.marker_ids` names the slots; a
    slot without an entry takes no part).  Returns a dict: frames (their numbers), status [n], R [n,3,3], T [n,3], mean_error
    [n], inlier_count [n] (NumPy, per frame), and over the frames that gave a pose: R_mean (the rotation nearest the mean of
    the matrices), T_mean, R_std [3,3] and T_std [3] (per component, ddof 0), n_ok."""
    import torch
    from .engine import pnp_ransac
    from . import ids as _ids
    t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.asarray(table, dtype=np.float32))
    if t.dim() != 3 or t.shape[2] != L.TABLE_COLS:
        raise ValueError(f"table must be [N, M, {L.TABLE_COLS}]")
    m = t.shape[1]
    if isinstance(world_by_id, dict):
        mid = _ids.marker_ids(ids) if ids is not None else np.arange(1, m + 1)
        world = np.zeros((m, 3))
        known = np.zeros(m, dtype=bool)
        for s, k in enumerate(mid.tolist()):
            if k in world_by_id:
                world[s], known[s] = np.asarray(world_by_id[k], dtype=np.float64).reshape(3), True
    else:
        world = np.asarray(world_by_id, dtype=np.float64).reshape(m, 3)
        known = np.isfinite(world).all(axis=1)
        world = np.where(known[:, None], world, 0.0)
    numbers = np.arange(t.shape[0])[frames]
    sub = t[frames]
    if not sub.is_cuda:
        sub = sub.cuda()
    valid = torch.as_tensor(known, device=sub.device)[None, :].expand(sub.shape[0], m)
    res = pnp_ransac(world, sub, _camera(K, dist), iterations=iterations, reproj_px=reproj_px, seed=seed, valid=valid,
                     device=sub.device.index)
    out = {"frames": numbers, "status": res["status"].cpu().numpy(), "R": res["R"].cpu().numpy(), "T": res["T"].cpu().numpy(),
           "mean_error": res["mean_error"].cpu().numpy(), "inlier_count": res["inlier_count"].cpu().numpy()}
    ok = out["status"] == L.VBS_OK
    out["n_ok"] = int(ok.sum())
    if out["n_ok"]:
        u, _, vt = np.linalg.svd(out["R"][ok].mean(axis=0))
        out["R_mean"] = u @ np.diag([1.0, 1.0, np.linalg.det(u @ vt)]) @ vt
        out["T_mean"] = out["T"][ok].mean(axis=0)
        out["R_std"] = out["R"][ok].std(axis=0)
        out["T_std"] = out["T"][ok].std(axis=0)
    else:
        out["R_mean"] = out["T_mean"] = out["R_std"] = out["T_std"] = None
    return out


def _sheet_rows(R, T, error):
    """The extrinsic sheet as (label, value, description) rows: the labels `MarkerAnalysis.load_parameters` looks up."""
    stamp = pd.Timestamp.now().strftime("%Y-%m-%d %H:%M:%S")
    head = [("--- Camera Extrinsic Parameters ---", "", ""), ("Calibration Date", stamp, ""),
            ("Reprojection Error (px)", error, ""), ("", "", ""), ("--- World to Camera Transformation ---", "", "")]
    rot = [(f"R_wc_{r + 1}{c + 1}", v, f"Rotation matrix element ({r + 1},{c + 1})")
           for (r, c), v in zip(np.ndindex(3, 3), np.asarray(R, dtype=np.float64).reshape(9))]
    tra = [(f"T_wc_{axis}", v, f"Translation in {axis}-axis (mm)")
           for axis, v in zip("XYZ", np.asarray(T, dtype=np.float64).reshape(3))]
    return head + rot + tra


def save_extrinsics_to_excel(R: np.ndarray, T: np.ndarray, error: float, filepath: str, description: str = "") -> bool:
    """Write the extrinsic sheet (columns Parameter, Value, Description; the reference's row labels) through
    `xlsx_io.write_xlsx`.  True on success; a failure is reported on the console and returns False."""
    from .xlsx_io import write_xlsx
    try:
        target = Path(filepath)
        target.parent.mkdir(parents=True, exist_ok=True)
        write_xlsx(target, SHEET_COLUMNS, _sheet_rows(R, T, error))
    except Exception as exc:
        print(f"Failed to save extrinsics: {exc}")
        return False
    print(f"Extrinsic parameters saved to {filepath}")
    return True


def plot_3d_calibration_result(world_points, R_wc, T_wc, title: str = "Extrinsic Calibration Result") -> None:
    raise NotImplementedError("plot_3d_calibration_result draws the calibration with matplotlib (mpl_toolkits.mplot3d), which is "
                              "out of this project's scope: plot the returned R, T with a tool of your own")


def merge_correspondences(df_world: pd.DataFrame, df_image: pd.DataFrame):
    """The correspondences `main` calibrates from: the markers present in BOTH sheets (joined on `marker_id`, in the order of
    the world sheet) -> (object_points float32 [k,3], image_points float32 [k,2], marker ids [k])."""
    both = df_world.merge(df_image, how="inner", on="marker_id", suffixes=("_world", "_image"))
    return (both[["Xw", "Yw", "Zw"]].to_numpy(dtype=np.float32), both[["u", "v"]].to_numpy(dtype=np.float32),
            both["marker_id"].to_numpy())


def main(data_dir=PREPROCESS_DIR):
    """IntrinsicParameters.xlsx + world_marker_CMM.csv + pixel_marker.csv of `data_dir` -> ExtrinsicParameters.xlsx there."""
    at = {k: Path(data_dir) / name for k, name in SHEETS.items()}
    K, dist = load_intrinsics_from_excel(str(at["intrinsic"]))
    if K is None:
        return
    try:
        world, pixels, _ = merge_correspondences(pd.read_csv(at["world_points"]), pd.read_csv(at["image_points"]))
    except Exception as exc:
        print(f"Error loading correspondences: {exc}")
        return
    R, T, error = calibrate_camera_extrinsics(world, pixels, K, dist)
    if R is not None:
        save_extrinsics_to_excel(R, T, error, str(at["extrinsic"]))


if __name__ == "__main__":
    main()
