"""Drop-in for the front half of the reference's `code/Marker_Calibration/intrinsic_calibration.py`: the same public names
(`crop_image`, `save_calib_results`, `calibrate_camera`, `plot_comparison`, `plot_3d_poses`) and console messages, with the
per-image work - crop, gray, `cv2.findChessboardCorners`, `cv2.cornerSubPix((11,11), (-1,-1), 30, 0.001)` (:71-82) - running
on the MI355X for all images of one size in one call (`Engine.find_chessboard_corners`, `Engine.corner_subpix`).  New here:
`collect_corners`, which returns what `calibrate_camera` builds in :57-83.

The last step, `cv2.calibrateCamera` (:97-98: a closed form for the focal lengths plus a joint refit), runs on the device too
(`engine.calibrate_camera_points`, k_calib.hip): `calibrate_points` returns cv2's five values, `calibrate_subsets` solves many
subsets of the views in one call, `jackknife` gives the leave-one-view-out standard error of the intrinsics.
`calibrate_camera(..., calibrate="device")` finishes as the reference does; WITHOUT that argument it still raises once the
corners are collected, as before - flipping the default is a change of its own.  The solver restates cv2's (DESIGN.md §7:
the closed form is recalled, the optimiser's path differs, the optimum is the same).  The finder is a restatement, not cv2's:
its start corner on a symmetric board is the one with the smallest (y, x).  The plots are out of scope.  There is no CPU path:
without a GPU `collect_corners` and the calibration entries raise `VbsError`."""
from __future__ import annotations

import os

import numpy as np

from . import _lib as L

CROP_RATIOS = (1 / 8, 1 / 8, 1 / 16, 0)
SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_MAX_ITER, SUBPIX_EPS = (11, 11), (-1, -1), 30, 0.001      # :80-81
MIN_VALID_IMAGES = 3                                                                           # :92
SHEET_COLUMNS = ("Param", "Value", "Desc")


def crop_image(img, ratios=CROP_RATIOS):
    """Crop image with given ratios (left, right, top, bottom) - a view, the reference's arithmetic (:24-31)."""
    h, w = img.shape[:2]
    left, right = int(w * ratios[0]), int(w * ratios[1])
    top, bottom = int(h * ratios[2]), int(h * ratios[3])
    return img[top:h - bottom, left:w - right]


def save_calib_results(mtx, dist, error, path):
    """The intrinsic sheet (:33-51): columns Param, Value, Desc and the reference's eleven rows, through `xlsx_io.write_xlsx`."""
    from .xlsx_io import write_xlsx
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    mtx, dist = np.asarray(mtx, dtype=np.float64), np.asarray(dist, dtype=np.float64).ravel()
    rows = [("fx", mtx[0, 0], "Focal length x"), ("fy", mtx[1, 1], "Focal length y"), ("cx", mtx[0, 2], "Principal point x"),
            ("cy", mtx[1, 2], "Principal point y"), ("skew", mtx[0, 1], "Skew coefficient"),
            ("k1", dist[0], "Radial dist coeff 1"), ("k2", dist[1], "Radial dist coeff 2"),
            ("p1", dist[2], "Tangential dist coeff 1"), ("p2", dist[3], "Tangential dist coeff 2"),
            ("k3", dist[4], "Radial dist coeff 3"), ("Reproj Error", float(error), "Mean error (px)")]
    write_xlsx(path, SHEET_COLUMNS, rows)


def object_points(pattern_size, square_size):
    """`objp` of :58-59: float32 [pw*ph, 3], corner (r, c) at (c, r, 0) * square_size."""
    objp = np.zeros((int(np.prod(pattern_size)), 3), np.float32)
    objp[:, :2] = np.mgrid[:pattern_size[0], :pattern_size[1]].T.reshape(-1, 2) * square_size
    return objp


def _read_dir(img_dir):
    """(names, BGR arrays) of the .png / .jpg files of a directory, in os.listdir order (:66-68), read with Pillow."""
    from PIL import Image
    names, imgs = [], []
    for f in [f for f in os.listdir(img_dir) if f.lower().endswith((".png", ".jpg"))]:
        try:
            with Image.open(os.path.join(img_dir, f)) as im:
                rgb = np.asarray(im.convert("RGB"))
        except Exception:
            continue                                     # cv2.imread returns None: the reference skips the file
        names.append(f)
        imgs.append(np.ascontiguousarray(rgb[:, :, ::-1]))
    return names, imgs


def collect_corners(images_or_dir, pattern_size, square_size):
    """What `calibrate_camera` builds in :57-83: (obj_points, img_points, valid_imgs, img_size).  `images_or_dir`: a directory,
    or a sequence of uncropped gray [H,W] / BGR [H,W,3] uint8 images (valid_imgs then holds their indices).  Every image is
    cropped (`crop_image`); all images of one size go through the finder and the (11,11) refinement in ONE device call each.
    obj_points: the float32 `objp` once per valid image; img_points: float32 [k,1,2] per valid image, as cv2 hands them on;
    img_size: (width, height) of the first image's crop, None without images."""
    import torch
    if not torch.cuda.is_available():
        raise L.VbsError("no GPU visible: intrinsic_calibration has no CPU path")
    from .diameter_validation import _engine_for
    if isinstance(images_or_dir, (str, os.PathLike)):
        names, imgs = _read_dir(images_or_dir)
    else:
        imgs = [np.asarray(im) for im in images_or_dir]
        names = list(range(len(imgs)))
    crops = [crop_image(im) for im in imgs]
    img_size = crops[0].shape[1::-1] if crops else None
    objp = object_points(pattern_size, square_size)
    refined = [None] * len(crops)
    groups = {}
    for i, c in enumerate(crops):
        groups.setdefault(c.shape, []).append(i)
    for shape, members in groups.items():
        batch = np.stack([crops[i] for i in members])
        eng = _engine_for(shape[0], shape[1], len(members))
        found, corners, _, _ = eng.find_chessboard_corners(batch, pattern_size)
        sub = eng.corner_subpix(batch, corners, SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_MAX_ITER, SUBPIX_EPS)
        found, sub = found.cpu().numpy(), sub.cpu().numpy()
        for j, i in enumerate(members):
            if found[j]:
                refined[i] = sub[j].astype(np.float32).reshape(-1, 1, 2)
    obj_points = [objp for r in refined if r is not None]
    img_points = [r for r in refined if r is not None]
    valid_imgs = [names[i] for i, r in enumerate(refined) if r is not None]
    return obj_points, img_points, valid_imgs, img_size


def rodrigues(R):
    """Rotation matrix -> rotation vector [3,1] (what cv2.Rodrigues returns for a matrix), float64."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    theta = np.arctan2(s, c)
    if s > 1e-8:
        return (w * (theta / (2.0 * s))).reshape(3, 1)
    if c > 0.0:
        return (0.5 * w).reshape(3, 1)                      # theta -> 0: R = I + [w]x
    axis = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))   # theta -> pi: R = 2 a a^T - I
    k = int(np.argmax(axis))
    sign = np.sign(R[k] + R[:, k])
    sign[k] = 1.0
    return (theta * axis * np.where(sign == 0, 1.0, sign)).reshape(3, 1)


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def calibrate_points(obj_points, img_points, img_size):
    """`cv2.calibrateCamera(obj_points, img_points, img_size, None, None)` (:97-98) -> (ret, mtx, dist, rvecs, tvecs): the RMS
    reprojection error, mtx 3 x 3 float64, dist [1,5] (k1 k2 p1 p2 k3), rvecs / tvecs tuples of [3,1] per view.  One planar
    board, at least 3 views (the reference's own floor, :92); raises `VbsError` on a degenerate set."""
    from .engine import calibrate_camera_points
    r = _host(calibrate_camera_points(obj_points, img_points, img_size))
    if r["status"][0] != L.VBS_OK:
        raise L.VbsError("calibrate_points: " + ("fewer than 3 views" if r["status"][0] == L.CALIB_FEW_VIEWS else
                                                 "degenerate views (VBS_CALIB_DEGENERATE: collinear corners, every view "
                                                 "fronto-parallel, or a board behind the camera)"))
    fx, fy, cx, cy = r["K4"][0]
    mtx = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    rvecs = tuple(rodrigues(R) for R in r["R"][0])
    tvecs = tuple(T.reshape(3, 1).copy() for T in r["T"][0])
    return float(r["rms"][0]), mtx, r["dist"][0].reshape(1, 5).copy(), rvecs, tvecs


def calibrate_subsets(obj_points, img_points, img_size, view_mask):
    """One calibration per row of `view_mask` [B,V] in one device call: `engine.calibrate_camera_points`'s dict as NumPy arrays
    (status, K4, dist, R, T, rms, view_rms, std_intrinsics, iterations per problem).  Failed problems are NaN, with their status."""
    from .engine import calibrate_camera_points
    return _host(calibrate_camera_points(obj_points, img_points, img_size, view_mask=view_mask))


def jackknife(obj_points, img_points, img_size):
    """V + 1 problems in one call: all views, then each view left out.  Returns the full-set result (row 0 of every array, as
    `calibrate_subsets`) plus `jackknife_se` [9] - sqrt((m - 1) / m * sum (theta_i - mean)^2) over the m leave-one-out fits
    that succeeded, in the order fx fy cx cy k1 k2 p1 p2 k3, next to the first-order `std_intrinsics` - `loo_intrinsics` [V,9]
    and `loo_status` [V]."""
    v = len(img_points)
    mask = np.ones((v + 1, v), dtype=np.uint8)
    mask[np.arange(1, v + 1), np.arange(v)] = 0
    r = calibrate_subsets(obj_points, img_points, img_size, mask)
    out = {k: a[0] for k, a in r.items() if k not in ("homography", "view_void")}
    loo = np.concatenate([r["K4"][1:], r["dist"][1:]], axis=1)
    ok = r["status"][1:] == L.VBS_OK
    m = int(ok.sum())
    se = np.full(9, np.nan)
    if m >= 2:
        se = np.sqrt((m - 1) / m * ((loo[ok] - loo[ok].mean(axis=0)) ** 2).sum(axis=0))
    out.update(jackknife_se=se, loo_intrinsics=loo, loo_status=r["status"][1:])
    return out


def calibrate_camera(img_dir, pattern_size, square_size, show_corners=False, calibrate=None):
    """`calibrate_camera` (:53-109): the reference's messages and None below 3 valid images.  `calibrate="device"` finishes as the
    reference does (:97-109): the dict `mtx, dist, error, obj_points, img_points, rvecs, tvecs, valid_imgs` with `error` the RMS
    that `cv2.calibrateCamera` returns.  The default (`calibrate=None`) is still the refusal that names `cv2.calibrateCamera`:
    callers rely on it, and flipping the default is a follow-up of its own.  `show_corners` draws with cv2 in the reference and
    is ignored."""
    if calibrate not in (None, "device"):
        raise ValueError('calibrate must be None or "device"')
    print(f"Processing images in: {img_dir}")
    obj_points, img_points, valid_imgs, img_size = collect_corners(img_dir, pattern_size, square_size)
    if len(obj_points) < MIN_VALID_IMAGES:
        print("Insufficient valid images")
        return None
    if calibrate == "device":
        ret, mtx, dist, rvecs, tvecs = calibrate_points(obj_points, img_points, img_size)
        return {"mtx": mtx, "dist": dist.flatten(), "error": ret, "obj_points": obj_points, "img_points": img_points, "rvecs": rvecs,
                "tvecs": tvecs, "valid_imgs": valid_imgs}
    raise NotImplementedError(f"calibrate_camera found the board in {len(valid_imgs)} images; its last step is "
                              "cv2.calibrateCamera (Zhang's closed form plus a joint refit), which is not in this project "
                              "yet: pass collect_corners(...)'s obj_points, img_points and img_size to a calibrator of your own")


def plot_comparison(img_path, mtx, dist, error):
    raise NotImplementedError("plot_comparison draws the original and the undistorted image with matplotlib, which is out of this "
                              "project's scope: Engine.set_undistort / undistort_frames give the undistorted image")


def plot_3d_poses(rvecs, tvecs, pattern_size, square_size):
    raise NotImplementedError("plot_3d_poses draws the camera poses with matplotlib (mpl_toolkits.mplot3d), which is out of this "
                              "project's scope")
