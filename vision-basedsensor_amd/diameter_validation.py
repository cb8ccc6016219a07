"""Drop-in for the numerical part of the reference's `code/Precision_Validation/DiameterValidation.py`.

`measure_markers` (:113-144) runs on the GPU (`Engine.measure_markers`: blur, threshold, contours, area, perimeter,
circularity, minimum enclosing circle, millimetres); `scale_from_corners` is `calculate_scale`'s arithmetic (:54-71) on
corners the caller supplies, and `scale_from_image` is the working form of `calculate_scale` (:48-74): the board is found on the
device (`Engine.find_chessboard_corners`, the project's restatement of `cv2.findChessboardCorners`).  Out of scope, as SURVEY
§2.1 sets out: the trackbar window (`select_threshold_interactive`) and the plots; `calculate_scale` itself keeps naming
`cv2.findChessboardCorners` when called.  There is no CPU path: without a GPU every compute entry raises `VbsError`.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

# The reference's settings under the reference's key names.  Read here: the two filters and the offset; kept only so that code
# written against the reference finds them: the file names and the chessboard description (inner corners, square edge in mm).
CONFIG = dict(MIN_AREA=100, MIN_CIRCULARITY=0.85, DIAMETER_OFFSET_MM=0.0)
CONFIG.update(CHESSBOARD_SIZE=(6, 6), SQUARE_SIZE_MM=3.0)
CONFIG.update(INPUT_IMAGE="markerdiameter/diameter1.jpg", OUTPUT_IMG="annotated_result.png",
              OUTPUT_PLOT="diameter_statistics.png")

_engines = {}               # (height, width, device index) -> Engine made here for calls without one; see close_engines


def _engine_for(height, width, frames):
    """One cached Engine per geometry for callers that pass none (a recording measured image by image builds ONE handle).
    Its pass holds up to 64 frames; longer batches are looped inside the library."""
    import torch
    from .engine import Engine
    key = (int(height), int(width), torch.cuda.current_device())
    if key not in _engines:
        _engines[key] = Engine(key[0], key[1], max_markers=512, max_batch=64 if frames > 1 else 1)
    elif frames > 1 and _engines[key].max_batch == 1:
        _engines.pop(key).close()
        _engines[key] = Engine(key[0], key[1], max_markers=512, max_batch=64)
    return _engines[key]


def close_engines():
    """Destroy the engines this module made for calls without an `engine` argument (their device workspaces)."""
    while _engines:
        _engines.popitem()[1].close()


def scale_from_corners(corners, pattern_size, square_mm):
    """Pixels per millimetre from chessboard corners (`calculate_scale` :54-71): the mean distance between corners adjacent
    along a row and along a column, over `square_mm`.  `corners`: pattern_size[0] * pattern_size[1] points in
    `findChessboardCorners`' layout ([k, 1, 2] or [k, 2]), corner (r, c) at index r * pattern_size[0] + c."""
    n0, n1 = int(pattern_size[0]), int(pattern_size[1])
    c = np.asarray(corners).reshape(-1, 2)
    if c.shape[0] != n0 * n1:
        raise ValueError(f"expected {n0 * n1} corners, got {c.shape[0]}")
    g = c.reshape(n1, n0, 2)
    d = np.concatenate([np.linalg.norm(g[:, :-1] - g[:, 1:], axis=2).ravel(),
                        np.linalg.norm(g[:-1] - g[1:], axis=2).ravel()])
    return np.mean(d) / square_mm


def calculate_scale(gray_img, pattern_size, square_mm):
    raise NotImplementedError("calculate_scale locates the chessboard with cv2.findChessboardCorners, which is out of this "
                              "project's scope: find the corners with a detector of your own and pass them to "
                              "scale_from_corners(corners, pattern_size, square_mm)")


def scale_from_image(gray_img, pattern_size, square_mm, engine=None):
    """The working form of `calculate_scale` (:48-74): find the `pattern_size` inner corners of the board in one gray [H,W] or
    BGR [H,W,3] image on the device and return (pixels per millimetre, corners float32 [k,1,2] as cv2 hands them on), or
    (None, None) when the board is not found.  Without `engine`, the cached engine of the image's size is used."""
    import torch
    if not torch.cuda.is_available():
        raise L.VbsError("no GPU visible: diameter_validation has no CPU path")
    f = _as_batch(gray_img)
    if f.shape[0] != 1:
        raise ValueError("scale_from_image takes one image")
    if engine is None:
        engine = _engine_for(f.shape[1], f.shape[2], 1)
    found, corners, _, _ = engine.find_chessboard_corners(f, pattern_size)
    if not int(found[0].item()):
        return None, None
    c = corners[0].cpu().numpy()
    return scale_from_corners(c, pattern_size, square_mm), c.astype(np.float32).reshape(-1, 1, 2)


def _as_batch(frames):
    """uint8 [H,W] | [H,W,3] | [N,H,W] | [N,H,W,3] (array or tensor) -> tensor [N,H,W] or [N,H,W,3].  A 3-D input whose last
    dimension is 3 is ONE BGR image (a gray batch of width 3 is below the library's minimum width anyway)."""
    import torch
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    if f.dim() == 2 or (f.dim() == 3 and f.shape[-1] == 3):
        f = f.unsqueeze(0)
    if f.dim() not in (3, 4) or (f.dim() == 4 and f.shape[-1] != 3) or f.dtype != torch.uint8:
        raise ValueError("expected uint8 images [H,W], [H,W,3], [N,H,W] or [N,H,W,3]")
    return f


def measure_frames(frames, scale, threshold, engine=None):
    """A whole recording at once: device tensors (records, counts, stats) of `Engine.measure_markers` with CONFIG's filters.
    Without `engine`, one engine per image size is made at first use and kept (`close_engines` releases them)."""
    import torch
    if not torch.cuda.is_available():
        raise L.VbsError("no GPU visible: diameter_validation has no CPU path")
    f = _as_batch(frames)
    if engine is None:
        engine = _engine_for(f.shape[1], f.shape[2], f.shape[0])
    f = f.to(engine.device)
    return engine.measure_markers(f, threshold, scale, CONFIG["MIN_AREA"], CONFIG["MIN_CIRCULARITY"],
                                  CONFIG["DIAMETER_OFFSET_MM"])


def measure_markers(gray_img, scale, threshold, engine=None):
    """`measure_markers(gray_img, scale, threshold)` for one gray [H,W] or BGR [H,W,3] image: (records, diameters).  The
    reference blurs in `main` (:218) and passes the blurred image; here the blur is part of the device pass, so pass the
    UNBLURRED image.  `records`: float64 array [k, DIAM_COLS], one row per valid marker in the reference's contour order
    (include/vbs.h lists the columns; the reference returns the contours themselves); `diameters`: list of k floats (mm).
    Raises VbsError when the frame exceeds a device capacity - never a truncated list."""
    f = _as_batch(gray_img)
    if f.shape[0] != 1:
        raise ValueError("measure_markers takes one image; measure_frames takes a batch")
    rec, counts, _ = measure_frames(f, scale, threshold, engine)
    k = int(counts[0].item())
    if k < 0:
        raise L.VbsError(f"measure_markers: {L.status_text(k)}, or a valid marker larger than {L.DIAM_MAX_EXTENT} px "
                         f"(status {k})")
    r = rec[0, :k].cpu().numpy()
    return r, [float(v) for v in r[:, 3]]


def summarize(diameters):
    """(mean, np.std) of the diameters, as the reference prints them (:233-234)."""
    d = np.asarray(diameters, dtype=np.float64)
    return float(np.mean(d)), float(np.std(d))
