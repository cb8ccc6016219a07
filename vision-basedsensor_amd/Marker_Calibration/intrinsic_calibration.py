"""Path-compatible stand-in for the reference's `code/Marker_Calibration/intrinsic_calibration.py`."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
from vbs_amd.intrinsic_calibration import (crop_image, save_calib_results, collect_corners, calibrate_camera,  # noqa: E402,F401
                                           plot_comparison, plot_3d_poses, calibrate_points, calibrate_subsets, jackknife,
                                           rodrigues)
