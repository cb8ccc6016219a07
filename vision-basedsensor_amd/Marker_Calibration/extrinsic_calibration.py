"""Path-compatible stand-in for the reference's `code/Marker_Calibration/extrinsic_calibration.py`."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
from vbs_amd.extrinsic_calibration import (CameraParameters, MARKER_DIAMETER_MM, load_intrinsics_from_excel,  # noqa: E402,F401
                                           calibrate_camera_extrinsics, calibrate_recording, save_extrinsics_to_excel,
                                           merge_correspondences, plot_3d_calibration_result, main)

if __name__ == "__main__":
    main()
