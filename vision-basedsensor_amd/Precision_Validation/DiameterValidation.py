"""Path-compatible stand-in for the reference's `code/Precision_Validation/DiameterValidation.py`."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
from vbs_amd.diameter_validation import (CONFIG, calculate_scale, scale_from_corners, measure_markers,  # noqa: E402,F401
                                         close_engines,
                                         measure_frames, summarize)
