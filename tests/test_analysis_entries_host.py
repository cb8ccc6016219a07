"""Host tests (no GPU) of the handle-free record entries of the C ABI (`vbs_fir_series_f64` .. `vbs_dwell_stats_f64`): the status
every entry answers to one defect at a time in otherwise valid small arguments, and `analysis._call`'s mapping of a status to an
exception.  A defect is refused before the entry selects a device, so the device index passed here is -1 and the device pointers
are dummies that nothing reads; what the entries read on the host (`half`, `thr`) are real arrays."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import vbs_amd._lib as L

N, S, COLS, NV = 4, 2, 4, 3
P = C.c_void_p(8)                                              # a device pointer nothing dereferences
NULL = C.c_void_p(0)
HALF = np.array([1.0, 0.5], dtype=np.float64)                  # read on the host: fir, window and polynomial entries
THR = np.zeros(4, dtype=np.float64)                            # read on the host: vbs_poly_fit_f64
HP, TP = HALF.ctypes.data_as(C.c_void_p), THR.ctypes.data_as(C.c_void_p)
GRID_SLOTS = 65535 * 64                                        # the slots one launch grid of the tiled entries holds

# entry -> its arguments between `device` and `stream`, in order, valid as they stand
ENTRIES = {
    "vbs_fir_series_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, half=HP, n_half=2, min_coverage=0.5, frame_begin=0,
                               frame_end=N, out=P),
    "vbs_hampel_series_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, half_window=1, min_count=2, k_sigma=3.0, min_scale=0.0,
                                  frame_begin=0, frame_end=N, out=P, clean=P),
    "vbs_window_moments_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, carrier=P, half=HP, n_half=2, frame_begin=0,
                                   frame_end=N, mom=P),
    "vbs_window_fit_f64": dict(mom=P, n=N, s=S, n_values=NV, sw=2.0, min_coverage=0.5, det_min=1e-3, fit=P),
    "vbs_poly_moments_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, half=HP, n_half=2, degree=2, frame_begin=0, frame_end=N,
                                 mom=P),
    "vbs_poly_fit_f64": dict(mom=P, rec=P, n=N, s=S, cols=COLS, n_values=NV, degree=2, half_window=1, thr=TP, fill_degree=1,
                             frame_begin=0, frame_end=N, fit=P, filled=P),
    "vbs_cross_moments_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, shift=P, mom=P),
    "vbs_covariance_f64": dict(mom=P, s=S, n_values=NV, mode=1, min_count=2, denom=3.0, slot_mask=P, cov=P, ok=P),
    "vbs_leading_modes_f64": dict(A=P, C=6, r=2, iters=8, tiny=1e-24, work=P, values=P, modes=P, resid=P, info=P),
    "vbs_mode_scores_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, center=P, modes=P, r=2, min_coverage=0.5, frame_begin=0,
                                frame_end=N, scores=P, energy=P),
    "vbs_field_map_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, W=P, wsum=P, P=5, min_coverage=0.5, frame_begin=0,
                              frame_end=N, map=P),
    "vbs_patch_stats_f64": dict(map=P, n=N, P=5, n_values=NV, grid_xy=P, component=2, sign=1.0, thr=0.0, patch=P),
    "vbs_project_series_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, basis=P, R=5, proj=P),
    "vbs_harmonic_fit_f64": dict(proj=P, s=S, R=5, n_values=NV, Q=1, min_count=3, det_min=1e-3, fit=P, peak=P),
    "vbs_motion_series_f64": dict(rec=P, n=N, s=S, cols=COLS, pos=P, slot_mask=P, reject_k=0.0, frame_begin=0, frame_end=N, grad=P,
                                  strain=P, residual=P),
    "vbs_local_strain_f64": dict(rec=P, n=N, s=S, cols=COLS, pos=P, nbr=P, K=4, min_count=4, det_rel=0.01, frame_begin=0,
                                 frame_end=N, out=P),
    "vbs_step_response_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, window=2, min_count=1, out=P),
    "vbs_find_steps_f64": dict(rec=P, n=N, s=S, cols=COLS, window=2, thr2=0.0, max_steps=4, steps=P),
    "vbs_dwell_stats_f64": dict(rec=P, n=N, s=S, cols=COLS, n_values=NV, steps=P, steps_rows=1, max_steps=4, guard=0, out=P),
}

# the pointers an entry refuses as null one at a time (the others are optional, or optional as a group: below)
REQUIRED = {
    "vbs_fir_series_f64": ("rec", "half", "out"),
    "vbs_hampel_series_f64": ("rec", "out"),
    "vbs_window_moments_f64": ("rec", "carrier", "half", "mom"),
    "vbs_window_fit_f64": ("mom", "fit"),
    "vbs_poly_moments_f64": ("rec", "half", "mom"),
    "vbs_poly_fit_f64": ("mom", "rec", "thr", "fit"),
    "vbs_cross_moments_f64": ("rec", "mom"),
    "vbs_covariance_f64": ("mom", "cov"),
    "vbs_leading_modes_f64": ("A", "work", "values", "modes", "resid", "info"),
    "vbs_mode_scores_f64": ("rec", "center", "modes", "scores"),
    "vbs_field_map_f64": ("rec", "W", "wsum", "map"),
    "vbs_patch_stats_f64": ("map", "grid_xy", "patch"),
    "vbs_project_series_f64": ("rec", "basis", "proj"),
    "vbs_harmonic_fit_f64": ("proj",),
    "vbs_motion_series_f64": ("rec", "pos"),
    "vbs_local_strain_f64": ("rec", "pos", "nbr", "out"),
    "vbs_step_response_f64": ("rec", "out"),
    "vbs_find_steps_f64": ("rec", "steps"),
    "vbs_dwell_stats_f64": ("rec", "steps", "out"),
}
ALL_OUTPUTS_NULL = {"vbs_harmonic_fit_f64": ("fit", "peak"), "vbs_motion_series_f64": ("grad", "strain", "residual")}

# over-capacity shapes: VBS_ECAPACITY, answered after every VBS_EINVAL check and before a device is selected
CAPACITY = {
    "vbs_window_moments_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)),
    "vbs_window_fit_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)),
    "vbs_poly_moments_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)),
    "vbs_poly_fit_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1)),
    "vbs_cross_moments_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.MOM_MAX_SLOTS + 1)),
    "vbs_covariance_f64": (dict(s=L.MOM_MAX_SLOTS + 1),),
    "vbs_leading_modes_f64": (dict(C=L.MODES_MAX_DIM + 1),),
    "vbs_mode_scores_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.MOM_MAX_SLOTS + 1)),
    "vbs_field_map_f64": (dict(s=L.FIELD_MAX_SLOTS + 1), dict(P=L.FIELD_MAX_POINTS + 1), dict(s=GRID_SLOTS + 1)),
    "vbs_patch_stats_f64": (dict(P=L.FIELD_MAX_POINTS + 1),),
    "vbs_project_series_f64": (dict(n=L.PROJ_MAX_FRAMES + 1), dict(s=L.PROJ_MAX_SLOTS + 1), dict(R=L.PROJ_MAX_ROWS + 1)),
    "vbs_motion_series_f64": (dict(s=L.FIELD_MAX_SLOTS + 1), dict(s=GRID_SLOTS + 1)),
    "vbs_local_strain_f64": (dict(s=L.FIELD_MAX_SLOTS + 1),),
}

# further VBS_EINVAL defects of the predicates the entries share
BAD_HALF = np.array([1.0, -0.5], dtype=np.float64)
NAN_HALF = np.array([1.0, np.nan], dtype=np.float64)
ZERO_CENTRE = np.array([0.0, 0.5], dtype=np.float64)
OTHER = {
    "vbs_fir_series_f64": (dict(s=GRID_SLOTS + 1), dict(min_coverage=0.0), dict(min_coverage=1.5), dict(min_coverage=float("nan")),
                           dict(n_half=129), dict(cols=9, n_values=3), dict(frame_begin=-1), dict(frame_end=N + 1)),
    "vbs_hampel_series_f64": (dict(s=GRID_SLOTS + 1), dict(cols=1, n_values=1), dict(frame_end=N + 1)),
    "vbs_window_moments_f64": (dict(n_values=4, cols=8), dict(half=BAD_HALF.ctypes.data_as(C.c_void_p)),
                               dict(half=NAN_HALF.ctypes.data_as(C.c_void_p)), dict(half=ZERO_CENTRE.ctypes.data_as(C.c_void_p)),
                               dict(frame_begin=-1)),
    "vbs_window_fit_f64": (dict(n_values=4), dict(min_coverage=0.0)),
    "vbs_poly_moments_f64": (dict(n_values=4, cols=8), dict(half=BAD_HALF.ctypes.data_as(C.c_void_p)),
                             dict(half=NAN_HALF.ctypes.data_as(C.c_void_p)), dict(half=ZERO_CENTRE.ctypes.data_as(C.c_void_p)),
                             dict(frame_end=N + 1)),
    "vbs_poly_fit_f64": (dict(n_values=4, cols=8), dict(frame_begin=-1)),
    "vbs_cross_moments_f64": (dict(n_values=4, cols=8), dict(n=0), dict(s=0), dict(cols=9)),
    "vbs_mode_scores_f64": (dict(n_values=4, cols=8), dict(min_coverage=0.0), dict(frame_end=N + 1)),
    "vbs_field_map_f64": (dict(n_values=4, cols=8), dict(min_coverage=1.5), dict(frame_begin=-1)),
    "vbs_project_series_f64": (dict(n_values=4, cols=8),),
    "vbs_motion_series_f64": (dict(cols=3), dict(cols=9), dict(frame_end=N + 1)),
    "vbs_local_strain_f64": (dict(cols=3), dict(frame_begin=-1)),
    "vbs_step_response_f64": (dict(s=GRID_SLOTS + 1), dict(cols=9, n_values=3), dict(n_values=0)),
    "vbs_find_steps_f64": (dict(s=GRID_SLOTS + 1), dict(cols=10), dict(cols=1)),
    "vbs_dwell_stats_f64": (dict(s=GRID_SLOTS + 1), dict(cols=1, n_values=1)),
}


def _cases():
    for name, args in ENTRIES.items():
        for p in REQUIRED[name]:
            yield name, {p: NULL}, L.VBS_EINVAL
        if name in ALL_OUTPUTS_NULL:
            yield name, {p: NULL for p in ALL_OUTPUTS_NULL[name]}, L.VBS_EINVAL
        if "frame_begin" in args:
            yield name, dict(frame_begin=3, frame_end=2), L.VBS_EINVAL
        if "n_values" in args and "cols" in args:
            yield name, dict(n_values=COLS), L.VBS_EINVAL
        for d in OTHER.get(name, ()):
            yield name, d, L.VBS_EINVAL
        for d in CAPACITY.get(name, ()):
            yield name, d, L.VBS_ECAPACITY


def _id(v):
    if isinstance(v, dict):
        return ",".join(f"{k}={'null' if isinstance(x, C.c_void_p) and not x.value else 'ptr' if isinstance(x, C.c_void_p) else x}"
                        for k, x in v.items())
    return str(v)


def test_the_table_names_every_record_entry():
    first, last = L.SYMBOLS.index("vbs_fir_series_f64"), len(L.SYMBOLS)
    record = {n for n in L.SYMBOLS[first:last] if n.endswith("_f64")}
    assert record == set(ENTRIES) == set(REQUIRED)
    assert set(CAPACITY) | set(OTHER) <= set(ENTRIES)


@pytest.mark.parametrize("name,defect,status", list(_cases()), ids=_id)
def test_entry_answers_a_defect_before_it_selects_a_device(name, defect, status):
    args = dict(ENTRIES[name])
    assert set(defect) <= set(args), (name, defect)
    args.update(defect)
    assert getattr(L.lib(), name)(-1, *args.values(), NULL) == status


# ---- analysis._call: the one place a status becomes an exception ----------------------------------------------------------------
@pytest.fixture
def call(monkeypatch):
    import torch
    from vbs_amd import analysis as A
    seen = []

    def entry_returning(rc):
        def vbs_stand_in(*args):
            seen.append(args)
            return rc
        monkeypatch.setattr(A.L, "lib", lambda: types.SimpleNamespace(vbs_stand_in=vbs_stand_in))
        return seen
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0x5a))
    return A, entry_returning, torch.device("cuda", 3)


def test_call_passes_device_arguments_stream_and_returns_on_ok(call):
    A, entry_returning, dev = call
    seen = entry_returning(L.VBS_OK)
    assert A._call("vbs_stand_in", "a hint", dev, 1, 2.5, None) is None
    (args,) = seen
    assert args[:4] == (3, 1, 2.5, None) and isinstance(args[4], C.c_void_p) and args[4].value == 0x5a and len(args) == 5


def test_call_maps_einval_to_value_error_with_the_hint(call):
    A, entry_returning, dev = call
    entry_returning(L.VBS_EINVAL)
    with pytest.raises(ValueError) as e:
        A._call("vbs_stand_in", "1 <= n_values < cols <= 8", dev)
    assert str(e.value) == "vbs_stand_in: bad argument (1 <= n_values < cols <= 8)"


def test_call_maps_ecapacity_to_its_text_where_the_entry_has_one(call):
    A, entry_returning, dev = call
    entry_returning(L.VBS_ECAPACITY)
    with pytest.raises(L.VbsError) as e:
        A._call("vbs_stand_in", "a hint", dev, capacity="more than VBS_X = 4 things")
    assert str(e.value) == "vbs_stand_in: more than VBS_X = 4 things (status -2)"
    with pytest.raises(L.VbsError) as e:
        A._call("vbs_stand_in", "a hint", dev)
    assert str(e.value) == "vbs_stand_in failed (-2)"


def test_call_maps_every_other_status_to_vbs_error(call):
    A, entry_returning, dev = call
    entry_returning(L.VBS_EHIP)
    with pytest.raises(L.VbsError) as e:
        A._call("vbs_stand_in", "a hint", dev, capacity="unused")
    assert str(e.value) == "vbs_stand_in failed (-3)" and not isinstance(e.value, ValueError)
