"""Comparison of `_marker_center` results (lists of {'center', 'major_axis', 'minor_axis', 'angle'}) with the oracle's, at
the tolerances stated in the header of tests/test_gpu_parity.py: centres bit-exact, axes within 1e-3 px, the angle mod
180 degrees within 0.05 degrees where major - minor > 1e-2 px."""

TOL_AX = 1e-3


def angle_close(a, b, tol=0.05):
    d = abs((a - b + 90.0) % 180.0 - 90.0)
    return d <= tol


def compare_markers(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["center"][0] == w["center"][0] and g["center"][1] == w["center"][1]      # bit-exact
        assert abs(g["major_axis"] - w["major_axis"]) <= TOL_AX
        assert abs(g["minor_axis"] - w["minor_axis"]) <= TOL_AX
        if w["major_axis"] - w["minor_axis"] > 1e-2:
            assert angle_close(g["angle"], w["angle"]), (g, w)
