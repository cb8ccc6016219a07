"""CPU tests of what k_ncc_mfma's pre-scan rests on (no GPU): the host's bound on the empty correlation window
(`vbs_ncc_trim_guard`: such a window must be background for every cut a frame size can produce before the kernel may skip
it), and the skipping rule itself, restated in NumPy and held against the oracle on the very inputs the GPU tests use: the
oracle's mask is zero wherever the rule lets the kernel write zeros without computing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vbs_amd._lib as L
from oracle import stages as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import ncc_trim_cases as TC                                   # noqa: E402

TEMPLATES = [(80, 13.0), (33, 7.4)]
SIZES = [(64, 128), (480, 4096), (481, 128), (1024, 1280), (1200, 1920)]
SHAPES = [(481, 128), (560, 320), (560, 244), (64, 128), (200, 256)]    # those of tests/test_gpu_ncc_trim.py


def guard(l, sigma, h, w, shift=0.0):
    mn = C.c_double(0.0)
    rc = L.lib().vbs_ncc_trim_guard(l, sigma, h, w, shift, C.byref(mn))
    assert rc in (0, 1), rc
    return rc == 1, mn.value


def window_cuts_min(l, sigma, h, w):
    """min of sum_t - n tbar over every window cut, straight from the oracle's template (float64)"""
    t = O.gkern(l, sigma)
    lo, hi = O.ncc_window(l)
    tbar = t.mean()

    def cuts(size):
        out = set()
        for p in list(range(min(size, l))) + list(range(max(size - l, 0), size)):
            out.add((max(0, -(p + lo)), min(l, size - (p + lo))))      # template indices [a, b) inside the image
        return sorted(out)
    cy = np.cumsum(np.vstack([np.zeros((1, l)), t]), axis=0)
    best = np.inf
    for a, b in cuts(h):
        rows = np.concatenate([[0.0], np.cumsum(cy[b] - cy[a])])
        for c, d in cuts(w):
            best = min(best, (rows[d] - rows[c]) - (b - a) * (d - c) * tbar)
    return best


@pytest.mark.parametrize("l,sigma", TEMPLATES)
@pytest.mark.parametrize("h,w", SIZES)
def test_guard_holds_for_both_templates(l, sigma, h, w):
    ok, mn = guard(l, sigma, h, w)
    want = window_cuts_min(l, sigma, h, w)
    print(f"l={l} {h}x{w}: min d0 = {mn:.3e} (oracle template: {want:.3e})")
    assert abs(mn - want) <= 1e-11                       # (two float64 sums of <= 6400 terms <= 1: 6400 * 2^-52 each, with room)
    assert ok and mn > -5e-5


@pytest.mark.parametrize("l,sigma", TEMPLATES)
def test_guard_fails_for_a_shifted_template_mean(l, sigma):
    """a template mean 1e-3 / l^2 too large makes the full window's d0 = 1 - l^2 tbar = -1e-3: the kernel must not trim"""
    ok, mn = guard(l, sigma, 1024, 1280, 1e-3 / (l * l))
    assert not ok and mn < -5e-5
    assert guard(l, sigma, 1024, 1280, -1e-3 / (l * l))[0]
    assert L.lib().vbs_ncc_trim_guard(1, sigma, 64, 128, 0.0, None) == L.VBS_EINVAL


@pytest.mark.parametrize("h,w", SHAPES)
def test_oracle_mask_is_zero_on_every_tile_the_rule_skips(h, w):
    l = O.branch_params(h)["tl"]
    skipped = 0
    for name, area in TC.patterns(h, w):
        dead = TC.dead_pixels(area, l)
        mask = TC.oracle_mask(area)
        assert not (mask & dead).any(), name
        skipped += int(dead.sum())
        if name in ("zero",):
            assert dead.all()
        if name in ("full",):
            assert not dead.any()
    assert skipped > 0
