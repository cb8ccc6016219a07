"""Tap designs for `engine.fir_series_f64` (NumPy only).  The device filter divides by the sum of the taps it could use, so
only the SHAPE of a design matters; the designs here still have unit DC gain, like their scipy counterparts."""
from __future__ import annotations

import numpy as np

SYMMETRY_TOL = 1e-12           # |w[k] - w[K-1-k]| <= SYMMETRY_TOL * max|w|, else the taps are refused


def _odd(n_taps) -> int:
    n = int(n_taps)
    if n != n_taps or n < 1 or n % 2 == 0:
        raise ValueError(f"n_taps must be a positive odd integer, got {n_taps!r}")
    return n


def lowpass_taps(n_taps: int, cutoff: float) -> np.ndarray:
    """The Hamming-windowed sinc with unit DC gain, `cutoff` as a fraction of the Nyquist frequency: what
    `scipy.signal.firwin(n_taps, cutoff)` returns (the same statements of the window method), then made exactly symmetric."""
    n = _odd(n_taps)
    cutoff = float(cutoff)
    if not (0.0 < cutoff < 1.0):
        raise ValueError(f"cutoff must lie inside (0, 1) (a fraction of Nyquist), got {cutoff!r}")
    m = np.arange(n) - 0.5 * (n - 1)
    h = cutoff * np.sinc(cutoff * m)
    win = 0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, n)) if n > 1 else np.ones(1)
    h = h * win
    h = h / h.sum()
    return 0.5 * (h + h[::-1])


def moving_average_taps(n_taps: int) -> np.ndarray:
    n = _odd(n_taps)
    return np.full(n, 1.0 / n)


KIN_MAX_HALF, KIN_MAX_DEGREE = 127, 3        # VBS_KIN_MAX_HALF, VBS_KIN_MAX_DEGREE of include/vbs.h


def poly_scale(half_window) -> int:
    """H of the local polynomial fit: the smallest power of two >= max(half_window, 1), so that u = delta / H is exact."""
    H = 1
    while H < int(half_window):
        H *= 2
    return H


def ldl_pivots(S, degree):
    """The square-root-free factorisation G = L diag(D) L^T of the Hankel matrix G[a][b] = S[a + b] in the order
    `vbs_poly_fit_f64` states (include/vbs.h), float64, every expression as written: -> (D [d + 1], L [d + 1, d + 1], unit lower
    triangle).  A zero or NaN pivot gives inf / NaN below it, as on the device; nothing is raised."""
    d = int(degree)
    S = np.asarray(S, dtype=np.float64)
    D = np.zeros(d + 1)
    Lm = np.eye(d + 1)
    V = np.zeros((d + 1, d + 1))
    with np.errstate(all="ignore"):
        for j in range(d + 1):
            t = S[2 * j]
            for m in range(j):
                t = t - V[j, m] * Lm[j, m]
            D[j] = t
            for a in range(j + 1, d + 1):
                w = S[a + j]
                for m in range(j):
                    w = w - V[a, m] * Lm[j, m]
                V[a, j] = w
                Lm[a, j] = w / t
    return D, Lm


def poly_window(half_window, window="hann") -> np.ndarray:
    """The 2h + 1 weights of the local polynomial fit: `spectra.window_taps(h, window)` for "hann" and "rect"; an array of
    2h + 1 weights is taken as it is once it is symmetric (`half_taps`), finite and >= 0 with a centre > 0."""
    from .spectra import window_taps
    h = int(half_window)
    if isinstance(window, str):
        return window_taps(h, window)
    w = np.asarray(window, dtype=np.float64)
    if w.shape != (2 * h + 1,):
        raise ValueError(f"a window given as weights must have 2 half_window + 1 = {2 * h + 1} of them")
    half = half_taps(w)
    if (half < 0.0).any() or not half[0] > 0.0:
        raise ValueError("the window's weights must be finite and >= 0, the centre > 0")
    return np.concatenate([half[:0:-1], half])


def poly_taps(half_window, degree, window="hann"):
    """The tap rows of the gap-aware local polynomial fit along time (`engine.poly_moments_f64`): -> (taps, sw,
    piv_full).  h = `half_window` in 0 .. 127, d = `degree` in 0 .. 3, w = `poly_window(h, window)` ("hann", "rect" or 2h + 1
    weights of the caller's), H = `poly_scale(h)`,
    u = delta / H.  taps float64 [2d + 1, 2h + 1], taps[k][delta + h] = w[delta] * u^k with u^k formed by repeated multiplication:
    |delta|^k < 2^42 and H is a power of two, so every power is EXACT and a tap carries ONE rounding, that of its product with w
    (none for "rect").  sw = the ascending sum of w.  piv_full float64 [d + 1] = the pivots D_0 .. D_d of the gap-free full
    window: `ldl_pivots` of the ascending sums of the tap rows."""
    h, d = int(half_window), int(degree)
    if h != half_window or not (0 <= h <= KIN_MAX_HALF):
        raise ValueError(f"half_window must be an integer in 0 .. {KIN_MAX_HALF}, got {half_window!r}")
    if d != degree or not (0 <= d <= KIN_MAX_DEGREE):
        raise ValueError(f"degree must be an integer in 0 .. {KIN_MAX_DEGREE}, got {degree!r}")
    w = poly_window(h, window)
    u = np.arange(-h, h + 1, dtype=np.float64) / poly_scale(h)
    taps = np.empty((2 * d + 1, 2 * h + 1))
    p = np.ones(2 * h + 1)
    for k in range(2 * d + 1):
        taps[k] = w * p
        p = p * u
    S = np.zeros(2 * d + 1)
    for j in range(2 * h + 1):
        S = S + taps[:, j]
    return taps, float(S[0]), ldl_pivots(S, d)[0]


def half_taps(taps) -> np.ndarray:
    """Full odd-length taps -> [centre, mean of the pair at distance 1, ..., at distance h]: what `vbs_fir_series_f64` takes.
    ValueError unless the array is symmetric within SYMMETRY_TOL * max|w| (an asymmetric filter would not be zero-phase)."""
    w = np.asarray(taps, dtype=np.float64)
    if w.ndim != 1 or w.size < 1 or w.size % 2 == 0:
        raise ValueError("taps must be a 1-D array of odd length")
    if not np.isfinite(w).all():
        raise ValueError("taps must be finite")
    if (np.abs(w - w[::-1]) > SYMMETRY_TOL * np.abs(w).max()).any():
        raise ValueError("taps are not symmetric (|w[k] - w[K-1-k]| > 1e-12 max|w|): the filter would not be zero-phase")
    h = w.size // 2
    return 0.5 * (w[h:] + w[h::-1])
