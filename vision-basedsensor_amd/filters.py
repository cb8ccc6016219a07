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
