"""Bases and frequency grids for `engine.project_series_f64` / `engine.harmonic_fit_f64` (NumPy only).  The basis is computed on
the host, as the FIR's taps (`filters.py`) and the smoother's weights (`fields.py`) are, so that no `sin` / `cos` of the device
enters a result; amplitude and phase are the caller's too: the fit kernel has no square root and no `atan2`."""
import numpy as np


def _freqs(freqs):
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    if nu.size < 1 or not np.isfinite(nu).all() or (nu <= 0.0).any() or (nu > 0.25).any():
        raise ValueError("freqs must be at least one finite frequency in cycles per frame, each in (0, 0.25] "
                         "(twice the frequency stays at or below Nyquist)")
    return nu


def harmonic_basis(n, freqs):
    """The basis `harmonic_fit_f64` expects, float64 [1 + 4 Q, n] for the Q frequencies `freqs` (cycles per frame, each in
    (0, 0.25]) and the frames f = 0 .. n-1: row 0 all ones; rows 1 + 2q, 2 + 2q the cos and sin of 2 pi nu_q f; rows
    1 + 2Q + 2q, 2 + 2Q + 2q the cos and sin of 2 pi (2 nu_q) f, whose sums over the valid frames stand in for the sums of
    cos^2, sin^2 and cos sin (the half-angle identities)."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    nu = _freqs(freqs)
    Q = nu.size
    f = np.arange(n, dtype=np.float64)
    B = np.empty((1 + 4 * Q, n), dtype=np.float64)
    B[0] = 1.0
    th = 2.0 * np.pi * nu[:, None] * f[None, :]
    B[1:1 + 2 * Q:2], B[2:2 + 2 * Q:2] = np.cos(th), np.sin(th)
    th = 2.0 * np.pi * (2.0 * nu)[:, None] * f[None, :]
    B[1 + 2 * Q::2], B[2 + 2 * Q::2] = np.cos(th), np.sin(th)
    return B


def carrier(n, nu):
    """The carrier `engine.window_moments_f64` expects, float64 [4, n]: cos and sin of 2 pi nu f and of 2 pi (2 nu) f at the frames
    f = 0 .. n-1 (rows 1, 2 and 3, 4 of `harmonic_basis(n, [nu])`, bit for bit).  nu in cycles per frame, in (0, 0.25]."""
    return np.ascontiguousarray(harmonic_basis(n, [float(nu)])[1:5])


def window_taps(half_window, kind="hann"):
    """The full odd-length window of 2 h + 1 weights for `engine.window_moments_f64`, exactly symmetric.  "hann":
    0.5 (1 + cos(pi k / (h + 1))), k = -h .. h, strictly positive (the zeros of the Hann window lie one step outside); "rect":
    all ones."""
    h = int(half_window)
    if h != half_window or h < 0:
        raise ValueError(f"half_window must be an integer >= 0, got {half_window!r}")
    if kind == "rect":
        return np.ones(2 * h + 1)
    if kind != "hann":
        raise ValueError('kind must be "hann" or "rect"')
    k = np.abs(np.arange(-h, h + 1)).astype(np.float64)
    return 0.5 * (1.0 + np.cos(np.pi * k / (h + 1)))


def zoom_grid(centre, half_width, Q):
    """Q equally spaced frequencies over [centre - half_width, centre + half_width] (Q = 1: the centre alone): a grid finer than
    the natural 1 / n round a known line.  With Q odd the centre is bin (Q - 1) / 2."""
    Q = int(Q)
    c, h = float(centre), float(half_width)
    if Q < 1 or not (np.isfinite(c) and np.isfinite(h) and h >= 0.0):
        raise ValueError("zoom_grid needs Q >= 1, a finite centre and a finite half_width >= 0")
    return _freqs(np.array([c]) if Q == 1 else c + h * np.linspace(-1.0, 1.0, Q))


def amplitude_phase(a, b):
    """Amplitude hypot(a, b) and phase degrees(arctan2(b, a)) of a cos(theta) + b sin(theta) = A cos(theta - phi)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.hypot(a, b), np.degrees(np.arctan2(b, a))


def to_hz(freqs, fps):
    """Cycles per frame -> Hz at `fps` frames per second."""
    fps = float(fps)
    if not (np.isfinite(fps) and fps > 0.0):
        raise ValueError("fps must be finite and > 0")
    return np.asarray(freqs, dtype=np.float64) * fps
