"""numpy restatement of the arithmetic ``iris.denoiser`` commits to (csrc/denoiser.h): spectral bias subtraction on the
Griffin-Lim stage's transforms (tests/griffin_lim_restatement.py; window and frames of tests/mel_restatement.py).

    a = stft(y)[t, k];  mag = sqrt(re re + im im);  g = max(mag - strength bias[k], 0);  scale = g / mag where mag > 0, else 0
    c = scale a;  out = istft(c)          bins 0 and n_fft / 2 are real
    bias estimate: the mean of mag[t, k] over the frames whose window lies wholly inside the signal

``dtype=np.float64`` runs it with the FFT; ``dtype=np.float32`` runs the same steps on fp32 arrays with fp32 products and sums
on the library's own design tables (``GriffinLim.design()``: ``dft``, ``idft``, ``wsq``), as matrix products -- the arithmetic
the device does, in numpy's order (the siblings' ``e32`` scheme).  Spectra are ``[T, K]``.
"""
from __future__ import annotations

import numpy as np

import griffin_lim_restatement as G


def stft_parts(y, n_fft: int, hop: int, win: int, dtype=np.float64, tables=None):
    """``(re, im) [T, K]`` of dtype, T = 1 + len(y) // hop; the imaginary parts of bins 0 and n_fft / 2 are exactly 0."""
    if dtype == np.float64:
        a = G.stft(y, n_fft, hop, win)
        re, im = a.real.copy(), a.imag.copy()
    else:
        re, im = G.stft_f32(np.asarray(y, dtype=np.float32), tables["dft"], n_fft, hop)
        assert re.dtype == np.float32 and im.dtype == np.float32
    im[:, 0] = 0
    im[:, -1] = 0
    return re, im


def magnitude(re, im):
    return np.sqrt(re * re + im * im)


def subtract(re, im, bias, strength: float):
    """``(cre, cim, clamped)``: the scaled spectrum and where the clamp at 0 is active (``mag <= strength bias``)."""
    dtype = re.dtype.type
    mag = magnitude(re, im)
    g = np.maximum(mag - dtype(strength) * np.asarray(bias, dtype=dtype)[None, :], dtype(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(mag > 0, g / mag, dtype(0))
    assert scale.dtype == re.dtype
    return scale * re, scale * im, g <= 0


def inverse(cre, cim, n_fft: int, hop: int, win: int, tables=None):
    if cre.dtype == np.float64:
        return G.istft(cre + 1j * cim, n_fft, hop, win)
    return G.istft_f32(cre, cim, tables["idft"], tables["wsq"], n_fft, hop)


def denoise(y, bias, strength: float, n_fft: int, hop: int, win: int, dtype=np.float64, tables=None):
    """``y [L]`` (L a multiple of hop) -> ``out [L]`` of dtype."""
    assert len(y) % hop == 0
    re, im = stft_parts(y, n_fft, hop, win, dtype, tables)
    cre, cim, _ = subtract(re, im, bias, strength)
    out = inverse(cre, cim, n_fft, hop, win, tables)
    assert out.shape == (len(y),) and out.dtype == dtype
    return out


def interior(T: int, n_fft: int, hop: int):
    """``(t_lo, t_hi)``: frames t_lo <= t < t_hi have their window ``[t hop - n_fft / 2, t hop + n_fft / 2)`` inside
    ``[0, hop (T - 1))``."""
    edge = -(-(n_fft // 2) // hop)
    return edge, T - edge


def estimate_bias(y, n_fft: int, hop: int, win: int, dtype=np.float64, tables=None):
    """``bias [K]`` of dtype: the terms are of dtype, their sum is float64 in ascending t and is rounded once."""
    re, im = stft_parts(y, n_fft, hop, win, dtype, tables)
    lo, hi = interior(re.shape[0], n_fft, hop)
    if hi <= lo:
        raise ValueError("no interior frame")
    mag = magnitude(re, im)[lo:hi].astype(np.float64)
    total = np.zeros(mag.shape[1])
    for t in range(mag.shape[0]):
        total = total + mag[t]
    return (total / (hi - lo)).astype(dtype)
