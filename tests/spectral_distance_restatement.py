"""numpy restatement of the rules ``iris.metrics`` commits to (csrc/spectral_distance.h), twice.

Per resolution ``(n_fft, hop, win)``, ``K = n_fft // 2 + 1``, an item of ``n`` samples has ``T = 1 + n // hop`` frames (0 for
``n == 0``); frame t covers samples ``[t hop - n_fft / 2, t hop + n_fft / 2)`` of the item, 0 outside ``[0, n)`` -- every sample
counts, ``n`` need not be a multiple of ``hop`` -- under a periodic Hann of ``win`` centred in ``n_fft``.  With ``A``, ``B`` the
magnitudes of ``ref`` and ``test``:

    d2 = sum (A - B)^2      a2 = sum A^2      l1 = sum |ln max(A, 1e-5) - ln max(B, 1e-5)|        over the T K cells
    e2 = sum (x - y)^2      x2 = sum x^2      emax = max |x - y| (the difference in float32)      over the n samples

``sums(ref, test, resolutions)`` is float64 throughout (FFT).  ``sums(..., f32=True)`` is the device's chain: the windowed DFT
table evaluated in double and rounded once to float32, and the transform as oracle/dsp_chain_cases.py restates ``stft_kernel``
-- one float32 fmaf chain per tap and 64 samples of a frame (the "Summation" paragraph of csrc/stft_f32.h), the chains added
one after the other -- then float32 ``sqrt(re re + im im)``, and from there on -- the sums over cells -- the same float64 steps
as the first.  The sample-domain sums
have no float32 step besides ``emax``, so both forms give the same values for them.
"""
from __future__ import annotations

import numpy as np

from oracle import dsp_chain_cases as D

FLOOR = 1e-5
DEFAULT = ((512, 128, 512), (1024, 256, 1024), (2048, 512, 2048))


def window(n_fft: int, win: int) -> np.ndarray:
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    lpad = (n_fft - win) // 2
    return np.pad(w, (lpad, n_fft - win - lpad))


def n_frames(n: int, hop: int) -> int:
    return 1 + n // hop if n > 0 else 0


def frames(x: np.ndarray, n_fft: int, hop: int) -> np.ndarray:
    """``[T, n_fft]`` of x's dtype: the frames of the zero-padded item, built one by one."""
    T = n_frames(len(x), hop)
    y = np.pad(x, (n_fft // 2, n_fft // 2))
    out = np.zeros((T, n_fft), dtype=x.dtype)
    for t in range(T):
        out[t] = y[t * hop:t * hop + n_fft]
    return out


def magnitudes(x, n_fft: int, hop: int, win: int) -> np.ndarray:
    """``[T, K]`` float64."""
    fr = frames(np.asarray(x, dtype=np.float64), n_fft, hop) * window(n_fft, win)[None, :]
    return np.abs(np.fft.rfft(fr, n=n_fft, axis=1)).reshape(fr.shape[0], n_fft // 2 + 1)


_TABLES = {}


def dft_table(n_fft: int, win: int):
    """``(cos, sin) [K, n_fft]`` float32: ``w[n] cos(2 pi k n / n_fft)`` and the sine in double, the angle reduced by
    ``(k n) mod n_fft``, rounded once (csrc/stft_f32.h, fill_dft)."""
    if (n_fft, win) not in _TABLES:
        w = window(n_fft, win)
        j = (np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]) % n_fft
        c, s = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft), np.sin(2.0 * np.pi * np.arange(n_fft) / n_fft)
        s[0] = 0.0
        s[n_fft // 2] = 0.0
        _TABLES[(n_fft, win)] = ((w[None, :] * c[j]).astype(np.float32), (w[None, :] * s[j]).astype(np.float32))
    return _TABLES[(n_fft, win)]


def magnitudes_f32(x, n_fft: int, hop: int, win: int, fma: int = 0) -> np.ndarray:
    """``[T, K]`` float32 by the device's chain, as oracle/dsp_chain_cases.py restates ``stft_kernel`` and ``dn::Magnitude``: one
    fmaf chain per tap and run of 64 samples, the chains added in that order; ``fma`` says how ``re re + im im`` is contracted
    (0: both products rounded, what dn_stft_kernel<magnitude> was measured to do)."""
    x = np.asarray(x, dtype=np.float32)
    cfg = dict(n_fft=n_fft, hop_length=hop, win_length=win, n_mels=1)
    acc = D.window_acc(x, 0, n_frames(len(x), hop), cfg, {"dft": np.stack(dft_table(n_fft, win))})
    mag = D.magnitude_launch(acc, cfg, {"mag": fma})
    assert mag.dtype == np.float32
    return mag


def cell_sums(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """``(d2, a2, l1)`` float64 from two magnitude arrays of one dtype; every term is formed in float64."""
    a, b = A.astype(np.float64), B.astype(np.float64)
    return np.array([np.sum((a - b) ** 2), np.sum(a * a), np.sum(np.abs(np.log(np.maximum(a, FLOOR)) - np.log(np.maximum(b, FLOOR))))])


def wave_sums(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """``(e2, x2, emax)`` float64 from two float32 signals."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if not len(x):
        return np.zeros(3)
    d = x.astype(np.float64) - y.astype(np.float64)
    return np.array([np.sum(d * d), np.sum(x.astype(np.float64) ** 2), float(np.max(np.abs(x - y)))])


def sums(ref, test, resolutions=DEFAULT, f32: bool = False) -> dict:
    """One item: ``{"spec": [R, 3], "wave": [3], "frames": [R]}``."""
    ref, test = np.asarray(ref, dtype=np.float32), np.asarray(test, dtype=np.float32)
    assert ref.shape == test.shape and ref.ndim == 1
    mags = magnitudes_f32 if f32 else magnitudes
    spec = np.zeros((len(resolutions), 3))
    for r, (n_fft, hop, win) in enumerate(resolutions):
        if len(ref):
            spec[r] = cell_sums(mags(ref, n_fft, hop, win), mags(test, n_fft, hop, win))
    return {"spec": spec, "wave": wave_sums(ref, test),
            "frames": np.array([n_frames(len(ref), hop) for _, hop, _ in resolutions], dtype=np.int32)}


def finish(s: dict, resolutions=DEFAULT) -> dict:
    """The finished measures of one item, float64, numpy's rules for divisions by zero."""
    bins = np.array([n // 2 + 1 for n, _, _ in resolutions], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.sqrt(s["spec"][:, 0] / s["spec"][:, 1])
        l1 = s["spec"][:, 2] / (s["frames"].astype(np.float64) * bins)
        snr = 10.0 * np.log10(s["wave"][1] / s["wave"][0])
    return {"spectral_convergence": sc, "log_stft_l1": l1, "mr_spectral_convergence": sc.mean(), "mr_log_stft_l1": l1.mean(),
            "snr_db": snr, "emax": s["wave"][2]}
