"""numpy restatement of the arithmetic ``iris.griffin_lim`` commits to (csrc/griffin_lim.h): the reference's
``--use_griffin_lim`` path (scripts/synthesize.py:174-194), i.e. ``exp(clip(logmel, -11.513, 2.0))``, librosa 0.11's
``mel_to_stft(power=1.0)`` and ``griffinlim``.  librosa cannot be imported here, so this is written from its rules, not run
against it ("parity unpinned").  Window, frames and filterbank are tests/mel_restatement.py's.

  * inversion, per frame: ``x0 = max(pinv(fb) m, 0)`` (librosa's start), then ``nnls_iters`` projected-gradient steps
    ``x <- max(x - s fb^T (fb x - m), 0)`` with ``s = 1 / lambda_max(fb fb^T)`` (in place of librosa's L-BFGS-B);
  * ``stft``: centred, zero padding -- frame ``t`` covers samples ``[t hop - n_fft / 2, t hop + n_fft / 2)``;
  * ``istft``: ``w[n] irfft(c[t])[n]`` overlap-added, divided by the window-sum-square where that exceeds FLT_MIN
    (``librosa.util.tiny`` of float32), ``n_fft / 2`` samples trimmed at each end, ``hop (T - 1)`` samples;
  * the loop: ``a = r - momentum / (1 + momentum) r_prev`` (``r_prev = 0`` in the first pass), ``c = S a / (|a| + FLT_MIN)``.

Spectra are ``[T, K]`` here (frame-major), ``phi0`` is ``[K, T]`` as the public interface takes it.  The float64 functions use
the FFT; ``stft_direct`` is the same by a DFT matrix.  The ``*_f32`` functions run the same steps on fp32 arrays with fp32
products and sums on the library's own design tables (``GriffinLim.design()``, ``inversion_tables()``), as matrix products
-- the arithmetic the device does, in numpy's order.
"""
from __future__ import annotations

import numpy as np

import mel_restatement as M

FLT_MIN = float(np.finfo(np.float32).tiny)
LOG_LO, LOG_HI = -11.513, 2.0


# ---- float64 ------------------------------------------------------------------------------------------------------------
def stft(y, n_fft: int, hop: int, win_length: int) -> np.ndarray:
    """``[1 + len(y) // hop, n_fft // 2 + 1]`` complex128."""
    fr = M.frames(np.asarray(y, dtype=np.float64), n_fft, hop) * M.window(n_fft, win_length)[None, :]
    return np.fft.rfft(fr, axis=1)


def stft_direct(y, n_fft: int, hop: int, win_length: int) -> np.ndarray:
    """The same by the DFT matrix ``exp(-2 pi i k n / n_fft)``, no FFT."""
    fr = M.frames(np.asarray(y, dtype=np.float64), n_fft, hop) * M.window(n_fft, win_length)[None, :]
    k, n = np.arange(n_fft // 2 + 1)[:, None], np.arange(n_fft)[None, :]
    return fr @ np.exp(-2j * np.pi * ((k * n) % n_fft) / n_fft).T


def window_sumsquare(T: int, n_fft: int, hop: int, win_length: int) -> np.ndarray:
    """``[n_fft + hop (T - 1)]``: the sum of ``w^2`` over the frames that cover each sample of the padded signal."""
    wsq = M.window(n_fft, win_length) ** 2
    out = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        out[t * hop:t * hop + n_fft] += wsq
    return out


def istft(c: np.ndarray, n_fft: int, hop: int, win_length: int) -> np.ndarray:
    """``c [T, K]`` complex -> ``[hop (T - 1)]`` float64."""
    T = c.shape[0]
    fr = np.fft.irfft(c, n=n_fft, axis=1) * M.window(n_fft, win_length)[None, :]
    y = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
    wss = window_sumsquare(T, n_fft, hop, win_length)
    nz = wss > FLT_MIN
    y[nz] /= wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (T - 1)]


def nnls_step(fb: np.ndarray) -> float:
    return 1.0 / float(np.linalg.eigvalsh(fb @ fb.T)[-1])


def invert(logmel: np.ndarray, fb: np.ndarray, nnls_iters: int) -> np.ndarray:
    """``logmel [n_mels, T]`` -> ``S [T, K]`` float64."""
    fb = np.asarray(fb, dtype=np.float64)
    m = np.exp(np.clip(np.asarray(logmel, dtype=np.float64), LOG_LO, LOG_HI)).T
    x = np.maximum(m @ np.linalg.pinv(fb).T, 0.0)
    s = nnls_step(fb)
    for _ in range(nnls_iters):
        x = np.maximum(x - s * ((x @ fb.T - m) @ fb), 0.0)
    return x


def griffin_lim(S: np.ndarray, phi0: np.ndarray, n_iters, momentum: float, n_fft: int, hop: int, win_length: int) -> dict:
    """``S [T, K]``, ``phi0 [K, T]`` -> ``{n_iter: waveform}`` for every ``n_iter`` in ``n_iters`` (one run of the loop)."""
    want = sorted(set(int(n) for n in n_iters))
    out = {}
    c = S * np.exp(1j * np.asarray(phi0, dtype=np.float64).T)
    alpha = momentum / (1.0 + momentum)
    r_prev = None
    for i in range(want[-1] + 1):
        y = istft(c, n_fft, hop, win_length)
        if i in want:
            out[i] = y
        if i == want[-1]:
            break
        r = stft(y, n_fft, hop, win_length)
        a = r if r_prev is None else r - alpha * r_prev
        c = S * a / (np.abs(a) + FLT_MIN)
        r_prev = r
    return out


def spectral_convergence(y, S: np.ndarray, n_fft: int, hop: int, win_length: int) -> float:
    """``|| |stft(y)| - S ||_F / ||S||_F`` with the float64 STFT."""
    return float(np.linalg.norm(np.abs(stft(y, n_fft, hop, win_length)) - S) / np.linalg.norm(S))


# ---- fp32 on the library's tables -----------------------------------------------------------------------------------------
def stft_f32(y: np.ndarray, dft: np.ndarray, n_fft: int, hop: int):
    """``(re, im) [T, K]`` float32: ``im`` is minus the sine sum, as the device negates it."""
    fr = M.frames(np.asarray(y, dtype=np.float32), n_fft, hop)
    return fr @ dft[0].T, -(fr @ dft[1].T)


def istft_f32(re: np.ndarray, im: np.ndarray, idft: np.ndarray, wsq: np.ndarray, n_fft: int, hop: int) -> np.ndarray:
    T = re.shape[0]
    fr = re @ idft[0] + im @ idft[1]
    assert fr.dtype == np.float32
    y = np.zeros(n_fft + hop * (T - 1), dtype=np.float32)
    wss = np.zeros_like(y)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
        wss[t * hop:t * hop + n_fft] += wsq
    nz = wss > np.float32(FLT_MIN)
    y[nz] /= wss[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (T - 1)]


def invert_f32(logmel: np.ndarray, fb: np.ndarray, P: np.ndarray, step: float, nnls_iters: int) -> np.ndarray:
    """``S [T, K]`` float32 from the designed ``fb [n_mels, K]``, ``P = pinv(fb) [K, n_mels]`` and the step (all fp32)."""
    assert fb.dtype == np.float32 and P.dtype == np.float32
    m = np.exp(np.clip(np.asarray(logmel, dtype=np.float32).astype(np.float64), LOG_LO, LOG_HI)).astype(np.float32).T
    x = np.maximum(m @ P.T, np.float32(0))
    s = np.float32(step)
    for _ in range(nnls_iters):
        x = np.maximum(x - s * ((x @ fb.T - m) @ fb), np.float32(0))
    assert x.dtype == np.float32
    return x


def griffin_lim_f32(S: np.ndarray, phi0: np.ndarray, n_iters, momentum: float, tables: dict, n_fft: int, hop: int) -> dict:
    assert S.dtype == np.float32
    want = sorted(set(int(n) for n in n_iters))
    out = {}
    phi = np.asarray(phi0, dtype=np.float64).T
    re, im = S * np.cos(phi).astype(np.float32), S * np.sin(phi).astype(np.float32)
    alpha = np.float32(momentum / (1.0 + momentum))
    tiny = np.float32(FLT_MIN)
    pr = pi = None
    for i in range(want[-1] + 1):
        y = istft_f32(re, im, tables["idft"], tables["wsq"], n_fft, hop)
        if i in want:
            out[i] = y
        if i == want[-1]:
            break
        rr, ri = stft_f32(y, tables["dft"], n_fft, hop)
        ar, ai = (rr, ri) if pr is None else (rr - alpha * pr, ri - alpha * pi)
        den = np.sqrt(ar * ar + ai * ai) + tiny
        re, im = S * ar / den, S * ai / den
        assert re.dtype == np.float32
        pr, pi = rr, ri
    return out
