"""numpy restatement of the reference's ``compute_mel_spectrogram`` (src/iris/data.py:25-67), i.e. of librosa 0.11.0's
``melspectrogram(y, sr, n_fft, hop_length, win_length, n_mels, fmin, fmax, power=1.0)`` with that version's defaults, then
``log(max(mel, 1e-5))``.  librosa cannot be imported here, so this is written from its rules, not run against it ("parity
unpinned"); it is independent of ``iris.mel``'s device path and of the library's design function.

Conventions:
  * framing: ``center=True``, ``pad_mode="constant"`` -- ``n_fft // 2`` ZEROS on each side (not reflection); ``n`` samples
    give ``1 + n // hop`` frames; frame ``t`` covers samples ``[t * hop - n_fft / 2, t * hop + n_fft / 2)``;
  * window: periodic Hann ``0.5 - 0.5 cos(2 pi n / win)`` (``scipy.signal.get_window("hann", win, fftbins=True)``), padded to
    ``n_fft`` with ``(n_fft - win) // 2`` zeros in front and the rest behind (``librosa.util.pad_center``);
  * magnitude: ``|np.fft.rfft(frame * window)|`` over ``n_fft / 2 + 1`` bins, not squared;
  * filterbank: ``librosa.filters.mel(htk=False, norm="slaney")`` -- Slaney's scale (200/3 Hz per mel below 1000 Hz,
    logarithmic above with step ``ln(6.4) / 27``), ``n_mels + 2`` edges from ``linspace`` in mel, triangles
    ``max(0, min(lower, upper))`` from the ramps ``mel_f[i] - fftfreq`` over ``diff(mel_f)``, each row scaled by
    ``2 / (mel_f[i + 2] - mel_f[i])``; ``fmax=None`` means ``sr / 2``.  Kept in float64 (librosa rounds it to float32).
    The linear part is written ``3 f / 200`` so that 1000 Hz is exactly 15 mel (librosa divides by the rounded ``200 / 3``
    and is one float64 ulp below; nothing downstream sees the difference).

``mel_np(audio, ...)`` is float64.  ``mel_np_f32(audio, dft, fb, ...)`` runs the same steps on fp32 arrays with fp32
products and sums, multiplying by the fp32 tables the device uploads (``MelFrontend.design()``), as matrix products instead
of an FFT -- the arithmetic the device does, in numpy's order.
"""
from __future__ import annotations

import numpy as np

CLIP = 1e-5


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    min_log_hz = 1000.0
    min_log_mel = 15.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, 3.0 * f / 200.0)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    min_log_hz = 1000.0
    min_log_mel = 15.0
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), 200.0 * m / 3.0)


def mel_edges(n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))


def filterbank(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax=None) -> np.ndarray:
    """``[n_mels, n_fft // 2 + 1]`` float64."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_edges(n_mels, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    weights = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0.0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return weights * enorm[:, None]


def window(n_fft: int, win_length: int) -> np.ndarray:
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    lpad = (n_fft - win_length) // 2
    return np.pad(w, (lpad, n_fft - win_length - lpad))


def n_frames(n: int, hop: int) -> int:
    return 1 + n // hop


def frames(audio: np.ndarray, n_fft: int, hop: int) -> np.ndarray:
    """``[1 + n // hop, n_fft]``: the explicitly built frames of the zero-padded signal."""
    y = np.pad(np.asarray(audio), (n_fft // 2, n_fft // 2))
    T = n_frames(len(audio), hop)
    return np.stack([y[t * hop: t * hop + n_fft] for t in range(T)])


def magnitudes(audio, n_fft: int = 1024, hop: int = 256, win_length: int = 1024) -> np.ndarray:
    """``[T, n_fft // 2 + 1]`` float64."""
    fr = frames(np.asarray(audio, dtype=np.float64), n_fft, hop) * window(n_fft, win_length)[None, :]
    return np.abs(np.fft.rfft(fr, axis=1))


def magnitudes_direct(audio, n_fft: int, hop: int, win_length: int) -> np.ndarray:
    """The same by the O(N^2) definition, with no FFT and no shared framing code: sample by sample."""
    x = np.asarray(audio, dtype=np.float64)
    w = window(n_fft, win_length)
    T = n_frames(len(x), hop)
    out = np.zeros((T, n_fft // 2 + 1))
    for t in range(T):
        for k in range(n_fft // 2 + 1):
            acc = 0j
            for n in range(n_fft):
                s = t * hop - n_fft // 2 + n
                if 0 <= s < len(x):
                    acc += x[s] * w[n] * np.exp(-2j * np.pi * k * n / n_fft)
            out[t, k] = abs(acc)
    return out


def mel_np(audio, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024, n_mels: int = 80,
           fmin: float = 0.0, fmax=8000.0) -> np.ndarray:
    """``[n_mels, T]`` float64."""
    mag = magnitudes(audio, n_fft, hop_length, win_length)
    mel = filterbank(sample_rate, n_fft, n_mels, fmin, fmax) @ mag.T
    return np.log(np.maximum(mel, CLIP))


def mel_np_f32(audio, dft: np.ndarray, fb: np.ndarray, n_fft: int = 1024, hop_length: int = 256) -> np.ndarray:
    """``[n_mels, T]`` float32 from fp32 samples and the fp32 design tables ``dft [2, bins, n_fft]``, ``fb [n_mels, bins]``."""
    assert dft.dtype == np.float32 and fb.dtype == np.float32
    fr = frames(np.asarray(audio, dtype=np.float32), n_fft, hop_length)
    re = fr @ dft[0].T
    im = fr @ dft[1].T
    mag = np.sqrt(re * re + im * im)
    assert mag.dtype == np.float32
    mel = fb @ mag.T
    return np.log(np.maximum(mel, np.float32(CLIP)))
