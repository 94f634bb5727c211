"""numpy restatement of the arithmetic ``iris.time_stretch`` commits to (csrc/time_stretch.h): librosa 0.11's
``effects.time_stretch`` -- ``stft``, ``phase_vocoder``, ``istft(length=)`` -- on the Griffin-Lim stage's transforms
(tests/griffin_lim_restatement.py; window and frames of tests/mel_restatement.py).  librosa cannot be imported here, so this
is written from its rules; ``librosa_loop`` is its ``phase_vocoder`` loop transcribed line by line, in radians.

    T_out = len(np.arange(0, T, rate));  step_t = t * rate;  i = floor(step_t);  alpha = step_t - i;  a column >= T is 0
    mag = (1 - alpha) |c[i]| + alpha |c[i + 1]|
    dphi = angle(c[i + 1]) - angle(c[i]) - adv;  dphi -= round(dphi)          in turns;  adv_k = (k hop mod n_fft) / n_fft
    acc[0] = angle(c[0]);  acc[t + 1] = acc[t] + adv + dphi;  out_c = mag (cos, sin)(2 pi acc)
    n_out = round(L / rate);  out = istft(out_c, length=n_out)

``dtype=np.float64`` runs it with the FFT and a float64 accumulator in turns.  ``dtype=np.float32`` runs the steps the device
runs -- fp32 products and sums on the library's own tables, the phase in 32-bit fixed-point turns (``fixed``, ``scan_fixed``)
-- in numpy's order (the siblings' ``e32`` scheme).  Spectra are ``[T, K]``.
"""
from __future__ import annotations

import numpy as np

import griffin_lim_restatement as G
import mel_restatement as M

from iris.resample import fmaf32

MASK = (1 << 32) - 1
INV_2PI32 = np.float32(0.15915494309189535)


def out_frames(T: int, rate: float) -> int:
    return len(np.arange(0, T, rate, dtype=np.float64))


def out_samples(L: int, rate: float) -> int:
    return int(round(L / rate))                                    # float64 quotient, half to even


def advance(n_fft: int, hop: int) -> np.ndarray:
    """``(k hop) mod n_fft`` per bin, as integers: ``adv_k`` is this over ``n_fft`` turns."""
    return (np.arange(n_fft // 2 + 1, dtype=np.int64) * hop) % n_fft


def advance_fixed(n_fft: int, hop: int) -> np.ndarray:
    return (advance(n_fft, hop) << 32) // n_fft


def fixed(x32: np.ndarray) -> np.ndarray:
    """fp32 turns -> uint32 fixed-point turns, held in int64: ``rint(x * 2^32) mod 2^32`` (the product is exact)."""
    assert x32.dtype == np.float32
    return np.rint(x32.astype(np.float64) * 4294967296.0).astype(np.int64) & MASK


def unfixed(a: np.ndarray) -> np.ndarray:
    """uint32 fixed-point turns -> fp32 turns in [-0.5, 0.5): the value as an int32, rounded to fp32, times 2^-32."""
    signed = np.where(a >= (1 << 31), a - (1 << 32), a)
    return signed.astype(np.float32) * np.float32(2.0 ** -32)


def scan_fixed(acc0: np.ndarray, inc: np.ndarray) -> np.ndarray:
    """``acc [T_out, K]``: the exclusive scan of ``inc`` along t from ``acc0``, modulo 2^32, the way the device's blocks run it:
    runs of ``ceil(T_out / 32)`` frames summed on their own, the run sums added in front, each run walked again."""
    To = inc.shape[0]
    acc = np.zeros_like(inc)
    if To == 0:
        return acc
    n = -(-To // 32)
    sums = [inc[r * n:(r + 1) * n].sum(axis=0) & MASK for r in range(32)]
    for r in range(32):
        a = acc0.copy()
        for q in range(r):
            a = (a + sums[q]) & MASK
        for t in range(r * n, min((r + 1) * n, To)):
            acc[t] = a
            a = (a + inc[t]) & MASK
    return acc


def positions(T: int, rate: float):
    """``(i [T_out] int, alpha [T_out] float64)``."""
    steps = np.arange(0, T, rate, dtype=np.float64)
    i = np.floor(steps)
    return i.astype(np.int64), steps - i


def middle(re: np.ndarray, im: np.ndarray, rate: float, n_fft: int, hop: int, dtype=np.float64) -> dict:
    """Launches 2 and 3 on a spectrum ``(re, im) [T, K]``: ``mag``, ``out_re``, ``out_im`` ``[T_out, K]`` of dtype, and in fp32
    ``inc`` and ``acc`` (int64 in [0, 2^32)).  float64 accepts fp32 inputs too (the device's own ``c``)."""
    T, K = re.shape
    idx, alpha = positions(T, rate)
    pad = np.zeros((2, K), dtype=dtype)
    re, im = np.concatenate([re.astype(dtype), pad]), np.concatenate([im.astype(dtype), pad])
    m = np.sqrt(re * re + im * im)
    r = advance(n_fft, hop)
    if dtype == np.float64:
        turn = np.arctan2(im, re) / (2.0 * np.pi)
        a = alpha[:, None]
        mag = (1.0 - a) * m[idx] + a * m[idx + 1]
        dphi = turn[idx + 1] - turn[idx] - (r / n_fft)[None, :]
        dphi = dphi - np.round(dphi)
        inc = (r / n_fft)[None, :] + dphi
        acc = turn[0][None, :] + np.concatenate([np.zeros((1, K)), np.cumsum(inc, axis=0)[:-1]])
        ang = 2.0 * np.pi * acc
        return {"mag": mag, "out_re": mag * np.cos(ang), "out_im": mag * np.sin(ang)}
    assert m.dtype == np.float32
    turn = np.arctan2(im, re) * INV_2PI32
    a = np.broadcast_to(alpha.astype(np.float32)[:, None], (len(idx), K))
    mag = fmaf32(a, m[idx + 1], (np.float32(1) - a) * m[idx])
    dphi = turn[idx + 1] - turn[idx] - (r.astype(np.float32) / np.float32(n_fft))[None, :]
    dphi = dphi - np.rint(dphi)
    assert dphi.dtype == np.float32
    inc = (advance_fixed(n_fft, hop)[None, :] + fixed(dphi)) & MASK
    acc = scan_fixed(fixed(turn[0]), inc)
    ang = np.float32(2.0 * np.pi) * unfixed(acc)
    assert ang.dtype == np.float32 and mag.dtype == np.float32
    return {"mag": mag, "out_re": mag * np.cos(ang), "out_im": mag * np.sin(ang), "inc": inc, "acc": acc}


def istft_length(cre: np.ndarray, cim: np.ndarray, n_out: int, n_fft: int, hop: int, win: int, tables=None) -> np.ndarray:
    """``istft(c, length=n_out)``: the overlap-add over the window-sum-square of the frames that exist, ``n_fft / 2`` samples
    trimmed in front only, then cropped or zero-padded to ``n_out``."""
    T = cre.shape[0]
    if cre.dtype == np.float64:
        fr = np.fft.irfft(cre + 1j * cim, n=n_fft, axis=1) * M.window(n_fft, win)[None, :]
        wsq = M.window(n_fft, win) ** 2
        tiny = G.FLT_MIN
    else:
        fr = cre @ tables["idft"][0] + cim @ tables["idft"][1]
        wsq = tables["wsq"]
        tiny = np.float32(G.FLT_MIN)
        assert fr.dtype == np.float32
    y = np.zeros(n_fft + hop * (T - 1), dtype=cre.dtype)
    wss = np.zeros_like(y)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
        wss[t * hop:t * hop + n_fft] += wsq
    nz = wss > tiny
    y[nz] /= wss[nz]
    y = y[n_fft // 2:]
    out = np.zeros(n_out, dtype=cre.dtype)
    n = min(n_out, len(y))
    out[:n] = y[:n]
    return out


def spectrum(y, n_fft: int, hop: int, win: int, dtype=np.float64, tables=None):
    """``(re, im) [T, K]`` of dtype; the imaginary parts of bins 0 and n_fft / 2 are exactly 0 (the device stores 0.f)."""
    if dtype == np.float64:
        a = G.stft(y, n_fft, hop, win)
        re, im = a.real.copy(), a.imag.copy()
    else:
        re, im = G.stft_f32(np.asarray(y, dtype=np.float32), tables["dft"], n_fft, hop)
    im[:, 0] = 0
    im[:, -1] = 0
    return re, im


def stretch(y, rate: float, n_fft: int, hop: int, win: int, dtype=np.float64, tables=None, taps: bool = False):
    """``y [L]`` (L a multiple of hop) -> ``out [round(L / rate)]`` of dtype; with ``taps`` also the dict of ``middle`` plus ``re``, ``im``."""
    assert len(y) % hop == 0
    if len(y) == 0:
        return (np.zeros(0, dtype=dtype), {}) if taps else np.zeros(0, dtype=dtype)
    re, im = spectrum(y, n_fft, hop, win, dtype, tables)
    mid = middle(re, im, rate, n_fft, hop, dtype)
    out = istft_length(mid["out_re"], mid["out_im"], out_samples(len(y), rate), n_fft, hop, win, tables)
    assert out.dtype == dtype
    return (out, {**mid, "re": re, "im": im}) if taps else out


def librosa_loop(D: np.ndarray, rate: float, n_fft: int, hop: int) -> np.ndarray:
    """librosa 0.11 ``phase_vocoder``, transcribed: ``D [K, T]`` complex -> ``[K, T_out]`` complex.  Radians, an unwrapped float64
    accumulator, ``np.mod(step, 1.0)``, two zero columns behind D."""
    time_steps = np.arange(0, D.shape[-1], rate, dtype=np.float64)
    d_stretch = np.zeros(D.shape[:-1] + (len(time_steps),), dtype=D.dtype)
    phi_advance = hop * np.linspace(0, np.pi, 1 + n_fft // 2)      # hop_length * fft_frequencies(sr=2 pi, n_fft)
    phase_acc = np.angle(D[..., 0])
    D = np.pad(D, [(0, 0), (0, 2)], mode="constant")
    for t, step in enumerate(time_steps):
        columns = D[..., int(step):int(step + 2)]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(columns[..., 0]) + alpha * np.abs(columns[..., 1])
        d_stretch[..., t] = mag * (np.cos(phase_acc) + 1j * np.sin(phase_acc))
        dphase = np.angle(columns[..., 1]) - np.angle(columns[..., 0]) - phi_advance
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc += phi_advance + dphase
    return d_stretch


def pitch_host(y: np.ndarray, ratio, n_fft: int, hop: int, win: int, resample) -> np.ndarray:
    """The pitch path's structure on the host, float64 stretch: stretch by ``q / p``, ``resample(x)`` by ``q / p``, crop or pad."""
    x = stretch(y, ratio.denominator / ratio.numerator, n_fft, hop, win)
    z = resample(x)
    out = np.zeros(len(y), dtype=z.dtype)
    n = min(len(y), len(z))
    out[:n] = z[:n]
    return out
