"""Sample-rate conversion of the vocoder's waveform on the device (``iris_resampler_*``, csrc/resample.h).

The generator produces 22 050 Hz and the reference never resamples: it only labels the WAV (``--sample_rate``).  A caller who
wants 8 / 16 / 44.1 / 48 kHz gets it here without taking the fp32 waveform to the host: a polyphase Kaiser-windowed sinc
filter runs as one further launch behind conv_post and stores fp32, 16-bit PCM, or peak-normalised PCM.

The filter is defined once, in the library (``include/iris_hifigan.h``): with ``g = gcd(rate_in, rate_out)``,
``up = rate_out / g``, ``down = rate_in / g``, ``s = min(1, up / down)``, ``Hw = ceil(zeros / s)``, ``taps = 2 * Hw``, output
``n`` (utterance-global) is the chain over ascending ``j`` of ``acc = fmaf(x[i0 - Hw + 1 + j], bank[p][j], acc)`` with
``i0 = floor(n * down / up)``, ``p = (n * down) mod up``, and ``x`` outside the item's own samples reading as 0.
``design_bank`` fetches the bank from the library's host-only function (no GPU needed), ``resample_host`` restates the
chain in numpy with an exact fused multiply-add, and ``Resampler`` runs the device kernel; the two agree bit for bit.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native

DEFAULT_RATE_IN = 22050


def design_bank(rate_out: int, rate_in: int = DEFAULT_RATE_IN, zeros: Optional[int] = None, beta: Optional[float] = None,
                rolloff: Optional[float] = None) -> Tuple[np.ndarray, int, int]:
    """``(bank, up, down)``: the fp32 coefficient bank ``[up, taps]`` exactly as the device multiplies by it, from the
    library's host-only ``iris_resampler_design``.  ``None`` takes a parameter's default (16, 9.0, 0.945)."""
    lib = _native.load()
    args = (int(rate_in), int(rate_out), 0 if zeros is None else int(zeros),
            ctypes.c_double(0.0 if beta is None else float(beta)), ctypes.c_double(0.0 if rolloff is None else float(rolloff)))
    up, down, taps = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _native.check("iris_resampler_design", lib.iris_resampler_design(
        *args, ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps), None, 0))
    bank = np.empty((up.value, taps.value), dtype=np.float32)
    _native.check("iris_resampler_design", lib.iris_resampler_design(
        *args, ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps),
        bank.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_uint64(bank.size)))
    return bank, int(up.value), int(down.value)


def _ceil_div(a: int, b: int) -> int:
    return -((-a) // b)


def out_range(up: int, down: int, origin: int, L: int) -> Tuple[int, int]:
    """``(n_lo, n_count)`` of a window of ``L`` input samples whose first one has the global index ``origin``: the outputs
    ``n`` with ``origin <= n * down / up < origin + L`` (Python integers: nothing wraps)."""
    n_lo = _ceil_div(int(origin) * up, down)
    return n_lo, _ceil_div((int(origin) + int(L)) * up, down) - n_lo


def fmaf32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """Elementwise float32 ``fmaf(a, b, c)``: ``a * b + c`` with ONE rounding, for finite values.

    The product of two float32 is exact in float64 (48 significant bits).  Its sum with ``c`` is formed in float64 rounded
    to ODD -- the truncated sum with the last bit set when anything was lost (the lost part is known exactly from the
    two-sum) -- and rounding that to float32 is then the correct single rounding, because float64 keeps more than two
    bits beyond float32 (a plain float64 add would round twice).  The tests hold it to libm's ``fmaf``."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                      # exact: s + err == p + c
    m = s.view(np.int64).copy()                          # sign-magnitude: +-1 on the integer moves |s| by one ulp
    inexact = err != 0.0
    away = inexact & ((err > 0.0) == (s > 0.0))          # the exact sum lies beyond s (in magnitude): truncation is s itself
    m = np.where(inexact & ~away, m - 1, m)              # otherwise it is the float64 just inside s
    m = np.where(inexact, m | 1, m)
    return m.view(np.float64).astype(np.float32)


def resample_host(wav, bank: np.ndarray, up: int, down: int, lengths=None, origin: int = 0) -> np.ndarray:
    """The exact numpy restatement of the device stage: ``wav [B, L]`` (or ``[L]``) fp32 -> ``[B, n_count]`` fp32, every
    output the ascending fmaf chain of the module docstring over ``bank`` (from ``design_bank``).  ``lengths``: the own
    input samples of each item (the device's ``lengths * row_scale``); samples past them are never read and the item's
    outputs past its own count are 0.  Test infrastructure: small inputs only."""
    w = np.asarray(wav, dtype=np.float32)
    squeeze = w.ndim == 1
    if squeeze:
        w = w[None]
    B, L = w.shape
    bank = np.asarray(bank, dtype=np.float32)
    taps = bank.shape[1]
    hw = taps // 2
    origin = int(origin)
    n_lo, n_count = out_range(up, down, origin, L)
    out = np.zeros((B, n_count), dtype=np.float32)
    own = np.full(B, L, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, L)
    for b in range(B):
        Lb = int(own[b])
        cnt = min(n_count, out_range(up, down, origin, Lb)[1])
        if cnt <= 0:
            continue
        q = (np.arange(cnt, dtype=np.int64) + n_lo) * down
        first = q // up - hw + 1 - origin                    # item index of x[i0 - Hw + 1]
        rows = bank[q % up]                                  # [cnt, taps]
        acc = np.zeros(cnt, dtype=np.float32)
        for j in range(taps):
            idx = first + j
            ok = (idx >= 0) & (idx < Lb)
            x = np.where(ok, w[b, np.clip(idx, 0, max(Lb - 1, 0))], np.float32(0.0)).astype(np.float32)
            acc = fmaf32(x, rows[:, j], acc)
        out[b, :cnt] = acc
    return out[0] if squeeze else out


class Resampler:
    """One resampling filter ``rate_in -> rate_out`` resident on one GPU (``iris_resampler_create``).

    ``forward`` is asynchronous on the current stream of the device and performs no native allocation; the tensors it
    returns come from torch's caching allocator."""

    def __init__(self, rate_out: int, rate_in: int = DEFAULT_RATE_IN, device=None, zeros: Optional[int] = None,
                 beta: Optional[float] = None, rolloff: Optional[float] = None):
        import torch

        from ._engine import require_gpu

        self.lib = _native.load()
        self.device = torch.device(device) if device is not None else require_gpu()
        if self.device.type != "cuda":
            raise RuntimeError(f"Resampler needs a HIP device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _native.check("iris_resampler_create", self.lib.iris_resampler_create(
                self.rate_in, self.rate_out, 0 if zeros is None else int(zeros),
                ctypes.c_double(0.0 if beta is None else float(beta)),
                ctypes.c_double(0.0 if rolloff is None else float(rolloff)), ctypes.byref(self._handle)))
        up, down, taps, hw = (ctypes.c_int32() for _ in range(4))
        _native.check("iris_resampler_info", self.lib.iris_resampler_info(
            self._handle, ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps), ctypes.byref(hw)))
        self.up, self.down, self.taps, self.half_width = int(up.value), int(down.value), int(taps.value), int(hw.value)

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self.lib.iris_resampler_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def out_range(self, origin: int, L: int) -> Tuple[int, int]:
        """``(n_lo, n_count)``: the global outputs a window of ``L`` samples at ``origin`` produces (``iris_resampler_out_range``)."""
        n_lo, n_count = ctypes.c_int64(), ctypes.c_int64()
        _native.check("iris_resampler_out_range", self.lib.iris_resampler_out_range(
            self._handle, ctypes.c_int64(int(origin)), ctypes.c_int64(int(L)), ctypes.byref(n_lo), ctypes.byref(n_count)))
        return int(n_lo.value), int(n_count.value)

    def forward(self, wav, lengths=None, row_scale: int = 1, origin: int = 0, pcm16: bool = False, normalize: bool = False,
                peak_target: float = 0.95):
        """``wav``: fp32 device tensor ``[B, L]`` whose first column has the utterance-global index ``origin`` ->
        ``[B, n_count]`` (``out_range(origin, L)``): fp32, or int16 with ``pcm16=True`` (bit for bit
        ``pcm16_from_float`` of the fp32 result).  ``normalize=True`` (with pcm16) scales every item to ``peak_target`` at
        its own peak first and returns ``(pcm, peaks)``, ``peaks`` the fp32 tensor [B] of the items' max |out|.
        ``lengths`` (a sequence or an integer tensor [B]) and ``row_scale``: item b owns
        ``min(L, lengths[b] * row_scale)`` samples; the rest is never read and its outputs past its own count are 0."""
        import torch

        if normalize and not pcm16:
            raise ValueError("normalize=True goes with pcm16=True")
        if normalize and not 0.0 < float(peak_target) <= 1.0:
            raise ValueError(f"peak_target must lie in (0, 1], got {peak_target}")
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"expected an fp32 waveform [B, L], got {wav.dtype} {tuple(wav.shape)}")
        if wav.device != self.device:
            raise ValueError(f"wav is on {wav.device}, resampler on {self.device}")
        if int(origin) < 0 or int(row_scale) < 1:
            raise ValueError("origin >= 0 and row_scale >= 1 are required")
        wav = wav.contiguous()
        B, L = wav.shape
        lengths_dev = None
        if lengths is not None:
            if isinstance(lengths, torch.Tensor) and lengths.device == self.device and lengths.dtype == torch.int32:
                lengths_dev = lengths.contiguous()
            else:
                host = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
                if host.size and not np.issubdtype(host.dtype, np.integer):
                    raise ValueError(f"lengths must be integers, got {host.dtype}")
                lengths_dev = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(self.device)
            if tuple(lengths_dev.shape) != (B,):
                raise ValueError(f"lengths must have shape [{B}], got {list(lengths_dev.shape)}")
        n_count = self.out_range(origin, L)[1] if B and L else 0
        out = torch.empty((B, n_count), dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        f32 = torch.empty((B, n_count), dtype=torch.float32, device=self.device) if normalize else None
        peaks = torch.zeros((B,), dtype=torch.float32, device=self.device) if normalize else None
        if B and L:
            stream = torch.cuda.current_stream(self.device).cuda_stream

            def ptr(t):
                return ctypes.c_void_p(t.data_ptr() if t is not None else None)

            # (an empty output has no address; the library launches nothing for it)
            out_f32, out_pcm = (f32, out) if normalize else ((None, out) if pcm16 else (out, None))
            if n_count:
                _native.check("iris_resampler_forward", self.lib.iris_resampler_forward(
                    self._handle, ctypes.c_void_p(wav.data_ptr()), B, L, ptr(lengths_dev), int(row_scale),
                    ctypes.c_int64(int(origin)), ptr(out_f32), ptr(out_pcm), ptr(peaks), int(bool(normalize)),
                    ctypes.c_float(float(peak_target)), ctypes.c_void_p(stream)))
        return (out, peaks) if normalize else out

    __call__ = forward


_shared: dict = {}


def shared_resampler(rate_out: int, device, rate_in: int = DEFAULT_RATE_IN) -> Resampler:
    """The default filter ``rate_in -> rate_out`` on ``device``, built on first use and kept (the drop-in entry points
    ``infer_hifigan(..., sample_rate_out=)`` and ``HiFiGANVocoder.infer(..., sample_rate_out=)`` have no object to own one)."""
    key = (int(rate_in), int(rate_out), str(device))
    rs = _shared.get(key)
    if rs is None:
        rs = _shared[key] = Resampler(rate_out, rate_in=rate_in, device=device)
    return rs
