"""A look-ahead true-peak limiter per item of a ragged batch of waveforms, on the device (``iris_limiter_*``, csrc/limiter.h): the
stage behind ``iris.loudness`` that holds a ceiling without turning the whole sentence down.  The contract is the rules below and
their numpy restatement with the kernel's own operations (``tests/limiter_restatement.py``: ``device_f32``), bit for bit.

With ceiling ``c``, lookahead ``A`` samples and item b owning ``L_b`` samples (``x = 0`` outside them), everything in fp32, nothing
contracted but the ``fmaf`` named here, the one division in fp64:

    ``u[n, q]``, q = 1, 2, 3: the three points between sample n and n + 1, a 12-tap ``fmaf`` chain over ``x[n - 5 .. n + 6]`` with
        the Kaiser-windowed sinc of ``iris.resample`` for 1 : 4 (6 zeros, its default beta and rolloff)
    ``p[n] = max(|x[n]|, |u[n-1, 1..3]|, |u[n, 1..3]|)``; the item's true peak ``tp_b = max p``
    ``r[n] = c / p[n]`` where ``p[n] > c``, else 1 (and 1 outside the item); ``m[n] = min r[n - A .. n + A]``
    ``g[n] = 1 - sum_j (1 - m[n + j]) w[j]``, ``w`` a Hann shape over ``-A .. A`` normalised to sum 1 and rounded to fp32 upward,
        so that the table never sums to less: an ``fmaf`` chain, j ascending
    ``out[b, n] = min(max(x[n] * g[n], -c), c)`` for ``n < L_b``, 0 behind

Every ``m[n + j]`` of the sum covers sample n, so ``g[n] <= r[n]`` but for rounding, which the clamp absorbs: ``|out| <= c``
always, and an item whose true peak stays under ``c`` comes out bit for bit as it went in.  A call is 2 launches on the current
stream -- one fused kernel over tiles of ``TILE`` samples with a halo of ``2A + 7`` in LDS, and the reduction of the tiles'
statistics; the host never reads a length, an item's result is that of its batch-of-one call, and two calls agree bit for bit.

``MelToWavePipeline(..., limiter=Limiter(...))`` runs it behind ``loudness=`` and in front of the join and the output stage.  Not
built: a chunked form (the reach is ``2A + 7`` samples per side, so one can follow), separate attack and release times (they need
a recursion), stereo linking and dither.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream

TILE = 2048                                     # csrc/limiter.h: kTile, the output samples of a block
MAX_LOOKAHEAD = 256                             # csrc/limiter.h: kMaxLookahead


class Limiter(_DeviceStage):
    """A limiter with fixed parameters, resident on one GPU (``device``, or the current one); the handle -- it owns the design
    table -- is built on first use.  ``ceiling_dbtp``: the true-peak ceiling in dB re full scale, at most 0; ``lookahead_ms``: how
    far ahead of a peak the gain starts to fall (and how far behind it has recovered), ``round(ms * rate / 1000)`` samples,
    1 .. 256."""

    _abi_name = "limiter"

    def __init__(self, sample_rate: int = 22050, ceiling_dbtp: float = -1.0, lookahead_ms: float = 1.5,
                 device: Optional[torch.device] = None):
        super().__init__(device)
        if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(sample_rate) < 1:
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        if not float(ceiling_dbtp) <= 0.0:                      # False for NaN too
            raise ValueError(f"ceiling_dbtp must be at most 0 dBTP, got {ceiling_dbtp!r}")
        if not 0.0 < float(lookahead_ms) < float("inf"):
            raise ValueError(f"lookahead_ms must be a finite time above 0, got {lookahead_ms!r}")
        self.sample_rate = int(sample_rate)
        self.ceiling_dbtp, self.lookahead_ms = float(ceiling_dbtp), float(lookahead_ms)
        self.ceiling = float(np.float32(10.0 ** (self.ceiling_dbtp / 20.0)))
        self.lookahead = int(round(self.lookahead_ms * self.sample_rate / 1000.0))
        if not 1 <= self.lookahead <= MAX_LOOKAHEAD:
            raise ValueError(f"lookahead_ms = {lookahead_ms!r} at {self.sample_rate} Hz is {self.lookahead} samples; 1 .. "
                             f"{MAX_LOOKAHEAD} are built")
        self.workspace_bytes(0, 0)                              # the library's own refusals, before any device work

    def get_config(self) -> dict:
        return {"sample_rate": self.sample_rate, "ceiling_dbtp": self.ceiling_dbtp, "lookahead_ms": self.lookahead_ms}

    def native_config(self) -> "_native.LimiterConfig":
        return _native.LimiterConfig(self.ceiling, self.lookahead)

    # -- host-only queries -------------------------------------------------------------------
    def design(self) -> np.ndarray:
        """The handle's table of ``36 + 2A + 1`` floats (include/iris_hifigan.h): ``bank[1..3][0..11]``, then ``w[-A .. A]``."""
        out = np.zeros(_native.LIMITER_BANK_FLOATS + 2 * self.lookahead + 1, dtype=np.float32)
        cfg = self.native_config()
        _native.check("iris_limiter_design", _native.load().iris_limiter_design(
            ctypes.byref(cfg), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size))
        return out

    def launch_count(self, B: int, L: int, measure_only: bool = False) -> int:
        """Kernel launches of one call: 2, to limit or to measure (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L, bool(measure_only))

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def _empty_stats(self, B: int) -> torch.Tensor:
        stats = torch.empty((B, 2), dtype=torch.float32, device=self._device)
        if B:
            stats[:, 0], stats[:, 1] = 0.0, 1.0
        return stats

    # -- the calls ---------------------------------------------------------------------------
    def limit_device(self, wav, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``wav [B, L]`` fp32, host or device -> ``(out [B, L] fp32, stats [B, 2] fp32)`` on the device: item b held under the
        ceiling and 0 behind its own samples; ``stats[b] = (true peak of the input, smallest gain applied)``.  Asynchronous on
        the current stream, 2 launches, nothing synchronises; two calls agree bit for bit.

        ``lengths`` (a host sequence of integers or an integer tensor ``[B]``, which the host never reads) and ``row_scale``:
        item b owns ``min(L, lengths[b] * row_scale)`` samples, as in ``LoudnessNormalizer.normalize_device``, and nothing past
        them is read.  The same ``lengths`` and ``row_scale`` describe ``out`` to the next stage."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        out = torch.empty((B, L), dtype=torch.float32, device=self._device)          # the stage stores every element itself
        if B == 0 or L == 0:
            return out, self._empty_stats(B)
        stats = torch.empty((B, 2), dtype=torch.float32, device=self._device)
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_limiter_forward_ragged", lib.iris_limiter_forward_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(out), _ptr(stats), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, stats

    def true_peak_device(self, wav, lengths=None, row_scale: int = 1) -> torch.Tensor:
        """``stats [B, 2]`` fp32 of ``limit_device`` alone: the same 2 launches, and no sample is stored."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        if B == 0 or L == 0:
            return self._empty_stats(B)
        stats = torch.empty((B, 2), dtype=torch.float32, device=self._device)
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_limiter_measure_ragged", lib.iris_limiter_measure_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(stats), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return stats

    @staticmethod
    def true_peak_dbtp(stats) -> np.ndarray:
        """``stats [B, 2]`` (device or host) -> the items' true peak in dBTP, float64 on the host: ``20 log10(tp_b)``, and
        ``-inf`` for a silent or empty item.  This is a read-back."""
        tp = stats[:, 0].detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)[:, 0]
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(tp.astype(np.float64))
