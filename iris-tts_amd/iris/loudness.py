"""ITU-R BS.1770-4 integrated loudness per item of a ragged batch, and the gain that brings each item to a target, on the device
(``iris_loudness_*``, csrc/loudness.h).  pyloudnorm cannot be imported here, so the contract is the rules below, held by two
float64 numpy restatements (``tests/loudness_restatement.py``): the plain loop, and the same in the kernels' own structure.

With ``step = sample_rate // 10`` and item b owning ``L_b`` samples, everything in fp64:

    K-weighting: a high shelf, then a high pass, derived for ``sample_rate`` with ``K = tan(pi f0 / fs)`` as libebur128 and
        pyloudnorm derive them; state 0 at sample 0 of every item
    block j covers filtered samples ``[j step, j step + 4 step)``; ``J_b = (L_b - 4 step) // step + 1`` (0 below ``4 step``)
    ``z_j`` the block's mean square; absolute gate ``z_j > 10 ** ((-70 + 0.691) / 10)``
    relative gate ``z_j > 0.1 * mean(z over the absolutely gated blocks)``                                  (both strict)
    ``ms_b`` = mean of ``z_j`` over the blocks passing both, 0 if none; loudness ``-0.691 + 10 log10(ms_b)``
    ``g_b = sqrt(10 ** ((target + 0.691) / 10) / ms_b)``, at most ``10 ** (max_gain_db / 20)`` and, with a ``peak_ceiling``,
        at most ``peak_ceiling / max|y_b|``; ``ms_b == 0`` (too short, or nothing above the absolute gate): ``g_b = 1``
    ``out[b, n] = y[b, n] * float32(g_b)`` for ``n < L_b``, 0 behind

The device never takes a logarithm.  A call is 4 launches on the current stream (3 to measure); the host never reads a length,
an item's result is that of its batch-of-one call, and two calls agree bit for bit.

``MelToWavePipeline(..., loudness=LoudnessNormalizer(...))`` levels every sentence behind the denoiser and the stretch and in
front of the join and the output stage.  ``peak_ceiling`` guards the sample peak by turning the whole item down; a true-peak
(oversampled) ceiling that leaves the item at its target is the stage behind this one, ``iris.limiter.Limiter``
(``MelToWavePipeline(..., loudness=LoudnessNormalizer(peak_ceiling=None), limiter=Limiter(...))``).  Not built: a pooled gain over
the whole batch, short-term / momentary loudness or loudness range, and a chunked form -- the measure is the whole item's.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _take_buffers

SEG, CHUNK_SEGS = 64, 128                       # csrc/loudness.h: kSeg, kChunkSegs


class LoudnessNormalizer(_DeviceStage):
    """Loudness measurement and gain with fixed parameters, resident on one GPU (``device``, or the current one); the handle --
    it owns the filter design -- is built on first use.  ``target_lufs``: the integrated loudness every item is brought to;
    ``max_gain_db``: a cap on the boost; ``peak_ceiling``: None, or the sample peak in (0, 1] no item may exceed afterwards."""

    _abi_name = "loudness"

    def __init__(self, sample_rate: int = 22050, target_lufs: float = -23.0, max_gain_db: float = 30.0,
                 peak_ceiling: Optional[float] = None, device: Optional[torch.device] = None):
        super().__init__(device)
        if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate:
            raise ValueError(f"sample_rate must be an integer, got {sample_rate!r}")
        if peak_ceiling is not None and not 0.0 < float(peak_ceiling) <= 1.0:
            raise ValueError(f"peak_ceiling must be None or an amplitude in (0, 1], got {peak_ceiling!r}")
        self.sample_rate = int(sample_rate)
        self.target_lufs, self.max_gain_db = float(target_lufs), float(max_gain_db)
        self.peak_ceiling = None if peak_ceiling is None else float(peak_ceiling)
        self.workspace_bytes(0, 0)                              # the library's own refusals, before any device work

    def get_config(self) -> dict:
        return {"sample_rate": self.sample_rate, "target_lufs": self.target_lufs, "max_gain_db": self.max_gain_db,
                "peak_ceiling": self.peak_ceiling}

    def native_config(self) -> "_native.LoudnessConfig":
        return _native.LoudnessConfig(self.sample_rate, self.target_lufs, self.max_gain_db,
                                      0.0 if self.peak_ceiling is None else self.peak_ceiling)

    # -- host-only queries -------------------------------------------------------------------
    def design(self) -> np.ndarray:
        """The handle's table of 144 doubles (include/iris_hifigan.h): both biquads, the thresholds, the matrix powers."""
        out = np.zeros(_native.LOUDNESS_DESIGN_DOUBLES, dtype=np.float64)
        cfg = self.native_config()
        _native.check("iris_loudness_design", _native.load().iris_loudness_design(
            ctypes.byref(cfg), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size))
        return out

    def launch_count(self, B: int, L: int, measure_only: bool = False) -> int:
        """Kernel launches of one call: 4, or 3 to measure (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L, bool(measure_only))

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def _workspace_layout(self, B: int, L: int):
        """``({buffer: (offset, shape, dtype)}, words)``: ``LdWorkspace`` (csrc/iris_loudness.hip) restated, offsets in 4-byte
        words (a double is two).  Host only."""
        segs = -(-L // (SEG * CHUNK_SEGS)) * CHUNK_SEGS
        hop_cap = L // (self.sample_rate // 10) + 1
        bufs = {"ends": ((B, segs, 4), torch.float64), "parts": ((B, segs, 2), torch.float64),
                "hops": ((B, hop_cap), torch.float64), "seg_peak": ((B, segs), torch.float32)}
        layout, words = _take_buffers((name, int(np.prod(shape)) * (2 if dtype == torch.float64 else 1))
                                      for name, (shape, dtype) in bufs.items())
        return {name: (layout[name][0], *bufs[name]) for name in bufs}, words

    def _read_buffers(self, B: int, L: int) -> dict:
        """Test-only: copies of the workspace's buffers as the last call of shape (B, L) left them (only what belongs to an
        item's own samples was written)."""
        layout, _ = self._workspace_layout(B, L)
        out = {}
        for name, (off, shape, dtype) in layout.items():
            n = int(np.prod(shape)) * (2 if dtype == torch.float64 else 1)
            out[name] = self._workspace[4 * off:4 * (off + n)].view(dtype).view(shape).clone()
        return out

    # -- the calls ---------------------------------------------------------------------------
    def normalize_device(self, wav, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``wav [B, L]`` fp32, host or device -> ``(out [B, L] fp32, stats [B, 2] float64)`` on the device: item b scaled by
        ``float32(stats[b, 1])`` and 0 behind its own samples; ``stats[b] = (ms_b, g_b)``.  Asynchronous on the current stream,
        4 launches, nothing synchronises; two calls agree bit for bit.

        ``lengths`` (a host sequence of integers or an integer tensor ``[B]``, which the host never reads) and ``row_scale``:
        item b owns ``min(L, lengths[b] * row_scale)`` samples -- mel frames and the vocoder's hop, or a stretch's ``counts``
        and 1 -- and nothing past them is read.  The same ``lengths`` and ``row_scale`` describe ``out`` to the next stage."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        out = torch.empty((B, L), dtype=torch.float32, device=self._device)          # the stage stores every element itself
        stats = torch.empty((B, 2), dtype=torch.float64, device=self._device)
        if B == 0 or L == 0:
            if B:
                stats[:, 0], stats[:, 1] = 0.0, 1.0
            return out, stats
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_loudness_normalize_ragged", lib.iris_loudness_normalize_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(out), _ptr(stats), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, stats

    def measure_device(self, wav, lengths=None, row_scale: int = 1) -> torch.Tensor:
        """``stats [B, 2]`` float64 of ``normalize_device`` alone: the same first 3 launches, and no sample is stored."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        stats = torch.empty((B, 2), dtype=torch.float64, device=self._device)
        if B == 0 or L == 0:
            if B:
                stats[:, 0], stats[:, 1] = 0.0, 1.0
            return stats
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_loudness_measure_ragged", lib.iris_loudness_measure_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(stats), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return stats

    @staticmethod
    def loudness_lufs(stats) -> np.ndarray:
        """``stats [B, 2]`` (device or host) -> the items' integrated loudness in LUFS, float64 on the host: ``-0.691 + 10
        log10(ms_b)``, and ``-inf`` for an item with ``ms_b == 0``.  This is a read-back."""
        ms = stats[:, 0].detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats, dtype=np.float64)[:, 0]
        with np.errstate(divide="ignore"):
            return -0.691 + 10.0 * np.log10(ms)
