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

``MelToWavePipeline(..., limiter=Limiter(...))`` runs it behind ``loudness=`` and in front of the join and the output stage.

Streaming: ``out[n]`` reads ``x[n - R .. n + R]`` and nothing else, ``R = 2A + 7``, so the stage is chunked exactly.
``Limiter.open_session()`` takes the waveform piece by piece (``LimiterSession``: one ``forward_window`` per push, the same 2
launches -- one kernel body -- on a window of the utterance, with tiles over the samples the window settles) and its output equals
``limit_device`` of the whole bit for bit, ``R`` samples late; with ``pcm16=True`` the same kernel stores 16-bit PCM, bit for bit
``pcm16_on_device`` of those samples.  ``lim.chunked()`` (``ChunkedLimiter``) is the opt-in with which a pipeline's ``stream`` /
``session`` run it last of all.  How fast a window is has not been measured on a GPU.

Many sessions in one call: ``Limiter.forward_windows`` and ``iris.stream_group``.  Not built: separate attack and release times (they need a recursion), stereo linking and dither.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _wave
from ._window_session import _RangeSession

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

    # -- windows of an utterance -------------------------------------------------------------
    def window_range(self, origin: int, Lw: int, final: bool) -> Tuple[int, int]:
        """``(out_lo, out_count)``: the samples of an utterance that the window ``[origin, origin + Lw)`` settles -- those whose
        ``2A + 7`` samples on either side each lie inside the window or outside the utterance (``iris_limiter_window_range``: the
        finality rule, written down on the C side only).  ``final``: the window ends where the utterance ends; a window with
        ``origin == 0`` starts it.  Any ``origin >= 0`` and ``Lw >= 0``: there is no hop to respect.  Host only."""
        return self._window_range(origin, Lw, final)

    def window_workspace_bytes(self, B: int, Lw: int) -> int:
        return self._query("window_workspace_bytes", B, Lw)

    def window_launch_count(self, B: int, Lw: int, origin: int, final: bool) -> int:
        """Kernel launches of one ``forward_window``: 2, or 0 where the window settles nothing (a dry run on the host)."""
        return self._query("window_launch_count", B, Lw, origin, bool(final))

    def forward_window(self, wav, origin: int, final: bool, pcm16: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """``wav [B, Lw]`` fp32 = samples ``[origin, origin + Lw)`` of B utterances of one length -> ``(out [B, out_count], stats
        [B, 2])`` on the device: the samples ``window_range(origin, Lw, final)`` names, each bit for bit the sample ``limit_device``
        of the whole utterance returns there -- or, with ``pcm16``, int16 and bit for bit ``pcm16_on_device`` of those -- and
        ``(max p, min g)`` over them, ``(0, 1)`` where there are none.  Stateless, asynchronous on the current stream, the same 2
        launches with tiles over the settled samples only; none when ``out_count == 0``.  ``LimiterSession`` keeps the
        bookkeeping.  How fast a window is has not been measured on a GPU."""
        wav = _wave(wav)
        B, Lw = int(wav.shape[0]), int(wav.shape[1])
        count = self.window_range(origin, Lw, final)[1]
        lib = self._ensure()
        out = torch.empty((B, count), dtype=torch.int16 if pcm16 else torch.float32, device=self._device)
        if B == 0 or count == 0:
            return out, self._empty_stats(B)
        wav = wav.to(self._device).contiguous()
        stats = torch.empty((B, 2), dtype=torch.float32, device=self._device)
        ws = self._ws(B, Lw)                                     # a window's workspace is that of a call of its shape
        with torch.cuda.device(self._device):
            _native.check("iris_limiter_forward_window", lib.iris_limiter_forward_window(
                self._handle, _ptr(wav), B, Lw, ctypes.c_int64(int(origin)), int(bool(final)), _ptr(out), int(bool(pcm16)),
                _ptr(stats), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, stats

    # -- groups of windows: one utterance per row ----------------------------------------------
    def _window_items(self, items):
        """``items``: a sequence of ``(origin, Lw, final)`` -> the C array ``iris_limiter_forward_windows`` takes."""
        arr = (_native.LimiterWindowItem * max(len(items), 1))()
        for b, (origin, Lw, final) in enumerate(items):
            arr[b].origin, arr[b].Lw, arr[b].final = int(origin), int(Lw), int(bool(final))
        return arr

    def windows_workspace_bytes(self, B: int, in_stride: int) -> int:
        return self._query("windows_workspace_bytes", B, in_stride)

    def windows_launch_count(self, items) -> int:
        """Kernel launches of one ``forward_windows``: 2, or 0 where no row settles anything (a dry run on the host)."""
        items = list(items)
        cfg, n = self.native_config(), ctypes.c_int32()
        _native.check("iris_limiter_windows_launch_count", _native.load().iris_limiter_windows_launch_count(
            ctypes.byref(cfg), len(items), self._window_items(items), ctypes.byref(n)))
        return int(n.value)

    def forward_windows(self, wav, items, pcm16: bool = False, out_stride: Optional[int] = None):
        """Windows of ``B`` DIFFERENT utterances in one call (``iris_limiter_forward_windows``): row b of ``wav [B, in_stride]``
        fp32 holds samples ``[origin_b, origin_b + Lw_b)`` of its own utterance in its first ``Lw_b`` slots, ``items[b] =
        (origin_b, Lw_b, final_b)`` -> ``(out [B, out_stride], stats [B, 2], counts)``: the first ``counts[b] =
        window_range(*items[b])[1]`` slots of row b are bit for bit ``forward_window`` of that item alone, the rest of the row is
        0, and ``stats[b]`` is that call's too (``(0, 1)`` for a row that settles nothing).  ``out_stride``: the largest count
        unless given.  The same 2 launches as one window, the descriptors by value in the kernel argument: nothing is copied or
        allocated natively.  At most ``_native.WINDOW_GROUP_MAX`` rows (the library refuses more; ``iris.stream_group`` splits).
        How fast a group call is: DESIGN.md, "Concurrent streams"."""
        wav, items = _wave(wav), [(int(o), int(n), bool(f)) for o, n, f in items]
        B, in_stride = int(wav.shape[0]), int(wav.shape[1])
        if len(items) != B:
            raise ValueError(f"{B} rows but {len(items)} items")
        counts = [self.window_range(o, n, f)[1] for o, n, f in items]
        most = max(counts, default=0)
        out_stride = most if out_stride is None else int(out_stride)
        lib = self._ensure()
        out = torch.empty((B, out_stride), dtype=torch.int16 if pcm16 else torch.float32, device=self._device)
        if B == 0 or most == 0:
            return out.zero_(), self._empty_stats(B), counts
        wav = wav.to(self._device).contiguous()
        stats = torch.empty((B, 2), dtype=torch.float32, device=self._device)
        ws = self._grow(self.windows_workspace_bytes(B, in_stride))
        with torch.cuda.device(self._device):
            _native.check("iris_limiter_forward_windows", lib.iris_limiter_forward_windows(
                self._handle, _ptr(wav), B, in_stride, self._window_items(items), _ptr(out), out_stride, int(bool(pcm16)),
                _ptr(stats), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, stats, counts

    def open_session(self, pcm16: bool = False) -> "LimiterSession":
        """A ``LimiterSession`` for one utterance (or a batch of equal lengths) that arrives piece by piece."""
        return LimiterSession(self, pcm16=pcm16)

    def chunked(self, pcm16: bool = False) -> "ChunkedLimiter":
        """This limiter as the opt-in a pipeline looks for before it streams (``ChunkedLimiter``)."""
        return ChunkedLimiter(self, pcm16=pcm16)


class LimiterSession(_RangeSession):
    """Pushed input for a limiter (``_WindowSession``: ``push`` pieces, ``flush`` at the end).  The concatenation of everything
    returned equals ``limit_device`` of the concatenated pieces bit for bit -- with ``pcm16=True`` it is int16 and equals
    ``pcm16_on_device`` of that: a sample's gain reads ``R = 2A + 7`` samples on either side and nothing else, every chain in its
    one order, so it is settled once those have arrived -- or lie past an end of the utterance, where the one-shot call reads
    zeros too (``Limiter.window_range``).

    ``lim``: a ``Limiter``, or any object with ``window_range(origin, Lw, final) -> (out_lo, out_count)`` and
    ``forward_window(wav, origin, final, pcm16=) -> (out [B, out_count], stats [B, 2])``.  The session keeps only the input the
    next window needs, from ``samples_emitted - R`` on, so ``samples_buffered`` stays within ``2R`` plus the piece just pushed;
    ``halo = (R, R)`` is asked of ``window_range``.  Pieces may have any length, 0 included.

    Latency: sample s leaves with the push that brings ``samples_received`` to ``s + R + 1``.  The first piece is therefore short
    by ``R`` samples (or empty, and then nothing is launched) and ``flush`` returns the last ``R``: 73 at 1.5 ms and 22.05 kHz.

    ``stats [B, 2]``: the running ``(max p, min g)`` of the windows so far, kept on the device by ``torch.maximum`` /
    ``torch.minimum`` with no read-back; ``(0, 1)`` before any window (None before any push), and after ``flush`` the one-shot
    call's ``stats`` bit for bit."""

    _ragged_call = "limit_device(lengths=)"

    def __init__(self, lim, pcm16: bool = False):
        self.pcm16 = bool(pcm16)
        super().__init__(lim, step=1, dtype=torch.int16 if self.pcm16 else torch.float32)
        self._stats: Optional[torch.Tensor] = None

    @property
    def stats(self) -> Optional[torch.Tensor]:
        if self._stats is None and self._buf is not None:     # no window yet: (0, 1) per item, where the pieces are
            return torch.tensor([0.0, 1.0], dtype=torch.float32, device=self._buf.device).repeat(self._buf.shape[0], 1)
        return self._stats

    def _forward_window(self, final: bool):
        return self._stage.forward_window(self._buf, self._base, final, pcm16=self.pcm16)

    def _take(self, plan, result):
        """``result``: the ``(out, stats)`` of the planned window, from ``forward_window`` or as a row of ``forward_windows``."""
        if not plan.launch:
            return super()._take(plan, None)
        out, stats = result
        # a window that still starts at sample 0 settles [0, ...) again; its stats then cover samples already counted, which
        # a maximum and a minimum do not mind
        if self._stats is not None:
            stats = torch.stack([torch.maximum(self._stats[:, 0], stats[:, 0]), torch.minimum(self._stats[:, 1], stats[:, 1])], dim=1)
        self._stats = stats
        return super()._take(plan, out)


class ChunkedLimiter:
    """``lim`` with the promise a streaming pipeline asks for: ``MelToWavePipeline(..., limiter=ChunkedLimiter(lim))`` -- or
    ``lim.chunked()`` -- lets ``stream`` and ``session`` run, every chunk going through one ``LimiterSession`` last of all.  The
    opt-in is explicit because the pieces such a pipeline yields are no longer all ``[B, hop * chunk]`` (the first is short by
    ``2A + 7`` samples and the last carries them); a plain ``Limiter`` keeps refusing.  ``pcm16=True``: the streamed pieces are
    int16, what ``infer(mel, pcm16=True)`` returns.  ``limit_device`` and ``true_peak_device`` are ``lim``'s."""

    chunked_sessions = True

    def __init__(self, lim, pcm16: bool = False):
        self.lim, self.pcm16 = lim, bool(pcm16)

    def limit_device(self, wav, lengths=None, row_scale: int = 1):
        return self.lim.limit_device(wav, lengths=lengths, row_scale=row_scale)

    def true_peak_device(self, wav, lengths=None, row_scale: int = 1):
        return self.lim.true_peak_device(wav, lengths=lengths, row_scale=row_scale)

    def open_session(self) -> LimiterSession:
        return LimiterSession(self.lim, pcm16=self.pcm16)
