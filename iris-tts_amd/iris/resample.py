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

Streaming.  Output ``n`` reads ``x[i0(n) - Hw + 1 .. i0(n) + Hw]`` (``Hw = half_width``) and nothing else, so the stage is chunked
exactly.  A window holds samples ``[origin, origin + Lw)`` of an utterance, ``n_next`` is the first output not yet emitted, and

    ``n_hi = ceil((origin + Lw) * up / down)`` if ``final`` else ``ceil(max(0, origin + Lw - Hw) * up / down)``

-- the outputs whose last tap lies inside the window; the window emits ``[n_next, n_hi)`` provided ``origin == 0`` or
``i0(n_next) - Hw + 1 >= origin``, and the next window must still hold the samples from ``keep_from = max(0, i0(n_hi) - Hw + 1)``
on (``window_plan``; the rule is written down once, in csrc/resample.h, ``struct Window``).  ``Resampler.forward_window`` is ONE
launch of the whole call's kernel on such a window, ``ResamplerSession`` keeps the two numbers and the held samples, and the
concatenation of its pieces equals ``Resampler.forward`` of the whole bit for bit -- as fp32, as int16, and as G.711 mu-law or
A-law bytes (``encoding=``: telephony, one byte per sample, the integer rules of ``iris.synthesis_output.ulaw_from_pcm16`` /
``alaw_from_pcm16`` applied to the int16 sample by the kernel's store).  ``res.chunked(encoding)`` (``ChunkedResampler``) is the
opt-in with which ``MelToWavePipeline(output=)`` runs such a session last of all.  Per-chunk ``forward(origin=running)`` calls do
NOT concatenate to the whole: they take the samples in front of ``origin`` for zeros.

Many sessions in one launch: ``Resampler.forward_windows`` and ``iris.stream_group``.  Not built: a normalised form in windows (the peak belongs to the whole item).
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._window_session import _WindowSession

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


def window_plan(up: int, down: int, half_width: int, origin: int, Lw: int, n_next: int, final: bool) -> Tuple[int, int]:
    """``(n_hi, keep_from)`` of the window ``[origin, origin + Lw)``: the host restatement of ``iris_resampler_window_plan``
    (module docstring) in Python integers: planning without a device, and a fake resampler built on ``resample_host``.
    ``ValueError`` where the precondition fails."""
    origin, Lw, n_next, hw = int(origin), int(Lw), int(n_next), int(half_width)
    end = origin + Lw
    if origin < 0 or Lw < 0 or not 0 <= n_next <= _ceil_div(end * up, down):
        raise ValueError(f"a window needs origin >= 0, Lw >= 0 and n_next within its outputs, got {origin}, {Lw}, {n_next}")
    if origin and n_next * down // up - hw + 1 < origin:
        raise ValueError(f"the window starts at sample {origin}, but output {n_next} reads from sample {n_next * down // up - hw + 1} on")
    n_hi = _ceil_div((end if final else max(0, end - hw)) * up, down)
    return n_hi, max(0, n_hi * down // up - hw + 1)


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
                peak_target: float = 0.95, encoding: Optional[str] = None):
        """``wav``: fp32 device tensor ``[B, L]`` whose first column has the utterance-global index ``origin`` ->
        ``[B, n_count]`` (``out_range(origin, L)``): fp32, or int16 with ``pcm16=True`` (bit for bit
        ``pcm16_from_float`` of the fp32 result).  ``normalize=True`` (with pcm16) scales every item to ``peak_target`` at
        its own peak first and returns ``(pcm, peaks)``, ``peaks`` the fp32 tensor [B] of the items' max |out|.
        ``lengths`` (a sequence or an integer tensor [B]) and ``row_scale``: item b owns
        ``min(L, lengths[b] * row_scale)`` samples; the rest is never read and its outputs past its own count are 0.
        ``encoding``: ``"f32"`` and ``"pcm16"`` say what ``pcm16=`` says; ``"ulaw"`` / ``"alaw"`` return uint8, the G.711 byte of
        every int16 sample, stored by the same launch (``iris_resampler_forward_g711``) -- an item's row past its own count
        then holds the law's code for 0 -- and refuse ``normalize=True``."""
        g711 = None
        if encoding is not None:
            if encoding not in _native.OUT_FORMS:
                raise ValueError(f"encoding must be one of {tuple(_native.OUT_FORMS)}, got {encoding!r}")
            if encoding in ("ulaw", "alaw"):
                if normalize or pcm16:
                    raise ValueError("a G.711 encoding has no normalised form and is no 16-bit PCM: pass neither normalize=True nor "
                                     "pcm16=True beside it")
                g711 = _native.OUT_FORMS[encoding]
            elif pcm16 and encoding == "f32":
                raise ValueError("encoding='f32' contradicts pcm16=True")
            else:
                pcm16 = pcm16 or encoding == "pcm16"
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
        if g711 is not None:
            out = torch.empty((B, n_count), dtype=torch.uint8, device=self.device)
            if B and L and n_count:
                _native.check("iris_resampler_forward_g711", self.lib.iris_resampler_forward_g711(
                    self._handle, ctypes.c_void_p(wav.data_ptr()), B, L,
                    ctypes.c_void_p(lengths_dev.data_ptr() if lengths_dev is not None else None), int(row_scale),
                    ctypes.c_int64(int(origin)), g711, ctypes.c_void_p(out.data_ptr()),
                    ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            return out
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

    # -- windows of an utterance -------------------------------------------------------------
    def window_plan(self, origin: int, Lw: int, n_next: int, final: bool) -> Tuple[int, int]:
        """``(n_hi, keep_from)``: the window ``[origin, origin + Lw)`` emits the outputs ``[n_next, n_hi)`` and the next window
        must hold the samples from ``keep_from`` on (``iris_resampler_window_plan``: the rule of the module docstring, written
        down on the C side only).  Host only; a violated precondition is a ``NativeCallError`` (invalid argument)."""
        n_hi, keep = ctypes.c_int64(), ctypes.c_int64()
        _native.check("iris_resampler_window_plan", self.lib.iris_resampler_window_plan(
            self._handle, ctypes.c_int64(int(origin)), ctypes.c_int64(int(Lw)), ctypes.c_int64(int(n_next)), int(bool(final)),
            ctypes.byref(n_hi), ctypes.byref(keep)))
        return int(n_hi.value), int(keep.value)

    def forward_window(self, wav, origin: int, n_next: int, final: bool, encoding: str = "f32"):
        """``wav [B, Lw]`` fp32 = samples ``[origin, origin + Lw)`` of B utterances of one length -> ``[B, n_hi - n_next]`` on the
        device: the outputs ``window_plan`` names, each bit for bit the one ``forward`` of the whole utterance returns there, as
        fp32, int16 (``"pcm16"``) or G.711 bytes (``"ulaw"``, ``"alaw"``).  Stateless, asynchronous on the current stream, ONE
        launch of ``forward``'s kernel, no workspace; none at all when nothing is final yet.  ``ResamplerSession`` keeps the
        bookkeeping."""
        if encoding not in _native.OUT_FORMS:
            raise ValueError(f"encoding must be one of {tuple(_native.OUT_FORMS)}, got {encoding!r}")
        if not isinstance(wav, torch.Tensor):
            wav = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32)))
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"expected an fp32 waveform [B, Lw], got {wav.dtype} {tuple(wav.shape)}")
        B, Lw = int(wav.shape[0]), int(wav.shape[1])
        count = max(0, self.window_plan(origin, Lw, n_next, final)[0] - int(n_next))
        out = torch.empty((B, count), dtype=_torch_dtype(encoding), device=self.device)
        if B and Lw and count:
            wav = wav.to(self.device).contiguous()
            with torch.cuda.device(self.device):
                _native.check("iris_resampler_forward_window", self.lib.iris_resampler_forward_window(
                    self._handle, ctypes.c_void_p(wav.data_ptr()), B, Lw, ctypes.c_int64(int(origin)), ctypes.c_int64(int(n_next)),
                    int(bool(final)), ctypes.c_void_p(out.data_ptr()), _native.OUT_FORMS[encoding],
                    ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def forward_windows(self, wav, items, encoding: str = "f32", out_stride: Optional[int] = None):
        """Windows of ``B`` DIFFERENT utterances in ONE launch (``iris_resampler_forward_windows``): row b of ``wav [B, in_stride]``
        fp32 holds samples ``[origin_b, origin_b + Lw_b)`` of its own utterance in its first ``Lw_b`` slots, ``items[b] =
        (origin_b, Lw_b, n_next_b, final_b)`` -> ``(out [B, out_stride], counts)``: the first ``counts[b] = n_hi_b - n_next_b``
        slots of row b are bit for bit ``forward_window`` of that item alone, in ``encoding``, and the rest of the row holds
        the code of sample 0 (0, 0, 0xFF, 0xD5).  ``out_stride``: the largest count unless given.  An item that fails
        ``window_plan``'s precondition fails the whole call.  The descriptors travel by value in the kernel argument: nothing
        is copied or allocated natively.  At most ``_native.WINDOW_GROUP_MAX`` rows (``iris.stream_group`` splits)."""
        if encoding not in _native.OUT_FORMS:
            raise ValueError(f"encoding must be one of {tuple(_native.OUT_FORMS)}, got {encoding!r}")
        if not isinstance(wav, torch.Tensor):
            wav = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32)))
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"expected an fp32 waveform [B, in_stride], got {wav.dtype} {tuple(wav.shape)}")
        items = [(int(o), int(n), int(k), bool(f)) for o, n, k, f in items]
        B, in_stride = int(wav.shape[0]), int(wav.shape[1])
        if len(items) != B:
            raise ValueError(f"{B} rows but {len(items)} items")
        counts = [max(0, self.window_plan(o, n, k, f)[0] - k) for o, n, k, f in items]
        most = max(counts, default=0)
        out_stride = most if out_stride is None else int(out_stride)
        out = torch.empty((B, out_stride), dtype=_torch_dtype(encoding), device=self.device)
        if B == 0 or most == 0:
            return out.fill_(_ZERO_CODE[encoding]), counts
        arr = (_native.ResamplerWindowItem * B)()
        for b, (o, n, k, f) in enumerate(items):
            arr[b].origin, arr[b].n_next, arr[b].Lw, arr[b].final = o, k, n, int(f)
        wav = wav.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            _native.check("iris_resampler_forward_windows", self.lib.iris_resampler_forward_windows(
                self._handle, ctypes.c_void_p(wav.data_ptr()), B, in_stride, arr, ctypes.c_void_p(out.data_ptr()), out_stride,
                _native.OUT_FORMS[encoding], ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out, counts

    def open_session(self, encoding: str = "f32") -> "ResamplerSession":
        """A ``ResamplerSession`` for one utterance (or a batch of equal lengths) that arrives piece by piece."""
        return ResamplerSession(self, encoding)

    def chunked(self, encoding: str = "f32") -> "ChunkedResampler":
        """This resampler as the output stage a streaming pipeline takes (``MelToWavePipeline(output=res.chunked("ulaw"))``)."""
        return ChunkedResampler(self, encoding)


ENCODINGS = ("f32", "pcm16", "ulaw", "alaw")


_ZERO_CODE = {"f32": 0, "pcm16": 0, "ulaw": 0xFF, "alaw": 0xD5}      # what sample 0 is in each encoding: a row's padding


def _torch_dtype(encoding: str):
    return {"f32": torch.float32, "pcm16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}[encoding]


class ResamplerSession(_WindowSession):
    """Pushed input for a resampler (``_WindowSession``: ``push`` pieces, ``flush`` at the end); converted samples leave as soon
    as their last tap has arrived -- past the end of the utterance the taps read zeros, as in the one-shot call.  The concatenation
    of everything returned equals ``Resampler.forward`` of the concatenated pieces bit for bit, in the session's ``encoding``
    (``"f32"``, ``"pcm16"``, ``"ulaw"``, ``"alaw"``), and has ``ceil(L * up / down)`` samples.

    ``res``: a ``Resampler``, or any object with ``window_plan(origin, Lw, n_next, final) -> (n_hi, keep_from)`` and
    ``forward_window(wav, origin, n_next, final, encoding=) -> [B, n_hi - n_next]``.  Each push is ONE window over what is held:
    the samples from the last window's ``keep_from`` on and the piece just pushed.  The session's whole state is those samples
    and the count ``n_next`` (``samples_emitted``), so ``samples_buffered`` stays under ``2 Hw + ceil(down / up)`` plus the piece
    just pushed.  Pieces may have any length, 0 included.

    Latency: output n leaves with the push that brings ``samples_received`` to ``i0(n) + Hw + 1``: ``Hw`` input samples, 45 at
    8 kHz from 22.05 kHz (2 ms).  ``flush`` returns the outputs that were waiting for them."""

    _ragged_call = "forward(lengths=)"

    def __init__(self, res, encoding: str = "f32"):
        if encoding not in ENCODINGS:
            raise ValueError(f"encoding must be one of {ENCODINGS}, got {encoding!r}")
        super().__init__(dtype=_torch_dtype(encoding))
        self._res, self.encoding = res, encoding
        self._next = 0                # the first output not yet emitted

    @property
    def samples_emitted(self) -> int:
        return self._next

    def _plan(self, final: bool) -> SimpleNamespace:
        """The window over everything held: ``origin``, ``Lw``, ``n_next``, ``final``, what ``window_plan`` answers for it, and
        ``launch``: whether an output became final.  (``iris.stream_group`` runs the planned windows of many sessions at once.)"""
        n_hi, keep_from = self._res.window_plan(self._base, self._total - self._base, self._next, final)
        return SimpleNamespace(origin=self._base, Lw=self._total - self._base, n_next=self._next, final=bool(final), n_hi=n_hi,
                               keep_from=keep_from, launch=n_hi > self._next)

    def _take(self, plan: SimpleNamespace, out):
        """``(piece, keep_from)`` of the planned window, whose forward returned ``out [B, n_hi - n_next]`` (None: no launch)."""
        if not plan.launch:
            return self._empty(), plan.keep_from                  # nothing became final: no launch
        self._next = plan.n_hi
        return out, plan.keep_from                                # the next window's left-hand taps

    def _window(self, final: bool):
        plan = self._plan(final)
        out = self._res.forward_window(self._buf, self._base, self._next, final, encoding=self.encoding) if plan.launch else None
        return self._take(plan, out)


class ChunkedResampler:
    """``res`` with an encoding, as the output stage of a pipeline: ``MelToWavePipeline(..., output=res.chunked("ulaw"))`` lets
    ``stream`` and ``session`` run one ``ResamplerSession`` last of all, and ``infer`` / ``infer_batch`` call ``forward``, which is
    ``res.forward(..., encoding=)``.  The pieces are fp32, int16 or uint8 at ``rate_out``."""

    chunked_sessions = True

    def __init__(self, res, encoding: str = "f32"):
        if encoding not in ENCODINGS:
            raise ValueError(f"encoding must be one of {ENCODINGS}, got {encoding!r}")
        self.res, self.encoding = res, encoding

    @property
    def rate_out(self) -> int:
        return self.res.rate_out

    def out_range(self, origin: int, L: int) -> Tuple[int, int]:
        return self.res.out_range(origin, L)

    def forward(self, wav, lengths=None, row_scale: int = 1, origin: int = 0, pcm16: bool = False, normalize: bool = False):
        if pcm16 or normalize:
            raise ValueError("an output stage stores its own encoding: pcm16= and normalize= do not go with it")
        return self.res.forward(wav, lengths=lengths, row_scale=row_scale, origin=origin, encoding=self.encoding)

    def open_session(self) -> ResamplerSession:
        return ResamplerSession(self.res, self.encoding)


_shared: dict = {}


def shared_resampler(rate_out: int, device, rate_in: int = DEFAULT_RATE_IN) -> Resampler:
    """The default filter ``rate_in -> rate_out`` on ``device``, built on first use and kept (the drop-in entry points
    ``infer_hifigan(..., sample_rate_out=)`` and ``HiFiGANVocoder.infer(..., sample_rate_out=)`` have no object to own one)."""
    key = (int(rate_in), int(rate_out), str(device))
    rs = _shared.get(key)
    if rs is None:
        rs = _shared[key] = Resampler(rate_out, rate_in=rate_in, device=device)
    return rs
