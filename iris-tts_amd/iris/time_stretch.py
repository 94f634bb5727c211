"""Time stretch and pitch shift on the device (``iris_time_stretch_*``, csrc/time_stretch.h): a phase vocoder between the two
transforms the DSP stages share.  ``TimeStretch`` is ``librosa.effects.time_stretch(y, rate=, n_fft=, hop_length=,
win_length=)`` under this project's frame rules (``center=True``, zero padding, periodic Hann centred in ``n_fft``); librosa
cannot be imported here, so the contract is the math below, held by a float64 numpy restatement
(``tests/time_stretch_restatement.py``).

With ``N = n_fft``, ``H = hop_length``: a waveform of ``L = H M`` samples has ``T = M + 1`` frames ``c = stft(wav)``, and

    ``T_out = len(np.arange(0, T, rate));  step_t = t * rate;  i = floor(step_t);  alpha = step_t - i``   (a column >= T is 0)
    ``mag[t, k] = (1 - alpha) |c[i, k]| + alpha |c[i + 1, k]|``
    ``dphi = angle(c[i + 1, k]) - angle(c[i, k]) - adv_k;  dphi -= round(dphi)``                       (in turns)
    ``acc[0, k] = angle(c[0, k]);  acc[t + 1, k] = acc[t, k] + adv_k + dphi;  out_c = mag (cos, sin)(2 pi acc)``
    ``n_out = round(L / rate);  out = istft(out_c, length=n_out)``

with ``adv_k = (k H mod N) / N``.  The phase is accumulated in 32-bit fixed-point turns: the sum wraps where an fp32 sum of
radians would lose the phase, and it is associative, so every run gives the same bits.  ``rate > 1`` is faster.

A forward is 4 launches on the current stream.  ``forward_device(lengths=)`` takes a ragged batch: item b is bit for bit its
batch-of-one call, the rest of its row is 0, and ``counts`` holds the items' samples for the next stage.
``pitch_shift_device`` is librosa's structure for ``pitch_shift`` -- stretch by ``2 ** (-n_steps / 12)``, resample back -- on
``iris.resample.Resampler``.  ``MelToWavePipeline(..., stretch=ts.at(rate))`` runs the stretch behind the denoiser.

Streaming: ``TimeStretch.open_session(rate)`` takes the waveform piece by piece (``StretchSession``: one ``forward_window`` per
push, the same launches on a window of the utterance, the phase and the last ``n_fft / hop - 1`` output frames carried in a
device state) and its output equals ``forward_device`` of the whole bit for bit; ``ts.at(rate).chunked()``
(``ChunkedStretch``) is the opt-in with which a pipeline's ``stream`` / ``session`` run it behind the vocoder.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _take_buffers, _take_shapes, _wave
from ._window_session import _WindowSession
from .vae import _lengths_on, check_lengths

RATE_RANGE = (0.25, 4.0)
_TAPS = ("c", "mag", "inc", "acc", "out_c")


def check_rate(rate) -> float:
    r = float(rate)
    if not math.isfinite(r) or not RATE_RANGE[0] <= r <= RATE_RANGE[1]:
        raise ValueError(f"rate must lie in [{RATE_RANGE[0]}, {RATE_RANGE[1]}], got {rate!r}")
    return r


class TimeStretch(_DeviceStage):
    """A phase vocoder with fixed transform parameters (librosa's defaults for this effect; 1024 / 256 works as well),
    resident on one GPU (``device``, or the current one); the handle is built on first use.  The rate belongs to a call."""

    _abi_name = "time_stretch"

    def __init__(self, n_fft: int = 2048, hop_length: int = 512, win_length: Optional[int] = None,
                 device: Optional[torch.device] = None):
        super().__init__(device)
        win_length = n_fft if win_length is None else win_length
        for name, v in (("n_fft", n_fft), ("hop_length", hop_length), ("win_length", win_length)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    def get_config(self) -> dict:
        return {"n_fft": self.n_fft, "hop_length": self.hop_length, "win_length": self.win_length}

    def native_config(self) -> "_native.MelFrontendConfig":
        """The front-end's config the C side takes; only the three transform fields are read."""
        return _native.MelFrontendConfig(22050, self.n_fft, self.hop_length, self.win_length, 1, 0, 0.0, 0.0)

    # -- host-only queries -------------------------------------------------------------------
    def out_frames_samples(self, L: int, rate) -> Tuple[int, int]:
        """``(T_out, n_out)`` of one item of ``L`` samples, from the library (the lines the device runs; no device needed)."""
        lib = _native.load()
        cfg, frames, samples = self.native_config(), ctypes.c_int32(), ctypes.c_int32()
        _native.check("iris_time_stretch_out_samples", lib.iris_time_stretch_out_samples(
            ctypes.byref(cfg), int(L), ctypes.c_double(float(rate)), ctypes.byref(frames), ctypes.byref(samples)))
        return int(frames.value), int(samples.value)

    def out_samples(self, L: int, rate) -> int:
        """``n_out = round(L / rate)`` (float64, half to even): what ``forward_device`` returns per row, and what ``counts``
        holds for an item of ``L`` samples."""
        return self.out_frames_samples(L, rate)[1]

    def launch_count(self, B: int, L: int, rate=1.0) -> int:
        """Kernel launches of one ``forward_device``: 4 (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L, rate)

    def workspace_bytes(self, B: int, L: int, rate=1.0) -> int:
        return self._query("workspace_bytes", B, L, rate)

    def _workspace_layout(self, B: int, L: int, rate):
        """``({buffer: (offset, shape)}, floats)``: ``TsWorkspace`` (csrc/iris_time_stretch.hip) restated -- the taps, then the
        items' ``frames``, ``frames_out`` and ``counts`` (int32), in ``WsTaker`` order.  Host only."""
        T, (T_out, _) = L // self.hop_length + 1, self.out_frames_samples(L, rate)
        ks, qp = (self.n_bins + 3) // 4 * 4, (self.n_fft + 2 + 7) // 8 * 8
        return _take_shapes({"c": (B, T, qp), "mag": (B, T_out, ks), "inc": (B, T_out, ks), "acc": (B, T_out, ks),
                             "out_c": (B, T_out, qp), "frames": (B,), "frames_out": (B,), "counts": (B,)})

    def _read_buffers(self, B: int, L: int, rate) -> dict:
        """Test-only: copies of the taps ``c``, ``mag``, ``out_c`` (fp32) and ``inc``, ``acc`` (as int64 in [0, 2^32)) and of the
        items' counts, as the last ``forward_device`` of shape (B, L) at ``rate`` left them in the workspace."""
        layout, _ = self._workspace_layout(B, L, rate)
        out = {}
        for name, (off, shape) in layout.items():
            n = int(np.prod(shape))
            if name in ("c", "mag", "out_c"):
                out[name] = self._workspace.view(torch.float32)[off:off + n].view(shape).clone()
            else:
                v = self._workspace.view(torch.int32)[off:off + n].view(shape).clone()
                out[name] = v.to(torch.int64) & 0xFFFFFFFF if name in ("inc", "acc") else v
        return out

    def _wav_on_device(self, wav) -> torch.Tensor:
        return _wave(wav, self.hop_length, "a vocoder emits whole mel frames")

    # -- the forward -------------------------------------------------------------------------
    def forward_device(self, wav, rate, lengths=None):
        """``wav [B, L]`` fp32, host or device, ``L`` a multiple of ``hop_length`` -> ``(out [B, n_out], counts [B])`` on the
        device, ``n_out = out_samples(L, rate)``; ``counts`` (int32) holds the items' own samples -- ``n_out`` for a dense call.
        Asynchronous on the current stream, 4 launches, nothing synchronises; two calls agree bit for bit.

        ``lengths``: item b's MEL frames ``M_b`` (it owns ``hop_length * M_b`` samples) -- a host sequence of integers in
        ``[0, L / hop_length]`` (``ValueError`` otherwise, before any device work) or an int32 device tensor ``[B]``, which the
        host never reads.  ``out[b, :counts[b]]`` is bit for bit the call on ``wav[b:b + 1, :hop_length * M_b]``, the rest
        of the row is 0, ``counts[b] = out_samples(hop_length * M_b, rate)``, and nothing past an item's own samples is read."""
        wav = self._wav_on_device(wav)
        rate = check_rate(rate)
        B, L = int(wav.shape[0]), int(wav.shape[1])
        if lengths is not None:
            lengths = check_lengths(lengths, B, L // self.hop_length, 1)
        lib = self._ensure()
        wav = wav.to(self._device).contiguous()
        if lengths is not None:
            lengths = _lengths_on(lengths, self._device)
        n_out = self.out_samples(L, rate) if L else 0
        out = torch.empty((B, n_out), dtype=torch.float32, device=self._device)
        counts = torch.full((B,), n_out, dtype=torch.int32, device=self._device)
        if B == 0 or L == 0:
            return out, counts
        ws = self._ws(B, L, rate)
        with torch.cuda.device(self._device):
            _native.check("iris_time_stretch_forward_ragged", lib.iris_time_stretch_forward_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), ctypes.c_double(rate), _ptr(out), _ptr(counts), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, counts

    def __call__(self, wav, rate) -> np.ndarray:
        """``[L]`` -> ``[n_out]``; ``[B, L]`` -> ``[B, n_out]``, numpy in and numpy out."""
        wav = wav.detach().cpu().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav, dtype=np.float32)
        if wav.ndim == 1:
            return self.forward_device(wav[None], rate)[0][0].cpu().numpy()
        return self.forward_device(wav, rate)[0].cpu().numpy()

    def at(self, rate) -> "StretchAt":
        """This stretch at one rate: what ``MelToWavePipeline(stretch=)`` takes."""
        return StretchAt(self, check_rate(rate))

    # -- windows of an utterance -------------------------------------------------------------
    def state_bytes(self, B: int) -> int:
        return self._query("state_bytes", B)

    def new_state(self, B: int) -> torch.Tensor:
        """The state a sequence of ``forward_window`` calls carries (``iris_time_stretch_state_bytes``): the phase at the next
        frame and the last ``n_fft / hop_length - 1`` output frames.  Uninitialised: the window with ``u == 0`` reads none of it."""
        self._ensure()
        return torch.empty(self.state_bytes(B), dtype=torch.uint8, device=self._device)

    def _state_views(self, state: torch.Tensor, B: int):
        """Test-only: ``(acc [B, Ks] as int64 in [0, 2^32), tail [B, taps - 1, Qp] fp32)``, views restated from ``TsState``."""
        ks, qp, rows = (self.n_bins + 3) // 4 * 4, (self.n_fft + 2 + 7) // 8 * 8, self.n_fft // self.hop_length - 1
        tail_off = _take_buffers((("acc", B * ks), ("tail", B * rows * qp)))[0]["tail"][0]
        acc = state.view(torch.int32)[:B * ks].view(B, ks).to(torch.int64) & 0xFFFFFFFF
        return acc, state.view(torch.float32)[tail_off:tail_off + B * rows * qp].view(B, rows, qp)

    def window_plan(self, rate, origin: int, Lw: int, final: bool, u: int):
        """``(u_hi, out_lo, out_count, keep_from)`` of the window ``[origin, origin + Lw)`` for a caller whose next output frame
        is ``u``: it computes frames ``[u, u_hi)`` and emits samples ``[out_lo, out_lo + out_count)`` of the stretched
        utterance; the next window must still hold the input from ``keep_from`` on (``iris_time_stretch_window_plan``: the
        rule is written down on the C side only).  Host only."""
        lib = _native.load()
        cfg, out = self.native_config(), [ctypes.c_int64() for _ in range(4)]
        _native.check("iris_time_stretch_window_plan", lib.iris_time_stretch_window_plan(
            ctypes.byref(cfg), ctypes.c_double(float(rate)), ctypes.c_int64(int(origin)), int(Lw), int(bool(final)), ctypes.c_int64(int(u)),
            *[ctypes.byref(v) for v in out]))
        return tuple(int(v.value) for v in out)

    def window_workspace_bytes(self, B: int, Lw: int, rate=1.0) -> int:
        return self._query("window_workspace_bytes", B, Lw, rate)

    def window_launch_count(self, B: int, Lw: int, rate, origin: int, final: bool, u: int) -> int:
        """Kernel launches of one ``forward_window``: 4; 3 where frames advance but no sample is emitted yet, 2 where a final
        window has samples left but no frame, 0 where it has neither (a dry run on the host)."""
        return self._query("window_launch_count", B, Lw, rate, origin, bool(final), u)

    def _window_workspace_layout(self, B: int, Lw: int, rate, frames: int, new: int, tail: int):
        """``{buffer: (offset, shape)}``: ``TsWindowWorkspace`` restated for a window that computed ``frames`` input rows and
        ``new`` output frames behind ``tail`` carried ones.  Offsets depend on (B, Lw, rate) alone.  Host only."""
        ks, qp, taps = (self.n_bins + 3) // 4 * 4, (self.n_fft + 2 + 7) // 8 * 8, self.n_fft // self.hop_length
        F, n = Lw // self.hop_length + 1, math.ceil((Lw // self.hop_length + 1) / float(rate)) + 1
        bufs = {"c": (B * F * qp, (B, frames, qp)), "mag": (B * n * ks, (B, new, ks)), "inc": (B * n * ks, (B, new, ks)),
                "acc": (B * n * ks, (B, new, ks)), "out_c": (B * (n + taps - 1) * qp, (B, tail + new, qp))}
        assert all(int(np.prod(shape)) <= room for room, shape in bufs.values())
        layout, _ = _take_buffers((name, room) for name, (room, _) in bufs.items())
        return {name: (layout[name][0], shape, room) for name, (room, shape) in bufs.items()}

    def forward_window(self, wav, rate, origin: int, final: bool, u: int, state: Optional[torch.Tensor]) -> torch.Tensor:
        """``wav [B, Lw]`` fp32 = samples ``[origin, origin + Lw)`` of an utterance (both multiples of ``hop_length``) -> the
        samples ``window_plan(rate, origin, Lw, final, u)`` names, ``[B, out_count]`` on the device, each bit for bit the sample
        ``forward_device`` of the whole utterance returns there.  ``state`` (``new_state(B)``) is read and written in place;
        None only for a final window with ``u == 0``.  Asynchronous, at most 4 launches, none when the plan is empty.
        ``StretchSession`` keeps the bookkeeping."""
        wav = self._wav_on_device(wav)
        rate = check_rate(rate)
        B, Lw = int(wav.shape[0]), int(wav.shape[1])
        u_hi, _, count, _ = self.window_plan(rate, origin, Lw, final, u)
        lib = self._ensure()
        out = torch.empty((B, count), dtype=torch.float32, device=self._device)
        if B == 0 or (u_hi == u and count == 0):
            return out
        wav = wav.to(self._device).contiguous()
        ws = self._grow(self.window_workspace_bytes(B, Lw, rate))
        with torch.cuda.device(self._device):
            _native.check("iris_time_stretch_forward_window", lib.iris_time_stretch_forward_window(
                self._handle, _ptr(wav), B, Lw, ctypes.c_int64(int(origin)), int(bool(final)), ctypes.c_double(rate), ctypes.c_int64(int(u)),
                _ptr(state), _ptr(out), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    def open_session(self, rate) -> "StretchSession":
        """A ``StretchSession`` at ``rate`` for one utterance (or a batch of equal lengths) that arrives piece by piece."""
        return StretchSession(self, check_rate(rate))


class StretchSession(_WindowSession):
    """Pushed input for a time stretch at ONE rate (``_WindowSession``: ``push`` pieces, ``flush`` at the end); stretched samples
    leave as soon as every frame under them is computable.  The concatenation of everything returned equals ``forward_device``
    of the concatenated pieces bit for bit: the phase is an exact integer sum carried in the state, an output frame depends on
    two input rows alone, and an output sample on its own ``n_fft / hop`` output frames, of which the state keeps the last
    ``n_fft / hop - 1``.

    ``ts``: a ``TimeStretch``, or any object with ``hop_length``, ``window_plan(rate, origin, Lw, final, u)``,
    ``forward_window(wav, rate, origin, final, u, state)`` and ``new_state(B)``.  Each push runs ONE window over the whole
    frames that are buffered, carries ``u`` (the next output frame) and the state tensor, and keeps the input from the plan's
    ``keep_from`` on.  Pieces may be empty -- a piece shorter than the halo settles nothing and launches nothing -- and
    ``flush`` returns what was waiting for context.  A piece need not be whole frames; the utterance must be by ``flush``."""

    def __init__(self, ts, rate: float):
        super().__init__()
        self._ts, self.rate = ts, float(rate)
        self.hop_length = int(ts.hop_length)
        self._emitted = 0
        self._u = 0
        self._state = None

    @property
    def samples_emitted(self) -> int:
        return self._emitted

    @property
    def frames_computed(self) -> int:
        """``u``: the next output frame."""
        return self._u

    def _window(self, final: bool) -> Tuple[torch.Tensor, int]:
        hop, held = self.hop_length, self._total - self._base
        if final and held % hop:
            raise ValueError(f"the utterance has {self._total} samples, no multiple of hop_length = {hop}; nothing is padded silently")
        Lw = held // hop * hop
        u_hi, lo, count, keep = self._ts.window_plan(self.rate, self._base, Lw, final, self._u)
        if u_hi == self._u and count == 0:
            return self._empty(), self._base                  # no frame and no sample: no launch
        if count and lo != self._emitted:
            raise RuntimeError(f"the window [{self._base}, {self._base + Lw}) emits samples from {lo} on, but {self._emitted} is due")
        if self._state is None:
            self._state = self._ts.new_state(int(self._buf.shape[0]))
        out = self._ts.forward_window(self._buf[:, :Lw], self.rate, self._base, final, self._u, self._state)
        self._emitted += count
        self._u = u_hi
        return out, min(keep, self._base + Lw)                # an origin at or below keep_from, a multiple of hop, inside the window


class StretchAt:
    """``ts`` bound to a rate: ``forward_device(wav, lengths=) -> (out, counts)`` and ``out_samples(L)``."""

    def __init__(self, ts: TimeStretch, rate: float):
        self.ts, self.rate = ts, rate

    @property
    def hop_length(self) -> int:
        return self.ts.hop_length

    def out_samples(self, L: int) -> int:
        return self.ts.out_samples(L, self.rate)

    def forward_device(self, wav, lengths=None):
        return self.ts.forward_device(wav, self.rate, lengths=lengths)

    def chunked(self) -> "ChunkedStretch":
        """This stretch as the opt-in a pipeline looks for before it streams (``ChunkedStretch``)."""
        return ChunkedStretch(self)


class ChunkedStretch(StretchAt):
    """``ts.at(rate)`` with the promise a streaming pipeline asks for: ``MelToWavePipeline(..., stretch=ts.at(rate).chunked())``
    lets ``stream`` and ``session`` run, every fp32 chunk -- the chunked denoiser's, where there is one -- going through one
    ``StretchSession``.  The opt-in is explicit because the pieces such a pipeline yields no longer have the chunks' lengths;
    a plain ``ts.at(rate)`` keeps refusing.  ``forward_device`` and ``out_samples`` are the whole-utterance ones."""

    chunked_sessions = True

    def __init__(self, at: StretchAt):
        super().__init__(at.ts, at.rate)

    def open_session(self) -> "StretchSession":
        return StretchSession(self.ts, self.rate)


def semitone_ratio(n_steps: float, max_den: int = 640) -> Fraction:
    """``2 ** (n_steps / 12)`` as the nearest fraction ``p / q`` with ``q <= max_den``: the frequency ratio of a shift by
    ``n_steps`` semitones in a form a polyphase resampler takes."""
    return Fraction(2.0 ** (float(n_steps) / 12.0)).limit_denominator(int(max_den))


def pitch_rates(ratio: Fraction, lo: int = 4000, hi: int = 192000) -> Tuple[int, int]:
    """``(rate_in, rate_out)`` for ``Resampler``: integer rates with ``rate_out / rate_in = q / p`` for ``ratio = p / q`` -- the
    resampler reduces them by their gcd and only the ratio matters -- scaled into ``[lo, hi]``, the range it accepts."""
    p, q = ratio.numerator, ratio.denominator
    m = -(-lo // min(p, q))
    if m * max(p, q) > hi:
        raise ValueError(f"no multiple of {p} / {q} lies inside [{lo}, {hi}] Hz: the ratio is too far from 1")
    return m * p, m * q


def pitch_compose(stretched: np.ndarray, counts, L: int, resample) -> np.ndarray:
    """The tail of the pitch path on the host, for tests: ``resample(stretched, counts)`` cropped or zero-padded to ``L``."""
    y = np.asarray(resample(stretched, counts))
    out = np.zeros((y.shape[0], L), dtype=y.dtype)
    n = min(L, y.shape[1])
    out[:, :n] = y[:, :n]
    return out


_pitch_resamplers: dict = {}


def pitch_resampler(ratio: Fraction, device):
    """The ``Resampler`` of ``pitch_shift_device`` for ``ratio = p / q`` (``up = q``, ``down = p``), built once per device."""
    from .resample import Resampler
    key = (ratio, str(device))
    if key not in _pitch_resamplers:
        rate_in, rate_out = pitch_rates(ratio)
        _pitch_resamplers[key] = Resampler(rate_out, rate_in=rate_in, device=device)
    return _pitch_resamplers[key]


def pitch_shift_device(ts: TimeStretch, wav, n_steps: float, lengths=None, max_den: int = 640) -> torch.Tensor:
    """``wav [B, L]`` shifted by ``n_steps`` semitones at its own length, ``[B, L]`` on the device: with ``p / q =
    semitone_ratio(n_steps)``, (1) ``ts.forward_device(wav, q / p, lengths=)``, (2) ``Resampler.forward(..., lengths=counts,
    row_scale=1)`` with ``up = q``, ``down = p``, (3) crop or zero-pad to ``L``.  A ragged item's samples past its own end stay 0.

    This is the structure of ``librosa.effects.pitch_shift``, not its samples: the resampling filter is this project's
    Kaiser-windowed sinc (``iris.resample``), not librosa's soxr."""
    ratio = semitone_ratio(n_steps, max_den)
    wav = ts._wav_on_device(wav)
    L = int(wav.shape[1])
    y, counts = ts.forward_device(wav, ratio.denominator / ratio.numerator, lengths=lengths)
    if ratio != 1:                                            # p == q: nothing to convert
        y = pitch_resampler(ratio, y.device).forward(y, lengths=counts, row_scale=1)
    out = torch.zeros((wav.shape[0], L), dtype=torch.float32, device=y.device)
    n = min(L, int(y.shape[1]))
    out[:, :n] = y[:, :n]
    return out
