"""Bias denoiser on the device (``iris_denoiser_*``, csrc/denoiser.h): the post-processing step HiFiGAN users run behind the
vocoder.  A GAN vocoder adds a constant hum; its magnitude spectrum -- the *bias*, measured on the vocoder's output for a silent
mel -- is subtracted, times ``strength``, from the magnitudes of every utterance, the phase is kept, and the result is
transformed back.  The reference has no such step, so the contract is the math below, held by a float64 numpy restatement
(``tests/denoiser_restatement.py``).

With ``N = n_fft``, ``H = hop_length`` and the Griffin-Lim stage's transforms unchanged (``iris.griffin_lim``: frame t covers
samples ``[t H - N / 2, t H + N / 2)``, 0 outside; the mel front-end's window and tables): a waveform of ``L = H M`` samples
(``M`` mel frames, what a vocoder emits) has ``T = M + 1`` frames, and per frame t and bin k of ``a = stft(wav)``

    ``mag = sqrtf(re re + im im);  g = fmaxf(fmaf(-strength, bias[k], mag), 0);  scale = mag > 0 ? g / mag : 0``
    ``c = (scale re, scale im);  out = istft(c)``

in fp32.  ``strength = 0`` reproduces ``istft(stft(wav))``; a ``strength`` at or above ``max(mag / bias)`` gives exactly 0.
The bias estimate of a waveform ``[1, L]`` is the mean of ``mag[t, k]`` over the frames whose window lies wholly inside the
signal, summed in fp64 in ascending t and rounded once.

A forward is 2 launches -- the STFT with the subtraction as its epilogue and the inverse STFT -- on the current stream; the
estimator is 2 as well.  ``forward_device(lengths=)`` takes a ragged batch: item b is bit for bit its batch-of-one call and the
rest of its row is 0.  ``MelToWavePipeline(..., denoiser=Denoiser(...))`` runs it between the vocoder and the output stage.

Streaming: ``Denoiser.open_session()`` takes the waveform piece by piece (``DenoiserSession``: one ``forward_window`` per push,
the same 2 launches on a window of the utterance) and its output equals ``forward_device`` of the whole bit for bit;
``dn.chunked()`` (``ChunkedDenoiser``) is the opt-in with which a pipeline's ``stream`` / ``session`` run it behind the vocoder.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, Optional

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _take_shapes, _wave
from ._window_session import _RangeSession
from .vae import _lengths_on, check_lengths


class Denoiser(_DeviceStage):
    """Spectral bias subtraction with fixed transform parameters, resident on one GPU (``device``, or the current one); the
    handle is built on first use.  ``bias``: ``[n_fft / 2 + 1]`` finite, non-negative magnitudes (host), or None for zeros --
    ``set_bias`` / ``from_vocoder`` install an estimate later.  ``strength``: the default multiple that is subtracted."""

    _abi_name = "denoiser"

    def __init__(self, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024, strength: float = 0.1, bias=None,
                 device: Optional[torch.device] = None):
        super().__init__(device)
        for name, v in (("n_fft", n_fft), ("hop_length", hop_length), ("win_length", win_length)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)
        self.strength = self._check_strength(strength)
        self._bias_host = None if bias is None else self._check_bias(bias)
        self._bias_dev: Optional[torch.Tensor] = None

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    @staticmethod
    def _check_strength(strength) -> float:
        s = float(strength)
        if not math.isfinite(s) or s < 0.0:
            raise ValueError(f"strength must be finite and not negative, got {strength!r}")
        return s

    def _check_bias(self, bias) -> np.ndarray:
        arr = np.ascontiguousarray(np.asarray(bias, dtype=np.float32))
        if arr.shape != (self.n_bins,):
            raise ValueError(f"expected a bias [{self.n_bins}], got shape {arr.shape}")
        if not np.isfinite(arr).all() or (arr < 0).any():
            raise ValueError("a bias is a magnitude spectrum: finite and not negative")
        return arr

    def get_config(self) -> dict:
        return {"n_fft": self.n_fft, "hop_length": self.hop_length, "win_length": self.win_length, "strength": self.strength}

    def native_config(self) -> "_native.MelFrontendConfig":
        """The front-end's config the C side takes; only the three transform fields matter (the rest pass its checks)."""
        return _native.MelFrontendConfig(22050, self.n_fft, self.hop_length, self.win_length, 1, 0, 0.0, 0.0)

    # -- host-only queries -------------------------------------------------------------------
    def launch_count(self, B: int, L: int) -> int:
        """Kernel launches of one ``forward_device``: 2 (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L)

    def estimate_launch_count(self, L: int) -> int:
        """Kernel launches of one ``estimate_bias``: 2 (likewise)."""
        return self._query("estimate_launch_count", L)

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def _workspace_layout(self, B: int, L: int):
        """``({buffer: (offset, shape)}, floats)``: ``DnWorkspace`` (csrc/iris_denoiser.hip) restated -- c ``[B, T, Qp]`` and the
        items' frame counts ``[B]`` (int32) in ``WsTaker`` order.  Host only."""
        return _take_shapes({"c": (B, L // self.hop_length + 1, (self.n_fft + 2 + 7) // 8 * 8), "frames": (B,)})

    def _read_c(self, B: int, L: int) -> torch.Tensor:
        """Test-only: the view ``c [B, T, Qp]`` of the workspace as the last ``forward_device`` of shape (B, L) left it."""
        off, shape = self._workspace_layout(B, L)[0]["c"]
        return self._workspace.view(torch.float32)[off:off + int(np.prod(shape))].view(shape)

    def _read_frames(self, B: int, L: int) -> torch.Tensor:
        """Test-only: the view ``frames [B]`` (int32) of the workspace, the items' T_b as the last ``forward_device`` of shape
        (B, L) stored them (a ``forward_window`` of shape (B, Lw) stores its frame count there)."""
        off, shape = self._workspace_layout(B, L)[0]["frames"]
        return self._workspace.view(torch.int32)[off:off + int(np.prod(shape))].view(shape)

    def _read_mag(self, L: int) -> torch.Tensor:
        """Test-only: the view ``mag [T, Ks]`` of the workspace as the last ``estimate_bias`` of ``L`` samples left it: the
        estimator keeps its magnitudes where a forward keeps c, at offset 0, in rows of ``Ks`` = the bins rounded up to 4."""
        off = self._workspace_layout(1, L)[0]["c"][0]
        T, ks = L // self.hop_length + 1, (self.n_bins + 3) // 4 * 4
        return self._workspace.view(torch.float32)[off:off + T * ks].view(T, ks)

    def _read_window_c(self, B: int, Lw: int, frames: int) -> torch.Tensor:
        """Test-only: the view ``c [B, frames, Qp]`` as the last ``forward_window`` of shape (B, Lw) left it -- in the window's
        own coordinates, ``frames`` = f_hi - f_lo rows per item (not the ``Lw / hop + 1`` the buffer has room for)."""
        off, (_, T, qp) = self._workspace_layout(B, Lw)[0]["c"]
        assert 0 <= frames <= T
        return self._workspace.view(torch.float32)[off:off + B * frames * qp].view(B, frames, qp)

    # -- the native handle -------------------------------------------------------------------
    def _upload_blob(self) -> np.ndarray:
        return np.zeros(0, dtype=np.float32) if self._bias_host is None else self._bias_host

    def _create(self, lib, weights, n_weights, handle_ref) -> int:
        cfg = self.native_config()
        return lib.iris_denoiser_create(ctypes.byref(cfg), weights if n_weights.value else None, handle_ref)

    def close(self) -> None:
        """Frees the native handle and the workspace; the next call builds them again (with the host bias of the constructor
        or the last host ``set_bias``; a device estimate has to be installed again)."""
        super().close()
        self._bias_dev = None

    # -- the bias ----------------------------------------------------------------------------
    @property
    def bias(self) -> torch.Tensor:
        """The bias in use, a device tensor ``[n_bins]`` fp32."""
        self._ensure()
        if self._bias_dev is None:
            host = np.zeros(self.n_bins, np.float32) if self._bias_host is None else self._bias_host
            self._bias_dev = torch.from_numpy(host).to(self._device)
        return self._bias_dev

    def set_bias(self, bias) -> None:
        """Installs ``bias [n_bins]``: a host array (checked: finite, not negative) or an fp32 device tensor, e.g. what
        ``estimate_bias`` returned, which is copied device to device on the current stream and never visits the host."""
        lib = self._ensure()
        if isinstance(bias, torch.Tensor) and bias.is_cuda:
            if tuple(bias.shape) != (self.n_bins,) or bias.dtype != torch.float32:
                raise ValueError(f"a device bias must be [{self.n_bins}] float32, got {bias.dtype} {tuple(bias.shape)}")
            dev = bias.to(self._device).contiguous().clone()
        else:
            self._bias_host = self._check_bias(bias.numpy() if isinstance(bias, torch.Tensor) else bias)
            dev = torch.from_numpy(self._bias_host).to(self._device)
        with torch.cuda.device(self._device):
            _native.check("iris_denoiser_set_bias", lib.iris_denoiser_set_bias(self._handle, _ptr(dev), _stream(self._device)))
        self._bias_dev = dev

    def _wav_on_device(self, wav) -> torch.Tensor:
        return _wave(wav, self.hop_length, "a vocoder emits hop_length samples per mel frame")

    def estimate_bias(self, wav) -> torch.Tensor:
        """``wav [1, L]`` (or ``[L]``), host or device: the vocoder's output for a silent mel -> its bias, a device tensor
        ``[n_bins]``: per bin the mean magnitude over the frames whose window lies wholly inside the signal (``ValueError``
        when there is none).  Two launches on the current stream; nothing is installed -- hand the result to ``set_bias``."""
        if not isinstance(wav, torch.Tensor):
            wav = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32)))
        wav = self._wav_on_device(wav[None] if wav.dim() == 1 else wav)
        if wav.shape[0] != 1:
            raise ValueError(f"expected one waveform [1, L], got a batch of {wav.shape[0]}")
        L, edge = int(wav.shape[1]), -(-(self.n_fft // 2) // self.hop_length)
        if L // self.hop_length + 1 - edge <= edge:
            raise ValueError(f"L = {L}: no frame of n_fft = {self.n_fft} lies wholly inside the signal")
        lib = self._ensure()
        wav = wav.to(self._device).contiguous()
        out = torch.empty((self.n_bins,), dtype=torch.float32, device=self._device)
        ws = self._ws(1, L)
        with torch.cuda.device(self._device):
            _native.check("iris_denoiser_estimate_bias", lib.iris_denoiser_estimate_bias(
                self._handle, _ptr(wav), L, _ptr(out), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    @classmethod
    def from_vocoder(cls, vocode: Callable, n_mels: int = 80, frames: int = 88, level: float = math.log(1e-5), **cfg) -> "Denoiser":
        """A denoiser whose bias is estimated from ``vocode`` itself: the vocoder (``GeneratorEngine.forward``, or any callable
        or object with ``forward_device`` mapping a device mel ``[1, n_mels, frames]`` to ``[1, L]``) runs on a constant mel at
        ``level`` -- the front-end's floor ``log(1e-5)``, what silence reads as -- and ``estimate_bias`` of its output is
        installed.  ``**cfg`` goes to the constructor."""
        dn = cls(**cfg)
        dn._ensure()
        mel = torch.full((1, int(n_mels), int(frames)), float(level), dtype=torch.float32, device=dn._device)
        wav = getattr(vocode, "forward_device", vocode)(mel)
        if not isinstance(wav, torch.Tensor):
            wav = torch.from_numpy(np.asarray(wav, dtype=np.float32))
        dn.set_bias(dn.estimate_bias(wav.float().reshape(1, -1)))
        return dn

    # -- the forward -------------------------------------------------------------------------
    def forward_device(self, wav, lengths=None, strength: Optional[float] = None) -> torch.Tensor:
        """``wav [B, L]`` fp32, host or device, ``L`` a multiple of ``hop_length`` -> the denoised waveform ``[B, L]`` on the
        device (a new tensor).  ``strength``: this call's multiple instead of the constructor's.  Asynchronous on the current
        stream, 2 launches, safe inside a graph capture once the workspace exists; two calls agree bit for bit.

        ``lengths``: item b's MEL frames ``M_b`` (it owns ``hop_length * M_b`` samples) -- a host sequence of integers in
        ``[0, L / hop_length]`` (``ValueError`` otherwise, before any device work) or an int32 device tensor ``[B]``, which the
        host never reads (the kernel clamps it) and which may change between the replays of a captured graph.
        ``out[b, :hop_length * M_b]`` is bit for bit the call on ``wav[b:b + 1, :hop_length * M_b]``, the rest of the row is 0,
        and nothing of ``wav`` past an item's own samples is read."""
        wav = self._wav_on_device(wav)
        strength = self.strength if strength is None else self._check_strength(strength)
        B, L = int(wav.shape[0]), int(wav.shape[1])
        if lengths is not None:
            lengths = check_lengths(lengths, B, L // self.hop_length, 1)
        lib = self._ensure()
        wav = wav.to(self._device).contiguous()
        if lengths is not None:
            lengths = _lengths_on(lengths, self._device)
        out = torch.empty((B, L), dtype=torch.float32, device=self._device)
        if B == 0 or L == 0:
            return out
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_denoiser_forward", lib.iris_denoiser_forward(
                self._handle, _ptr(wav), B, L, _ptr(lengths), ctypes.c_float(strength), _ptr(out), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    def __call__(self, wav, strength: Optional[float] = None) -> np.ndarray:
        """``[L]`` -> ``[L]``; ``[B, L]`` -> ``[B, L]``, numpy in and numpy out (as ``HiFiGANVocoder.infer``)."""
        wav = wav.detach().cpu().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav, dtype=np.float32)
        if wav.ndim == 1:
            return self.forward_device(wav[None], strength=strength)[0].cpu().numpy()
        return self.forward_device(wav, strength=strength).cpu().numpy()

    # -- windows of an utterance -------------------------------------------------------------
    def window_range(self, origin: int, Lw: int, final: bool):
        """``(out_lo, out_count)``: the samples of an utterance that the window ``[origin, origin + Lw)`` settles -- those whose
        ``n_fft / hop_length`` frames each lie inside the window or do not exist (``iris_denoiser_window_range``: the finality
        rule, written down on the C side only).  ``final``: the window ends where the utterance ends.  Host only."""
        return self._window_range(origin, Lw, final)

    def window_workspace_bytes(self, B: int, Lw: int) -> int:
        return self._query("window_workspace_bytes", B, Lw)

    def window_launch_count(self, B: int, Lw: int, origin: int, final: bool) -> int:
        """Kernel launches of one ``forward_window``: 2, or 0 where the window settles nothing (a dry run on the host)."""
        return self._query("window_launch_count", B, Lw, origin, bool(final))

    def forward_window(self, wav, origin: int, final: bool, strength: Optional[float] = None) -> torch.Tensor:
        """``wav [B, Lw]`` fp32 = samples ``[origin, origin + Lw)`` of an utterance (both multiples of ``hop_length``) -> the
        samples ``window_range(origin, Lw, final)`` names, ``[B, out_count]`` on the device, each bit for bit the sample
        ``forward_device`` of the whole utterance returns there.  Stateless, asynchronous, 2 launches; none when
        ``out_count == 0``.  ``DenoiserSession`` keeps the bookkeeping."""
        wav = self._wav_on_device(wav)
        strength = self.strength if strength is None else self._check_strength(strength)
        B, Lw = int(wav.shape[0]), int(wav.shape[1])
        count = self.window_range(origin, Lw, final)[1]
        lib = self._ensure()
        out = torch.empty((B, count), dtype=torch.float32, device=self._device)
        if B == 0 or count == 0:
            return out
        wav = wav.to(self._device).contiguous()
        ws = self._ws(B, Lw)                                     # a window's workspace is that of a forward of its shape
        with torch.cuda.device(self._device):
            _native.check("iris_denoiser_forward_window", lib.iris_denoiser_forward_window(
                self._handle, _ptr(wav), B, Lw, ctypes.c_int64(int(origin)), int(bool(final)), ctypes.c_float(strength), _ptr(out),
                _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    def open_session(self, strength: Optional[float] = None) -> "DenoiserSession":
        """A ``DenoiserSession`` for one utterance (or a batch of equal lengths) that arrives piece by piece."""
        return DenoiserSession(self, strength=None if strength is None else self._check_strength(strength))

    def chunked(self) -> "ChunkedDenoiser":
        """This denoiser as the opt-in a pipeline looks for before it streams (``ChunkedDenoiser``)."""
        return ChunkedDenoiser(self)


class DenoiserSession(_RangeSession):
    """Pushed input for a denoiser (``_WindowSession``: ``push`` pieces ``[B, hop * m]``, ``flush`` at the end).  The
    concatenation of everything returned equals ``forward_device`` of the concatenated pieces bit for bit: a sample is the sum
    over its ``n_fft / hop`` frames, each a fixed-order sum over its own ``n_fft`` samples, so it is final once those samples
    have arrived -- or lie past an end of the utterance, where the one-shot reads zeros too (``Denoiser.window_range``).

    ``dn``: a ``Denoiser``, or any object with ``hop_length``, ``window_range(origin, Lw, final) -> (out_lo, out_count)`` and
    ``forward_window(wav, origin, final, strength=) -> [B, out_count]``.  A window starts on a multiple of ``hop_length`` and
    the session keeps only the input tail the next one needs: ``halo = (left, right)`` samples, asked of ``window_range`` (768
    and 768 at 1024 / 256, three frames each; 128 and 128 at 256 / 128), so ``samples_buffered`` stays within ``left + right``
    plus the piece just pushed, and the frames inside that tail are the only work done twice.

    Latency: sample s leaves with the push that brings ``samples_received`` to ``s + right``.  Pieces therefore do not have
    the lengths of the pushes: the first is short by ``right`` samples (or empty, and then nothing is launched) and ``flush``
    returns the last ``right``."""

    def __init__(self, dn, strength: Optional[float] = None):
        self.strength, self.hop_length = strength, int(dn.hop_length)
        super().__init__(dn, step=self.hop_length, piece_multiple=self.hop_length)

    def _forward_window(self, final: bool) -> torch.Tensor:
        return self._stage.forward_window(self._buf, self._base, final, strength=self.strength)


class ChunkedDenoiser:
    """``dn`` with the promise a streaming pipeline asks for: ``MelToWavePipeline(..., denoiser=ChunkedDenoiser(dn))`` -- or
    ``dn.chunked()`` -- lets ``stream`` and ``session`` run, every chunk of the vocoder going through one ``DenoiserSession``.
    The opt-in is explicit because the pieces such a pipeline yields are no longer all ``[B, hop * chunk]``; a plain
    ``Denoiser`` keeps refusing.  ``forward_device``, ``bias`` and ``strength`` are ``dn``'s."""

    chunked_sessions = True

    def __init__(self, dn):
        self.dn = dn

    @property
    def bias(self):
        return self.dn.bias

    @property
    def strength(self):
        return self.dn.strength

    @property
    def hop_length(self) -> int:
        return self.dn.hop_length

    def forward_device(self, wav, lengths=None, strength: Optional[float] = None):
        return self.dn.forward_device(wav, lengths=lengths, strength=strength)

    def open_session(self, strength: Optional[float] = None) -> DenoiserSession:
        return self.dn.open_session(strength=strength)
