"""Log-mel -> waveform on the device without a trained vocoder (``iris_griffin_lim_*``, csrc/griffin_lim.h): the reference's
``--use_griffin_lim`` path (``scripts/synthesize.py:174-194``) -- ``exp(clip(logmel, -11.513, 2.0))``, librosa 0.11's
``feature.inverse.mel_to_stft(power=1.0)`` and ``griffinlim(S, n_iter=60, hop_length=256, win_length=1024)``.

The arithmetic the stage commits to (librosa cannot be imported where this project is built, so parity is unpinned; the tests
hold the device to a float64 numpy restatement of these rules, ``tests/griffin_lim_restatement.py``):

  * mel inversion, per frame: ``min ||fb x - m||, x >= 0`` started like librosa from the clipped least-squares solution
    ``max(pinv(fb) m, 0)``, then ``nnls_iters`` projected-gradient steps of size ``1 / lambda_max(fb fb^T)`` in place of
    L-BFGS-B (each step cannot increase the residual); ``pinv`` and the step are computed here in float64;
  * phase retrieval: librosa's fast Griffin-Lim -- ``c = S a / (|a| + tiny)`` with ``a = r - momentum / (1 + momentum) r_prev``
    -- from a caller-supplied (or seeded) start phase; ``stft`` / ``istft`` are centred with zero padding, on the mel
    front-end's window, and the output has ``hop * (T - 1)`` samples.

``2 * n_iter + 2`` launches: the inversion, ``n_iter`` times (inverse STFT, STFT with the phase update), one inverse STFT.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _NativeModel, _ptr, _stream
from .mel import MelFrontend

DEFAULT_NNLS_ITERS = 32        # DESIGN.md, "Griffin-Lim": the residual table this is read from


def start_phase(B: int, n_bins: int, T: int, seed: int = 1337) -> np.ndarray:
    """``phi0 [B, n_bins, T]`` float64: ``2 pi * numpy.random.default_rng(seed).random((B, n_bins, T))``."""
    return 2.0 * np.pi * np.random.default_rng(seed).random((B, n_bins, T))


def pack_phase(phi0: np.ndarray) -> np.ndarray:
    """``phi0 [B, n_bins, T]`` -> what the device reads: fp32 ``[B, T, n_bins, 2]``, cos and sin taken in float64 and rounded once."""
    phi = np.transpose(np.asarray(phi0, dtype=np.float64), (0, 2, 1))
    return np.ascontiguousarray(np.stack([np.cos(phi), np.sin(phi)], axis=-1).astype(np.float32))


class GriffinLim(_NativeModel):
    """The Griffin-Lim vocoder with fixed parameters (the reference script's), resident on one GPU.  Usable as the ``vocode``
    of ``MelToWavePipeline``; ``whole_utterance`` tells the pipeline that a mel cannot be cut into chunks (every frame's
    phase depends on the whole item) and that the output has ``hop * (T - 1)`` samples."""

    _abi_name = "griffin_lim"
    whole_utterance = True

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024,
                 n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0, n_iter: int = 60, momentum: float = 0.99,
                 nnls_iters: int = DEFAULT_NNLS_ITERS):
        super().__init__()
        self._mel = MelFrontend(sample_rate, n_fft, hop_length, win_length, n_mels, fmin, fmax)     # validates the shared fields
        for name, v in (("n_iter", n_iter), ("nnls_iters", nnls_iters)):
            if int(v) != v or int(v) < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"0 <= momentum < 1 is required, got {momentum}")
        self.sample_rate, self.n_fft, self.hop_length = self._mel.sample_rate, self._mel.n_fft, self._mel.hop_length
        self.win_length, self.n_mels, self.fmin, self.fmax = self._mel.win_length, self._mel.n_mels, self._mel.fmin, self._mel.fmax
        self.n_iter, self.nnls_iters, self.momentum = int(n_iter), int(nnls_iters), float(momentum)
        self._inverse = None

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    def get_config(self) -> dict:
        return {**self._mel.get_config(), "n_iter": self.n_iter, "momentum": self.momentum, "nnls_iters": self.nnls_iters}

    def inversion_tables(self) -> Tuple[np.ndarray, float]:
        """``(P, step)``: ``pinv(fb) [n_bins, n_mels]`` computed in float64 from the designed fp32 filterbank and rounded once,
        and ``1 / lambda_max(fb fb^T)`` in float64."""
        if self._inverse is None:
            fb = self._mel.design()[1].astype(np.float64)
            step = 1.0 / float(np.linalg.eigvalsh(fb @ fb.T)[-1])
            self._inverse = (np.ascontiguousarray(np.linalg.pinv(fb).astype(np.float32)), step)
        return self._inverse

    def native_config(self, with_step: bool = True) -> "_native.GriffinLimConfig":
        """``with_step=False``: a placeholder step, for the queries that need no filterbank (and so no design call)."""
        step = self.inversion_tables()[1] if with_step else 1.0
        return _native.GriffinLimConfig(self.sample_rate, self.n_fft, self.hop_length, self.win_length, self.n_mels, self.n_iter,
                                        self.fmin, 0.0 if self.fmax is None else self.fmax, self.nnls_iters, 0, self.momentum, step)

    # -- host-only queries -------------------------------------------------------------------
    def _query(self, what: str, B: int, T: int, ctype) -> int:
        lib = _native.load()
        out = ctype()
        cfg = self.native_config(with_step=False)
        name = f"iris_griffin_lim_{what}"
        _native.check(name, getattr(lib, name)(ctypes.byref(cfg), int(B), int(T), ctypes.byref(out)))
        return int(out.value)

    def launch_count(self, B: int, T: int) -> int:
        """Kernel launches of one ``forward_device``: ``2 * n_iter + 2`` (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, T, ctypes.c_int32)

    def workspace_bytes(self, B: int, T: int) -> int:
        return self._query("workspace_bytes", B, T, ctypes.c_uint64)

    def samples_of(self, frames: int) -> int:
        return self.hop_length * (int(frames) - 1)

    def design(self) -> dict:
        """The fp32 tables the handle uploads (``iris_griffin_lim_design``: host only): ``dft`` and ``idft`` ``[2, n_bins,
        n_fft]``, ``fb [n_mels, n_bins]`` and ``wsq [n_fft]``."""
        lib = _native.load()
        cfg = self.native_config(with_step=False)
        bins = ctypes.c_int32()
        _native.check("iris_griffin_lim_design", lib.iris_griffin_lim_design(ctypes.byref(cfg), ctypes.byref(bins), None, 0, None, 0,
                                                                             None, 0, None, 0))
        out = {"dft": np.empty((2, bins.value, self.n_fft), dtype=np.float32), "idft": np.empty((2, bins.value, self.n_fft), dtype=np.float32),
               "fb": np.empty((self.n_mels, bins.value), dtype=np.float32), "wsq": np.empty(self.n_fft, dtype=np.float32)}
        fp = ctypes.POINTER(ctypes.c_float)
        args = []
        for key in ("dft", "idft", "fb", "wsq"):
            args += [out[key].ctypes.data_as(fp), ctypes.c_uint64(out[key].size)]
        _native.check("iris_griffin_lim_design", lib.iris_griffin_lim_design(ctypes.byref(cfg), ctypes.byref(bins), *args))
        return out

    # -- the native handle -------------------------------------------------------------------
    def _upload_blob(self) -> np.ndarray:
        return self.inversion_tables()[0].reshape(-1)

    def forward_device(self, logmel, phase0=None, seed: int = 1337) -> torch.Tensor:
        """``logmel [B, n_mels, T]`` fp32, host or device, ``T >= 2`` -> the waveform ``[B, hop * (T - 1)]`` on the device.
        ``phase0 [B, n_bins, T]`` (radians, any float type, host): the start phase; None draws
        ``2 pi * numpy.random.default_rng(seed).random((B, n_bins, T))``.  A device tensor ``[B, T, n_bins, 2]`` fp32 is taken
        as the packed cos / sin (``pack_phase``) and not copied.  Asynchronous on the current stream; two calls agree bit for
        bit and item b is its batch-of-one call on ``phase0[b]``."""
        if not isinstance(logmel, torch.Tensor):
            logmel = torch.from_numpy(np.ascontiguousarray(np.asarray(logmel, dtype=np.float32)))
        if logmel.dim() != 3 or logmel.shape[1] != self.n_mels or logmel.dtype != torch.float32:
            raise ValueError(f"expected a log-mel [B, {self.n_mels}, T] float32, got {logmel.dtype} {tuple(logmel.shape)}")
        B, T = int(logmel.shape[0]), int(logmel.shape[2])
        if T < 2:
            raise ValueError(f"T = {T}: Griffin-Lim needs at least 2 frames (the output has hop * (T - 1) samples)")
        packed_shape = (B, T, self.n_bins, 2)
        if isinstance(phase0, torch.Tensor) and phase0.is_cuda:
            if tuple(phase0.shape) != packed_shape or phase0.dtype != torch.float32:
                raise ValueError(f"a device phase0 must be the packed cos / sin {list(packed_shape)} float32, got {phase0.dtype} {tuple(phase0.shape)}")
            packed = phase0
        else:
            if phase0 is None:
                phase0 = start_phase(B, self.n_bins, T, seed)
            phase0 = phase0.detach().cpu().numpy() if isinstance(phase0, torch.Tensor) else np.asarray(phase0)
            if phase0.shape != (B, self.n_bins, T):
                raise ValueError(f"expected phase0 [{B}, {self.n_bins}, {T}], got {phase0.shape}")
            packed = torch.from_numpy(pack_phase(phase0))
        lib = self._ensure()
        logmel = logmel.to(self._device).contiguous()
        packed = packed.to(self._device).contiguous()
        wav = torch.empty((B, self.samples_of(T)), dtype=torch.float32, device=self._device)
        if B == 0:
            return wav
        ws = self._ws(B, T)
        with torch.cuda.device(self._device):
            _native.check("iris_griffin_lim_forward", lib.iris_griffin_lim_forward(
                self._handle, _ptr(logmel), _ptr(packed), B, T, _ptr(wav), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return wav

    def magnitudes(self, B: int, T: int) -> torch.Tensor:
        """``S [B, n_bins, T]``: the inverted magnitudes the last ``forward_device`` of shape (B, T) left at the start of its
        workspace (``[B][T][Ks]``, ``Ks`` = ``n_bins`` rounded up to 4).  For tests."""
        ks = (self.n_bins + 3) // 4 * 4
        s = self._workspace[:B * T * ks * 4].view(torch.float32).view(B, T, ks)
        return s[:, :, :self.n_bins].transpose(1, 2).contiguous()

    def __call__(self, mel, phase0=None, seed: int = 1337) -> np.ndarray:
        """``[n_mels, T]`` -> ``[samples]``; ``[B, n_mels, T]`` -> ``[B, samples]``, on the host (as ``HiFiGANVocoder.infer``)."""
        mel = mel.detach().cpu().numpy() if isinstance(mel, torch.Tensor) else np.asarray(mel, dtype=np.float32)
        if mel.ndim == 2:
            return self.forward_device(mel[None], None if phase0 is None else np.asarray(phase0)[None], seed)[0].cpu().numpy()
        return self.forward_device(mel, phase0, seed).cpu().numpy()
