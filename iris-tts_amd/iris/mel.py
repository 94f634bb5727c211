"""Waveform -> log-mel on the device (``iris_mel_frontend_*``, csrc/mel_frontend.h): the reference's
``compute_mel_spectrogram`` (``src/iris/data.py:25-67``), the one step between a recorded file's samples and the posterior
side of ``iris.vae`` (``reconstruct``, ``vae_losses``) and ``MelToWavePipeline.resynthesize``.

Semantics are librosa 0.11's ``melspectrogram(y, sr, n_fft, hop_length, win_length, n_mels, fmin, fmax, power=1.0)`` with
that version's defaults, then ``log(max(mel, 1e-5))``:

  * ``center=True``, ``pad_mode="constant"``: ``n_fft / 2`` zeros on each side; ``n`` samples give ``1 + n // hop`` frames;
  * a periodic Hann window of ``win_length``, zero-padded symmetrically to ``n_fft``;
  * ``|rfft|`` (not squared) over ``n_fft / 2 + 1`` bins;
  * ``librosa.filters.mel(htk=False, norm="slaney")``; ``fmax=None`` means ``sample_rate / 2``.

librosa cannot be imported where this project is built, so parity is unpinned, as for ``iris.vae``: the tests hold the device
to a float64 numpy restatement of the rules above (``tests/mel_restatement.py``).

The whole stage is one launch: the windowed DFT runs as an implicit-GEMM convolution over the samples viewed as rows of
``hop`` floats, the magnitudes stay in LDS, the filterbank is a second GEMM on that tile, and the log-mel is stored
channels-first ``[B, n_mels, T]``.  Samples may be int16 (a 16-bit WAV as read): they are taken as ``x / 32768`` on the device.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream


class MelFrontend(_DeviceStage):
    """``compute_mel_spectrogram`` with fixed parameters, resident on one GPU.  The handle is built on first use."""

    _abi_name = "mel_frontend"

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024,
                 n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0):
        super().__init__()
        for name, v in (("sample_rate", sample_rate), ("n_fft", n_fft), ("hop_length", hop_length), ("win_length", win_length),
                        ("n_mels", n_mels)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        nyquist = 0.5 * int(sample_rate)
        top = nyquist if fmax is None else float(fmax)
        if not 0.0 <= float(fmin) < top <= nyquist:
            raise ValueError(f"0 <= fmin < fmax <= sample_rate / 2 is required, got fmin={fmin}, fmax={fmax}")
        self.sample_rate, self.n_fft, self.hop_length = int(sample_rate), int(n_fft), int(hop_length)
        self.win_length, self.n_mels = int(win_length), int(n_mels)
        self.fmin, self.fmax = float(fmin), (None if fmax is None else float(fmax))

    def get_config(self) -> dict:
        return {"sample_rate": self.sample_rate, "n_fft": self.n_fft, "hop_length": self.hop_length,
                "win_length": self.win_length, "n_mels": self.n_mels, "fmin": self.fmin, "fmax": self.fmax}

    def native_config(self) -> "_native.MelFrontendConfig":
        return _native.MelFrontendConfig(self.sample_rate, self.n_fft, self.hop_length, self.win_length, self.n_mels, 0,
                                         self.fmin, 0.0 if self.fmax is None else self.fmax)

    # -- host-only queries -------------------------------------------------------------------
    def launch_count(self, B: int, L: int) -> int:
        """Kernel launches of one ``forward_device`` (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L)

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def frames_of(self, n_samples: int) -> int:
        return 1 + int(n_samples) // self.hop_length

    def design(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(dft, fb)``: the fp32 windowed DFT table ``[2, n_bins, n_fft]`` (cosines, then sines) and the fp32 filterbank
        ``[n_mels, n_bins]`` exactly as the device multiplies by them (``iris_mel_frontend_design``: host only)."""
        lib = _native.load()
        cfg = self.native_config()
        bins = ctypes.c_int32()
        _native.check("iris_mel_frontend_design", lib.iris_mel_frontend_design(ctypes.byref(cfg), ctypes.byref(bins), None, 0, None, 0))
        dft = np.empty((2, bins.value, self.n_fft), dtype=np.float32)
        fb = np.empty((self.n_mels, bins.value), dtype=np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        _native.check("iris_mel_frontend_design", lib.iris_mel_frontend_design(
            ctypes.byref(cfg), ctypes.byref(bins), dft.ctypes.data_as(fp), ctypes.c_uint64(dft.size),
            fb.ctypes.data_as(fp), ctypes.c_uint64(fb.size)))
        return dft, fb

    # -- the native handle -------------------------------------------------------------------
    def _counts_dev(self, values, B: int, what: str) -> Optional[torch.Tensor]:
        if values is None:
            return None
        if isinstance(values, torch.Tensor) and values.device == self._device and values.dtype == torch.int32:
            t = values.contiguous()
        else:
            host = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
            if host.size and not np.issubdtype(host.dtype, np.integer):
                raise ValueError(f"{what} must be integers, got {host.dtype}")
            t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(self._device)
        if tuple(t.shape) != (B,):
            raise ValueError(f"{what} must have shape [{B}], got {list(t.shape)}")
        return t

    def forward_device(self, audio, lengths=None, max_frames=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``audio [B, L]`` float32 or int16, host or device -> ``(mel [B, n_mels, 1 + L // hop] fp32, frames [B] int32)``,
        both on the device.  ``lengths`` (a sequence or an int32 device tensor ``[B]``): the own samples of each item; the
        rest of its row is never read.  ``max_frames`` (likewise): a cap on each item's frames, as the reference trims the mel
        to the duration total.  Item b has ``min(1 + lengths[b] // hop, max_frames[b])`` frames, ``mel[b, :, frames[b]:]`` is
        0, and the item is bit for bit its batch-of-one call.  Asynchronous on the current stream."""
        if not isinstance(audio, torch.Tensor):
            audio = np.asarray(audio)
            if audio.dtype != np.int16:
                audio = audio.astype(np.float32, copy=False)
            audio = torch.from_numpy(np.ascontiguousarray(audio))
        if audio.dim() != 2 or audio.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"expected audio [B, L] float32 or int16, got {audio.dtype} {tuple(audio.shape)}")
        lib = self._ensure()
        audio = audio.to(self._device).contiguous()
        B, L = int(audio.shape[0]), int(audio.shape[1])
        T = self.frames_of(L)
        n_dev = self._counts_dev(lengths, B, "lengths")
        cap_dev = self._counts_dev(max_frames, B, "max_frames")
        if cap_dev is not None and n_dev is None:
            n_dev = torch.full((B,), L, dtype=torch.int32, device=self._device)
        mel = torch.empty((B, self.n_mels, T), dtype=torch.float32, device=self._device)
        frames = torch.full((B,), T, dtype=torch.int32, device=self._device)
        if B == 0:
            return mel, frames
        ws = self._ws(B, L)
        fmt = _native.MEL_SAMPLES_I16 if audio.dtype == torch.int16 else _native.MEL_SAMPLES_F32
        src = _ptr(audio if L else None)
        with torch.cuda.device(self._device):
            if n_dev is None:
                _native.check("iris_mel_frontend_forward", lib.iris_mel_frontend_forward(
                    self._handle, src, fmt, B, L, _ptr(mel), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
            else:
                _native.check("iris_mel_frontend_forward_ragged", lib.iris_mel_frontend_forward_ragged(
                    self._handle, src, fmt, B, L, _ptr(n_dev), _ptr(cap_dev), _ptr(mel), _ptr(frames), _ptr(ws),
                    ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return mel, frames

    __call__ = forward_device

    def compute(self, audio) -> np.ndarray:
        """One waveform ``[n]`` (float or int16) -> the host array ``[n_mels, 1 + n // hop]`` float32."""
        audio = audio.detach().cpu().numpy() if isinstance(audio, torch.Tensor) else np.asarray(audio)
        if audio.ndim != 1:
            raise ValueError(f"expected one waveform [n], got shape {audio.shape}")
        return self.forward_device(audio[None])[0][0].cpu().numpy()


_shared: dict = {}


def compute_mel_spectrogram(audio, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024,
                            n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0) -> np.ndarray:
    """The reference's function (``src/iris/data.py:25-67``), computed on the GPU: ``audio [n]`` -> ``[n_mels, time]`` float32
    on the host.  The front-end of a parameter set is built on first use and kept."""
    key = (int(sample_rate), int(n_fft), int(hop_length), int(win_length), int(n_mels), float(fmin), None if fmax is None else float(fmax))
    fe = _shared.get(key)
    if fe is None:
        fe = _shared[key] = MelFrontend(*key)
    return fe.compute(audio)
