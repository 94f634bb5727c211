"""How far apart two waveforms are, as spectra and as samples, per item of a ragged batch, on the device
(``iris_spectral_distance_*``, csrc/spectral_distance.h): the multi-resolution STFT distance and the SNR, for the choices whose
outputs differ by far more than the fp32 path's 1e-4 in samples -- bf16 or ``f32s`` against fp32, Griffin-Lim against the
checkpoint, a denoiser strength, copy-synthesis against the recording, a streamed chain against the whole call -- without
either waveform leaving the device.

``ref`` and ``test`` ``[B, L]`` fp32 share ``lengths`` and ``row_scale``; item b owns ``n_b = min(L, lengths[b] * row_scale)``
samples of both.  Per resolution ``(n_fft, hop, win)``, with ``K = n_fft // 2 + 1``:

    the transform of the mel front-end, Griffin-Lim and the denoiser (``center=True``, constant padding, periodic Hann of
        ``win`` centred in ``n_fft``); item b has ``T_b = 1 + n_b // hop`` frames and all of its samples count
    ``A``, ``B`` the fp32 magnitudes of ``ref`` and ``test``; over the item's ``T_b K`` cells, in fp64:
        ``d2 = sum (A - B)^2``   ``a2 = sum A^2``   ``l1 = sum |ln max(A, 1e-5) - ln max(B, 1e-5)|``
    over the item's samples: ``e2 = sum (x - y)^2``, ``x2 = sum x^2`` in fp64, ``emax = max |x - y|`` in fp32

The device leaves the sums (``forward_device``: 3 launches per resolution and 2 more, fixed order, no atomics -- an item's sums
are those of its batch-of-one call and two calls agree bit for bit); the host finishes them in float64 (``finish``):

    ``spectral_convergence = sqrt(d2 / a2)``   ``log_stft_l1 = l1 / (T_b K)``   ``snr_db = 10 log10(x2 / e2)``

and their means over the resolutions are the multi-resolution STFT distance.  A division by zero gives ``nan`` or ``inf`` under
numpy's rules (an empty item: ``nan``; identical signals: ``snr_db = inf``), not an error.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _wave

DEFAULT_RESOLUTIONS = ((512, 128, 512), (1024, 256, 1024), (2048, 512, 2048))     # (n_fft, hop, win)
TILE_FRAMES, CHUNK = 8, 4096                    # csrc/spectral_distance.h: kTileFrames, kChunk


def record_dtype(n_res: int) -> np.dtype:
    """One item's finished measures (``SpectralDistance.finish``)."""
    return np.dtype([("frames", np.int32, (n_res,)), ("spectral_convergence", np.float64, (n_res,)),
                     ("log_stft_l1", np.float64, (n_res,)), ("mr_spectral_convergence", np.float64),
                     ("mr_log_stft_l1", np.float64), ("snr_db", np.float64), ("emax", np.float64)])


class SpectralDistance(_DeviceStage):
    """The distance stage for a fixed list of at most 4 resolutions ``(n_fft, hop, win)``, resident on one GPU (``device``, or
    the current one); the handle -- it owns one packed windowed DFT per resolution -- is built on first use."""

    _abi_name = "spectral_distance"

    def __init__(self, resolutions: Sequence[Tuple[int, int, int]] = DEFAULT_RESOLUTIONS, device: Optional[torch.device] = None):
        super().__init__(device)
        res = [tuple(r) for r in resolutions]
        if not res or any(len(r) != 3 or any(isinstance(v, bool) or int(v) != v for v in r) for r in res):
            raise ValueError(f"resolutions must be a list of (n_fft, hop, win) integers, got {resolutions!r}")
        self.resolutions = tuple(tuple(int(v) for v in r) for r in res)
        self.workspace_bytes(0, 0)                              # the library's own refusals, before any device work

    def get_config(self) -> dict:
        return {"resolutions": [list(r) for r in self.resolutions]}

    def native_config(self):
        """``resolutions [n_res][3]`` as the int32 array the entry points take."""
        flat = [v for r in self.resolutions for v in r]
        return (ctypes.c_int32 * len(flat))(*flat)

    @property
    def bins(self) -> np.ndarray:
        return np.array([r[0] // 2 + 1 for r in self.resolutions], dtype=np.int64)

    # -- host-only queries -------------------------------------------------------------------
    def _query(self, what: str, *args) -> int:
        name = f"iris_{self._abi_name}_{what}"
        fn = getattr(_native.load(), name)
        out = fn.argtypes[-1]._type_()
        _native.check(name, fn(self.native_config(), len(self.resolutions), *(int(v) for v in args), ctypes.byref(out)))
        return int(out.value)

    def launch_count(self, B: int, L: int) -> int:
        """Kernel launches of one call: 3 per resolution and 2 (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L)

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def _create(self, lib, weights, n_weights, handle_ref) -> int:
        return lib.iris_spectral_distance_create(self.native_config(), len(self.resolutions), handle_ref)

    # -- the calls ---------------------------------------------------------------------------
    def forward_device(self, ref, test, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``ref``, ``test`` ``[B, L]`` fp32, host or device -> ``(spec [B, R, 3], wave [B, 3], frames [B, R])`` on the device:
        ``(d2, a2, l1)`` per resolution and ``(e2, x2, emax)`` in float64, and the ``T_b`` used in int32.  Asynchronous on the
        current stream, nothing synchronises.  ``lengths`` (a host sequence of integers or an integer tensor ``[B]``, which the
        host never reads) and ``row_scale`` as every waveform stage takes them; nothing past an item's samples is read."""
        ref, test = _wave(ref), _wave(test)
        if ref.shape != test.shape:
            raise ValueError(f"ref is {tuple(ref.shape)} and test {tuple(test.shape)}: the two batches must have one shape")
        lib, ref, lengths, B, L = self._ragged_wave(ref, lengths, row_scale)
        test = test.to(self._device).contiguous()
        R = len(self.resolutions)
        spec = torch.zeros((B, R, 3), dtype=torch.float64, device=self._device)
        wave = torch.zeros((B, 3), dtype=torch.float64, device=self._device)
        frames = torch.zeros((B, R), dtype=torch.int32, device=self._device)
        if B == 0 or L == 0:
            return spec, wave, frames
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_spectral_distance_forward", lib.iris_spectral_distance_forward(
                self._handle, _ptr(ref), _ptr(test), B, L, _ptr(lengths), int(row_scale), _ptr(spec), _ptr(wave), _ptr(frames),
                _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return spec, wave, frames

    def finish(self, spec, wave, frames) -> np.ndarray:
        """The sums of ``forward_device`` (device or host) -> one record per item (``record_dtype``), float64 on the host.  This
        is a read-back.  Divisions by zero follow numpy: ``nan`` or ``inf``, no error."""
        host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        spec, wave, frames = host(spec).astype(np.float64), host(wave).astype(np.float64), host(frames).astype(np.int32)
        out = np.zeros(spec.shape[0], dtype=record_dtype(len(self.resolutions)))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["frames"] = frames
            out["spectral_convergence"] = np.sqrt(spec[:, :, 0] / spec[:, :, 1])
            out["log_stft_l1"] = spec[:, :, 2] / (frames.astype(np.float64) * self.bins[None, :])
            out["mr_spectral_convergence"] = out["spectral_convergence"].mean(axis=1)
            out["mr_log_stft_l1"] = out["log_stft_l1"].mean(axis=1)
            out["snr_db"] = 10.0 * np.log10(wave[:, 1] / wave[:, 0])
            out["emax"] = wave[:, 2]
        return out

    def measure(self, ref, test, lengths=None, row_scale: int = 1) -> np.ndarray:
        """``finish(*forward_device(...))``: one record of the finished measures per item."""
        return self.finish(*self.forward_device(ref, test, lengths, row_scale))

    def compare_dtypes(self, engine, mel, a: str = "f32", b: str = "bf16", lengths=None) -> np.ndarray:
        """The distance of ``engine.forward(mel, dtype=b)`` from ``engine.forward(mel, dtype=a)``, one record per item; neither
        waveform leaves the device.  ``lengths`` (mel frames per item) always bounds what is measured -- item b's first
        ``hop * lengths[b]`` samples -- and is handed to the two forwards only where both admit it, ``a == b == "f32"``: a ragged
        forward is fp32 only, and a ragged reference against a dense candidate would count the padding's reach into the item
        as a distance between dtypes."""
        ragged = lengths if a == "f32" and b == "f32" else None
        ya = engine.forward(mel, dtype=a, lengths=ragged)
        yb = engine.forward(mel, dtype=b, lengths=ragged)
        return self.measure(ya, yb, lengths=lengths, row_scale=engine.hop_length if lengths is not None else 1)
