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
The same launches take a ragged batch (``forward_device(lengths=)``: every kernel bounds item b by its own frame count, so
it is bit for bit its batch-of-one call) and can draw the start phase themselves (``phase0="device"``: Philox4x32-10 keyed
by the seed and the item's stream number, restated in numpy by ``philox_phase_np``).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _DeviceStage, _NativeModel, _ptr, _stream, _take_shapes
from .mel import MelFrontend
from .vae import _lengths_on, check_lengths as _check_frame_counts

DEFAULT_NNLS_ITERS = 32        # DESIGN.md, "Griffin-Lim": the residual table this is read from


def start_phase(B: int, n_bins: int, T: int, seed: int = 1337) -> np.ndarray:
    """``phi0 [B, n_bins, T]`` float64: ``2 pi * numpy.random.default_rng(seed).random((B, n_bins, T))``."""
    return 2.0 * np.pi * np.random.default_rng(seed).random((B, n_bins, T))


def pack_phase(phi0: np.ndarray) -> np.ndarray:
    """``phi0 [B, n_bins, T]`` -> what the device reads: fp32 ``[B, T, n_bins, 2]``, cos and sin taken in float64 and rounded once."""
    phi = np.transpose(np.asarray(phi0, dtype=np.float64), (0, 2, 1))
    return np.ascontiguousarray(np.stack([np.cos(phi), np.sin(phi)], axis=-1).astype(np.float32))


_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10_np(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ``counter [..., 4]`` and
    ``key (k0, k1)`` of 32-bit words -> the four output words ``[..., 4]`` as uint64 values below 2^32.  The integer work is in
    uint64 with masks (a 32 x 32 product fits), the restatement of ``philox4x32_10`` in csrc/griffin_lim.h."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & _M32 for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return np.stack(c, axis=-1)


def philox_uniform_np(seed: int, item: int, n_bins: int, T: int) -> np.ndarray:
    """``u [T, n_bins]`` float32 in [0, 1) of the device draw: key ``(seed & 0xffffffff, seed >> 32)``, counter
    ``(k >> 2, t, item, 0)``, output word ``k & 3`` for bin k of frame t; ``u = (x >> 8) * 2^-24`` (exact in fp32)."""
    groups = (n_bins + 3) // 4
    counter = np.zeros((T, groups, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(groups, dtype=np.uint64)[None, :]
    counter[..., 1] = np.arange(T, dtype=np.uint64)[:, None]
    counter[..., 2] = np.uint64(int(item) & 0xFFFFFFFF)
    words = philox4x32_10_np(counter, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)).reshape(T, 4 * groups)[:, :n_bins]
    return (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_phase_np(seed: int, item: int, n_bins: int, T: int) -> np.ndarray:
    """The device-drawn start phase of item stream ``item``, packed ``[T, n_bins, 2]`` float64: the angle is the ONE fp32
    product ``6.2831855f * u`` the device forms (``philox_uniform_np``), its cos and sin are taken in float64 -- what is left
    between this and ``GriffinLim.draw_phase`` is the error of the device's ``cosf`` / ``sinf``."""
    ang = (np.float32(6.2831855) * philox_uniform_np(seed, item, n_bins, T)).astype(np.float64)
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1)


def check_lengths(lengths, B: int, T: int):
    """``lengths`` of a ragged call, checked the way ``iris.vae.check_lengths`` checks its own: an int32 device tensor ``[B]``
    is passed through unread (the kernels sanitise it); host lengths must be integers in ``{0} U [2, T]`` -- an item of one
    frame has no sample -- and come back as an int32 array.  Raises before any device work."""
    out = _check_frame_counts(lengths, B, T, 1)
    if not isinstance(out, torch.Tensor):
        for b, n in enumerate(out.tolist()):
            if n == 1:
                raise ValueError(f"lengths[{b}] = 1: an item has 0 frames (empty) or at least 2 (hop * (T_b - 1) samples)")
    return out


class GriffinLim(_DeviceStage):
    """The Griffin-Lim vocoder with fixed parameters (the reference script's), resident on one GPU.  Usable as the ``vocode``
    of ``MelToWavePipeline``; ``whole_utterance`` tells the pipeline that a mel cannot be cut into chunks (every frame's
    phase depends on the whole item) and that the output has ``hop * (T - 1)`` samples.

    ``phase``: where ``forward_device(phase0=None)`` gets its start phase -- ``"host"`` (numpy's generator, uploaded) or
    ``"device"`` (drawn by the inversion kernel, nothing uploaded).  ``ragged=True`` sets ``takes_lengths``, which lets
    ``MelToWavePipeline.infer_batch`` hand a batch of unequal lengths to ONE ``forward_device(..., lengths=)``."""

    _abi_name = "griffin_lim"
    whole_utterance = True

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024,
                 n_mels: int = 80, fmin: float = 0.0, fmax: Optional[float] = 8000.0, n_iter: int = 60, momentum: float = 0.99,
                 nnls_iters: int = DEFAULT_NNLS_ITERS, phase: str = "host", ragged: bool = False):
        super().__init__()
        if phase not in ("host", "device"):
            raise ValueError(f"phase must be 'host' or 'device', got {phase!r}")
        self.phase, self.takes_lengths = phase, bool(ragged)
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
    def _query_config(self):
        return self.native_config(with_step=False)

    def launch_count(self, B: int, T: int) -> int:
        """Kernel launches of one ``forward_device``: ``2 * n_iter + 2`` (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, T)

    def workspace_bytes(self, B: int, T: int) -> int:
        return self._query("workspace_bytes", B, T)

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

    _create = _NativeModel._create                     # iris_griffin_lim_create takes the array

    @staticmethod
    def _check_stream(seed, first_item, B: int) -> Tuple[int, int]:
        if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        if int(first_item) != first_item or not 0 <= int(first_item) <= 2 ** 31 - 1 - B:
            raise ValueError(f"first_item must be an integer in [0, 2^31 - B), got {first_item!r}")
        return int(seed), int(first_item)

    def _ragged_host_phase(self, lengths: np.ndarray, T: int, seed: int) -> np.ndarray:
        """The packed phase of a ragged call with host lengths: item b holds ``start_phase(1, n_bins, T_b, seed)[0]``, what
        its stand-alone call draws (not a slice of the dense draw); rows past ``T_b`` stay 0 and are never read."""
        packed = np.zeros((len(lengths), T, self.n_bins, 2), dtype=np.float32)
        drawn = {}
        for b, n in enumerate(int(v) for v in lengths):
            if n and n not in drawn:
                drawn[n] = pack_phase(start_phase(1, self.n_bins, n, seed))[0]
            if n:
                packed[b, :n] = drawn[n]
        return packed

    def forward_device(self, logmel, phase0=None, seed: int = 1337, lengths=None, first_item: int = 0) -> torch.Tensor:
        """``logmel [B, n_mels, T]`` fp32, host or device, ``T >= 2`` -> the waveform ``[B, hop * (T - 1)]`` on the device.
        ``phase0 [B, n_bins, T]`` (radians, any float type, host): the start phase; None draws
        ``2 pi * numpy.random.default_rng(seed).random((B, n_bins, T))`` (or, for a ``GriffinLim(phase="device")``, stands for
        ``"device"``).  A device tensor ``[B, T, n_bins, 2]`` fp32 is taken as the packed cos / sin (``pack_phase``) and not
        copied.  ``phase0="device"``: the inversion kernel draws the phase itself (``philox_phase_np`` restates it) from
        ``seed`` and the item's stream number ``first_item + b``; nothing is uploaded.  Asynchronous on the current stream;
        two calls agree bit for bit and item b is its batch-of-one call on ``phase0[b]`` (``first_item=b`` for a device draw).

        ``lengths``: item b's frame count ``T_b`` -- a host sequence of integers in ``{0} U [2, T]`` (``ValueError`` otherwise,
        before any device work) or an int32 device tensor ``[B]``, which is never read by the host (the kernels clamp an entry
        to ``[0, T]`` and take one below 2 as 0) and may change between the replays of a captured graph.  The result keeps its
        shape; ``wav[b, :hop * (T_b - 1)]`` is bit for bit the stand-alone call on ``logmel[b:b + 1, :, :T_b]`` and the rest of
        the row is 0.  With host lengths and ``phase0=None`` on the host, item b's phase is ``start_phase(1, n_bins, T_b,
        seed)[0]``, its stand-alone call's draw; device lengths need ``phase0="device"`` or an explicit ``phase0``."""
        if not isinstance(logmel, torch.Tensor):
            logmel = torch.from_numpy(np.ascontiguousarray(np.asarray(logmel, dtype=np.float32)))
        if logmel.dim() != 3 or logmel.shape[1] != self.n_mels or logmel.dtype != torch.float32:
            raise ValueError(f"expected a log-mel [B, {self.n_mels}, T] float32, got {logmel.dtype} {tuple(logmel.shape)}")
        B, T = int(logmel.shape[0]), int(logmel.shape[2])
        if T < 2:
            raise ValueError(f"T = {T}: Griffin-Lim needs at least 2 frames (the output has hop * (T - 1) samples)")
        if lengths is not None:
            lengths = check_lengths(lengths, B, T)
        if phase0 is None and self.phase == "device":
            phase0 = "device"
        packed_shape = (B, T, self.n_bins, 2)
        if isinstance(phase0, str):
            if phase0 != "device":
                raise ValueError(f"phase0 must be an array, a tensor, None or 'device', got {phase0!r}")
            seed, first_item = self._check_stream(seed, first_item, B)
            packed = None
        elif isinstance(phase0, torch.Tensor) and phase0.is_cuda:
            if tuple(phase0.shape) != packed_shape or phase0.dtype != torch.float32:
                raise ValueError(f"a device phase0 must be the packed cos / sin {list(packed_shape)} float32, got {phase0.dtype} {tuple(phase0.shape)}")
            packed = phase0
        elif phase0 is None and lengths is not None:
            if isinstance(lengths, torch.Tensor):
                raise ValueError("device lengths are never read by the host, so no per-item host phase can be drawn: pass "
                                 "phase0='device' or an explicit phase0")
            packed = torch.from_numpy(self._ragged_host_phase(lengths, T, seed))
        else:
            if phase0 is None:
                phase0 = start_phase(B, self.n_bins, T, seed)
            phase0 = phase0.detach().cpu().numpy() if isinstance(phase0, torch.Tensor) else np.asarray(phase0)
            if phase0.shape != (B, self.n_bins, T):
                raise ValueError(f"expected phase0 [{B}, {self.n_bins}, {T}], got {phase0.shape}")
            packed = torch.from_numpy(pack_phase(phase0))
        lib = self._ensure()
        logmel = logmel.to(self._device).contiguous()
        if packed is not None:
            packed = packed.to(self._device).contiguous()
        if lengths is not None:
            lengths = _lengths_on(lengths, self._device)
        wav = torch.empty((B, self.samples_of(T)), dtype=torch.float32, device=self._device)
        if B == 0:
            return wav
        ws = self._ws(B, T)
        with torch.cuda.device(self._device):
            _native.check("iris_griffin_lim_forward_ragged", lib.iris_griffin_lim_forward_ragged(
                self._handle, _ptr(logmel), _ptr(packed), ctypes.c_uint64(int(seed) if packed is None else 0),
                int(first_item) if packed is None else 0, B, T, _ptr(lengths), _ptr(wav), _ptr(ws), ctypes.c_uint64(ws.numel()),
                _stream(self._device)))
        return wav

    def draw_phase(self, B: int, T: int, seed: int = 1337, first_item: int = 0) -> torch.Tensor:
        """The start phase ``forward_device(phase0="device", seed=seed, first_item=first_item)`` draws for a batch of shape
        (B, T), as the packed device tensor ``[B, T, n_bins, 2]`` it also accepts as ``phase0`` (one launch)."""
        B, T = int(B), int(T)
        if B < 0 or T < 2:
            raise ValueError(f"B >= 0 and T >= 2 are required, got B = {B}, T = {T}")
        seed, first_item = self._check_stream(seed, first_item, B)
        lib = self._ensure()
        out = torch.empty((B, T, self.n_bins, 2), dtype=torch.float32, device=self._device)
        if B:
            with torch.cuda.device(self._device):
                _native.check("iris_griffin_lim_draw_phase", lib.iris_griffin_lim_draw_phase(
                    self._handle, ctypes.c_uint64(seed), first_item, B, T, _ptr(out), _stream(self._device)))
        return out

    def magnitudes(self, B: int, T: int) -> torch.Tensor:
        """``S [B, n_bins, T]``: the inverted magnitudes the last ``forward_device`` of shape (B, T) left at the start of its
        workspace (``[B][T][Ks]``, ``Ks`` = ``n_bins`` rounded up to 4).  For tests."""
        ks = (self.n_bins + 3) // 4 * 4
        s = self._workspace[:B * T * ks * 4].view(torch.float32).view(B, T, ks)
        return s[:, :, :self.n_bins].transpose(1, 2).contiguous()

    def _workspace_layout(self, B: int, T: int):
        """``({buffer: (offset, shape)}, floats)``: ``GlWorkspace`` (csrc/iris_griffin_lim.hip) restated -- S, c, r and the
        in-loop waveform y in ``WsTaker`` order.  Host only."""
        ks, qp = (self.n_bins + 3) // 4 * 4, (self.n_fft + 2 + 7) // 8 * 8
        return _take_shapes({"S": (B, T, ks), "c": (B, T, qp), "r": (B, T, qp), "y": (B, self.hop_length * (T - 1))})

    def _read_buffers(self, B: int, T: int) -> dict:
        """Test-only: the views ``S [B, T, Ks]``, ``c [B, T, Qp]``, ``r [B, T, Qp]`` and ``y [B, hop (T - 1)]`` of the workspace
        as the last ``forward_device`` of shape (B, T) left it.  Which launch wrote a buffer last is the reader's to know
        (``gl_forward``): S the inversion, c and r the last update (c0 the inversion when ``n_iter`` is 0; r nothing then), y
        the last in-loop inverse transform."""
        layout, _ = self._workspace_layout(B, T)
        ws = self._workspace.view(torch.float32)
        return {name: ws[off:off + int(np.prod(shape))].view(shape) for name, (off, shape) in layout.items()}

    def __call__(self, mel, phase0=None, seed: int = 1337) -> np.ndarray:
        """``[n_mels, T]`` -> ``[samples]``; ``[B, n_mels, T]`` -> ``[B, samples]``, on the host (as ``HiFiGANVocoder.infer``)."""
        mel = mel.detach().cpu().numpy() if isinstance(mel, torch.Tensor) else np.asarray(mel, dtype=np.float32)
        if mel.ndim == 2:
            return self.forward_device(mel[None], None if phase0 is None else np.asarray(phase0)[None], seed)[0].cpu().numpy()
        return self.forward_device(mel, phase0, seed).cpu().numpy()
