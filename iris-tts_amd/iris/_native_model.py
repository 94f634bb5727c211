"""What the models around the vocoder share (``iris.encoder``, ``iris.vae``, ``iris.postnet``): weights kept in Keras
layouts, ``.npz`` files, and a native handle with its workspace, both built on first use and dropped when a weight changes.
``_DeviceStage`` is the base of the stages that have a config and no weights (``iris.mel``, ``iris.griffin_lim``,
``iris.denoiser``, ``iris.time_stretch``, ``iris.assemble``, ``iris.loudness``, ``iris.limiter``, ``iris.metrics``).
"""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from . import _native
from ._engine import require_gpu


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _take_buffers(sizes):
    """``WsTaker`` (csrc/stage_host.h): the buffers one behind the other, each rounded up to 64 floats."""
    layout, off = {}, 0
    for name, n in sizes:
        layout[name] = (off, n)
        off += (n + 63) & ~63
    return layout, off


def _take_shapes(shapes: dict):
    """``_take_buffers`` for buffers of one word per element, named by shape: ``({buffer: (offset, shape)}, words)``."""
    layout, total = _take_buffers((name, int(np.prod(shape))) for name, shape in shapes.items())
    return {name: (layout[name][0], shape) for name, shape in shapes.items()}, total


def _wave(wav, hop_length: Optional[int] = None, why: str = "") -> torch.Tensor:
    """``wav`` as a ``[B, L]`` float32 tensor, from host or device, where it is.  ``hop_length``: ``L`` must be a multiple of
    it; ``why`` is the calling stage's own sentence for that refusal."""
    if not isinstance(wav, torch.Tensor):
        wav = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32)))
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError(f"expected a waveform [B, L] float32, got {wav.dtype} {tuple(wav.shape)}")
    if hop_length and wav.shape[1] % hop_length:
        raise ValueError(f"L = {wav.shape[1]} is not a multiple of hop_length = {hop_length}: {why}; nothing is padded silently")
    return wav


class _NativeModel:
    """Weights in Keras layouts + a native handle built on first use.  A model names its entry points (``_abi_name``) and
    says how its handle is made (``_create``, from ``_upload_blob``) and how large a workspace is (``workspace_bytes``)."""

    _abi_name = ""                                      # iris_<_abi_name>_create, iris_<_abi_name>_destroy, ...

    def __init__(self):
        self.weights: Dict[str, np.ndarray] = {}
        self._handle = None
        self._workspace = None
        self._device = None

    # -- parameters --------------------------------------------------------------------------
    def set_weights_dict(self, weights: Dict[str, np.ndarray]) -> None:
        """Takes every tensor of this model from ``weights``; other keys are ignored."""
        for key, cur in self.weights.items():
            if key not in weights:
                raise KeyError(f"weights are missing {key}")
            arr = np.asarray(weights[key], dtype=np.float32)
            if arr.shape != cur.shape:
                raise ValueError(f"{key}: shape {arr.shape} != expected {cur.shape}")
            self.weights[key] = np.ascontiguousarray(arr)
        self._drop()

    def save_weights(self, path: str) -> None:
        if Path(path).suffix in (".h5", ".keras"):
            raise NotImplementedError("Keras .h5/.keras files need h5py, which this build does not use; save to .npz")
        np.savez(str(path), **self.weights)

    def load_weights(self, path: str) -> None:
        if Path(path).suffix in (".h5", ".keras"):
            raise NotImplementedError(f"{Path(path).name}: reading Keras weight files needs h5py, which is not available")
        with np.load(str(path), allow_pickle=False) as data:
            self.set_weights_dict({k: data[k] for k in data.files})

    def blob_size(self) -> int:
        """Values in ``weights``, and so in ``blob()``, which holds the same tensors in the order the C side reads them
        (``iris_<_abi_name>_weight_count`` computes the same).  ``PostNet.folded_blob()`` is smaller: its BatchNorm is folded."""
        return sum(int(v.size) for v in self.weights.values())

    # -- the native handle -------------------------------------------------------------------
    def _upload_blob(self) -> np.ndarray:
        """The flat fp32 array ``iris_<_abi_name>_create`` reads."""
        return self.blob()

    def _create(self, lib, weights, n_weights, handle_ref) -> int:
        """Calls ``iris_<_abi_name>_create``; returns its status.  The default passes ``native_config()`` by reference."""
        cfg = self.native_config()
        return getattr(lib, f"iris_{self._abi_name}_create")(ctypes.byref(cfg), weights, n_weights, handle_ref)

    def _drop(self) -> None:
        if self._handle is not None:
            getattr(_native.load(), f"iris_{self._abi_name}_destroy")(self._handle)
        self._handle = None
        self._workspace = None

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _ensure(self):
        lib = _native.load()
        if self._handle is None:
            self._device = require_gpu()
            blob = self._upload_blob()
            h = ctypes.c_void_p()
            with torch.cuda.device(self._device):
                _native.check(f"iris_{self._abi_name}_create", self._create(
                    lib, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_uint64(blob.size), ctypes.byref(h)))
            self._handle = h
        return lib

    def workspace_bytes(self, B: int, n: int) -> int:
        """Bytes a forward of shape (B, n) needs, asked of the handle (``iris_<_abi_name>_workspace_bytes``)."""
        lib = self._ensure()
        out = ctypes.c_uint64()
        name = f"iris_{self._abi_name}_workspace_bytes"
        _native.check(name, getattr(lib, name)(self._handle, B, n, ctypes.byref(out)))
        return int(out.value)

    def _grow(self, need: int) -> torch.Tensor:
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=self._device)
        return self._workspace

    def _ws(self, *shape) -> torch.Tensor:
        """The workspace, grown to what a forward of ``shape`` -- whatever ``workspace_bytes`` takes -- needs."""
        return self._grow(self.workspace_bytes(*shape))

    _ws_for = _ws           # the name the stage classes had for it; earlier revisions of the stretch's GPU tests call it


class _DeviceStage(_NativeModel):
    """A stage that is a config and no weights: its host-only queries take ``native_config()`` by reference, its handle
    is built on ``device`` (None: the current one) and owns whatever tables the library designs for the config."""

    def __init__(self, device=None):
        super().__init__()
        self._want_device = None if device is None else torch.device(device)

    # -- host-only queries -------------------------------------------------------------------
    def _query_config(self):
        return self.native_config()

    def _query(self, what: str, *args) -> int:
        """``iris_<_abi_name>_<what>(config, *args, &out)``: no device needed.  The symbol table (``iris._native``) says what
        ``out`` and every argument are."""
        name = f"iris_{self._abi_name}_{what}"
        fn = getattr(_native.load(), name)
        cfg, out = self._query_config(), fn.argtypes[-1]._type_()
        args = [float(v) if t is ctypes.c_double else int(v) for t, v in zip(fn.argtypes[1:-1], args)]
        _native.check(name, fn(ctypes.byref(cfg), *args, ctypes.byref(out)))
        return int(out.value)

    def _window_range(self, origin: int, Lw: int, final: bool):
        """``iris_<_abi_name>_window_range(config, origin, Lw, final, &out_lo, &out_count)``: the samples of an utterance the
        window ``[origin, origin + Lw)`` settles.  No device needed."""
        name = f"iris_{self._abi_name}_window_range"
        cfg, lo, count = self._query_config(), ctypes.c_int64(), ctypes.c_int64()
        _native.check(name, getattr(_native.load(), name)(
            ctypes.byref(cfg), ctypes.c_int64(int(origin)), int(Lw), int(bool(final)), ctypes.byref(lo), ctypes.byref(count)))
        return int(lo.value), int(count.value)

    # -- the native handle -------------------------------------------------------------------
    def _upload_blob(self) -> np.ndarray:
        return np.zeros(0, dtype=np.float32)            # the library designs its own tables

    def _create(self, lib, weights, n_weights, handle_ref) -> int:
        cfg = self.native_config()
        return getattr(lib, f"iris_{self._abi_name}_create")(ctypes.byref(cfg), handle_ref)

    def _ensure(self):
        if self._handle is None and self._want_device is not None:
            with torch.cuda.device(self._want_device):
                return super()._ensure()
        return super()._ensure()

    def close(self) -> None:
        """Frees the native handle and the workspace; the next call builds them again."""
        self._drop()

    # -- what the calls take ------------------------------------------------------------------
    def _ragged_wave(self, wav, lengths, row_scale):
        """``(lib, wav, lengths, B, L)`` of a call on a ragged batch of waveforms: ``wav [B, L]`` fp32 and ``lengths`` (None,
        a host sequence of integers or an integer tensor ``[B]``) on the handle's device, checked before any device work."""
        wav = _wave(wav)
        if isinstance(row_scale, bool) or int(row_scale) != row_scale or int(row_scale) < 1:
            raise ValueError(f"row_scale must be an integer >= 1, got {row_scale!r}")
        B = int(wav.shape[0])
        if lengths is not None and not isinstance(lengths, torch.Tensor):
            host = np.asarray(lengths)
            if host.shape != (B,) or (host.size and not np.issubdtype(host.dtype, np.integer)):
                raise ValueError(f"lengths must be {B} integers, got {host.dtype} {host.shape}")
            lengths = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32))
        if lengths is not None and (tuple(lengths.shape) != (B,) or lengths.dtype not in (torch.int32, torch.int64)):
            raise ValueError(f"lengths must be an integer tensor [{B}], got {lengths.dtype} {tuple(lengths.shape)}")
        lib = self._ensure()
        wav = wav.to(self._device).contiguous()
        if lengths is not None:
            lengths = lengths.to(device=self._device, dtype=torch.int32).contiguous()
        return lib, wav, lengths, B, int(wav.shape[1])
