"""What the models around the vocoder share (``iris.encoder``, ``iris.vae``, ``iris.postnet``): weights kept in Keras
layouts, ``.npz`` files, and a native handle with its workspace, both built on first use and dropped when a weight changes.
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

    def _ws(self, B: int, n: int) -> torch.Tensor:
        """The workspace, grown to what a forward of shape (B, n) needs."""
        need = self.workspace_bytes(B, n)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=self._device)
        return self._workspace
