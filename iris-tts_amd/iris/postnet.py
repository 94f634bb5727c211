"""MI355X drop-in for the reference module ``iris.postnet`` (Tacotron2-style PostNet, Keras).

Call surface kept from ``/root/reference/src/iris/postnet.py``: ``PostNet(n_mels, num_layers=4,
channels=256, kernel_size=5, dropout=0.5, name=None)`` (:16-46) and ``postnet(mels_bt_f,
training=False) -> [B, n_mels, T]`` = input + residual (:48-67); ``scripts/synthesize.py:152-166``
builds it with ``num_layers=3, channels=256, kernel_size=5`` and applies it right before the vocoder.

Parameters are kept in the Keras layouts and names (``Conv1D`` kernel ``[k, C_in, C_out]``, bias;
``BatchNormalization`` gamma, beta, moving_mean, moving_variance, epsilon 1e-3 = the Keras default).
At upload the inference BatchNorm is folded into the convolution, so a layer is one launch of the MFMA
conv kernel with a tanh epilogue (``iris-tts_amd/csrc/postnet.h``).  Inference only (dropout is the
identity); ``training=True`` raises.

Parity note: the reference PostNet exists only in Keras/JAX, which cannot run in this pipeline, and
the reference ships no vectors for it: the device path is checked against ``oracle/postnet_oracle.py``
(a numpy restatement of postnet.py:48-67) -- "parity unpinned".  ``.weights.h5`` files need h5py;
``load_weights``/``save_weights`` use ``.npz``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _native
from ._engine import _check_lengths
from ._native_model import _NativeModel, _ptr, _stream

BN_EPSILON = 1e-3  # keras.layers.BatchNormalization default


def fold_batchnorm(kernel: np.ndarray, bias: np.ndarray, gamma: np.ndarray, beta: np.ndarray,
                   mean: np.ndarray, var: np.ndarray, eps: float = BN_EPSILON):
    """Conv1D kernel [k, C_in, C_out] + inference BatchNorm -> (weight [C_out, C_in, k], bias [C_out]).
    BN(y) = gamma * (y - mean) / sqrt(var + eps) + beta, applied per output channel."""
    scale = (gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps))
    w = kernel.astype(np.float64).transpose(2, 1, 0) * scale[:, None, None]
    b = (bias.astype(np.float64) - mean.astype(np.float64)) * scale + beta.astype(np.float64)
    return np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


class PostNet(_NativeModel):
    _abi_name = "postnet"

    def __init__(self, n_mels: int, num_layers: int = 4, channels: int = 256, kernel_size: int = 5,
                 dropout: float = 0.5, name: Optional[str] = None, seed: Optional[int] = None):
        assert num_layers >= 2, "PostNet needs at least 2 layers"
        self.n_mels, self.num_layers, self.channels = n_mels, num_layers, channels
        self.kernel_size, self.dropout_rate, self.name = kernel_size, dropout, name or "post_net"
        super().__init__()
        rng = np.random.default_rng(seed)
        for i in range(num_layers):
            c_in = n_mels if i == 0 else channels
            c_out = n_mels if i == num_layers - 1 else channels
            limit = np.sqrt(6.0 / ((c_in + c_out) * kernel_size))            # glorot_uniform
            p = self._prefix(i)
            self.weights[f"{p}.kernel"] = rng.uniform(-limit, limit, (kernel_size, c_in, c_out)).astype(np.float32)
            self.weights[f"{p}.bias"] = np.zeros(c_out, np.float32)
            self.weights[f"{p}.gamma"] = np.ones(c_out, np.float32)
            self.weights[f"{p}.beta"] = np.zeros(c_out, np.float32)
            self.weights[f"{p}.moving_mean"] = np.zeros(c_out, np.float32)
            self.weights[f"{p}.moving_variance"] = np.ones(c_out, np.float32)

    def _prefix(self, i: int) -> str:
        return "conv_out" if i == self.num_layers - 1 else f"convs.{i}"

    def get_config(self) -> dict:
        return {"n_mels": self.n_mels, "num_layers": self.num_layers, "channels": self.channels,
                "kernel_size": self.kernel_size, "dropout": self.dropout_rate}

    def folded_blob(self) -> np.ndarray:
        parts = []
        for i in range(self.num_layers):
            p = self._prefix(i)
            w, b = fold_batchnorm(*(self.weights[f"{p}.{n}"] for n in
                                    ("kernel", "bias", "gamma", "beta", "moving_mean", "moving_variance")))
            parts += [w.ravel(), b.ravel()]
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    # -- execution ---------------------------------------------------------------------------
    def _upload_blob(self) -> np.ndarray:
        return self.folded_blob()

    def _create(self, lib, weights, n_weights, handle_ref) -> int:
        return lib.iris_postnet_create(self.n_mels, self.num_layers, self.channels, self.kernel_size, weights, n_weights, handle_ref)

    @property
    def receptive_field_frames(self) -> int:
        """Mel frames on either side that can reach one refined frame: every layer is a 'same' convolution that widens the
        dependence by (kernel_size - 1) / 2 (6 for the 3 x k5 net of scripts/synthesize.py:152-158)."""
        return self.num_layers * (self.kernel_size - 1) // 2

    def forward_device(self, mel: torch.Tensor, lengths=None) -> torch.Tensor:
        """[B, n_mels, T] fp32 device tensor -> refined mel, same shape (asynchronous on the current stream).

        ``lengths`` (a ragged batch): the frames of each item, a sequence or integer tensor [B] with
        0 <= lengths[b] <= T.  Item b is then refined bit for bit as ``forward_device(mel[b:b+1, :, :lengths[b]])`` would
        refine it -- frames past its length are never read -- and ``out[b, :, lengths[b]:]`` is 0
        (``iris_postnet_forward_ragged``)."""
        lib = self._ensure()
        if mel.dim() != 3 or mel.shape[1] != self.n_mels:
            raise ValueError(f"expected mel [B, {self.n_mels}, T], got {tuple(mel.shape)}")
        mel = mel.to(device=self._device, dtype=torch.float32).contiguous()
        B, _, T = mel.shape
        lengths_host = None if lengths is None else _check_lengths(lengths, B, T)
        out = torch.empty_like(mel)
        if B == 0 or T == 0:
            return out
        ws = self._ws(B, T)
        if lengths_host is not None:
            # (a stream-ordered allocation: the caching allocator hands the block out again only behind this stream's kernels)
            lengths_dev = torch.from_numpy(lengths_host).to(self._device)
            _native.check("iris_postnet_forward_ragged", lib.iris_postnet_forward_ragged(
                self._handle, _ptr(mel), B, T, _ptr(lengths_dev), _ptr(out), _ptr(ws), ctypes.c_uint64(ws.numel()),
                _stream(self._device)))
            return out
        _native.check("iris_postnet_forward", lib.iris_postnet_forward(
            self._handle, _ptr(mel), B, T, _ptr(out), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    def _workspace_layout(self, B: int, T: int):
        """Test-only: ``postnet_ws`` (csrc/iris_hifigan.hip) restated: float offsets of hid[0], hid[1] ([B, T, channels]
        each) and res ([B, T, n_mels]) and the total, every buffer starting on a 256-byte boundary (64 floats)."""
        offs, off = [], 0
        for n in (B * T * self.channels, B * T * self.channels, B * T * self.n_mels):
            offs.append(off)
            off += (n + 63) & ~63
        return offs[0], offs[1], offs[2], off

    def _read_layers(self, B: int, T: int):
        """Test-only: the layer outputs the last ``forward_device`` of shape (B, T) left in the workspace, as
        ({layer index: [B, T, C] copy}, bytes of the layout).  Layer i wrote hid[i & 1] and the last layer res, so what
        survives is every layer of a 2- or 3-layer net and the layers L-3, L-2 and L-1 (res) of a deeper one."""
        h0, h1, res, total = self._workspace_layout(B, T)
        ws = self._workspace.view(torch.float32)
        L = self.num_layers
        out = {L - 1: ws[res:res + B * T * self.n_mels].clone().view(B, T, self.n_mels)}
        for i in range(max(0, L - 3), L - 1):
            off = h1 if i & 1 else h0
            out[i] = ws[off:off + B * T * self.channels].clone().view(B, T, self.channels)
        return out, 4 * total

    def __call__(self, mels_bt_f, training: bool = False) -> np.ndarray:
        """[B, n_mels, T] -> [B, n_mels, T] (input + residual), reference postnet.py:48-67."""
        if training:
            raise NotImplementedError("the MI355X build is inference-only")
        if isinstance(mels_bt_f, torch.Tensor):
            return self.forward_device(mels_bt_f)
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(mels_bt_f, dtype=np.float32)))
        self._ensure()
        return self.forward_device(x.to(self._device)).cpu().numpy()

    call = __call__
