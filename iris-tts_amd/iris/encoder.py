"""MI355X drop-in for the inference half of the reference module ``iris.encoder`` (Keras/JAX): the Transformer phoneme
encoder, the duration head and the length regulator -- phoneme ids in, frame-level conditioning for ``iris.vae`` out.

Call surface kept from the reference's ``src/iris/encoder.py``: ``PhonemeEncoder(vocab_size, embed_dim=256, num_blocks=4,
num_heads=4, ffn_dim=None, max_length=1000, dropout=0.1)`` (:115-212), ``DurationPredictor(hidden_dim=256, num_layers=2,
kernel_size=3, dropout=0.1)`` (:228-315), ``create_encoder``, ``create_duration_predictor``, ``create_padding_mask``,
``length_regulate`` and ``get_config``.  ``training=True`` raises and ``compute_duration_loss`` is not built.  Added here:
``predict_durations`` (``scripts/synthesize.py:41-45``), ``forward_device`` on both models and ``frame_conditioning``, which
is ``synthesize.py:107-122`` on the device: encoder, head, prefix sum, ONE read-back (the frame totals, ``B`` int32 -- the
padded length ``T_pad`` sizes the output tensor, so the host has to know it) and the gather.

    x = phoneme_embedding[ids] + position_embedding[0..P)
    for each block:                                   # TransformerBlock.call, :82-102
        q, k, v = x Wq + bq, x Wk + bk, x Wv + bv     # per head h: columns h * key_dim .. (h + 1) * key_dim
        a = softmax((q / sqrt(key_dim)) k^T) v        # per head; keys past the item's length have weight 0
        x = LayerNorm(x + a Wo + bo);  x = LayerNorm(x + relu(x W1 + b1) W2 + b2)
    enc_out = LayerNorm(x)                            # encoder_output_norm
    h = enc_out;  for each layer: h = LayerNorm(relu(Conv1D_same(h)))          # :302-305
    pred = softplus(duration_output(h));  frames = clip(round(exp(pred) - 1), 1, 1e6)

Keras cannot run in this pipeline, so the conventions below are ASSUMPTIONS read from the Keras 3 sources and
documentation, pinned by the numpy restatement the tests compare against (``tests/encoder_restatement.py``) -- "parity
unpinned", as for ``iris.vae``:
  * ``MultiHeadAttention`` projects with per-head einsum kernels: query/key/value ``[E, H, key_dim]`` with bias
    ``[H, key_dim]``, output ``[H, key_dim, E]`` with bias ``[E]``; ``value_dim = key_dim``.
  * The query is scaled by ``1 / sqrt(key_dim)`` AFTER its bias (``q = (x Wq + bq) * scale``), the softmax runs over keys.
  * A padding mask adds ``-1e9`` to the masked scores; in fp32 their exponentials underflow to exactly 0, which is what
    the kernel stores.  The reference hands ``mask [B, P]`` to ``attention_mask``; here it is the KEY mask of a prefix
    (``create_padding_mask``), and rows past an item's length are additionally returned as zeros (the reference leaves
    them holding values nobody reads).  A non-prefix mask raises ``ValueError``.
  * ``LayerNormalization(epsilon=1e-6)`` normalises over the channel axis with the biased variance, ``gamma`` and
    ``beta``; the kernels take the mean first and the squared deviations second.
  * ``Dense`` is ``x @ kernel[in, out] + bias``; ``Conv1D`` kernels are ``[k, C_in, C_out]``, a cross-correlation with
    ``(k - 1) / 2`` zeros on both sides for ``padding='same'`` -- at the item's own length in a ragged batch.
  * ``ops.softplus`` is ``logaddexp(x, 0)``; ``jnp.round`` rounds half to even.
  * ``Dropout`` is the identity at inference.

Parameters are kept in the Keras layouts under attribute-path names (``phoneme_embedding.embeddings``,
``positional_embedding.position_embedding.embeddings``, ``transformer_block_0.attention.query.kernel``,
``transformer_block_0.ffn.0.kernel``, ``encoder_output_norm.gamma``, ``duration_conv_0.kernel``, ...).
``.weights.h5`` files need h5py; ``load_weights`` / ``save_weights`` use ``.npz``.

Phoneme ids given as numpy are checked on the host (``ValueError`` outside ``[0, vocab_size)``); ids given as a device
tensor are not read back -- the kernel clamps them into the table.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._engine import require_gpu
from ._native_model import _NativeModel, _ptr, _stream, _take_buffers
from .vae import _read_buffers

DEFAULT_MAX_FRAMES = 65536          # frames of one utterance batch item that frame_conditioning accepts by default


def create_padding_mask(lengths, max_len: int) -> np.ndarray:
    """Boolean ``[B, max_len]``, True = valid position (reference :419-434)."""
    lengths = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64)
    return np.arange(int(max_len))[None, :] < lengths[:, None]


def _lengths_from(mask, lengths, B: int, P: int) -> Optional[np.ndarray]:
    """The per-item lengths a call means: from ``lengths``, from a prefix ``mask``, or None (every item has P phonemes)."""
    if mask is not None:
        m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
        if m.shape != (B, P):
            raise ValueError(f"expected mask [{B}, {P}], got {m.shape}")
        from_mask = m.sum(axis=1).astype(np.int64)
        if not np.array_equal(m, create_padding_mask(from_mask, P)):
            raise ValueError("mask is not a prefix mask (create_padding_mask(lengths, P)): only padding at the end is supported")
        if lengths is not None and not np.array_equal(np.asarray(lengths).astype(np.int64), from_mask):
            raise ValueError("mask and lengths disagree")
        lengths = from_mask
    if lengths is None:
        return None
    lengths = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
    if lengths.shape != (B,) or not np.issubdtype(lengths.dtype, np.integer):
        raise ValueError(f"expected {B} integer lengths, got shape {lengths.shape} dtype {lengths.dtype}")
    if lengths.min(initial=1) < 1 or lengths.max(initial=1) > P:
        raise ValueError(f"lengths must lie in [1, {P}], got {lengths.tolist()}")
    return lengths.astype(np.int32)


class _TextModel(_NativeModel):
    """The two models of the text stage: their host-only queries and their tap take the config, not the handle."""

    # -- host-only queries -------------------------------------------------------------------
    def _query(self, what: str, B: int, P: int, ctype):
        lib = _native.load()
        out = ctype()
        cfg = self.native_config()
        name = f"iris_{self._abi_name}_{what}"
        _native.check(name, getattr(lib, name)(ctypes.byref(cfg), B, P, ctypes.byref(out)))
        return int(out.value)

    def launch_count(self, B: int, P: int) -> int:
        """Kernel launches of one ``forward_device`` (computed on the host, no device needed)."""
        return self._query("launch_count", B, P, ctypes.c_int32)

    def workspace_bytes(self, B: int, P: int) -> int:
        return self._query("workspace_bytes", B, P, ctypes.c_uint64)

    def _lengths_dev(self, lengths: Optional[np.ndarray]) -> Optional[torch.Tensor]:
        return None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(self._device)

    def _read_tap(self, B: int, P: int, channels: int) -> torch.Tensor:
        lib = self._ensure()
        off, n = ctypes.c_uint64(), ctypes.c_uint64()
        cfg = self.native_config()
        name = f"iris_{self._abi_name}_tap"
        _native.check(name, getattr(lib, name)(ctypes.byref(cfg), B, P, ctypes.byref(off), ctypes.byref(n)))
        raw = self._workspace[off.value:off.value + 4 * n.value].clone()
        return raw.view(torch.float32).view(B, P, channels)


class PhonemeEncoder(_TextModel):
    _abi_name = "phoneme_encoder"

    def __init__(self, vocab_size: int, embed_dim: int = 256, num_blocks: int = 4, num_heads: int = 4,
                 ffn_dim: Optional[int] = None, max_length: int = 1000, dropout: float = 0.1, name: Optional[str] = None,
                 seed: Optional[int] = None):
        super().__init__()
        self.vocab_size, self.embed_dim, self.num_blocks, self.num_heads = vocab_size, embed_dim, num_blocks, num_heads
        self.ffn_dim = ffn_dim or (4 * embed_dim)
        self.max_length, self.dropout_rate, self.name = max_length, dropout, name or "phoneme_encoder"
        if embed_dim % num_heads:
            raise ValueError(f"embed_dim {embed_dim} is not a multiple of num_heads {num_heads}")
        rng = np.random.default_rng(seed)
        E, H, F = embed_dim, num_heads, self.ffn_dim
        Dk = E // H
        w = self.weights

        def glorot(shape, fan_in, fan_out):
            limit = np.sqrt(6.0 / (fan_in + fan_out))
            return rng.uniform(-limit, limit, shape).astype(np.float32)

        def norm(prefix):
            w[f"{prefix}.gamma"] = np.ones(E, np.float32)
            w[f"{prefix}.beta"] = np.zeros(E, np.float32)

        w["phoneme_embedding.embeddings"] = rng.uniform(-0.05, 0.05, (vocab_size, E)).astype(np.float32)
        w["positional_embedding.position_embedding.embeddings"] = rng.uniform(-0.05, 0.05, (max_length, E)).astype(np.float32)
        for i in range(num_blocks):
            p = f"transformer_block_{i}"
            for part in ("query", "key", "value"):
                w[f"{p}.attention.{part}.kernel"] = glorot((E, H, Dk), E, H * Dk)
                w[f"{p}.attention.{part}.bias"] = np.zeros((H, Dk), np.float32)
            w[f"{p}.attention.output.kernel"] = glorot((H, Dk, E), H * Dk, E)
            w[f"{p}.attention.output.bias"] = np.zeros(E, np.float32)
            norm(f"{p}.attention_norm")
            w[f"{p}.ffn.0.kernel"] = glorot((E, F), E, F)
            w[f"{p}.ffn.0.bias"] = np.zeros(F, np.float32)
            w[f"{p}.ffn.2.kernel"] = glorot((F, E), F, E)
            w[f"{p}.ffn.2.bias"] = np.zeros(E, np.float32)
            norm(f"{p}.ffn_norm")
        norm("encoder_output_norm")

    def get_config(self) -> dict:
        return {"vocab_size": self.vocab_size, "embed_dim": self.embed_dim, "num_blocks": self.num_blocks,
                "num_heads": self.num_heads, "ffn_dim": self.ffn_dim, "max_length": self.max_length, "dropout": self.dropout_rate}

    def native_config(self) -> "_native.PhonemeEncoderConfig":
        return _native.PhonemeEncoderConfig(self.vocab_size, self.embed_dim, self.num_blocks, self.num_heads, self.ffn_dim,
                                            self.max_length)

    def blob(self) -> np.ndarray:
        """The weights in the order and layouts ``iris_phoneme_encoder_create`` reads (include/iris_hifigan.h): the tables
        as they are, every projection transposed to ``[C_out][C_in]``, query | key | value as one ``[3E][E]`` matrix."""
        w, E = self.weights, self.embed_dim
        parts = [w["phoneme_embedding.embeddings"].ravel(), w["positional_embedding.position_embedding.embeddings"].ravel()]
        for i in range(self.num_blocks):
            p = f"transformer_block_{i}"
            qkv = [w[f"{p}.attention.{part}.kernel"].reshape(E, E).T for part in ("query", "key", "value")]
            parts.append(np.ascontiguousarray(np.concatenate(qkv, axis=0)).ravel())
            parts.extend(w[f"{p}.attention.{part}.bias"].ravel() for part in ("query", "key", "value"))
            parts.extend([np.ascontiguousarray(w[f"{p}.attention.output.kernel"].reshape(E, E).T).ravel(),
                          w[f"{p}.attention.output.bias"], w[f"{p}.attention_norm.gamma"], w[f"{p}.attention_norm.beta"],
                          np.ascontiguousarray(w[f"{p}.ffn.0.kernel"].T).ravel(), w[f"{p}.ffn.0.bias"],
                          np.ascontiguousarray(w[f"{p}.ffn.2.kernel"].T).ravel(), w[f"{p}.ffn.2.bias"],
                          w[f"{p}.ffn_norm.gamma"], w[f"{p}.ffn_norm.beta"]])
        parts.extend([w["encoder_output_norm.gamma"], w["encoder_output_norm.beta"]])
        return np.ascontiguousarray(np.concatenate([np.asarray(x).ravel() for x in parts]), dtype=np.float32)

    def _check_ids_shape(self, shape) -> Tuple[int, int]:
        if len(shape) != 2:
            raise ValueError(f"expected phoneme_ids [B, P], got shape {tuple(shape)}")
        B, P = int(shape[0]), int(shape[1])
        if P < 1:
            raise ValueError("at least one phoneme is required")
        if P > self.max_length:
            raise ValueError(f"P = {P} exceeds max_length = {self.max_length}")
        return B, P

    def forward_device(self, ids: torch.Tensor, lengths=None) -> torch.Tensor:
        """``ids`` integer ``[B, P]`` (device tensor; not range-checked, the kernel clamps) and optional per-item lengths ->
        ``enc_out [B, P, embed_dim]`` fp32 on the device, asynchronous on the current stream; rows past an item's length
        are zeros."""
        B, P = self._check_ids_shape(tuple(ids.shape))
        lens = _lengths_from(None, lengths, B, P)
        lib = self._ensure()
        ids = ids.to(device=self._device, dtype=torch.int32).contiguous()
        out = torch.empty((B, P, self.embed_dim), dtype=torch.float32, device=self._device)
        if B == 0:
            return out
        ws = self._ws(B, P)
        lens_dev = self._lengths_dev(lens)
        _native.check("iris_phoneme_encoder_forward", lib.iris_phoneme_encoder_forward(
            self._handle, _ptr(ids), _ptr(lens_dev), B, P, _ptr(out), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out

    def _host_ids(self, phoneme_ids) -> np.ndarray:
        ids = np.asarray(phoneme_ids)
        if not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"phoneme ids must be integers, got {ids.dtype}")
        self._check_ids_shape(ids.shape)
        if ids.size and (ids.min() < 0 or ids.max() >= self.vocab_size):
            raise ValueError(f"phoneme ids must lie in [0, {self.vocab_size}), got [{ids.min()}, {ids.max()}]")
        return np.ascontiguousarray(ids, dtype=np.int32)

    def __call__(self, phoneme_ids, training: bool = False, mask=None, lengths=None):
        """Reference ``call`` (:186-212): numpy in -> numpy out, device tensors in -> device tensors out."""
        if training:
            raise NotImplementedError("the MI355X build holds the inference half only: training=True is not built")
        if isinstance(phoneme_ids, torch.Tensor):
            B, P = self._check_ids_shape(tuple(phoneme_ids.shape))
            return self.forward_device(phoneme_ids, _lengths_from(mask, lengths, B, P))
        ids = self._host_ids(phoneme_ids)
        lens = _lengths_from(mask, lengths, *ids.shape)
        if lens is not None:                                # ids past an item's length are never read
            ids = np.where(create_padding_mask(lens, ids.shape[1]), ids, 0).astype(np.int32)
        self._ensure()
        return self.forward_device(torch.from_numpy(ids).to(self._device), lens).cpu().numpy()

    call = __call__

    def _read_block0(self, B: int, P: int) -> torch.Tensor:
        """Test-only: the output of block 0 the last ``forward_device`` of shape (B, P) left in the workspace (a copy)."""
        return self._read_tap(B, P, self.embed_dim)

    def _workspace_layout(self, B: int, P: int):
        """Test-only: ``enc_ws`` (csrc/iris_text_encoder.hip) restated -- ``({buffer: (float offset, floats)}, total floats)``
        in the struct's order: x0, x1, t0 (rows x E), qkv (rows x 3E), attn (rows x E), ffn (rows x ffn_dim).  Needs no device."""
        rows, E = B * P, self.embed_dim
        return _take_buffers((("x0", rows * E), ("x1", rows * E), ("t0", rows * E), ("qkv", rows * 3 * E), ("attn", rows * E),
                              ("ffn", rows * self.ffn_dim)))

    def _read_buffers(self, B: int, P: int):
        """Test-only: every workspace buffer as the last ``forward_device`` of shape (B, P) left it -- ``({buffer: flat fp32
        copy}, bytes of the layout)``.  Which launch wrote a buffer last is the reader's to know (``enc_forward``)."""
        return _read_buffers(self, *self._workspace_layout(B, P))


class DurationPredictor(_TextModel):
    """``in_dim``: channels of the encoder output (Keras builds the first conv lazily; ``hidden_dim`` when omitted, as in the
    reference's scripts).  ``max_frames_per_phoneme``: the upper clip of ``predict_durations`` (1e6 in the reference)."""

    _abi_name = "duration_predictor"

    def __init__(self, hidden_dim: int = 256, num_layers: int = 2, kernel_size: int = 3, dropout: float = 0.1,
                 in_dim: Optional[int] = None, max_frames_per_phoneme: int = 1_000_000, name: Optional[str] = None,
                 seed: Optional[int] = None):
        super().__init__()
        self.hidden_dim, self.num_layers, self.kernel_size, self.dropout_rate = hidden_dim, num_layers, kernel_size, dropout
        self.in_dim = in_dim or hidden_dim
        self.max_frames_per_phoneme, self.name = int(max_frames_per_phoneme), name or "duration_predictor"
        rng = np.random.default_rng(seed)
        w = self.weights
        for i in range(num_layers):
            c_in = self.in_dim if i == 0 else hidden_dim
            limit = np.sqrt(6.0 / ((c_in + hidden_dim) * kernel_size))
            w[f"duration_conv_{i}.kernel"] = rng.uniform(-limit, limit, (kernel_size, c_in, hidden_dim)).astype(np.float32)
            w[f"duration_conv_{i}.bias"] = np.zeros(hidden_dim, np.float32)
            w[f"duration_norm_{i}.gamma"] = np.ones(hidden_dim, np.float32)
            w[f"duration_norm_{i}.beta"] = np.zeros(hidden_dim, np.float32)
        c = self.out_channels
        limit = np.sqrt(6.0 / (c + 1))
        w["duration_output.kernel"] = rng.uniform(-limit, limit, (1, c, 1)).astype(np.float32)
        w["duration_output.bias"] = np.zeros(1, np.float32)

    @property
    def out_channels(self) -> int:
        return self.hidden_dim if self.num_layers else self.in_dim

    def get_config(self) -> dict:
        return {"hidden_dim": self.hidden_dim, "num_layers": self.num_layers, "kernel_size": self.kernel_size,
                "dropout": self.dropout_rate}

    def native_config(self) -> "_native.DurationPredictorConfig":
        return _native.DurationPredictorConfig(self.in_dim, self.hidden_dim, self.num_layers, self.kernel_size,
                                               self.max_frames_per_phoneme)

    def blob(self) -> np.ndarray:
        """The weights as ``iris_duration_predictor_create`` reads them: convs transposed to ``[C_out][C_in][k]``."""
        w = self.weights
        parts = []
        for i in range(self.num_layers):
            parts.extend([np.ascontiguousarray(w[f"duration_conv_{i}.kernel"].transpose(2, 1, 0)).ravel(), w[f"duration_conv_{i}.bias"],
                          w[f"duration_norm_{i}.gamma"], w[f"duration_norm_{i}.beta"]])
        parts.extend([w["duration_output.kernel"].ravel(), w["duration_output.bias"]])
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    def _check_enc(self, shape) -> Tuple[int, int]:
        if len(shape) != 3 or shape[2] != self.in_dim:
            raise ValueError(f"expected encoder_output [B, P, {self.in_dim}], got {tuple(shape)}")
        if shape[1] < 1:
            raise ValueError("at least one phoneme is required")
        return int(shape[0]), int(shape[1])

    def forward_device(self, enc_out: torch.Tensor, lengths=None):
        """``enc_out [B, P, in_dim]`` -> ``(pred [B, P] fp32, frames [B, P] int32, offsets [B, P + 1] int32, totals [B]
        int32)`` on the device, asynchronous on the current stream: the softplus output, ``predict_durations`` of it, the
        exclusive prefix sum of each item's frames and their sums.  Positions past an item's length hold 0."""
        B, P = self._check_enc(tuple(enc_out.shape))
        lens = _lengths_from(None, lengths, B, P)
        lib = self._ensure()
        enc_out = enc_out.to(device=self._device, dtype=torch.float32).contiguous()
        pred = torch.empty((B, P), dtype=torch.float32, device=self._device)
        frames = torch.empty((B, P), dtype=torch.int32, device=self._device)
        offsets = torch.empty((B, P + 1), dtype=torch.int32, device=self._device)
        totals = torch.empty((B,), dtype=torch.int32, device=self._device)
        if B == 0:
            return pred, frames, offsets, totals
        ws = self._ws(B, P)
        lens_dev = self._lengths_dev(lens)
        _native.check("iris_duration_predictor_forward", lib.iris_duration_predictor_forward(
            self._handle, _ptr(enc_out), _ptr(lens_dev), B, P, _ptr(pred), _ptr(frames), _ptr(offsets), _ptr(totals), _ptr(ws),
            ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return pred, frames, offsets, totals

    def __call__(self, encoder_output, training: bool = False, lengths=None):
        """Reference ``call`` (:288-315): ``[B, P, in_dim]`` -> the softplus output ``[B, P, 1]``."""
        if training:
            raise NotImplementedError("the MI355X build holds the inference half only: training=True is not built")
        if isinstance(encoder_output, torch.Tensor):
            return self.forward_device(encoder_output, lengths)[0].unsqueeze(-1)
        enc = np.ascontiguousarray(np.asarray(encoder_output, dtype=np.float32))
        self._check_enc(enc.shape)
        self._ensure()
        return self.forward_device(torch.from_numpy(enc).to(self._device), lengths)[0].cpu().numpy()[..., None]

    call = __call__

    def _read_layer0(self, B: int, P: int) -> torch.Tensor:
        """Test-only: the output of the first layer the last ``forward_device`` of shape (B, P) left in the workspace."""
        return self._read_tap(B, P, self.hidden_dim)

    def _workspace_layout(self, B: int, P: int):
        """Test-only: ``dur_ws`` restated, as ``PhonemeEncoder._workspace_layout``: d0, d1, d2 (rows x hidden_dim); layer 0
        writes d0, the later layers alternate d2, d1."""
        n = B * P * self.hidden_dim
        return _take_buffers((("d0", n), ("d1", n), ("d2", n)))

    def _read_buffers(self, B: int, P: int):
        """Test-only, as ``PhonemeEncoder._read_buffers`` (``dur_forward``)."""
        return _read_buffers(self, *self._workspace_layout(B, P))


def create_encoder(vocab_size: int, embed_dim: int = 256, num_blocks: int = 4, num_heads: int = 4, **kwargs) -> PhonemeEncoder:
    return PhonemeEncoder(vocab_size=vocab_size, embed_dim=embed_dim, num_blocks=num_blocks, num_heads=num_heads, **kwargs)


def create_duration_predictor(hidden_dim: int = 256, **kwargs) -> DurationPredictor:
    return DurationPredictor(hidden_dim=hidden_dim, **kwargs)


def predict_durations(encoder_out, duration_head: DurationPredictor, lengths=None):
    """``scripts/synthesize.py:41-45``: int32 frames ``[B, P]`` = ``clip(round(exp(pred) - 1), 1, 1e6)``; numpy in -> numpy
    out, device tensor in -> device tensor out."""
    if isinstance(encoder_out, torch.Tensor):
        return duration_head.forward_device(encoder_out, lengths)[1]
    enc = np.ascontiguousarray(np.asarray(encoder_out, dtype=np.float32))
    duration_head._check_enc(enc.shape)
    duration_head._ensure()
    return duration_head.forward_device(torch.from_numpy(enc).to(duration_head._device), lengths)[1].cpu().numpy()


# ---- length regulator ----------------------------------------------------------------------------
def _host_durations(durations, B: int, P: int, lengths: Optional[np.ndarray], max_frames: Optional[int]) -> np.ndarray:
    d = np.asarray(durations.cpu() if isinstance(durations, torch.Tensor) else durations)
    if d.shape != (B, P):
        raise ValueError(f"expected durations [{B}, {P}], got {d.shape}")
    if not np.issubdtype(d.dtype, np.integer):
        raise ValueError(f"durations must be integer frame counts, got {d.dtype}")
    if d.size and d.min() < 0:
        raise ValueError("durations must be >= 0")
    d = d.astype(np.int64)
    if lengths is not None:
        d = np.where(create_padding_mask(lengths, P), d, 0)
    total = int(d.sum(axis=1).max(initial=0))
    if total > (max_frames if max_frames is not None else 2 ** 31 - 1):
        raise ValueError(f"durations sum to {total} frames, more than max_frames = {max_frames}")
    return d.astype(np.int32)


def scan_device(frames: torch.Tensor, lengths_dev: Optional[torch.Tensor] = None):
    """int32 device frames ``[B, P]`` -> ``(offsets [B, P + 1], totals [B])`` (``iris_length_scan``), asynchronous."""
    lib = _native.load()
    B, P = int(frames.shape[0]), int(frames.shape[1])
    frames = frames.to(dtype=torch.int32).contiguous()
    offsets = torch.empty((B, P + 1), dtype=torch.int32, device=frames.device)
    totals = torch.empty((B,), dtype=torch.int32, device=frames.device)
    if B:
        with torch.cuda.device(frames.device):
            _native.check("iris_length_scan", lib.iris_length_scan(_ptr(frames), _ptr(lengths_dev), B, P, _ptr(offsets), _ptr(totals),
                                                                   _stream(frames.device)))
    return offsets, totals


def regulate_device(enc_out: torch.Tensor, offsets: torch.Tensor, totals: torch.Tensor, T_pad: int) -> torch.Tensor:
    """``cond [B, T_pad, E]``: row t of item b is the encoder row of the phoneme whose frames cover t, 0 from ``totals[b]``
    on (``iris_length_regulate``), asynchronous on the current stream."""
    lib = _native.load()
    B, P, E = (int(s) for s in enc_out.shape)
    enc_out = enc_out.to(dtype=torch.float32).contiguous()
    cond = torch.empty((B, int(T_pad), E), dtype=torch.float32, device=enc_out.device)
    if B and T_pad:
        with torch.cuda.device(enc_out.device):
            _native.check("iris_length_regulate", lib.iris_length_regulate(_ptr(enc_out), _ptr(offsets), _ptr(totals), B, P, E, int(T_pad),
                                                                           _ptr(cond), _stream(enc_out.device)))
    return cond


def _pad_to(n: int, factor: int) -> int:
    return -(-n // factor) * factor


def length_regulate(encoder_output, durations, factor: int = 1):
    """Reference ``length_regulate`` (:378-416): ``[B, P, E]`` and integer durations ``[B, P]`` -> ``[B, T, E]`` with
    ``T = max_b sum(durations[b])`` (rounded up to ``factor``); numpy in -> numpy out, device tensor in -> device tensor
    out.  Frames past an item's own total are ZEROS (what ``scripts/synthesize.py:117-122`` pads with); the reference's
    jitted batch form fills them with a repeated row instead, which nothing downstream reads."""
    host = not isinstance(encoder_output, torch.Tensor)
    shape = tuple(np.shape(encoder_output)) if host else tuple(encoder_output.shape)
    if len(shape) != 3:
        raise ValueError(f"expected encoder_output [B, P, E], got {shape}")
    d = _host_durations(durations, shape[0], shape[1], None, None)
    device = require_gpu() if host else encoder_output.device
    enc = torch.from_numpy(np.ascontiguousarray(np.asarray(encoder_output, dtype=np.float32))).to(device) if host else encoder_output
    offsets, totals = scan_device(torch.from_numpy(d).to(device))
    cond = regulate_device(enc, offsets, totals, _pad_to(int(d.sum(axis=1).max(initial=0)), factor))
    return cond.cpu().numpy() if host else cond


def frame_conditioning(encoder: PhonemeEncoder, duration_head: Optional[DurationPredictor], ids, lengths=None, durations=None,
                       factor: int = 4, max_frames: int = DEFAULT_MAX_FRAMES):
    """Phoneme ids ``[B, P]`` -> ``(cond [B, T_pad, embed_dim] on the device, frames_per_item)``: encoder, duration head,
    prefix sum and gather on the current stream (``scripts/synthesize.py:107-122``).  ``frames_per_item[b]`` is item b's
    frame total; ``T_pad`` is the largest of them rounded up to ``factor`` (``2^down_stages`` of the VAE), and rows from an
    item's total on are zeros.  The totals (``B`` int32) are read back -- the one synchronising copy of the stage.
    ``durations`` (integer ``[B, P]``, >= 0, host) replaces the head's prediction, e.g. an aligner's; the duration head may
    then be None.  A total above ``max_frames`` raises ``ValueError`` before the conditioning is allocated."""
    if isinstance(ids, torch.Tensor):
        B, P = encoder._check_ids_shape(tuple(ids.shape))
        lens = _lengths_from(None, lengths, B, P)
        ids_dev = ids
    else:
        host_ids = encoder._host_ids(ids)
        B, P = host_ids.shape
        lens = _lengths_from(None, lengths, B, P)
        if lens is not None:
            host_ids = np.where(create_padding_mask(lens, P), host_ids, 0).astype(np.int32)
        ids_dev = None
    if durations is not None:
        d = _host_durations(durations, B, P, lens, max_frames)     # before any launch
    elif duration_head is None:
        raise ValueError("frame_conditioning needs a duration head or durations=")
    encoder._ensure()
    if ids_dev is None:
        ids_dev = torch.from_numpy(host_ids).to(encoder._device)
    enc_out = encoder.forward_device(ids_dev, lens)
    if durations is not None:
        offsets, totals = scan_device(torch.from_numpy(d).to(enc_out.device), encoder._lengths_dev(lens))
        per_item = [int(t) for t in d.sum(axis=1)]
    else:
        _, _, offsets, totals = duration_head.forward_device(enc_out, lens)
        per_item = [int(t) for t in totals.cpu().tolist()]          # the stage's one read-back
        if max(per_item, default=0) > max_frames:
            raise ValueError(f"the duration head predicts {max(per_item)} frames, more than max_frames = {max_frames}")
    cond = regulate_device(enc_out, offsets, totals, _pad_to(max(per_item, default=0), factor))
    return cond, per_item
