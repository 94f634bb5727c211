"""MI355X drop-in for the inference half of the reference module ``iris.vae`` (TextConditionedVAE, Keras/JAX).

Call surface kept from the reference's ``src/iris/vae.py``: the constructor ``TextConditionedVAE(n_mels, cond_dim,
model_channels=192, latent_dim=16, num_wavenet_blocks=8, decoder_blocks=4, wavenet_kernel_size=5, down_stages=2,
flow_layers=4, flow_hidden=64, dropout=0.1, name=None)`` (:263-351) and ``generate(frame_text_cond, z_prior=None) ->
(mel [B, n_mels, T], residual [B, T, cond_dim])`` (:448-482), which ``scripts/synthesize.py:125-145`` calls right before
the PostNet.  ``TextConditionedVAE`` holds the decoder half only: its ``__call__`` raises, and encoder-side keys in a
weight file are ignored by it.  The encoder half (``in_proj``, ``enc_blocks``, ``latent_*_proj``) is
``VAEPosteriorEncoder``, and ``reconstruct(encoder, vae, mels, frame_text_cond)`` is the reference's
``call(training=False)`` (:366-422) over the two: posterior statistics, forward flow, decoded reconstruction -- with
``lengths=`` over a ragged batch of recorded utterances in one pass, and with ``losses=True`` followed by ``vae_losses``,
the masked ``compute_recon_l1`` / ``compute_kl`` (:424-446) reduced on the device.

    h = in_proj(mels^T)                                 # the mel arrives channels-first [B, n_mels, T]           :382-385
    for i, block in enumerate(enc_blocks):              # WaveNetResBlock, dilation 2^(i % 4), FiLM on frame_cond :388-389
        g, b = split(block.film.proj(frame_cond)); h = h + block.res_proj(g * gelu(block.conv(h)) + b)
    lat_h = downsample(h)                               # the weights lat_cond goes through                       :393
    mean, logvar = latent_mean_proj(lat_h), latent_logvar_proj(lat_h);  z = mean                                 :396-398
    z_flow = flow(z, lat_cond, reverse=False)           # couplings in order, x2 + (g * t + b)                    :401
    then latent_dec_proj, dec_blocks, upsample, out_proj / residual_proj as in generate() below.

    lat_cond = downsample(down_cond_proj(frame_cond))   # 1x1 conv, then S x (Conv1D k5 stride 2 'same' + gelu)   :360-364
    z = z_prior                                         # [B, T / 2^S, latent_dim]
    for coupling in reversed(flow layers):              # APCoupling, reverse=True                               :182-208
        x1, x2 = split(z); ce = gelu(cond_proj(lat_cond))
        t = net_post(gelu(net_pre(x1 + ce)));  g, b = split(film.proj(ce));  z = concat(x1, x2 - (g * t + b))
    d = latent_dec_proj(z)
    for i, block in enumerate(dec_blocks):              # WaveNetResBlock, dilation 2^(i % 4)                    :57-67
        h = gelu(conv(d)); g, b = split(film.proj(lat_cond)); d = d + res_proj(g * h + b)
    for each upsample stage: d = gelu(Conv1D_k5_same(repeat_each_row_twice(d)))                                  :141-147
    mel = transpose(out_proj(d));  residual = residual_proj(d)

Keras cannot run in this pipeline, so the conventions below are ASSUMPTIONS read from the Keras 3 / XLA documentation,
pinned by the numpy restatement the tests compare against (``tests/vae_restatement.py``) -- "parity unpinned", as for
``iris.postnet``:
  * ``Conv1D`` kernels are ``[k, C_in, C_out]`` and the layer is a cross-correlation.
  * ``padding='same'``, stride 1: ``dilation * (k - 1) / 2`` zeros on both sides.
  * ``padding='same'``, stride 2, k = 5, even input length: 1 zero on the left and 2 on the right, i.e.
    ``y[i] = sum_kappa x[2 i - 1 + kappa] W[kappa]`` (the TF/XLA SAME rule, ``pad_left = total // 2``).
  * ``Dense`` is ``x @ kernel[in, out] + bias``.
  * ``ops.split(x, 2, axis=-1)`` returns the first half of the channels first (gamma, then beta).
  * ``ops.gelu`` is the tanh approximation (Keras 3 default ``approximate=True``):
    ``0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))``.
  * ``Dropout`` is the identity at inference.

Parameters are kept in the Keras layouts under attribute-path names (``down_cond_proj.kernel``,
``downsample.blocks.0.bias``, ``vpflow.ap_2.net_pre.kernel``, ``dec_block_1.film.proj.kernel``,
``upsample.refine.0.kernel``, ...).  ``generate`` assumes ``T % 2^down_stages == 0`` as the reference does
(``synthesize.py:117-122`` pads to it); other lengths raise ``ValueError`` -- nothing is padded silently.
``.weights.h5`` files need h5py; ``load_weights`` / ``save_weights`` use ``.npz``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native_model import _NativeModel, _ptr, _stream, _take_buffers


def check_lengths(lengths, B: int, T: int, factor: int):
    """``lengths`` of a ragged call -> an int32 device tensor, passed through unread, or a validated int32 host array.
    Host lengths are checked here, before any device work; a device tensor is sanitised by the kernels instead."""
    if isinstance(lengths, torch.Tensor) and lengths.device.type != "cpu":
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise ValueError(f"device lengths must be an int32 tensor of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        return lengths
    arr = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
    if arr.ndim != 1 or arr.shape[0] != B:
        raise ValueError(f"lengths must hold {B} frame counts (one per item), got shape {tuple(arr.shape)}")
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"lengths must be integers, got {arr.dtype}")
    arr = arr.astype(np.int64)
    for b, n in enumerate(arr.tolist()):
        if not 0 <= n <= T:
            raise ValueError(f"lengths[{b}] = {n} is outside [0, T = {T}]")
        if n % factor:
            raise ValueError(f"lengths[{b}] = {n} is not a multiple of 2^down_stages = {factor}: pad the "
                             "item first; nothing is padded silently")
    return arr.astype(np.int32)


def _lengths_on(lengths, device) -> torch.Tensor:
    """What ``check_lengths`` returned, as a contiguous int32 tensor on ``device``."""
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.from_numpy(lengths)
    return lengths.to(device).contiguous()


def _read_buffers(model, layout, total):
    ws = model._workspace.view(torch.float32)
    return {name: ws[off:off + n].clone() for name, (off, n) in layout.items()}, 4 * total


class TextConditionedVAE(_NativeModel):
    _abi_name = "vae_decoder"

    #: ``generate`` / ``generate_device`` take ``lengths=`` (a ragged batch in one forward); ``MelToWavePipeline`` checks this
    takes_lengths = True

    def __init__(self, n_mels: int, cond_dim: int, model_channels: int = 192, latent_dim: int = 16,
                 num_wavenet_blocks: int = 8, decoder_blocks: int = 4, wavenet_kernel_size: int = 5, down_stages: int = 2,
                 flow_layers: int = 4, flow_hidden: int = 64, dropout: float = 0.1, name: Optional[str] = None,
                 seed: Optional[int] = None):
        if latent_dim % 2:
            raise ValueError("Flow channels must be even.")                      # vae.py:223
        self.n_mels, self.cond_dim, self.model_channels, self.latent_dim = n_mels, cond_dim, model_channels, latent_dim
        self.num_wavenet_blocks, self.decoder_blocks = num_wavenet_blocks, decoder_blocks      # (the first: encoder side)
        self.wavenet_kernel_size, self.down_stages = wavenet_kernel_size, down_stages
        self.flow_layers, self.flow_hidden = flow_layers, flow_hidden
        self.dropout_rate, self.name = dropout, name or "text_conditioned_vae"
        super().__init__()
        rng = np.random.default_rng(seed)

        def conv(prefix, k, c_in, c_out, zero=False):
            limit = np.sqrt(6.0 / ((c_in + c_out) * k))                          # glorot_uniform
            w = np.zeros((k, c_in, c_out)) if zero else rng.uniform(-limit, limit, (k, c_in, c_out))
            self.weights[f"{prefix}.kernel"] = w.astype(np.float32)
            self.weights[f"{prefix}.bias"] = np.zeros(c_out, np.float32)

        def dense(prefix, c_in, c_out):
            limit = np.sqrt(6.0 / (c_in + c_out))
            self.weights[f"{prefix}.kernel"] = rng.uniform(-limit, limit, (c_in, c_out)).astype(np.float32)
            self.weights[f"{prefix}.bias"] = np.zeros(c_out, np.float32)

        C, half = model_channels, latent_dim // 2
        conv("down_cond_proj", 1, cond_dim, C)
        for s in range(down_stages):
            conv(f"downsample.blocks.{s}", 5, C, C)
        for j in range(flow_layers):
            p = f"vpflow.ap_{j}"
            dense(f"{p}.cond_proj", C, half)
            conv(f"{p}.net_pre", 3, half, flow_hidden)
            conv(f"{p}.net_post", 1, flow_hidden, half, zero=True)               # zero-initialised, vae.py:172-178
            dense(f"{p}.film.proj", half, 2 * half)
        dense("latent_dec_proj", latent_dim, C)
        for i in range(decoder_blocks):
            p = f"dec_block_{i}"
            conv(f"{p}.conv", wavenet_kernel_size, C, C)
            dense(f"{p}.film.proj", C, 2 * C)
            conv(f"{p}.res_proj", 1, C, C)
        for s in range(down_stages):
            conv(f"upsample.refine.{s}", 5, C, C)
        conv("out_proj", 1, C, n_mels)
        dense("residual_proj", C, cond_dim)

    def get_config(self) -> dict:
        return {"n_mels": self.n_mels, "cond_dim": self.cond_dim, "model_channels": self.model_channels,
                "latent_dim": self.latent_dim, "num_wavenet_blocks": self.num_wavenet_blocks,
                "decoder_blocks": self.decoder_blocks, "wavenet_kernel_size": self.wavenet_kernel_size,
                "down_stages": self.down_stages, "flow_layers": self.flow_layers, "flow_hidden": self.flow_hidden,
                "dropout": self.dropout_rate}

    @property
    def downsample_factor(self) -> int:
        return 2 ** self.down_stages

    # -- parameters (set_weights_dict ignores the encoder half of a full checkpoint) ----------
    def native_config(self) -> "_native.VaeDecoderConfig":
        return _native.VaeDecoderConfig(self.n_mels, self.cond_dim, self.model_channels, self.latent_dim, self.decoder_blocks,
                                        self.wavenet_kernel_size, self.down_stages, self.flow_layers, self.flow_hidden)

    def blob(self) -> np.ndarray:
        """The weights in the order and layouts ``iris_vae_decoder_create`` reads (include/iris_hifigan.h): convolutions and
        Dense layers that run as GEMMs transposed to ``[C_out][C_in][k]``, the flow's small tensors as Keras stores them."""
        w = self.weights
        parts = []

        def gemm(prefix):                        # Conv1D [k, in, out] or Dense [in, out] -> [out][in][k]
            k = w[f"{prefix}.kernel"]
            k = k[None] if k.ndim == 2 else k
            parts.extend([np.ascontiguousarray(k.transpose(2, 1, 0)).ravel(), w[f"{prefix}.bias"].ravel()])

        def raw(prefix):
            parts.extend([w[f"{prefix}.kernel"].ravel(), w[f"{prefix}.bias"].ravel()])

        gemm("down_cond_proj")
        for s in range(self.down_stages):
            gemm(f"downsample.blocks.{s}")
        for j in range(self.flow_layers):
            p = f"vpflow.ap_{j}"
            gemm(f"{p}.cond_proj")
            raw(f"{p}.net_pre"); raw(f"{p}.net_post"); raw(f"{p}.film.proj")
        raw("latent_dec_proj")
        for i in range(self.decoder_blocks):
            p = f"dec_block_{i}"
            gemm(f"{p}.conv"); gemm(f"{p}.film.proj"); gemm(f"{p}.res_proj")
        for s in range(self.down_stages):
            gemm(f"upsample.refine.{s}")
        gemm("out_proj")
        gemm("residual_proj")
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    # -- execution ---------------------------------------------------------------------------
    def _check_cond(self, shape) -> Tuple[int, int]:
        if len(shape) != 3 or shape[2] != self.cond_dim:
            raise ValueError(f"expected frame_text_cond [B, T, {self.cond_dim}], got {tuple(shape)}")
        B, T = int(shape[0]), int(shape[1])
        if T % self.downsample_factor:
            raise ValueError(f"T = {T} is not a multiple of 2^down_stages = {self.downsample_factor}: pad the conditioning "
                             "first (scripts/synthesize.py:117-122 does); nothing is padded silently")
        return B, T

    def _check_lengths(self, lengths, B: int, T: int):
        """``check_lengths`` with this model's ``2^down_stages``."""
        return check_lengths(lengths, B, T, self.downsample_factor)

    def launch_count(self, B: int, T: int) -> int:
        """Kernel launches of one ``generate_device(..., want_residual=True)`` (one fewer without the residual)."""
        lib = self._ensure()
        n = ctypes.c_int32()
        _native.check("iris_vae_decoder_launch_count", lib.iris_vae_decoder_launch_count(self._handle, B, T, ctypes.byref(n)))
        return int(n.value)

    def generate_device(self, cond: torch.Tensor, z_prior: Optional[torch.Tensor] = None, want_residual: bool = True,
                        generator: Optional[torch.Generator] = None, lengths=None):
        """``cond [B, T, cond_dim]``, ``z_prior [B, T / 2^S, latent_dim]`` (fp32 device tensors) -> ``(mel [B, n_mels, T],
        residual [B, T, cond_dim] or None)``, asynchronous on the current stream; the mel is contiguous and channels-first,
        as ``PostNet.forward_device`` and ``GeneratorEngine.forward`` read it.  ``z_prior=None`` draws ``torch.randn`` on the
        device (from ``generator`` when given): a standard normal as in the reference, but NOT the numbers JAX would draw
        from ``SeedGenerator(1337)`` -- pass ``z_prior`` to reproduce a reference run.

        ``lengths`` (``B`` frame counts: a host sequence or numpy array, or an int32 device tensor) makes the batch ragged in
        ONE forward (``iris_vae_decoder_forward_ragged``): item b is bit for bit the batch-of-one call on ``cond[b:b+1,
        :lengths[b]]`` and ``z_prior[b:b+1, :lengths[b] / 2^S]``, ``mel[b, :, lengths[b]:]`` and ``residual[b, lengths[b]:]``
        are 0, and ``cond`` / ``z_prior`` rows past an item's length are never read.  Host lengths must lie in ``[0, T]`` and
        be multiples of ``2^S`` (``ValueError`` otherwise, before any device work); a device tensor is never read by the
        host -- the kernels clamp it to ``[0, T]`` and round it down to a multiple of ``2^S``."""
        B, T = self._check_cond(tuple(cond.shape))
        if lengths is not None:
            lengths = self._check_lengths(lengths, B, T)
        lib = self._ensure()
        cond = cond.to(device=self._device, dtype=torch.float32).contiguous()
        Tq = T // self.downsample_factor
        if z_prior is None:
            z_prior = torch.randn((B, Tq, self.latent_dim), device=self._device, dtype=torch.float32, generator=generator)
        elif tuple(z_prior.shape) != (B, Tq, self.latent_dim):
            raise ValueError(f"expected z_prior [{B}, {Tq}, {self.latent_dim}], got {tuple(z_prior.shape)}")
        z_prior = z_prior.to(device=self._device, dtype=torch.float32).contiguous()
        mel = torch.empty((B, self.n_mels, T), dtype=torch.float32, device=self._device)
        residual = torch.empty((B, T, self.cond_dim), dtype=torch.float32, device=self._device) if want_residual else None
        if B == 0 or T == 0:
            return mel, residual
        ws = self._ws(B, T)
        out = (_ptr(mel), _ptr(residual), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device))
        if lengths is None:
            _native.check("iris_vae_decoder_forward", lib.iris_vae_decoder_forward(self._handle, _ptr(cond), _ptr(z_prior), B, T, *out))
            return mel, residual
        lengths = _lengths_on(lengths, self._device)
        _native.check("iris_vae_decoder_forward_ragged", lib.iris_vae_decoder_forward_ragged(
            self._handle, _ptr(cond), _ptr(z_prior), B, T, _ptr(lengths), *out))
        return mel, residual

    def generate(self, frame_text_cond, z_prior=None, generator: Optional[torch.Generator] = None, lengths=None):
        """Reference ``generate`` (vae.py:448-482): numpy in -> numpy out, device tensors in -> device tensors out.
        ``lengths``: a ragged batch, as in ``generate_device``."""
        if isinstance(frame_text_cond, torch.Tensor):
            return self.generate_device(frame_text_cond, z_prior, True, generator, lengths)
        cond = np.ascontiguousarray(np.asarray(frame_text_cond, dtype=np.float32))
        B, T = self._check_cond(cond.shape)
        if lengths is not None:
            lengths = self._check_lengths(lengths, B, T)
        self._ensure()
        z = None if z_prior is None else torch.from_numpy(np.ascontiguousarray(np.asarray(z_prior, dtype=np.float32))).to(self._device)
        mel, residual = self.generate_device(torch.from_numpy(cond).to(self._device), z, True, generator, lengths)
        return mel.cpu().numpy(), residual.cpu().numpy()

    def decode_posterior_device(self, cond: torch.Tensor, z: torch.Tensor, want_residual: bool = True, lengths=None):
        """The decoder half of the reference's ``call(training=False)`` (vae.py:401-422): ``z [B, T / 2^S, latent_dim]`` is a
        posterior latent (``VAEPosteriorEncoder.encode_device``'s mean) and the flow runs forwards; shapes, outputs and
        launches are ``generate_device``'s (``iris_vae_decoder_forward_posterior``), and so is ``lengths``
        (``iris_vae_decoder_forward_posterior_ragged``)."""
        B, T = self._check_cond(tuple(cond.shape))
        if lengths is not None:
            lengths = self._check_lengths(lengths, B, T)
        Tq = T // self.downsample_factor
        if tuple(z.shape) != (B, Tq, self.latent_dim):
            raise ValueError(f"expected z [{B}, {Tq}, {self.latent_dim}], got {tuple(z.shape)}")
        lib = self._ensure()
        cond = cond.to(device=self._device, dtype=torch.float32).contiguous()
        z = z.to(device=self._device, dtype=torch.float32).contiguous()
        mel = torch.empty((B, self.n_mels, T), dtype=torch.float32, device=self._device)
        residual = torch.empty((B, T, self.cond_dim), dtype=torch.float32, device=self._device) if want_residual else None
        if B == 0 or T == 0:
            return mel, residual
        ws = self._ws(B, T)
        out = (_ptr(mel), _ptr(residual), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device))
        if lengths is None:
            _native.check("iris_vae_decoder_forward_posterior", lib.iris_vae_decoder_forward_posterior(
                self._handle, _ptr(cond), _ptr(z), B, T, *out))
            return mel, residual
        lengths = _lengths_on(lengths, self._device)
        _native.check("iris_vae_decoder_forward_posterior_ragged", lib.iris_vae_decoder_forward_posterior_ragged(
            self._handle, _ptr(cond), _ptr(z), B, T, _ptr(lengths), *out))
        return mel, residual

    def _read_tap(self, which: int, B: int, T: int) -> torch.Tensor:
        """Test-only: the intermediate ``which`` (``_native.VAE_TAP_*``) the last ``generate_device`` of shape (B, T) left in
        the workspace, ``[B, T / 2^S, model_channels]`` (a copy)."""
        lib = self._ensure()
        off, n = ctypes.c_uint64(), ctypes.c_uint64()
        _native.check("iris_vae_decoder_tap", lib.iris_vae_decoder_tap(self._handle, B, T, which, ctypes.byref(off), ctypes.byref(n)))
        raw = self._workspace[off.value:off.value + 4 * n.value].clone()
        return raw.view(torch.float32).view(B, T // self.downsample_factor, self.model_channels)

    def _workspace_layout(self, B: int, T: int):
        """Test-only: ``vae_ws`` (csrc/iris_vae_decoder.hip) restated -- ``({buffer: (float offset, floats)}, total floats)``
        in the struct's order: p, q (frames x C), latcond (latent rows x C), film (latent rows x film_cols), d0, da, db
        (latent rows x C).  Needs no device."""
        C, frames = self.model_channels, B * T
        lat = frames >> self.down_stages
        hp = (self.latent_dim // 2 + 3) & ~3
        film_cols = self.decoder_blocks * 2 * C + self.flow_layers * hp
        return _take_buffers((("p", frames * C), ("q", frames * C), ("latcond", lat * C), ("film", lat * film_cols),
                              ("d0", lat * C), ("da", lat * C), ("db", lat * C)))

    def _read_buffers(self, B: int, T: int):
        """Test-only: every workspace buffer as the last forward of shape (B, T) left it -- ``({buffer: flat fp32 copy},
        bytes of the layout)``.  Which launch wrote a buffer last is the reader's to know (``vae_forward``)."""
        return _read_buffers(self, *self._workspace_layout(B, T))

    def __call__(self, mels_bt_f=None, frame_text_cond=None, training: bool = False):
        raise NotImplementedError("the MI355X build holds the inference half only (generate()): the encoder of "
                                  "TextConditionedVAE.call() and training are not built")

    call = __call__


class VAEPosteriorEncoder(_NativeModel):
    """The encoder half of the reference's ``TextConditionedVAE`` (vae.py:294-325, 381-398): mel ``[B, n_mels, T]`` and frame
    conditioning ``[B, T, cond_dim]`` -> posterior ``(mean, logvar)``, ``[B, T / 2^S, latent_dim]`` each.  Weights under the
    reference's attribute paths: ``in_proj.*``, ``enc_block_{i}.conv.*`` / ``.film.proj.*`` / ``.res_proj.*``,
    ``downsample.blocks.{s}.*`` (the tensors ``TextConditionedVAE`` holds too: the reference has one set),
    ``latent_mean_proj.*``, ``latent_logvar_proj.*``.  One full-checkpoint ``.npz`` loads into both classes."""

    _abi_name = "vae_encoder"

    #: ``encode`` / ``encode_device`` take ``lengths=`` (a ragged batch in one forward)
    takes_lengths = True

    def __init__(self, n_mels: int, cond_dim: int, model_channels: int = 192, latent_dim: int = 16,
                 num_wavenet_blocks: int = 8, wavenet_kernel_size: int = 5, down_stages: int = 2,
                 seed: Optional[int] = None):
        self.n_mels, self.cond_dim, self.model_channels, self.latent_dim = n_mels, cond_dim, model_channels, latent_dim
        self.num_wavenet_blocks, self.wavenet_kernel_size, self.down_stages = num_wavenet_blocks, wavenet_kernel_size, down_stages
        super().__init__()
        rng = np.random.default_rng(seed)

        def conv(prefix, k, c_in, c_out):
            limit = np.sqrt(6.0 / ((c_in + c_out) * k))                          # glorot_uniform
            self.weights[f"{prefix}.kernel"] = rng.uniform(-limit, limit, (k, c_in, c_out)).astype(np.float32)
            self.weights[f"{prefix}.bias"] = np.zeros(c_out, np.float32)

        def dense(prefix, c_in, c_out, zero=False):
            limit = np.sqrt(6.0 / (c_in + c_out))
            w = np.zeros((c_in, c_out)) if zero else rng.uniform(-limit, limit, (c_in, c_out))
            self.weights[f"{prefix}.kernel"] = w.astype(np.float32)
            self.weights[f"{prefix}.bias"] = np.zeros(c_out, np.float32)

        C = model_channels
        conv("in_proj", 1, n_mels, C)
        for i in range(num_wavenet_blocks):
            p = f"enc_block_{i}"
            conv(f"{p}.conv", wavenet_kernel_size, C, C)
            dense(f"{p}.film.proj", cond_dim, 2 * C)
            conv(f"{p}.res_proj", 1, C, C)
        for s in range(down_stages):
            conv(f"downsample.blocks.{s}", 5, C, C)
        dense("latent_mean_proj", C, latent_dim)
        dense("latent_logvar_proj", C, latent_dim, zero=True)                    # zero-initialised, vae.py:320-325

    def get_config(self) -> dict:
        return {"n_mels": self.n_mels, "cond_dim": self.cond_dim, "model_channels": self.model_channels,
                "latent_dim": self.latent_dim, "num_wavenet_blocks": self.num_wavenet_blocks,
                "wavenet_kernel_size": self.wavenet_kernel_size, "down_stages": self.down_stages}

    @property
    def downsample_factor(self) -> int:
        return 2 ** self.down_stages

    def native_config(self) -> "_native.VaeEncoderConfig":
        return _native.VaeEncoderConfig(self.n_mels, self.cond_dim, self.model_channels, self.latent_dim, self.num_wavenet_blocks,
                                        self.wavenet_kernel_size, self.down_stages)

    def blob(self) -> np.ndarray:
        """The weights in the order ``iris_vae_encoder_create`` reads (include/iris_hifigan.h), every kernel transposed to
        ``[C_out][C_in][k]``."""
        w = self.weights
        parts = []

        def gemm(prefix):                        # Conv1D [k, in, out] or Dense [in, out] -> [out][in][k]
            k = w[f"{prefix}.kernel"]
            k = k[None] if k.ndim == 2 else k
            parts.extend([np.ascontiguousarray(k.transpose(2, 1, 0)).ravel(), w[f"{prefix}.bias"].ravel()])

        gemm("in_proj")
        for i in range(self.num_wavenet_blocks):
            p = f"enc_block_{i}"
            gemm(f"{p}.conv"); gemm(f"{p}.film.proj"); gemm(f"{p}.res_proj")
        for s in range(self.down_stages):
            gemm(f"downsample.blocks.{s}")
        gemm("latent_mean_proj")
        gemm("latent_logvar_proj")
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    def _check_inputs(self, mel_shape, cond_shape) -> Tuple[int, int]:
        if len(mel_shape) != 3 or mel_shape[1] != self.n_mels:
            raise ValueError(f"expected mels [B, {self.n_mels}, T], got {tuple(mel_shape)}")
        B, T = int(mel_shape[0]), int(mel_shape[2])
        if tuple(cond_shape) != (B, T, self.cond_dim):
            raise ValueError(f"expected frame_text_cond [{B}, {T}, {self.cond_dim}], got {tuple(cond_shape)}")
        if T % self.downsample_factor:
            raise ValueError(f"T = {T} is not a multiple of 2^down_stages = {self.downsample_factor}: pad the mel and the "
                             "conditioning first (the reference's training script does); nothing is padded silently")
        return B, T

    def launch_count(self, B: int, T: int) -> int:
        """Kernel launches of one ``encode_device``: ``num_wavenet_blocks + down_stages + 3``."""
        lib = self._ensure()
        n = ctypes.c_int32()
        _native.check("iris_vae_encoder_launch_count", lib.iris_vae_encoder_launch_count(self._handle, B, T, ctypes.byref(n)))
        return int(n.value)

    def encode_device(self, mel: torch.Tensor, cond: torch.Tensor, lengths=None):
        """``mel [B, n_mels, T]`` (channels-first, read as it lies), ``cond [B, T, cond_dim]`` (fp32 device tensors) ->
        ``(mean, logvar)``, ``[B, T / 2^S, latent_dim]`` each, asynchronous on the current stream.  Neither input is written.

        ``lengths`` (``B`` frame counts, under ``TextConditionedVAE.generate_device``'s rules: a validated host sequence, or
        an int32 device tensor the host never reads) makes the batch ragged in ONE forward
        (``iris_vae_posterior_encode_ragged``): item b is bit for bit the batch-of-one call on ``mel[b:b+1, :, :lengths[b]]``
        and ``cond[b:b+1, :lengths[b]]``, frames past an item's length are never read, and ``mean`` / ``logvar`` rows from
        ``lengths[b] / 2^S`` on are 0."""
        B, T = self._check_inputs(tuple(mel.shape), tuple(cond.shape))
        if lengths is not None:
            lengths = check_lengths(lengths, B, T, self.downsample_factor)
        lib = self._ensure()
        mel = mel.to(device=self._device, dtype=torch.float32).contiguous()
        cond = cond.to(device=self._device, dtype=torch.float32).contiguous()
        Tq = T // self.downsample_factor
        mean = torch.empty((B, Tq, self.latent_dim), dtype=torch.float32, device=self._device)
        logvar = torch.empty_like(mean)
        if B == 0 or T == 0:
            return mean, logvar
        ws = self._ws(B, T)
        out = (_ptr(mean), _ptr(logvar), _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(self._device))
        if lengths is None:
            _native.check("iris_vae_encoder_forward", lib.iris_vae_encoder_forward(self._handle, _ptr(mel), _ptr(cond), B, T, *out))
            return mean, logvar
        lengths = _lengths_on(lengths, self._device)
        _native.check("iris_vae_posterior_encode_ragged", lib.iris_vae_posterior_encode_ragged(
            self._handle, _ptr(mel), _ptr(cond), B, T, _ptr(lengths), *out))
        return mean, logvar

    def encode(self, mels, frame_text_cond, lengths=None):
        """numpy in -> numpy out, device tensors in -> device tensors out.  ``lengths``: a ragged batch, as in
        ``encode_device``."""
        if isinstance(mels, torch.Tensor):
            return self.encode_device(mels, frame_text_cond, lengths)
        mels = np.ascontiguousarray(np.asarray(mels, dtype=np.float32))
        cond = np.ascontiguousarray(np.asarray(frame_text_cond, dtype=np.float32))
        B, T = self._check_inputs(mels.shape, cond.shape)
        if lengths is not None:
            lengths = check_lengths(lengths, B, T, self.downsample_factor)
        self._ensure()
        mean, logvar = self.encode_device(torch.from_numpy(mels).to(self._device), torch.from_numpy(cond).to(self._device), lengths)
        return mean.cpu().numpy(), logvar.cpu().numpy()

    def _read_tap(self, which: int, B: int, T: int) -> torch.Tensor:
        """Test-only: the intermediate ``which`` (``_native.VAE_ENC_TAP_*``) the last ``encode_device`` of shape (B, T) left in
        the workspace, ``[B, T, model_channels]`` (``LAT_H``: ``[B, T / 2^S, model_channels]``), a copy."""
        lib = self._ensure()
        off, n = ctypes.c_uint64(), ctypes.c_uint64()
        _native.check("iris_vae_encoder_tap", lib.iris_vae_encoder_tap(self._handle, B, T, which, ctypes.byref(off), ctypes.byref(n)))
        raw = self._workspace[off.value:off.value + 4 * n.value].clone()
        return raw.view(torch.float32).view(B, -1, self.model_channels)

    def _workspace_layout(self, B: int, T: int):
        """Test-only: ``enc_ws`` (csrc/iris_vae_encoder.hip) restated, as ``TextConditionedVAE._workspace_layout``: film
        (frames x N * 2C), h0, ha, hb (frames x C), d0 (frames / 2 x C), d1 (frames / 4 x C)."""
        C, frames = self.model_channels, B * T
        return _take_buffers((("film", frames * self.num_wavenet_blocks * 2 * C), ("h0", frames * C), ("ha", frames * C),
                              ("hb", frames * C), ("d0", (frames >> 1) * C), ("d1", (frames >> 2) * C)))

    def _read_buffers(self, B: int, T: int):
        """Test-only: every workspace buffer as the last ``encode_device`` of shape (B, T) left it (``enc_forward``) --
        ``({buffer: flat fp32 copy}, bytes of the layout)``."""
        return _read_buffers(self, *self._workspace_layout(B, T))


_SHARED_SIZES = ("n_mels", "cond_dim", "model_channels", "latent_dim", "down_stages")


def check_pair(encoder: VAEPosteriorEncoder, vae: TextConditionedVAE) -> None:
    """``ValueError`` unless the two halves belong to one model: equal sizes and the same ``downsample.blocks.*`` tensors."""
    for name in _SHARED_SIZES:
        if getattr(encoder, name) != getattr(vae, name):
            raise ValueError(f"the encoder and the decoder disagree on {name}: {getattr(encoder, name)} != {getattr(vae, name)}")
    for s in range(vae.down_stages):
        for leaf in ("kernel", "bias"):
            key = f"downsample.blocks.{s}.{leaf}"
            if not np.array_equal(encoder.weights[key], vae.weights[key]):
                raise ValueError(f"the encoder and the decoder hold different {key}: the reference has one downsample stack, "
                                 "load both halves from the same checkpoint")


_losses_ws = {}                                         # device -> the loss reduction's workspace, grown on demand


def vae_losses(target, recon, mean, logvar, down_stages: int, lengths=None):
    """The reference's ``compute_recon_l1(target, recon, mask)`` and ``compute_kl(mean, logvar, mask[:, ::2^S])``
    (vae.py:424-446, scripts/train_vae.py:94-103) with the mask given as ``lengths`` -> ``(recon_l1, kl, per_item_l1_sum
    [B], per_item_kl_sum [B])``.  ``target`` / ``recon`` ``[B, n_mels, T]``, ``mean`` / ``logvar`` ``[B, T / 2^S, latent]``.

    ``recon_l1 = sum |target - recon| over t < lengths[b]  /  (sum(lengths) * n_mels + 1e-6)`` and ``kl = sum -0.5 (1 + logvar -
    mean^2 - exp(logvar)) over latent rows < lengths[b] / 2^S  /  (sum(lengths / 2^S) + 1e-8)`` -- rows, not rows x channels, as
    the reference has it; ``lengths=None`` gives the plain means.  ``lengths`` follows ``generate_device``'s rules; nothing
    past an item's length is read.  One reduction on the device (``iris_vae_losses``): fp32 terms, fp64 sums in a fixed
    order, so two calls agree bit for bit and an item's sums do not depend on the batch around it.

    Device tensors in -> device tensors out (``recon_l1`` and ``kl`` 0-d), asynchronous on the current stream, nothing is
    synchronised; numpy in -> two floats and two numpy arrays."""
    on_host = not isinstance(target, torch.Tensor)
    if on_host:
        target, recon, mean, logvar = (torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
                                       for a in (target, recon, mean, logvar))
    if target.dim() != 3 or tuple(recon.shape) != tuple(target.shape):
        raise ValueError(f"expected target and recon [B, n_mels, T], got {tuple(target.shape)} and {tuple(recon.shape)}")
    B, n_mels, T = (int(v) for v in target.shape)
    factor = 2 ** int(down_stages)
    if T % factor:
        raise ValueError(f"T = {T} is not a multiple of 2^down_stages = {factor}")
    if mean.dim() != 3 or tuple(mean.shape[:2]) != (B, T // factor) or tuple(logvar.shape) != tuple(mean.shape):
        raise ValueError(f"expected mean and logvar [{B}, {T // factor}, latent], got {tuple(mean.shape)} and {tuple(logvar.shape)}")
    latent = int(mean.shape[2])
    if lengths is not None:
        lengths = check_lengths(lengths, B, T, factor)
    lib = _native.load()
    if on_host:
        from ._engine import require_gpu
        device = require_gpu()
    else:
        device = target.device
        if device.type != "cuda":
            raise ValueError("vae_losses reduces on the device: pass device tensors, or numpy arrays")
    target, recon, mean, logvar = (a.to(device=device, dtype=torch.float32).contiguous() for a in (target, recon, mean, logvar))
    if lengths is not None:
        lengths = _lengths_on(lengths, device)
    need = ctypes.c_uint64()
    _native.check("iris_vae_losses_workspace_bytes",
                  lib.iris_vae_losses_workspace_bytes(B, n_mels, T, latent, int(down_stages), ctypes.byref(need)))
    ws = _losses_ws.get(device)
    if ws is None or ws.numel() < need.value:
        ws = _losses_ws[device] = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=device)
    out = torch.empty(2 + 2 * B, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _native.check("iris_vae_losses", lib.iris_vae_losses(
            _ptr(target), _ptr(recon), _ptr(mean), _ptr(logvar), B, n_mels, T, latent, int(down_stages), _ptr(lengths), _ptr(out),
            _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(device)))
    result = (out[0], out[1], out[2:2 + B], out[2 + B:])
    if on_host:
        host = out.cpu().numpy()
        return float(host[0]), float(host[1]), host[2:2 + B].copy(), host[2 + B:].copy()
    return result


def reconstruct(encoder: VAEPosteriorEncoder, vae: TextConditionedVAE, mels, frame_text_cond, lengths=None, losses: bool = False):
    """The reference's ``TextConditionedVAE.call(mels, frame_text_cond, training=False)`` (vae.py:366-422) ->
    ``(recon [B, n_mels, T], (mean, logvar), residual [B, T, cond_dim])``: ``encode_device`` then
    ``decode_posterior_device(cond, mean)`` on the current stream, nothing returning to the host in between.  numpy in ->
    numpy out, device tensors in -> device tensors out.

    ``lengths`` (``generate_device``'s rules): the batch is ragged and both calls are the ragged ones, on one stream -- item b
    is bit for bit the call on its own ``lengths[b]`` frames, and everything past them is 0 in all four outputs.
    ``losses=True`` appends ``vae_losses(mels, recon, mean, logvar, down_stages, lengths)`` -- ``(recon_l1, kl,
    per_item_l1_sum, per_item_kl_sum)`` -- to the returned tuple."""
    check_pair(encoder, vae)
    on_host = not isinstance(mels, torch.Tensor)
    if on_host:
        mels = torch.from_numpy(np.ascontiguousarray(np.asarray(mels, dtype=np.float32)))
        frame_text_cond = torch.from_numpy(np.ascontiguousarray(np.asarray(frame_text_cond, dtype=np.float32)))
    B, T = encoder._check_inputs(tuple(mels.shape), tuple(frame_text_cond.shape))
    if lengths is not None:
        lengths = check_lengths(lengths, B, T, encoder.downsample_factor)
    if on_host:
        encoder._ensure()
        mels, frame_text_cond = mels.to(encoder._device), frame_text_cond.to(encoder._device)
    if lengths is not None:
        encoder._ensure()
        lengths = _lengths_on(lengths, encoder._device)                               # one upload for both calls and the losses
    mean, logvar = encoder.encode_device(mels, frame_text_cond, lengths)
    recon, residual = vae.decode_posterior_device(frame_text_cond, mean, lengths=lengths)
    loss = vae_losses(mels.to(recon.device), recon, mean, logvar, encoder.down_stages, lengths) if losses else None
    if on_host:
        recon, mean, logvar, residual = (t.cpu().numpy() for t in (recon, mean, logvar, residual))
        if losses:
            loss = (float(loss[0]), float(loss[1]), loss[2].cpu().numpy(), loss[3].cpu().numpy())
    out = (recon, (mean, logvar), residual)
    return out + (loss,) if losses else out
