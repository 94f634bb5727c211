"""numpy restatement of ``TextConditionedVAE.call(mels, frame_text_cond, training=False)`` (reference src/iris/vae.py:366-422),
written from the reference's text and built from the pieces of ``vae_restatement`` (same assumed Keras conventions).

``reconstruct_np(enc_weights, dec_weights, cfg, mels, cond, dtype=np.float64, taps=None)`` -> ``(recon [B, n_mels, T],
(mean, logvar), residual [B, T, cond_dim])`` in ``dtype``.  ``enc_weights`` holds the encoder-side tensors (``in_proj``,
``enc_block_*``, ``latent_*_proj``), ``dec_weights`` everything ``generate_np`` reads; ``downsample.blocks.*`` is taken from
``dec_weights`` for both uses, as the reference has one stack.  ``cfg`` needs ``num_wavenet_blocks`` beside the decoder's
keys.  ``taps`` (a dict) receives ``h_in`` (after in_proj), ``h_out`` (after the last encoder block), ``lat_h``, ``z_flow``.
"""
from __future__ import annotations

import numpy as np

from vae_restatement import conv1d_same, dense, flow, gelu, lat_cond_np, upsample_np


def downsample_np(w, cfg, h):
    for s in range(cfg["down_stages"]):
        h = gelu(conv1d_same(h, w[f"downsample.blocks.{s}.kernel"], w[f"downsample.blocks.{s}.bias"], stride=2))
    return h


def encode_np(we, wd, cfg, mels, cond, taps=None):
    """-> (mean, logvar); ``we`` / ``wd`` already in the working dtype."""
    C = cfg["model_channels"]
    h = conv1d_same(np.ascontiguousarray(mels.transpose(0, 2, 1)), we["in_proj.kernel"], we["in_proj.bias"])
    if taps is not None:
        taps["h_in"] = h
    for i in range(cfg["num_wavenet_blocks"]):
        p = f"enc_block_{i}"
        a = gelu(conv1d_same(h, we[f"{p}.conv.kernel"], we[f"{p}.conv.bias"], dil=2 ** (i % 4)))
        gb = dense(cond, we[f"{p}.film.proj.kernel"], we[f"{p}.film.proj.bias"])
        a = gb[..., :C] * a + gb[..., C:]
        h = h + conv1d_same(a, we[f"{p}.res_proj.kernel"], we[f"{p}.res_proj.bias"])
    lat_h = downsample_np(wd, cfg, h)
    if taps is not None:
        taps["h_out"], taps["lat_h"] = h, lat_h
    return (dense(lat_h, we["latent_mean_proj.kernel"], we["latent_mean_proj.bias"]),
            dense(lat_h, we["latent_logvar_proj.kernel"], we["latent_logvar_proj.bias"]))


def decode_np(wd, cfg, cond, z, reverse: bool, taps=None):
    """The decoder from a latent on: flow in the given direction, latent_dec_proj, dec_blocks, upsample, both projections."""
    C = cfg["model_channels"]
    lat_cond = lat_cond_np(wd, cfg, cond)
    z = flow(wd, cfg, z, lat_cond, reverse=reverse)
    if taps is not None:
        taps["z_flow"] = z
    d = dense(z, wd["latent_dec_proj.kernel"], wd["latent_dec_proj.bias"])
    for i in range(cfg["decoder_blocks"]):
        p = f"dec_block_{i}"
        h = gelu(conv1d_same(d, wd[f"{p}.conv.kernel"], wd[f"{p}.conv.bias"], dil=2 ** (i % 4)))
        gb = dense(lat_cond, wd[f"{p}.film.proj.kernel"], wd[f"{p}.film.proj.bias"])
        d = d + conv1d_same(gb[..., :C] * h + gb[..., C:], wd[f"{p}.res_proj.kernel"], wd[f"{p}.res_proj.bias"])
    d = upsample_np(wd, cfg, d)
    out = conv1d_same(d, wd["out_proj.kernel"], wd["out_proj.bias"])
    residual = dense(d, wd["residual_proj.kernel"], wd["residual_proj.bias"])
    return np.ascontiguousarray(out.transpose(0, 2, 1)), residual


def reconstruct_np(enc_weights, dec_weights, cfg, mels, cond, dtype=np.float64, taps=None):
    we = {k: np.asarray(v).astype(dtype) for k, v in enc_weights.items()}
    wd = {k: np.asarray(v).astype(dtype) for k, v in dec_weights.items()}
    mels, cond = np.asarray(mels).astype(dtype), np.asarray(cond).astype(dtype)
    mean, logvar = encode_np(we, wd, cfg, mels, cond, taps)
    recon, residual = decode_np(wd, cfg, cond, mean, reverse=False, taps=taps)      # z = mean when not training
    assert recon.dtype == dtype and residual.dtype == dtype and mean.dtype == dtype and logvar.dtype == dtype
    return recon, (mean, logvar), residual
