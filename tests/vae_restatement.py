"""numpy restatement of ``TextConditionedVAE.generate`` (reference src/iris/vae.py:448-482), written from the reference's
text; independent of ``iris.vae``'s device path.  Keras/JAX cannot run here, so the Keras conventions are assumptions
(listed in ``iris/vae.py``'s docstring): Conv1D kernels ``[k, C_in, C_out]`` as cross-correlation, 'same' padding
``dil * (k - 1) / 2`` at stride 1 and (1, 2) for k = 5 at stride 2 on an even length (``pad_left = total // 2``), Dense
``x @ kernel + bias``, ``split`` = first half first, tanh-GELU, dropout = identity.

``generate_np(weights, cfg, cond, z_prior, dtype=np.float64)``: float64 by default; ``dtype=np.float32`` runs the same
function on fp32 arrays with fp32 accumulation (every matmul's operands and result are fp32).  ``taps`` (a dict) receives
``lat_cond``, ``dec_in`` (after flow + latent_dec_proj) and ``dec_out`` (after the last decoder block).
"""
from __future__ import annotations

import numpy as np


def gelu(x):
    dt = x.dtype.type
    return dt(0.5) * x * (dt(1.0) + np.tanh(dt(np.sqrt(2.0 / np.pi)) * (x + dt(0.044715) * x * x * x)))


def dense(x, kernel, bias):
    return x @ kernel + bias


def same_pads(length: int, k: int, stride: int, dil: int):
    """TF/XLA SAME: out = ceil(L / stride), total = max((out - 1) * stride + (k - 1) * dil + 1 - L, 0), left = total // 2."""
    out = -(-length // stride)
    total = max((out - 1) * stride + (k - 1) * dil + 1 - length, 0)
    return total // 2, total - total // 2, out


def conv1d_same(x, kernel, bias, stride: int = 1, dil: int = 1):
    """x [B, L, C_in], kernel [k, C_in, C_out] -> [B, ceil(L / stride), C_out]; y[i] = sum_kap x[stride i - left + kap dil] W[kap]."""
    k = kernel.shape[0]
    left, right, out = same_pads(x.shape[1], k, stride, dil)
    xp = np.pad(x, ((0, 0), (left, right), (0, 0)))
    y = np.zeros((x.shape[0], out, kernel.shape[2]), x.dtype) + bias
    for kap in range(k):
        rows = xp[:, kap * dil: kap * dil + (out - 1) * stride + 1: stride, :]
        y = y + rows @ kernel[kap]
    return y


def upsample2x(x):
    b, t, c = x.shape
    return np.repeat(x.reshape(b, t, 1, c), 2, axis=2).reshape(b, 2 * t, c)


def coupling(w, p, z, lat_cond, reverse: bool):
    """APCoupling.call (vae.py:182-208)."""
    half = z.shape[-1] // 2
    x1, x2 = z[..., :half], z[..., half:]
    ce = gelu(dense(lat_cond, w[f"{p}.cond_proj.kernel"], w[f"{p}.cond_proj.bias"]))
    h = gelu(conv1d_same(x1 + ce, w[f"{p}.net_pre.kernel"], w[f"{p}.net_pre.bias"]))
    t = conv1d_same(h, w[f"{p}.net_post.kernel"], w[f"{p}.net_post.bias"])
    gb = dense(ce, w[f"{p}.film.proj.kernel"], w[f"{p}.film.proj.bias"])
    t = gb[..., :half] * t + gb[..., half:]
    return np.concatenate([x1, x2 - t if reverse else x2 + t], axis=-1)


def flow(w, cfg, z, lat_cond, reverse: bool):
    """VolumePreservingFlow.call (vae.py:229-243)."""
    order = range(cfg["flow_layers"])
    for j in (reversed(order) if reverse else order):
        z = coupling(w, f"vpflow.ap_{j}", z, lat_cond, reverse)
    return z


def lat_cond_np(w, cfg, cond):
    h = conv1d_same(cond, w["down_cond_proj.kernel"], w["down_cond_proj.bias"])
    for s in range(cfg["down_stages"]):
        h = gelu(conv1d_same(h, w[f"downsample.blocks.{s}.kernel"], w[f"downsample.blocks.{s}.bias"], stride=2))
    return h


def upsample_np(w, cfg, d):
    for s in range(cfg["down_stages"]):
        d = gelu(conv1d_same(upsample2x(d), w[f"upsample.refine.{s}.kernel"], w[f"upsample.refine.{s}.bias"]))
    return d


def generate_np(weights, cfg, cond, z_prior, dtype=np.float64, taps=None):
    """-> (mel [B, n_mels, T], residual [B, T, cond_dim]) in ``dtype``."""
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items()}
    cond, z = np.asarray(cond).astype(dtype), np.asarray(z_prior).astype(dtype)
    lat_cond = lat_cond_np(w, cfg, cond)
    z = flow(w, cfg, z, lat_cond, reverse=True)
    d = dense(z, w["latent_dec_proj.kernel"], w["latent_dec_proj.bias"])
    if taps is not None:
        taps["lat_cond"], taps["dec_in"] = lat_cond, d
    C = cfg["model_channels"]
    for i in range(cfg["decoder_blocks"]):
        p = f"dec_block_{i}"
        h = gelu(conv1d_same(d, w[f"{p}.conv.kernel"], w[f"{p}.conv.bias"], dil=2 ** (i % 4)))
        gb = dense(lat_cond, w[f"{p}.film.proj.kernel"], w[f"{p}.film.proj.bias"])
        h = gb[..., :C] * h + gb[..., C:]
        d = d + conv1d_same(h, w[f"{p}.res_proj.kernel"], w[f"{p}.res_proj.bias"])
    if taps is not None:
        taps["dec_out"] = d
    d = upsample_np(w, cfg, d)
    out = conv1d_same(d, w["out_proj.kernel"], w["out_proj.bias"])
    residual = dense(d, w["residual_proj.kernel"], w["residual_proj.bias"])
    assert out.dtype == dtype and residual.dtype == dtype
    return np.ascontiguousarray(out.transpose(0, 2, 1)), residual


def randomise(vae, seed: int, scale: float = 1.0):
    """EVERY parameter of an ``iris.vae.TextConditionedVAE`` randomised (biases, net_post and FiLM included): kernels
    glorot-like in size times ``scale``, FiLM biases so that gamma is near 1, other biases +-0.1."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, cur in vae.weights.items():
        if key.endswith(".kernel"):
            fan = int(np.prod(cur.shape[:-1])) + cur.shape[-1]
            lim = scale * np.sqrt(6.0 / fan)
            out[key] = rng.uniform(-lim, lim, cur.shape).astype(np.float32)
        else:
            b = rng.uniform(-0.1, 0.1, cur.shape)
            if ".film.proj." in key:
                b[: cur.shape[0] // 2] += 1.0
            out[key] = b.astype(np.float32)
    vae.set_weights_dict(out)
    return out
