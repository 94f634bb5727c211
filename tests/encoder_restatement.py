"""A numpy restatement of the reference's text side, written from ``src/iris/encoder.py`` and ``scripts/synthesize.py`` read
as text: PhonemeEncoder (:115-212), TransformerBlock (:47-102), DurationPredictor (:228-315), predict_durations
(synthesize.py:41-45) and the length regulator (synthesize.py:48-61, 112-122).  ``dtype`` selects float64 (the yardstick)
or float32 (its own rounding error measures the bar of tests/test_gpu_encoder.py).  Conventions: see ``iris/encoder.py``.

A ragged batch is computed item by item on the item's own prefix, and rows past it are zeros: that is the definition the
device code is held to (no padded key, no padded conv tap, reaches an item).
"""
from __future__ import annotations

import numpy as np

EPS = 1e-6


def layer_norm(x, gamma, beta):
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)            # biased
    return (x - mean) / np.sqrt(var + x.dtype.type(EPS)) * gamma + beta


def attention(x, w, p, num_heads, probs_out=None):
    """keras.layers.MultiHeadAttention(num_heads, key_dim = E / H)(x, x) on one item ``x [P, E]``."""
    P, E = x.shape
    dk = E // num_heads
    q = np.einsum("pe,ehd->phd", x, w[f"{p}.query.kernel"]) + w[f"{p}.query.bias"]
    k = np.einsum("pe,ehd->phd", x, w[f"{p}.key.kernel"]) + w[f"{p}.key.bias"]
    v = np.einsum("pe,ehd->phd", x, w[f"{p}.value.kernel"]) + w[f"{p}.value.bias"]
    q = q * x.dtype.type(1.0 / np.sqrt(float(dk)))                  # after the bias
    s = np.einsum("phd,jhd->hpj", q, k)
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    a = e / e.sum(axis=-1, keepdims=True)
    if probs_out is not None:
        probs_out.append(a)
    o = np.einsum("hpj,jhd->phd", a, v)
    return np.einsum("phd,hde->pe", o, w[f"{p}.output.kernel"]) + w[f"{p}.output.bias"]


def encoder_item(cfg, w, ids, taps=None):
    """One item, ``ids [P]`` -> ``[P, E]``."""
    P = len(ids)
    x = w["phoneme_embedding.embeddings"][ids] + w["positional_embedding.position_embedding.embeddings"][:P]
    for i in range(cfg["num_blocks"]):
        p = f"transformer_block_{i}"
        x = layer_norm(x + attention(x, w, f"{p}.attention", cfg["num_heads"]), w[f"{p}.attention_norm.gamma"], w[f"{p}.attention_norm.beta"])
        h = np.maximum(x @ w[f"{p}.ffn.0.kernel"] + w[f"{p}.ffn.0.bias"], 0)
        x = layer_norm(x + (h @ w[f"{p}.ffn.2.kernel"] + w[f"{p}.ffn.2.bias"]), w[f"{p}.ffn_norm.gamma"], w[f"{p}.ffn_norm.beta"])
        if i == 0 and taps is not None:
            taps["block0"] = x
    return layer_norm(x, w["encoder_output_norm.gamma"], w["encoder_output_norm.beta"])


def conv1d_same(x, kernel, bias):
    """Keras Conv1D(padding='same'), stride 1, odd k: ``x [P, C_in]``, ``kernel [k, C_in, C_out]``."""
    k = kernel.shape[0]
    pad = (k - 1) // 2
    xp = np.concatenate([np.zeros((pad, x.shape[1]), x.dtype), x, np.zeros((k - 1 - pad, x.shape[1]), x.dtype)])
    y = sum(xp[kap:kap + x.shape[0]] @ kernel[kap] for kap in range(k))
    return y + bias


def softplus(u):
    return np.logaddexp(u, u.dtype.type(0))


def duration_item(cfg, w, enc, taps=None):
    """One item, ``enc [P, C]`` -> softplus output ``[P]``."""
    x = enc
    for i in range(cfg["num_layers"]):
        x = np.maximum(conv1d_same(x, w[f"duration_conv_{i}.kernel"], w[f"duration_conv_{i}.bias"]), 0)
        x = layer_norm(x, w[f"duration_norm_{i}.gamma"], w[f"duration_norm_{i}.beta"])
        if i == 0 and taps is not None:
            taps["layer0"] = x
    u = x @ w["duration_output.kernel"][0, :, 0] + w["duration_output.bias"][0]
    return softplus(u)


def _cast(weights, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in weights.items()}


def _ragged(fn, B, P, lengths, tail_shape, dtype, tap_names):
    out = np.zeros((B, P) + tail_shape, dtype)
    taps = {}
    for b in range(B):
        n = P if lengths is None else int(lengths[b])
        t = {}
        out[b, :n] = fn(b, n, t)
        for name in tap_names:
            if name in t:
                taps.setdefault(name, np.zeros((B, P) + t[name].shape[1:], dtype))[b, :n] = t[name]
    return out, taps


def encoder_forward(cfg, weights, ids, lengths=None, dtype=np.float64):
    """``ids [B, P]`` -> ``(enc_out [B, P, E], {'block0': [B, P, E]})``."""
    w = _cast(weights, dtype)
    ids = np.asarray(ids)
    B, P = ids.shape
    return _ragged(lambda b, n, t: encoder_item(cfg, w, ids[b, :n], t), B, P, lengths, (cfg["embed_dim"],), dtype, ("block0",))


def duration_forward(cfg, weights, enc_out, lengths=None, dtype=np.float64):
    """``enc_out [B, P, C]`` -> ``(pred [B, P], {'layer0': [B, P, hidden]})``."""
    w = _cast(weights, dtype)
    enc_out = np.asarray(enc_out).astype(dtype)
    B, P = enc_out.shape[:2]
    return _ragged(lambda b, n, t: duration_item(cfg, w, enc_out[b, :n], t), B, P, lengths, (), dtype, ("layer0",))


def raw_frames(pred):
    """``exp(pred) - 1`` before rounding (synthesize.py:44)."""
    return np.exp(pred) - pred.dtype.type(1)


def predict_frames(pred, lengths=None, max_frames_per_phoneme=1_000_000):
    """synthesize.py:41-45: ``clip(round(exp(pred) - 1), 1, 1e6)`` as int32 (np.round: half to even, like jnp.round);
    0 past an item's length."""
    frames = np.clip(np.round(raw_frames(pred)), 1.0, float(max_frames_per_phoneme)).astype(np.int32)
    if lengths is not None:
        frames = np.where(np.arange(pred.shape[1])[None, :] < np.asarray(lengths)[:, None], frames, 0).astype(np.int32)
    return frames


def length_regulate(enc_out, durations, factor=1):
    """np.repeat per item (synthesize.py:48-61 without its ``maximum(durs, 1)``: zeros are honoured, as in encoder.py:378-416)
    and zero padding to the longest item rounded up to ``factor`` (synthesize.py:116-121)."""
    enc_out, durations = np.asarray(enc_out), np.asarray(durations)
    rows = [np.repeat(enc_out[b], durations[b], axis=0) for b in range(enc_out.shape[0])]
    T = max(len(r) for r in rows)
    T = -(-T // factor) * factor
    out = np.zeros((enc_out.shape[0], T, enc_out.shape[2]), enc_out.dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def randomise(model, seed: int, scale: float = 1.0, duration_bias: float = 1.0, duration_gain: float = 1.0):
    """EVERY parameter of an ``iris.encoder`` model randomised: kernels glorot-like in size times ``scale``, embeddings
    +-0.5, LayerNorm gamma 1 +- 0.2, biases and beta +-0.1; ``duration_output`` gets ``duration_bias`` and a kernel times
    ``duration_gain`` so that the predicted frames spread over a useful range."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, cur in model.weights.items():
        if key.endswith(".embeddings"):
            out[key] = rng.uniform(-0.5, 0.5, cur.shape)
        elif key.endswith(".kernel"):
            if ".attention.output." in key:
                fan = int(np.prod(cur.shape[:2])) + cur.shape[2]
            elif ".attention." in key:
                fan = cur.shape[0] + int(np.prod(cur.shape[1:]))
            else:
                fan = int(np.prod(cur.shape[:-1])) + cur.shape[-1]
            lim = scale * np.sqrt(6.0 / fan) * (duration_gain if key.startswith("duration_output") else 1.0)
            out[key] = rng.uniform(-lim, lim, cur.shape)
        elif key.endswith(".gamma"):
            out[key] = 1.0 + rng.uniform(-0.2, 0.2, cur.shape)
        else:
            out[key] = rng.uniform(-0.1, 0.1, cur.shape) + (duration_bias if key == "duration_output.bias" else 0.0)
        out[key] = out[key].astype(np.float32)
    model.set_weights_dict(out)
    return out
