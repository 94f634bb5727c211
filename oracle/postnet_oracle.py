"""CPU restatement of the reference PostNet at inference.  TEST INFRASTRUCTURE ONLY.

Follows ``/root/reference/src/iris/postnet.py:48-67`` read as text: transpose to [B, T, C]; for the
first L-1 layers Conv1D(k, padding='same') -> BatchNormalization(inference) -> tanh (dropout is the
identity at inference); then Conv1D(n_mels) -> BatchNormalization; transpose back and add to the input.
Keras semantics used: Conv1D kernel [k, C_in, C_out] with cross-correlation and symmetric zero padding
for odd k; BatchNormalization(y) = gamma * (y - moving_mean) / sqrt(moving_variance + 1e-3) + beta.
The BatchNorm is applied UNFOLDED here, so the product's fold is checked, not assumed.

Parity unpinned: Keras/JAX cannot run in this pipeline and the reference ships no PostNet vectors.
"""
import numpy as np

BN_EPSILON = 1e-3


def conv1d_same_keras(x_btc: np.ndarray, kernel: np.ndarray, bias: np.ndarray, dtype=np.float64) -> np.ndarray:
    """x [B, T, C_in], kernel [k, C_in, C_out] -> [B, T, C_out]; accumulation in ``dtype`` (fp64)."""
    k = kernel.shape[0]
    pad = (k - 1) // 2
    B, T, _ = x_btc.shape
    xp = np.zeros((B, T + 2 * pad, x_btc.shape[2]), dtype=dtype)
    xp[:, pad:pad + T] = x_btc
    y = np.zeros((B, T, kernel.shape[2]), dtype=dtype)
    for kap in range(k):
        y += xp[:, kap:kap + T] @ kernel[kap].astype(dtype)
    return y + bias.astype(dtype)


def postnet_forward_raw(weights: dict, mels_bt_f: np.ndarray, num_layers: int, dtype=np.float64) -> np.ndarray:
    """The forward with every operation in ``dtype``, returned in ``dtype`` (fp64: the reference; fp32: what a plain fp32
    implementation of the same text gives, the yardstick of ``e32``)."""
    x = np.transpose(np.asarray(mels_bt_f, dtype=dtype), (0, 2, 1))
    h = x
    for i in range(num_layers):
        p = "conv_out" if i == num_layers - 1 else f"convs.{i}"
        h = conv1d_same_keras(h, weights[f"{p}.kernel"], weights[f"{p}.bias"], dtype)
        h = (weights[f"{p}.gamma"].astype(dtype) * (h - weights[f"{p}.moving_mean"].astype(dtype))
             / np.sqrt(weights[f"{p}.moving_variance"].astype(dtype) + dtype(BN_EPSILON)) + weights[f"{p}.beta"].astype(dtype))
        if i < num_layers - 1:
            h = np.tanh(h)
    out = np.asarray(mels_bt_f, dtype=dtype) + np.transpose(h, (0, 2, 1))
    assert out.dtype == dtype
    return out


def postnet_forward_np(weights: dict, mels_bt_f: np.ndarray, num_layers: int) -> np.ndarray:
    return postnet_forward_raw(weights, mels_bt_f, num_layers).astype(np.float32)


def e32(weights: dict, mels_bt_f: np.ndarray, num_layers: int) -> float:
    """max |fp32 restatement - fp64 restatement| / max(1, max |fp64|) on exactly these inputs: the reference's own fp32 error."""
    want = postnet_forward_raw(weights, mels_bt_f, num_layers, np.float64)
    got = postnet_forward_raw(weights, mels_bt_f, num_layers, np.float32)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
