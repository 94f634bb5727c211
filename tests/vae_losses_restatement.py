"""numpy restatement of the two losses a validation pass takes from a reconstruction, written from their definition in the
reference (``TextConditionedVAE.compute_recon_l1`` and ``compute_kl``, src/iris/vae.py:424-446, called with ``mask`` and
``mask[:, ::2^S]`` by scripts/train_vae.py:94-103), with the mask given as per-item frame counts.

``losses_np(target, recon, mean, logvar, S, lengths=None, dtype=np.float64)`` -> ``(recon_l1, kl, item_l1_sum [B],
item_kl_sum [B])`` in ``dtype``; ``target`` / ``recon`` ``[B, n_mels, T]``, ``mean`` / ``logvar`` ``[B, T / 2^S, latent]``.
With ``lengths`` (multiples of ``2^S`` in ``[0, T]``):
    recon_l1 = sum_b sum_{t < len_b} |target - recon|                        /  (sum_b len_b * n_mels + 1e-6)
    kl       = sum_b sum_{rows < len_b / 2^S} -0.5 (1 + lv - m^2 - e^lv)     /  (sum_b len_b / 2^S + 1e-8)
-- the KL denominator counts latent rows, not rows x channels: ``ops.sum(m)`` of a mask ``[B, T', 1]``.  Frames and rows
past an item's length are cut away, not multiplied by 0, so they may hold NaN.  Without ``lengths`` both are ``mean()``.
"""
from __future__ import annotations

import numpy as np


def kl_terms(mean, logvar):
    return -0.5 * (1 + logvar - np.square(mean) - np.exp(logvar))


def losses_np(target, recon, mean, logvar, S, lengths=None, dtype=np.float64):
    target, recon, mean, logvar = (np.asarray(a).astype(dtype) for a in (target, recon, mean, logvar))
    B, n_mels, T = target.shape
    assert recon.shape == target.shape and mean.shape == logvar.shape and mean.shape[:2] == (B, T >> S) and T % (1 << S) == 0
    full = lengths is None
    lengths = [T] * B if full else [int(n) for n in lengths]
    assert len(lengths) == B and all(0 <= n <= T and n % (1 << S) == 0 for n in lengths)
    item_l1 = np.zeros(B, dtype)
    item_kl = np.zeros(B, dtype)
    for b, n in enumerate(lengths):
        item_l1[b] = np.abs(target[b, :, :n] - recon[b, :, :n]).sum(dtype=dtype)
        item_kl[b] = kl_terms(mean[b, :n >> S], logvar[b, :n >> S]).sum(dtype=dtype)
    frames, rows = sum(lengths), sum(n >> S for n in lengths)
    if full:
        with np.errstate(invalid="ignore", divide="ignore"):
            return (item_l1.sum(dtype=dtype) / dtype(frames * n_mels), item_kl.sum(dtype=dtype) / dtype(rows * mean.shape[2]),
                    item_l1, item_kl)
    l1 = item_l1.sum(dtype=dtype) / (dtype(frames) * dtype(n_mels) + dtype(1e-6))
    kl = item_kl.sum(dtype=dtype) / (dtype(rows) + dtype(1e-8))
    return l1, kl, item_l1, item_kl
