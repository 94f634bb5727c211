"""Ragged batches: utterances of different lengths through ONE fp32 forward.

    padded, lengths = pack_mels([mel_a, mel_b, mel_c])            # [B, n_mels, T_max], int32 [B]
    wav = engine.forward(padded_on_device, lengths=lengths)       # iris_hifigan_forward_ragged
    waves = split_waveforms(wav, lengths, engine.hop_length)      # one [hop * T_i] per utterance

Padding to the longest item and running a plain batch is NOT the same as running each item alone: the generator
sees about 13 mel frames on each side (iris/streaming.py), so the padded frames reach the last samples of every short
item (conv_pre adds its bias, so even zero padding is no longer zero one layer in).  The ragged forward bounds every
layer of item b by its own length, which gives the stand-alone result bit for bit; the frames past it are never read
(they may hold anything) and its waveform past ``hop * lengths[b]`` is 0.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

ArrayLike = Union[np.ndarray, torch.Tensor]

__all__ = ["pack_mels", "split_waveforms"]


def pack_mels(mels: Sequence[ArrayLike], fill: float = 0.0) -> Tuple[ArrayLike, np.ndarray]:
    """List of mels [n_mels, T_i] -> (padded [B, n_mels, T_max] float32, lengths int32 [B]).

    Numpy inputs give a numpy batch; if any input is a torch tensor the batch is a torch tensor on the first tensor's
    device.  Frames past T_i hold ``fill`` (the ragged forward never reads them)."""
    if isinstance(mels, (np.ndarray, torch.Tensor)) and mels.ndim == 3:
        mels = list(mels)
    mels = list(mels)
    if not mels:
        raise ValueError("pack_mels needs at least one mel")
    shapes = []
    for i, m in enumerate(mels):
        if not isinstance(m, (np.ndarray, torch.Tensor)):
            m = mels[i] = np.asarray(m)
        if m.ndim != 2:
            raise ValueError(f"mel {i}: expected [n_mels, T], got shape {tuple(m.shape)}")
        shapes.append(tuple(m.shape))
    n_mels = shapes[0][0]
    if any(s[0] != n_mels for s in shapes):
        raise ValueError(f"every mel must have the same number of mel channels, got {sorted({s[0] for s in shapes})}")
    lengths = np.array([s[1] for s in shapes], dtype=np.int32)
    t_max = int(lengths.max())
    tensors = [m for m in mels if isinstance(m, torch.Tensor)]
    if tensors:
        out = torch.full((len(mels), n_mels, t_max), fill, dtype=torch.float32, device=tensors[0].device)
        for i, m in enumerate(mels):
            out[i, :, :lengths[i]] = torch.as_tensor(m).to(device=out.device, dtype=torch.float32)
    else:
        out = np.full((len(mels), n_mels, t_max), fill, dtype=np.float32)
        for i, m in enumerate(mels):
            out[i, :, :lengths[i]] = m
    return out, lengths


def split_waveforms(wav: ArrayLike, lengths, hop: int) -> List[ArrayLike]:
    """Waveform batch [B, S] (S >= hop * max(lengths)) -> list of B waveforms [hop * lengths[b]] (views into ``wav``)."""
    lengths = np.asarray(lengths.detach().cpu() if isinstance(lengths, torch.Tensor) else lengths)
    if wav.ndim != 2:
        raise ValueError(f"expected a waveform batch [B, samples], got shape {tuple(wav.shape)}")
    if lengths.shape != (wav.shape[0],):
        raise ValueError(f"lengths must have shape [{wav.shape[0]}], got {list(lengths.shape)}")
    if lengths.size and not np.issubdtype(lengths.dtype, np.integer):
        raise ValueError(f"lengths must be integers, got {lengths.dtype}")
    if int(hop) < 1:
        raise ValueError(f"hop must be positive, got {hop}")
    if lengths.size and (lengths.min() < 0 or int(lengths.max()) * int(hop) > wav.shape[1]):
        raise ValueError(f"lengths must lie in [0, {wav.shape[1] // int(hop)}] for {wav.shape[1]} samples at hop {hop}")
    return [wav[b, :int(n) * int(hop)] for b, n in enumerate(lengths)]
