"""Configs, shapes and seeded inputs shared by tests/test_denoiser.py and tests/test_gpu_denoiser.py.

A case's waveform is seeded: two tones at 1 % and 9 % of the sample rate, amplitudes 0.7 and 0.1, plus white noise at 1e-3, of
``hop M`` samples (M mel frames; T = M + 1 STFT frames) -- its peak stays below 0.9.  The bias of a case is
``bias[k] = u_k median_t mag[t, k]`` from the float64 restatement, ``u_k`` seeded uniform in [0, 2] and the product rounded to
fp32 (what the device is handed): at ``STRENGTH`` = 1 a bin is clamped in about half its frames where ``u_k`` is near 1, in
all of them where it is near 2 and in none where it is near 0, so both branches of the clamp are live in every case.
"""
from __future__ import annotations

import numpy as np

from oracle import dsp_chain_cases as O

import denoiser_restatement as D
import griffin_lim_cases as GC

# default 1024 / 256 / 1024, small 64 / 16 / 48, two_tap 256 / 128 / 256 (griffin_lim_cases's), and for the chain tests
# (tests/test_gpu_denoiser_chain.py) odd_hop 96 / 12 / 80 and wide_hop 1024 / 512 / 1024
CONFIGS = {**GC.CONFIGS, **{name: O.GL_CONFIGS[name] for name in ("odd_hop", "wide_hop")}}

# (config, B, M): one frame past a 32-frame block edge; 40 frames; fewer frames than taps; three blocks; two taps
CASES = (("default", 2, 32), ("default", 2, 39), ("small", 1, 2), ("small", 1, 69), ("two_tap", 1, 33))
STRENGTH = 1.0
PEAK = 0.9


def case_id(case) -> str:
    return f"{case[0]}-B{case[1]}-M{case[2]}"


def stft_args(name: str):
    cfg = CONFIGS[name]
    return cfg["n_fft"], cfg["hop_length"], cfg["win_length"]


waveform_item = O.dn_waveform_item        # (n, cfg, seed): the recipe lives beside the chain oracle's cases, which draw on it too


_cache: dict = {}


def waveform(case) -> np.ndarray:
    """``[B, hop M]`` float32."""
    if ("wav", case) not in _cache:
        name, B, M = case
        cfg = CONFIGS[name]
        _cache[("wav", case)] = np.stack([waveform_item(cfg["hop_length"] * M, cfg, seed=b) for b in range(B)])
    return _cache[("wav", case)]


def magnitudes64(case) -> np.ndarray:
    """``[B, T, K]`` float64 of the restatement."""
    if ("mag", case) not in _cache:
        _cache[("mag", case)] = np.stack([D.magnitude(*D.stft_parts(y, *stft_args(case[0]))) for y in waveform(case)])
    return _cache[("mag", case)]


def bias(case) -> np.ndarray:
    """``[K]`` float32: ``u_k`` times the median over the frames of every item."""
    if ("bias", case) not in _cache:
        mag = magnitudes64(case)
        u = np.random.default_rng(81 + 7 * case[2]).uniform(0.0, 2.0, mag.shape[2])
        _cache[("bias", case)] = (u * np.median(mag.reshape(-1, mag.shape[2]), axis=0)).astype(np.float32)
    return _cache[("bias", case)]


def tables(name: str) -> dict:
    """The library's fp32 tables (``dft``, ``idft``, ``wsq``) of config `name`: the Griffin-Lim stage's, host only."""
    return GC.tables(name) if name in GC.CONFIGS else O.gl_tables(name)


def config_bias(name: str) -> np.ndarray:
    """The bias of the largest chain case (``O.DN_CASES``) of config `name`: what that config's ragged, window and silence cases use."""
    return bias(next(c for c in O.DN_CASES if c[0] == name and c[2] == O.dn_case_m(name)))


def restated(case, strength: float = STRENGTH, f32: bool = False) -> np.ndarray:
    """``out [B, hop M]`` of the restatement, float64 or fp32 on the library's tables; cached and never changed."""
    key = ("out", case, float(strength), f32)
    if key not in _cache:
        name = case[0]
        kw = dict(dtype=np.float32, tables=tables(name)) if f32 else {}
        out = np.stack([D.denoise(y, bias(case), strength, *stft_args(name), **kw) for y in waveform(case)])
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def restated_bias(case, f32: bool = False) -> np.ndarray:
    """``estimate_bias`` of item 0 (``[K]``), or None where the case has no interior frame."""
    key = ("est", case, f32)
    if key not in _cache:
        name = case[0]
        n_fft, hop, _ = stft_args(name)
        lo, hi = D.interior(case[2] + 1, n_fft, hop)
        kw = dict(dtype=np.float32, tables=tables(name)) if f32 else {}
        _cache[key] = None if hi <= lo else D.estimate_bias(waveform(case)[0], *stft_args(name), **kw)
    return _cache[key]


def e32() -> dict:
    """``{"out": .., "bias": ..}``: the largest |fp32 restatement - float64 restatement| / max(1, max |float64|) over the cases,
    for the denoised waveform and for the bias estimate; ``"per_case"`` holds the rows."""
    if "e32" not in _cache:
        worst, rows = {"out": 0.0, "bias": 0.0}, {}
        for case in CASES:
            w64, w32 = restated(case), restated(case, f32=True)
            row = {"out": float(np.abs(w32 - w64).max() / max(1.0, np.abs(w64).max()))}
            b64, b32 = restated_bias(case), restated_bias(case, f32=True)
            if b64 is not None:
                row["bias"] = float(np.abs(b32 - b64).max() / max(1.0, np.abs(b64).max()))
            for k, v in row.items():
                worst[k] = max(worst[k], v)
            rows[case] = row
        _cache["e32"] = {**worst, "per_case": rows}
    return _cache["e32"]
