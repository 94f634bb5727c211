"""Configs, shapes and seeded inputs shared by tests/test_griffin_lim.py and tests/test_gpu_griffin_lim.py.

A case's log-mel comes from a seeded waveform -- two tones at 1 % and 9 % of the sample rate, amplitudes 0.9 and 0.1, plus
white noise at 1e-3 -- of ``hop (T - 1)`` samples run through the mel front-end's float64 restatement
(tests/mel_restatement.py) and rounded to fp32: ``T`` frames of a realistic mel.  At the default config the loud tone
drives its mel bins above the upper clip (``log-mel > 2.0``), so the clip is exercised.
"""
from __future__ import annotations

import numpy as np

import griffin_lim_restatement as G
import mel_restatement as M

DEFAULT = dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0)
SMALL = dict(sample_rate=8000, n_fft=64, hop_length=16, win_length=48, n_mels=12, fmin=0.0, fmax=None)
TWO_TAP = dict(sample_rate=16000, n_fft=256, hop_length=128, win_length=256, n_mels=20, fmin=0.0, fmax=None)
CONFIGS = {"default": DEFAULT, "small": SMALL, "two_tap": TWO_TAP}

# (config, B, T): the defaults across a 32-frame block; fewer frames than taps; three blocks; two taps
CASES = (("default", 2, 33), ("default", 2, 40), ("small", 1, 3), ("small", 1, 70), ("two_tap", 1, 34))
MOMENTUM = 0.99
NNLS_ITERS = 32
PHASE_SEED = 1337


def case_id(case) -> str:
    return f"{case[0]}-B{case[1]}-T{case[2]}"


def waveform(n: int, cfg: dict, seed: int) -> np.ndarray:
    rng = np.random.default_rng(9100 + 13 * n + seed)
    t = np.arange(n, dtype=np.float64) / cfg["sample_rate"]
    x = 1e-3 * rng.standard_normal(n)
    for f, a in ((0.01 * cfg["sample_rate"], 0.9), (0.09 * cfg["sample_rate"], 0.1)):
        x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0.0, 2.0 * np.pi))
    return x.astype(np.float32)


_cache: dict = {}


def logmel(case) -> np.ndarray:
    """``[B, n_mels, T]`` float32."""
    if ("mel", case) not in _cache:
        name, B, T = case
        cfg = CONFIGS[name]
        items = [M.mel_np(waveform(cfg["hop_length"] * (T - 1), cfg, seed=b), **cfg) for b in range(B)]
        assert all(m.shape == (cfg["n_mels"], T) for m in items)
        _cache[("mel", case)] = np.stack(items).astype(np.float32)
    return _cache[("mel", case)]


def phase(case, seed: int = PHASE_SEED) -> np.ndarray:
    """``phi0 [B, K, T]`` float64: what ``forward_device(phase0=None, seed=seed)`` draws."""
    name, B, T = case
    return 2.0 * np.pi * np.random.default_rng(seed).random((B, CONFIGS[name]["n_fft"] // 2 + 1, T))


def model(name: str, **kw):
    """The ``GriffinLim`` of config `name` (host object; no device is touched until a forward)."""
    from iris.griffin_lim import GriffinLim
    return GriffinLim(**CONFIGS[name], momentum=MOMENTUM, nnls_iters=kw.pop("nnls_iters", NNLS_ITERS), **kw)


def tables(name: str) -> dict:
    """The library's fp32 tables of config `name` with ``P`` and ``step``, fetched once."""
    if ("tab", name) not in _cache:
        gl = model(name)
        t = gl.design()
        t["P"], t["step"] = gl.inversion_tables()
        _cache[("tab", name)] = t
    return _cache[("tab", name)]


def fb64(name: str) -> np.ndarray:
    cfg = CONFIGS[name]
    return M.filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])


def stft_args(name: str):
    cfg = CONFIGS[name]
    return cfg["n_fft"], cfg["hop_length"], cfg["win_length"]


def restated(case, n_iters, seed: int = PHASE_SEED, f32: bool = False):
    """``(S [B, T, K], {n_iter: wav [B, hop (T - 1)]})`` of the restatement, float64 or fp32 on the library's tables; cached."""
    key = ("run", case, tuple(n_iters), seed, f32)
    if key not in _cache:
        name, B, T = case
        n_fft, hop, win = stft_args(name)
        lm, phi = logmel(case), phase(case, seed)
        S, wavs = [], {n: [] for n in n_iters}
        for b in range(B):
            if f32:
                t = tables(name)
                s = G.invert_f32(lm[b], t["fb"], t["P"], t["step"], NNLS_ITERS)
                out = G.griffin_lim_f32(s, phi[b], n_iters, MOMENTUM, t, n_fft, hop)
            else:
                s = G.invert(lm[b], fb64(name), NNLS_ITERS)
                out = G.griffin_lim(s, phi[b], n_iters, MOMENTUM, n_fft, hop, win)
            S.append(s)
            for n in n_iters:
                wavs[n].append(out[n])
        _cache[key] = (np.stack(S), {n: np.stack(w) for n, w in wavs.items()})
    return _cache[key]


def e32(n_iters=(0, 1, 2)) -> dict:
    """``{"S": .., 0: .., 1: .., 2: ..}``: the largest |fp32 restatement - float64 restatement| / max(1, max |float64|) over the
    cases, for the inverted magnitudes and for the waveform after each ``n_iter``; and ``"peak"``: per case, max |wav| at 2."""
    if "e32" not in _cache:
        worst = {"S": 0.0, **{n: 0.0 for n in n_iters}}
        peaks, per_case = {}, {}
        for case in CASES:
            S64, w64 = restated(case, n_iters)
            S32, w32 = restated(case, n_iters, f32=True)
            row = {"S": float(np.abs(S32 - S64).max() / max(1.0, np.abs(S64).max()))}
            for n in n_iters:
                row[n] = float(np.abs(w32[n] - w64[n]).max() / max(1.0, np.abs(w64[n]).max()))
            for k, v in row.items():
                worst[k] = max(worst[k], v)
            per_case[case] = row
            peaks[case] = float(np.abs(w64[n_iters[-1]]).max())
        _cache["e32"] = {**worst, "peak": peaks, "per_case": per_case}
    return _cache["e32"]
