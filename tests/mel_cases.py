"""Seeded waveforms and configs shared by tests/test_mel_frontend.py and tests/test_gpu_mel_frontend.py.

A waveform is a sum of three tones -- 220, 1900 and 6100 Hz at amplitudes 0.5 / 0.05 / 0.005 -- plus white noise at 1e-3,
rounded to fp32.  Where it is long enough (``n >= 4 * n_fft``) one stretch of ``2 * n_fft + hop`` samples is set to exact
zeros: the frames wholly inside it have magnitude 0 and give exact ``log(1e-5)``, so such a case has mel bins on both sides of
the clip (a shorter case has no room for the stretch beside any signal).
"""
from __future__ import annotations

import numpy as np

DEFAULT = dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0)
SMALL = dict(sample_rate=16000, n_fft=256, hop_length=64, win_length=192, n_mels=20, fmin=50.0, fmax=None)
CONFIGS = {"default": DEFAULT, "small": SMALL}

DENSE_LENGTHS = (0, 255, 256, 1023, 8229)        # 8229: 33 frames -- a second 32-frame block, whose frame reads past the end
SMALL_LENGTH = 2085
RAGGED_L = 8229
RAGGED_SAMPLES = (8229, 4096, 300, 0)
RAGGED_CAPS = (16, 100, 1, 0)

TONES = ((220.0, 0.5), (1900.0, 0.05), (6100.0, 0.005))
NOISE = 1e-3


def zero_stretch(n: int, cfg: dict):
    """(start, stop) of the stretch of zeros in a waveform of n samples, or None."""
    n_fft, hop = cfg["n_fft"], cfg["hop_length"]
    if n < 4 * n_fft:
        return None
    start = (n // 3) | 1
    return start, start + 2 * n_fft + hop


def waveform(n: int, cfg: dict, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(4100 + 7 * n + seed)
    t = np.arange(n, dtype=np.float64) / cfg["sample_rate"]
    x = NOISE * rng.standard_normal(n)
    for f, a in TONES:
        x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0.0, 2.0 * np.pi))
    z = zero_stretch(n, cfg)
    if z is not None:
        x[z[0]:z[1]] = 0.0
    return x.astype(np.float32)


def zero_frames(n: int, cfg: dict):
    """Frames of a waveform of n samples that lie wholly inside its zero stretch."""
    z = zero_stretch(n, cfg)
    if z is None:
        return []
    n_fft, hop = cfg["n_fft"], cfg["hop_length"]
    return [t for t in range(1 + n // hop) if t * hop - n_fft // 2 >= z[0] and t * hop + n_fft // 2 <= z[1]]


_tables = {}


def design_tables(name: str):
    """The fp32 tables the device uploads for config `name` (host only), fetched once."""
    if name not in _tables:
        from iris.mel import MelFrontend
        _tables[name] = MelFrontend(**CONFIGS[name]).design()
    return _tables[name]


def e32_of(name: str, x: np.ndarray) -> float:
    """max |restatement in fp32 on the design tables - restatement in float64| / max(1, max |float64|) of one waveform."""
    import mel_restatement as R
    cfg = CONFIGS[name]
    dft, fb = design_tables(name)
    want = R.mel_np(x, **cfg)
    got = R.mel_np_f32(x, dft, fb, cfg["n_fft"], cfg["hop_length"])
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def accuracy_cases():
    """(config name, waveform) of every case the accuracy bar is measured over: the dense lengths, the second item of the
    B = 2 call, and the small config."""
    out = [("default", waveform(n, DEFAULT)) for n in DENSE_LENGTHS]
    out.append(("default", waveform(8229, DEFAULT, seed=1)))
    out.append(("small", waveform(SMALL_LENGTH, SMALL)))
    return out
