"""Seeded signals for the spectral-distance tests, and what the two restatements give on them (computed once per process).

A signal is white noise plus three sinusoids, peak about 0.3, so that every ``a2`` and ``x2`` lies far from 0; the candidate is
the reference turned down and disturbed by other noise, so that no distance is a small difference of large numbers.

    ragged   row_scale 256, lengths [0, 1, 3, 16, 37], L = 37 * 256: an empty item; items of 1 and 3 rows, shorter than
             n_fft / 2 at 2048, the second of them (768 samples) no multiple of hop 512; 75 frames at hop 128, three blocks of the
             transform
    dense    B = 1, L = 20000, lengths None: a multiple of no hop, 40 frames at hop 512 (two blocks of the transform) and five
             chunks of 4096 samples
"""
from __future__ import annotations

import functools

import numpy as np

import spectral_distance_restatement as R

RESOLUTIONS = R.DEFAULT
ROW_SCALE = 256
RAGGED_LENGTHS = (0, 1, 3, 16, 37)
RAGGED_L = 37 * ROW_SCALE
DENSE_L = 20000


def signal(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    y = 0.07 * rng.standard_normal(n)
    for f, a in ((220.0, 0.08), (1330.0, 0.05), (4700.0, 0.03)):
        y = y + a * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return y.astype(np.float32)


def pair(seed: int, n: int):
    """``(ref, test) [n]`` float32."""
    ref = signal(seed, n)
    noise = np.random.default_rng(seed + 1000).standard_normal(n)
    return ref, (0.8 * ref.astype(np.float64) + 0.02 * noise).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ragged():
    """``(ref, test) [5, L]`` float32, NaN behind every item's own samples, and the items' sample counts."""
    counts = [n * ROW_SCALE for n in RAGGED_LENGTHS]
    ref = np.full((len(counts), RAGGED_L), np.nan, dtype=np.float32)
    test = np.full_like(ref, np.nan)
    for b, n in enumerate(counts):
        ref[b, :n], test[b, :n] = pair(10 + b, n)
    return ref, test, counts


@functools.lru_cache(maxsize=None)
def dense():
    ref, test = pair(77, DENSE_L)
    return ref[None, :], test[None, :]


def items():
    """Every item of both cases, none left out: ``(name, ref, test)`` on the item's own samples."""
    ref, test, counts = ragged()
    out = [(f"ragged[{b}]", ref[b, :n], test[b, :n]) for b, n in enumerate(counts)]
    dref, dtest = dense()
    return out + [("dense[0]", dref[0], dtest[0])]


@functools.lru_cache(maxsize=None)
def restated(f32: bool = False):
    """``{name: sums}`` over ``items()``; float64 throughout, or the device's float32 chain."""
    return {name: R.sums(x, y, RESOLUTIONS, f32=f32) for name, x, y in items()}


def relative(got: float, want: float) -> float:
    return 0.0 if got == want else abs(got - want) / abs(want)


@functools.lru_cache(maxsize=None)
def e32():
    """``{name: {"spec": [R, 3], "wave": [3]}}``: the relative error of the float32 chain against float64, per output, on exactly
    these inputs (the empty item has none: its outputs are exact zeros)."""
    r64, r32 = restated(False), restated(True)
    out = {}
    for name, x, _ in items():
        if not len(x):
            continue
        out[name] = {"spec": np.array([[relative(r32[name]["spec"][r, w], r64[name]["spec"][r, w]) for w in range(3)]
                                       for r in range(len(RESOLUTIONS))]),
                     "wave": np.array([relative(r32[name]["wave"][w], r64[name]["wave"][w]) for w in range(3)])}
    return out
