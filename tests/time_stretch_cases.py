"""Configs, shapes and seeded inputs shared by tests/test_time_stretch.py and tests/test_gpu_time_stretch.py.

Configs are tests/denoiser_cases.py's (``small`` 64 / 16 / 48, ``two_tap`` 256 / 128 / 256, ``default`` 1024 / 256 / 1024) and a
case's waveform is that file's recipe (``O.dn_waveform_item``): two tones at 1 % and 9 % of the sample rate, amplitudes 0.7 and
0.1, plus white noise at 1e-3, ``hop M`` samples.  tests/test_time_stretch.py asserts what each case is here for.
"""
from __future__ import annotations

import numpy as np

import denoiser_cases as DC
import time_stretch_restatement as R

CONFIGS = {name: DC.CONFIGS[name] for name in ("default", "small", "two_tap")}
SEMITONE_DOWN = 2.0 ** (-1.0 / 12.0)

# (config, B, M, rate)
CASES = (
    ("default", 2, 32, 1.0),             # rate 1; T_out = 33: one past a 32-frame block edge, and no multiple of the scan's run of 2
    ("small", 1, 69, SEMITONE_DOWN),     # a non-dyadic rate; T_out = 75: three blocks
    ("small", 1, 2, 0.8),                # T = 3: fewer frames than taps
    ("small", 1, 1, 4.0),                # T = 2, T_out = 1
    ("default", 2, 32, 0.8),             # n_out = 10240 < H (T_out - 1) = 10496: the crop is live
    ("default", 2, 39, 1.25),            # n_out = 7987 > H (T_out - 1) = 7936: the tail rule is live
    ("two_tap", 1, 33, 1.5),             # T_out = 23: fewer frames than the scan has runs
)
SCAN_RUNS = 32                           # ts::kScanRuns (csrc/time_stretch.h)
BLOCK_FRAMES = 32                        # stft::kRows


def case_id(case) -> str:
    return f"{case[0]}-B{case[1]}-M{case[2]}-r{case[3]:.4g}"


stft_args = DC.stft_args
tables = DC.tables
waveform_item = DC.waveform_item


def shape(case) -> dict:
    """``T``, ``T_out``, ``L``, ``n_out`` and the transform sizes of a case, from the restatement's rules."""
    name, _, M, rate = case
    n_fft, hop, _ = stft_args(name)
    return dict(n_fft=n_fft, hop=hop, taps=n_fft // hop, T=M + 1, L=hop * M, T_out=R.out_frames(M + 1, rate), n_out=R.out_samples(hop * M, rate))


_cache: dict = {}


def waveform(case) -> np.ndarray:
    """``[B, hop M]`` float32."""
    key = ("wav",) + tuple(case[:3])
    if key not in _cache:
        name, B, M = case[:3]
        cfg = CONFIGS[name]
        _cache[key] = np.stack([waveform_item(cfg["hop_length"] * M, cfg, seed=b) for b in range(B)])
        _cache[key].setflags(write=False)
    return _cache[key]


def restated(case, f32: bool = False):
    """``(out [B, n_out], taps)`` of the restatement, float64 or fp32 on the library's tables; ``taps`` is a list of per-item
    dicts (``re``, ``im``, ``mag``, ``out_re``, ``out_im``, and in fp32 ``inc``, ``acc``).  Cached and never changed."""
    key = ("out", case, f32)
    if key not in _cache:
        name, rate = case[0], case[3]
        kw = dict(dtype=np.float32, tables=tables(name)) if f32 else {}
        runs = [R.stretch(y, rate, *stft_args(name), taps=True, **kw) for y in waveform(case)]
        out = np.stack([r[0] for r in runs])
        out.setflags(write=False)
        _cache[key] = (out, [r[1] for r in runs])
    return _cache[key]


def rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def e32() -> dict:
    """``{"out": .., "mag": .., "out_c": ..}``: the largest |fp32 restatement - float64 restatement| / max(1, max |float64|) over
    the cases.  ``out``: the whole stretch, both from the waveform.  ``mag`` and ``out_c``: launches 2 and 3 alone -- the fp32
    step against the float64 step on the SAME fp32 spectrum, so that the conditioning of a near-empty bin's phase (which the
    spectrum's own rounding moves) stays out of the step's bar.  ``"per_case"`` holds the rows."""
    if "e32" not in _cache:
        worst, rows = {"out": 0.0, "mag": 0.0, "out_c": 0.0}, {}
        for case in CASES:
            name, rate = case[0], case[3]
            n_fft, hop, _ = stft_args(name)
            (w64, _), (w32, t32) = restated(case), restated(case, f32=True)
            row = {"out": rel(w32, w64), "mag": 0.0, "out_c": 0.0}
            for tap in t32:
                m64 = R.middle(tap["re"], tap["im"], rate, n_fft, hop, np.float64)
                row["mag"] = max(row["mag"], rel(tap["mag"], m64["mag"]))
                want = np.stack([m64["out_re"], m64["out_im"]])
                row["out_c"] = max(row["out_c"], rel(np.stack([tap["out_re"], tap["out_im"]]), want))
            for k, v in row.items():
                worst[k] = max(worst[k], v)
            rows[case] = row
        _cache["e32"] = {**worst, "per_case": rows}
    return _cache["e32"]
