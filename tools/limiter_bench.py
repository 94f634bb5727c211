#!/usr/bin/env python3
"""Times the device limiter (iris.limiter.Limiter.limit_device: 2 launches, no read-back) beside
(a) the same rules in torch ops on the same GPU: ``conv1d`` with the interpolation bank, the maximum, the division,
    ``-max_pool1d(-r)`` over ``2A + 1`` samples, ``conv1d`` with the smoothing weights, the product and the clamp, masked by the
    lengths, with no read-back -- and
(b) the host route it replaces: copy the batch out, the rules in numpy per item (tests/limiter_restatement.py: plain_f64), copy back.

    python tools/limiter_bench.py [--iters 10] [--rounds 5] [--out profiles/limiter_bench.json]

Two shapes of vocoder output at hop 256 (``row_scale = 256``), 22 050 Hz: 8 utterances of 128 .. 1024 mel frames, and 32 x 500.
Every item is a tone in noise at its own level with a quiet lead-in and tail and a few plosive-like peaks; the ceiling is -1 dBTP
and the lookahead 1.5 ms (A = 33).  Device events around `iters` back-to-back calls after a warm-up (a host clock for the host
route, which ends on the host); the three alternate in every round and the median round is reported with the spread.  Before
timing, the three routes' samples are compared: the device against the float64 rules and the torch route within 1e-5.  The stage's
bytes -- every item's samples read once and [B, L] samples written -- over its time stand beside the achievable HBM bandwidth.
Needs a GPU: there is no CPU fallback and no number without one.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tools"), str(REPO / "tests")]

from iris.limiter import Limiter  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402
import limiter_restatement as R  # noqa: E402

HOP, RATE = 256, 22050
HBM_ACHIEVABLE = 6.3e12           # bytes / s, the streaming figure for this GPU


def utterances(frames, seed):
    """``wav [B, HOP * max(frames)]``: item b is a 220 Hz tone in noise at its own level between a lead-in and tail of 1e-4, with
    a peak of 1.2 .. 1.6 every 4000 samples or so in every second item."""
    rng = np.random.default_rng(seed)
    wav = np.zeros((len(frames), HOP * max(frames)), dtype=np.float32)
    for b, m in enumerate(frames):
        n = HOP * m
        y = 1e-4 * rng.standard_normal(n)
        lo, hi = int(0.08 * n) + 37 * b, int(0.9 * n) - 53 * b
        t = np.arange(hi - lo) / float(RATE)
        level = 0.1 * (1.0 + b % 5)
        y[lo:hi] = level * np.sin(2.0 * np.pi * 220.0 * t) + 0.1 * level * rng.standard_normal(hi - lo)
        if b % 2 == 0:
            at = rng.integers(lo, hi, size=max(1, n // 4000))
            y[at] = rng.uniform(1.2, 1.6, size=len(at)) * rng.choice([-1.0, 1.0], size=len(at))
        wav[b, :n] = y
    return wav


class TorchLimiter:
    """The rules in torch ops, fp32 (the division in fp64); nothing comes back to the host."""

    def __init__(self, lm: Limiter, device):
        table = torch.from_numpy(lm.design()).to(device)
        self.A, self.c = lm.lookahead, float(lm.ceiling)
        self.bank = table[:36].reshape(3, 1, 12).contiguous()
        self.w = table[36:].reshape(1, 1, -1).contiguous()

    def __call__(self, wav, lengths):
        A, c = self.A, self.c
        B, L = wav.shape
        own = (torch.arange(L, device=wav.device)[None, :] < (lengths.to(torch.int64) * HOP)[:, None])
        x = torch.where(own, wav, torch.zeros((), device=wav.device))
        u = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (6, 6))[:, None, :], self.bank).abs().amax(dim=1)   # u[-1 .. L - 1]
        p = torch.maximum(x.abs(), torch.maximum(u[:, :-1], u[:, 1:]))
        r = torch.where(own & (p > c), (c / p.double()).float(), torch.ones((), device=wav.device))
        m = -torch.nn.functional.max_pool1d(-torch.nn.functional.pad(r, (2 * A, 2 * A), value=1.0)[:, None, :], 2 * A + 1, stride=1)
        g = 1.0 - torch.nn.functional.conv1d(1.0 - m, self.w)[:, 0, :]
        out = torch.where(own, (x * g).clamp(-c, c), torch.zeros((), device=wav.device))
        return out, torch.stack([p.amax(dim=1), torch.where(own, g, torch.ones((), device=wav.device)).amin(dim=1)], dim=1)


def host_route(lm: Limiter, table, wav, lengths_host):
    """Copy-out, the rules per item in numpy, copy back: what a caller did before the stage existed."""
    w = wav.cpu().numpy()
    out = np.zeros_like(w)
    for b, m in enumerate(lengths_host):
        out[b, :HOP * m] = R.plain_f64(w[b, :HOP * m], lm.ceiling, lm.lookahead, table)["out"]
    return torch.from_numpy(out).to(wav.device)


def host_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _summary(name: str, samples) -> dict:
    return {f"{name}_ms": float(np.median(samples)), f"{name}_ms_min_max": [float(min(samples)), float(max(samples))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("limiter_bench needs a GPU")
    dev = torch.device("cuda", 0)
    lm = Limiter(RATE, ceiling_dbtp=-1.0, lookahead_ms=1.5, device=dev)
    table = lm.design()
    ref = TorchLimiter(lm, dev)
    results = []
    for name, frames in (("8 x 128..1024", [128 * (i + 1) for i in range(8)]), ("32 x 500", [500] * 32)):
        wav = torch.from_numpy(utterances(frames, len(frames))).to(dev)
        lengths = torch.tensor(frames, dtype=torch.int32, device=dev)
        B, L = wav.shape
        ours = lambda: lm.limit_device(wav, lengths=lengths, row_scale=HOP)
        theirs = lambda: ref(wav, lengths)
        host = lambda: host_route(lm, table, wav, frames)
        out, stats = ours()
        t_out, t_stats = theirs()
        h_out = host()
        stats_h = stats.cpu().numpy()
        if not ((stats_h[:, 0] > lm.ceiling).any() and (stats_h[:, 0] <= lm.ceiling).any()):
            sys.exit(f"{name}: the batch should hold items over and under the ceiling")
        d_host = float((out - h_out).abs().max())
        d_torch = float((t_out - h_out).abs().max())
        if d_host > 1e-5 or d_torch > 1e-5 or float(out.abs().max()) > lm.ceiling:
            sys.exit(f"{name}: the three routes disagree on the samples: device {d_host:.3e}, torch {d_torch:.3e} off the float64 rules")
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_, c_ = [], [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
            c_.append(host_ms(host, max(1, args.iters // 5)))
        moved = 4 * (HOP * sum(frames) + B * L)
        rec = {"shape": name, "B": B, "L": L, "samples_in": HOP * sum(frames), "iters": args.iters, "rounds": args.rounds,
               "launches": lm.launch_count(B, L), "true_peak_dbtp": [float(v) for v in lm.true_peak_dbtp(stats_h)],
               "min_gain_db": [float(20.0 * np.log10(g)) for g in stats_h[:, 1]],
               **_summary("limit_device", a), **_summary("torch_ops", b_), **_summary("host_numpy", c_),
               "ratio_torch_over_device": float(np.median(b_) / np.median(a)), "ratio_host_over_device": float(np.median(c_) / np.median(a)),
               "device_vs_float64_rules_abs": d_host, "torch_vs_float64_rules_abs": d_torch,
               "bytes_moved": moved, "bytes_per_s": float(moved / (np.median(a) * 1e-3)),
               "share_of_achievable_hbm": float(moved / (np.median(a) * 1e-3) / HBM_ACHIEVABLE), "routes_agree": True}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/limiter_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": lm.get_config(),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
