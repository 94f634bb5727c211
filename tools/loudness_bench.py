#!/usr/bin/env python3
"""Times the device loudness stage (iris.loudness.LoudnessNormalizer.normalize_device: 4 launches, no read-back) beside
(a) the same measure in torch ops on the same GPU, as far as torch can express it: the K-weighting recurrence has no torch op, so
    the two biquads are applied as their frequency response on a zero-padded float64 FFT (the impulse response has decayed below
    1e-16 long before the padding ends), then unfold, mean, the two gates, the gain and the product, with no read-back -- and
(b) the host route it replaces: copy the batch out, the plain BS.1770 loop in numpy / scipy per item
    (tests/loudness_restatement.py: reference_f64), scale, copy back.

    python tools/loudness_bench.py [--iters 10] [--rounds 5] [--out profiles/loudness_bench.json]

Two shapes of vocoder output at hop 256 (``row_scale = 256``), 22 050 Hz: 8 utterances of 128 .. 1024 mel frames, and 32 x 500.
Every item is a tone in noise at its own level with a quiet lead-in and tail.  Target -23 LUFS, a +30 dB cap, a ceiling of 0.95.
Device events around `iters` back-to-back calls after a warm-up (a host clock for the host route, which ends on the host); the
three alternate in every round and the median round is reported with the spread.  Before timing, the three routes' ``ms_b``, gains
and samples are compared: the device against the plain loop within 1e-12 (rounding order), the FFT route within 1e-9.  The stage's
bytes -- every item's samples read by the local pass, by the rerun and by the product, and [B, L] samples written -- over its
time stand beside the achievable HBM bandwidth.  Needs a GPU: there is no CPU fallback and no number without one.
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

from iris.loudness import LoudnessNormalizer  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402
import loudness_restatement as R  # noqa: E402

HOP, RATE = 256, 22050
HBM_ACHIEVABLE = 6.3e12           # bytes / s, the streaming figure for this GPU


def utterances(frames, seed):
    """``wav [B, HOP * max(frames)]``: item b is a 220 Hz tone in noise at its own level between a lead-in and tail of 1e-4."""
    rng = np.random.default_rng(seed)
    wav = np.zeros((len(frames), HOP * max(frames)), dtype=np.float32)
    for b, m in enumerate(frames):
        n = HOP * m
        y = 1e-4 * rng.standard_normal(n)
        lo, hi = int(0.08 * n) + 37 * b, int(0.9 * n) - 53 * b
        t = np.arange(hi - lo) / float(RATE)
        level = 0.05 * (1.0 + b % 5)
        y[lo:hi] = level * np.sin(2.0 * np.pi * 220.0 * t) + 0.1 * level * rng.standard_normal(hi - lo)
        wav[b, :n] = y
    return wav


class TorchLoudness:
    """The measure in torch ops, float64, the filters in the frequency domain; nothing comes back to the host."""

    def __init__(self, a: LoudnessNormalizer, L: int, device):
        d = a.design()
        self.d, self.step = d, a.sample_rate // 10
        self.nfft = 1 << int(np.ceil(np.log2(2 * L)))
        w = torch.exp(-2j * np.pi * torch.arange(self.nfft // 2 + 1, dtype=torch.float64, device=device) / self.nfft)
        sec = lambda o: (d[o] + d[o + 1] * w + d[o + 2] * w * w) / (1.0 + d[o + 3] * w + d[o + 4] * w * w)
        self.H = sec(R.SHELF) * sec(R.HIGH_PASS)

    def __call__(self, wav, lengths):
        d, step = self.d, self.step
        B, L = wav.shape
        own = lengths.to(torch.int64) * HOP
        idx = torch.arange(L, device=wav.device)
        y = torch.where(idx[None, :] < own[:, None], wav, torch.zeros((), device=wav.device))
        v = torch.fft.irfft(torch.fft.rfft(y.double(), n=self.nfft) * self.H, n=self.nfft)[:, :L]
        z = v.square().unfold(1, 4 * step, step).mean(dim=2)                                      # [B, J]
        valid = torch.arange(z.shape[1], device=wav.device)[None, :] < ((own - 4 * step) // step + 1).clamp_min(0)[:, None]
        gate1 = valid & (z > d[R.ABS_THR])
        n1 = gate1.sum(dim=1)
        rel = 0.1 * (z * gate1).sum(dim=1) / n1.clamp_min(1)
        gate2 = gate1 & (z > rel[:, None])
        n2 = gate2.sum(dim=1)
        ms = torch.where(n2 > 0, (z * gate2).sum(dim=1) / n2.clamp_min(1), torch.zeros((), dtype=torch.float64, device=wav.device))
        peak = y.abs().amax(dim=1).double()
        g = torch.sqrt(d[R.TARGET_MS] / ms.clamp_min(1e-300)).clamp_max(d[R.MAX_GAIN])
        if d[R.CEILING] > 0:
            g = torch.minimum(g, d[R.CEILING] / peak.clamp_min(1e-300))
        g = torch.where(ms > 0, g, torch.ones((), dtype=torch.float64, device=wav.device))
        return y * g.float()[:, None], torch.stack([ms, g], dim=1)


def host_route(a: LoudnessNormalizer, d, wav, lengths_host):
    """Copy-out, the plain loop per item, scale, copy back: what a caller did before the stage existed."""
    w = wav.cpu().numpy()
    out = np.zeros_like(w)
    stats = []
    for b, m in enumerate(lengths_host):
        r = R.reference_f64(w[b, :HOP * m], a.sample_rate, d)
        out[b, :HOP * m] = w[b, :HOP * m] * np.float32(r["gain"])
        stats.append((r["ms"], r["gain"]))
    return torch.from_numpy(out).to(wav.device), np.array(stats)


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
        sys.exit("loudness_bench needs a GPU")
    dev = torch.device("cuda", 0)
    ld = LoudnessNormalizer(RATE, target_lufs=-23.0, max_gain_db=30.0, peak_ceiling=0.95, device=dev)
    table = ld.design()
    results = []
    for name, frames in (("8 x 128..1024", [128 * (i + 1) for i in range(8)]), ("32 x 500", [500] * 32)):
        wav = torch.from_numpy(utterances(frames, len(frames))).to(dev)
        lengths = torch.tensor(frames, dtype=torch.int32, device=dev)
        B, L = wav.shape
        ref = TorchLoudness(ld, L, dev)
        ours = lambda: ld.normalize_device(wav, lengths=lengths, row_scale=HOP)
        theirs = lambda: ref(wav, lengths)
        host = lambda: host_route(ld, table, wav, frames)
        out, stats = ours()
        t_out, t_stats = theirs()
        h_out, h_stats = host()
        stats_h, t_stats_h = stats.cpu().numpy(), t_stats.cpu().numpy()
        if not (stats_h[:, 0] > 0).all():
            sys.exit(f"{name}: an item was not measured")
        d_host = float(np.abs(stats_h / h_stats - 1.0).max())
        d_torch = float(np.abs(t_stats_h / h_stats - 1.0).max())
        if d_host > 1e-12 or d_torch > 1e-9:
            sys.exit(f"{name}: the three routes disagree on ms_b / g_b: device {d_host:.3e}, torch {d_torch:.3e} off the plain loop")
        # a gain one float32 ulp apart moves a sample by one ulp: 2^-23 relative, with room for the product's own rounding
        if not (torch.allclose(out, h_out, rtol=2.0 ** -22, atol=0.0) and torch.allclose(t_out, h_out, rtol=2.0 ** -22, atol=0.0)):
            sys.exit(f"{name}: the three routes disagree on the samples")
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_, c_ = [], [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
            c_.append(host_ms(host, max(1, args.iters // 5)))
        moved = 4 * (3 * HOP * sum(frames) + B * L)
        rec = {"shape": name, "B": B, "L": L, "samples_in": HOP * sum(frames), "iters": args.iters, "rounds": args.rounds,
               "launches": ld.launch_count(B, L), "lufs_in": [float(v) for v in ld.loudness_lufs(stats_h)],
               "gain_db": [float(20.0 * np.log10(g)) for g in stats_h[:, 1]],
               **_summary("normalize_device", a), **_summary("torch_ops", b_), **_summary("host_numpy", c_),
               "ratio_torch_over_device": float(np.median(b_) / np.median(a)), "ratio_host_over_device": float(np.median(c_) / np.median(a)),
               "device_vs_plain_loop_rel": d_host, "torch_vs_plain_loop_rel": d_torch,
               "bytes_moved": moved, "bytes_per_s": float(moved / (np.median(a) * 1e-3)),
               "share_of_achievable_hbm": float(moved / (np.median(a) * 1e-3) / HBM_ACHIEVABLE), "routes_agree": True}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/loudness_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": ld.get_config(),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
