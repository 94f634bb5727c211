#!/usr/bin/env python3
"""Times the device time stretch (iris.time_stretch.TimeStretch.forward_device: 4 launches) beside
(a) Denoiser.forward_device at strength 0 on the same input -- the same two transforms, so the difference is what the phase
    vocoder's step and scan cost -- and
(b) the same algorithm in torch ops (torch.stft, cumsum, torch.istft) on the same GPU.

    python tools/time_stretch_bench.py [--rate 1.0] [--iters 10] [--rounds 5] [--out profiles/time_stretch_bench.json]
    python tools/time_stretch_bench.py --chunked 256 [--rate 0.9] [--out profiles/time_stretch_bench.json]

``--chunked FRAMES`` times the chunked form instead: 1 x 1000 frames pushed into a ``StretchSession`` in pieces of FRAMES mel
frames (and flushed) against the whole-utterance call on the same input, alternating in every round; the session's result is
compared with the whole one bit for bit first.  With ``--out`` the record goes under ``"chunked"`` of that file, beside what
it holds.

Two shapes at n_fft 1024, hop 256: 1 x 1000 and 32 x 500 mel frames of vocoder output.  Device events around `iters`
back-to-back calls, after a warm-up; the three alternate in every round and the median round is reported with the spread.
Before timing, the device result is compared with the torch one on the interior samples.  Needs a GPU: there is no CPU fallback
and no number without one.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tools")]

from iris.denoiser import Denoiser  # noqa: E402
from iris.time_stretch import TimeStretch  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402


class TorchStretch:
    """librosa's phase_vocoder in torch ops, vectorised over time: the increments are independent, the accumulator a cumsum."""

    def __init__(self, ts: TimeStretch, dev):
        self.ts = ts
        self.win = torch.hann_window(ts.win_length, periodic=True, dtype=torch.float32, device=dev)
        k = torch.arange(ts.n_bins, device=dev, dtype=torch.float32)
        self.adv = (math.pi * ts.hop_length * k / (ts.n_fft // 2))[None, :, None]

    def __call__(self, wav, rate):
        d = self.ts
        a = torch.stft(wav, d.n_fft, hop_length=d.hop_length, win_length=d.win_length, window=self.win, center=True,
                       pad_mode="constant", return_complex=True)                         # [B, K, T]
        T = a.shape[2]
        steps = torch.arange(0, T, rate, dtype=torch.float64, device=wav.device)
        idx = steps.floor().long()
        alpha = (steps - idx).float()[None, None, :]
        a = torch.nn.functional.pad(a, (0, 2))
        c0, c1 = a[:, :, idx], a[:, :, idx + 1]
        mag = (1.0 - alpha) * c0.abs() + alpha * c1.abs()
        dphi = c1.angle() - c0.angle() - self.adv
        dphi = dphi - 2.0 * math.pi * torch.round(dphi / (2.0 * math.pi))
        inc = self.adv + dphi
        acc = a[:, :, :1].angle() + torch.cumsum(inc, dim=2) - inc
        out = torch.polar(mag, acc)
        return torch.istft(out, d.n_fft, hop_length=d.hop_length, win_length=d.win_length, window=self.win, center=True,
                           length=int(round(wav.shape[1] / rate)))


def _summary(name: str, samples) -> dict:
    return {f"{name}_ms": float(np.median(samples)), f"{name}_ms_min_max": [float(min(samples)), float(max(samples))]}


def chunked(ts: TimeStretch, dev, frames: int, rate: float, iters: int, rounds: int) -> dict:
    M, hop = 1000, ts.hop_length
    rng = np.random.default_rng(M)
    t = np.arange(hop * M) / 22050.0
    wav = torch.from_numpy((0.5 * np.sin(2.0 * np.pi * 220.0 * t)[None, :] + 0.05 * rng.standard_normal((1, hop * M))).astype(np.float32)).to(dev)
    pieces = [wav[:, at:at + hop * frames].contiguous() for at in range(0, hop * M, hop * frames)]
    windows = []

    def session():
        s = ts.open_session(rate)
        out = [s.push(p) for p in pieces] + [s.flush()]
        return torch.cat(out, dim=1)

    whole = lambda: ts.forward_device(wav, rate)[0]
    if not torch.equal(session(), whole()):
        sys.exit("the session's output differs from the whole-utterance call")
    base = total = u = 0
    for n, final in [(p.shape[1], False) for p in pieces] + [(0, True)]:                 # the windows the session ran, from the plan
        total += n
        u_hi, _, count, keep = ts.window_plan(rate, base, total - base, final, u)
        if u_hi > u or count:
            windows.append({"origin": base, "samples": total - base, "frames": u_hi - u, "emitted": count,
                            "launches": ts.window_launch_count(1, total - base, rate, base, final, u)})
        u, base = u_hi, max(base, min(keep, total))
    for fn in (session, whole):
        time_ms(fn, 2, dev)
    a, b = [], []
    for _ in range(rounds):
        a.append(time_ms(session, iters, dev))
        b.append(time_ms(whole, iters, dev))
    extra = float(np.median(a) - np.median(b))
    return {"shape": f"1x{M}", "rate": rate, "push_frames": frames, "pushes": len(pieces), "windows": windows, "iters": iters, "rounds": rounds,
            **_summary("session", a), **_summary("whole", b), "extra_ms": extra, "extra_ms_per_window": extra / len(windows),
            "bit_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunked", type=int, default=0, metavar="FRAMES")
    ap.add_argument("--rate", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_stretch_bench needs a GPU")
    dev = torch.device("cuda", 0)
    ts = TimeStretch(1024, 256, device=dev)
    if args.chunked:
        rec = chunked(ts, dev, args.chunked, args.rate, args.iters, args.rounds)
        print(json.dumps(rec))
        if args.out:
            path = Path(args.out)
            out = json.loads(path.read_text()) if path.exists() else {"tool": "tools/time_stretch_bench.py", "gpu": torch.cuda.get_device_name(dev),
                                                                      "config": ts.get_config()}
            out["chunked"] = rec
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(out, indent=1) + "\n")
        return
    dn = Denoiser(1024, 256, 1024, strength=0.0, device=dev)
    ref = TorchStretch(ts, dev)
    results = []
    for B, M in ((1, 1000), (32, 500)):
        rng = np.random.default_rng(B * M)
        L = ts.hop_length * M
        t = np.arange(L) / 22050.0
        tone = 0.5 * np.sin(2.0 * np.pi * 220.0 * t)[None, :] + 0.05 * rng.standard_normal((B, L))
        wav = torch.from_numpy(tone.astype(np.float32)).to(dev)
        ours = lambda: ts.forward_device(wav, args.rate)[0]
        plain = lambda: dn.forward_device(wav)
        theirs = lambda: ref(wav, args.rate)
        got, want = ours(), theirs()
        interior = slice(ts.n_fft, min(got.shape[1], want.shape[1]) - 2 * ts.n_fft)
        diff = float((got[:, interior] - want[:, interior]).abs().max())
        for fn in (ours, plain, theirs):
            time_ms(fn, 2, dev)
        a, b_, c_ = [], [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(plain, args.iters, dev))
            c_.append(time_ms(theirs, args.iters, dev))
        rec = {"shape": f"{B}x{M}", "rate": args.rate, "samples_in": B * L, "samples_out": B * got.shape[1], "iters": args.iters,
               "rounds": args.rounds, "launches": ts.launch_count(B, L, args.rate), **_summary("stretch", a),
               **_summary("denoiser_strength_0", b_), **_summary("torch", c_),
               "step_and_scan_ms": float(np.median(a) - np.median(b_)), "ratio_torch_over_stretch": float(np.median(c_) / np.median(a)),
               "max_abs_diff_vs_torch_interior": diff}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/time_stretch_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": ts.get_config(), "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
