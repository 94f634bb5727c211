#!/usr/bin/env python3
"""Times the device trim-and-join (iris.assemble.Assembler.join_device: 3 launches, no read-back) beside
(a) the same decision in torch ops on the same GPU -- pad, unfold, square, mean, compare, then per-item slices and torch.cat,
    which must read the bounds on the host -- and
(b) the host route it replaces: copy the batch out, the numpy restatement of librosa's loop per item, concatenate.

    python tools/assemble_bench.py [--iters 10] [--rounds 5] [--out profiles/assemble_bench.json]

Two shapes of vocoder output at hop 256 (``row_scale = 256``): 8 utterances of 128 .. 1024 mel frames, and 32 x 500.  Every item
is a tone in noise with a quiet lead-in and tail, so there is something to trim.  frame_length 2048, hop_length 512, top_db 40,
a pause of 0.25 s at 22 050 Hz, no fade (the torch and numpy routes have none).  Device events around `iters` back-to-back calls
after a warm-up (a host clock for the host route, which ends on the host); the three alternate in every round and the median
round is reported with the spread.  Before timing, the three routes' bounds and joined samples are compared.  The stage's
bytes -- every item's samples read once for the energies, the kept samples read again and `cap` samples written by the gather
-- over its time stand beside the achievable HBM bandwidth.  Needs a GPU: there is no CPU fallback and no number without one.
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

from iris.assemble import Assembler  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402
import assemble_restatement as R  # noqa: E402

HOP = 256
HBM_ACHIEVABLE = 6.3e12           # bytes / s, the streaming figure for this GPU


def utterances(frames, seed):
    """``wav [B, HOP * max(frames)]``: item b is a 220 Hz tone in noise between a quiet lead-in and tail of 1e-4."""
    rng = np.random.default_rng(seed)
    wav = np.zeros((len(frames), HOP * max(frames)), dtype=np.float32)
    for b, m in enumerate(frames):
        n = HOP * m
        y = 1e-4 * rng.standard_normal(n)
        lo, hi = int(0.08 * n) + 37 * b, int(0.9 * n) - 53 * b
        t = np.arange(hi - lo) / 22050.0
        y[lo:hi] = 0.5 * np.sin(2.0 * np.pi * 220.0 * t) + 0.05 * rng.standard_normal(hi - lo)
        wav[b, :n] = y
    return wav


class TorchJoin:
    """The decision in torch ops; the bounds come back to the host, where the slices are cut."""

    def __init__(self, a: Assembler):
        self.a, self.k = a, float(R.k_of(a.top_db))

    def __call__(self, wav, lengths_host):
        a = self.a
        F, H = a.frame_length, a.hop_length
        own = torch.tensor(lengths_host, device=wav.device) * HOP
        idx = torch.arange(wav.shape[1], device=wav.device)
        y = torch.where(idx[None, :] < own[:, None], wav, torch.zeros((), device=wav.device))
        mse = torch.nn.functional.pad(y, (F // 2, F // 2)).unfold(1, F, H).square().mean(dim=2)       # [B, T]
        valid = torch.arange(mse.shape[1], device=wav.device)[None, :] < (own // H + 1)[:, None]
        ref = mse.masked_fill(~valid, 0.0).amax(dim=1, keepdim=True)
        loud = (mse.clamp_min(R.AMIN) > ref.clamp_min(R.AMIN) * self.k) & valid
        t = torch.arange(mse.shape[1], device=wav.device)[None, :]
        first = torch.where(loud, t, mse.shape[1]).amin(dim=1)
        last = torch.where(loud, t, -1).amax(dim=1)
        bounds = torch.stack([first, last], dim=1).tolist()                                          # the host reads the bounds
        pieces, spans = [], []
        gap = torch.zeros(a.pause, device=wav.device)
        for b, (t0, t1) in enumerate(bounds):
            Lb = lengths_host[b] * HOP
            s, e = (t0 * H, min(Lb, (t1 + 1) * H)) if t1 >= 0 else (0, 0)
            s, e = max(0, s - a.pad), min(Lb, e + a.pad)
            spans.append((s, e))
            if e > s:
                if pieces:
                    pieces.append(gap)
                pieces.append(wav[b, s:e])
        return (torch.cat(pieces) if pieces else wav.new_zeros(0)), spans


def host_route(a: Assembler, wav, lengths_host):
    """Copy-out, librosa's loop in numpy per item, concatenate: what a caller did before the stage existed."""
    w = wav.cpu().numpy()
    items = [w[b, :HOP * m] for b, m in enumerate(lengths_host)]
    spans = R.spans_f64(items, a.frame_length, a.hop_length, a.top_db, a.ref, a.pad)
    pieces = []
    for y, (s, e) in zip(items, spans):
        if e > s:
            if pieces:
                pieces.append(np.zeros(a.pause, dtype=np.float32))
            pieces.append(y[s:e])
    return (np.concatenate(pieces) if pieces else np.zeros(0, np.float32)), spans


def host_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
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
        sys.exit("assemble_bench needs a GPU")
    dev = torch.device("cuda", 0)
    asm = Assembler(2048, 512, top_db=40.0, pause=5512, device=dev)
    ref = TorchJoin(asm)
    results = []
    for name, frames in (("8 x 128..1024", [128 * (i + 1) for i in range(8)]), ("32 x 500", [500] * 32)):
        wav = torch.from_numpy(utterances(frames, len(frames))).to(dev)
        lengths = torch.tensor(frames, dtype=torch.int32, device=dev)
        B, L = wav.shape
        ours = lambda: asm.join_device(wav, lengths=lengths, row_scale=HOP)
        theirs = lambda: ref(wav, frames)
        host = lambda: host_route(asm, wav, frames)
        out, offsets, spans = ours()
        total = int(offsets[-1])
        t_out, t_spans = theirs()
        h_out, h_spans = host()
        got_spans = [tuple(s) for s in spans.cpu().tolist()]
        if not (got_spans == t_spans == h_spans):
            sys.exit(f"{name}: the three routes disagree on the bounds: {got_spans} / {t_spans} / {h_spans}")
        if not (torch.equal(out[:total], t_out) and np.array_equal(out[:total].cpu().numpy(), h_out)):
            sys.exit(f"{name}: the three routes disagree on the joined samples")
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_, c_ = [], [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
            c_.append(host_ms(host, max(1, args.iters // 5)))
        kept = sum(e - s for s, e in got_spans)
        moved = 4 * (HOP * sum(frames) + kept + asm.capacity(B, L))
        rec = {"shape": name, "B": B, "L": L, "samples_in": HOP * sum(frames), "samples_kept": kept, "total": total, "cap": asm.capacity(B, L),
               "iters": args.iters, "rounds": args.rounds, "launches": asm.launch_count(B, L), **_summary("join_device", a),
               **_summary("torch_ops", b_), **_summary("host_numpy", c_),
               "ratio_torch_over_join": float(np.median(b_) / np.median(a)), "ratio_host_over_join": float(np.median(c_) / np.median(a)),
               "bytes_moved": moved, "bytes_per_s": float(moved / (np.median(a) * 1e-3)),
               "share_of_achievable_hbm": float(moved / (np.median(a) * 1e-3) / HBM_ACHIEVABLE), "routes_agree": True}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/assemble_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": asm.get_config(),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
