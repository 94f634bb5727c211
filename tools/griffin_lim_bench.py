#!/usr/bin/env python3
"""Times the device Griffin-Lim vocoder (iris.griffin_lim.GriffinLim.forward_device: 2 * n_iter + 2 launches) against the same
loop written with torch.istft / torch.stft and elementwise ops on the same GPU, from the same inverted magnitudes and the same
start phase.

    python tools/griffin_lim_bench.py [--iters 10] [--rounds 5] [--out profiles/griffin_lim_bench.json]

Two shapes at the defaults (n_iter 60): 1 x 1000 and 8 x 500 frames.  Device events around `iters` back-to-back calls, after a
warm-up; the implementations alternate in every round and the median round is reported with the spread.  Before timing, the
first iSTFT of both (n_iter = 0, linear) is compared.  The mel inversion is in the device's time and not in torch's, which
starts from the device's magnitudes.  Needs a GPU: there is no CPU fallback and no number without one.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tools")]

from iris.griffin_lim import GriffinLim, pack_phase, start_phase  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402

TINY = float(np.finfo(np.float32).tiny)


class TorchGriffinLim:
    def __init__(self, gl: GriffinLim, dev):
        self.gl = gl
        self.win = torch.hann_window(gl.win_length, periodic=True, dtype=torch.float32, device=dev)
        self.alpha = gl.momentum / (1.0 + gl.momentum)

    def _stft(self, y):
        g = self.gl
        return torch.stft(y, g.n_fft, hop_length=g.hop_length, win_length=g.win_length, window=self.win, center=True,
                          pad_mode="constant", return_complex=True)

    def _istft(self, c, n):
        g = self.gl
        return torch.istft(c, g.n_fft, hop_length=g.hop_length, win_length=g.win_length, window=self.win, center=True, length=n)

    def __call__(self, S, c0, n_iter):
        """``S [B, K, T]`` real, ``c0 [B, K, T]`` complex."""
        n = self.gl.samples_of(S.shape[2])
        c, prev = c0, None
        for _ in range(n_iter):
            r = self._stft(self._istft(c, n))
            a = r if prev is None else r - self.alpha * prev
            c = S * a / (a.abs() + TINY)
            prev = r
        return self._istft(c, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("griffin_lim_bench needs a GPU")
    dev = torch.device("cuda", 0)
    gl, gl0 = GriffinLim(), GriffinLim(n_iter=0)
    ref = TorchGriffinLim(gl, dev)
    results = []
    for B, T in ((1, 1000), (8, 500)):
        rng = np.random.default_rng(B * T)
        logmel = torch.from_numpy((-6.0 + 3.0 * rng.standard_normal((B, gl.n_mels, T))).astype(np.float32)).to(dev)
        phi = start_phase(B, gl.n_bins, T)
        packed = torch.from_numpy(pack_phase(phi)).to(dev)
        first = gl0.forward_device(logmel, packed)                       # n_iter = 0: S and one iSTFT
        S = gl0.magnitudes(B, T)
        c0 = S * torch.polar(torch.ones_like(S), torch.from_numpy(phi.astype(np.float32)).to(dev))
        diff0 = float((ref(S, c0, 0) - first).abs().max())
        ours = lambda: gl.forward_device(logmel, packed)
        theirs = lambda: ref(S, c0, gl.n_iter)
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_ = [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
        rec = {"shape": f"{B}x{T}", "n_iter": gl.n_iter, "iters": args.iters, "rounds": args.rounds,
               "device_ms": float(np.median(a)), "device_ms_min_max": [float(min(a)), float(max(a))],
               "torch_ms": float(np.median(b_)), "torch_ms_min_max": [float(min(b_)), float(max(b_))],
               "ratio_torch_over_device": float(np.median(b_) / np.median(a)), "launches": gl.launch_count(B, T),
               "max_abs_diff_first_istft_vs_torch": diff0}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/griffin_lim_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": gl.get_config(), "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
