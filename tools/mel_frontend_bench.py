#!/usr/bin/env python3
"""Times the device mel front-end (iris.mel.MelFrontend.forward_device: one launch) against torch.stft + matmul + log on the
same GPU, with the same window and the filterbank the library designs.

    python tools/mel_frontend_bench.py [--iters 100] [--rounds 5] [--out profiles/mel_frontend_bench.json]

Two shapes: one utterance of 1000 frames (255 744 samples), and 8 ragged utterances of 128, 256, ..., 1024 frames in one
call (the torch side runs the padded batch: it has no ragged form, so its numbers past an item's end are not the item's).
Device events around `iters` back-to-back calls, after a warm-up; the implementations alternate in every round and the
median round is reported with the spread.  Outputs are compared before timing.  Needs a GPU: there is no CPU fallback and
no number without one.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tests"), str(REPO / "tools")]

from iris.mel import MelFrontend  # noqa: E402
from mel_cases import DEFAULT, waveform  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402


class TorchMel:
    def __init__(self, fe: MelFrontend, dev):
        self.fe = fe
        self.fb = torch.from_numpy(fe.design()[1]).to(dev)
        self.win = torch.hann_window(fe.win_length, periodic=True, dtype=torch.float32, device=dev)

    def __call__(self, audio):
        fe = self.fe
        spec = torch.stft(audio, fe.n_fft, hop_length=fe.hop_length, win_length=fe.win_length, window=self.win, center=True,
                          pad_mode="constant", return_complex=True)
        return torch.log(torch.clamp(torch.matmul(self.fb, spec.abs()), min=1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mel_frontend_bench needs a GPU")
    dev = torch.device("cuda", 0)
    fe = MelFrontend(**DEFAULT)
    ref = TorchMel(fe, dev)
    hop = fe.hop_length
    results = []
    frames = [128 * (i + 1) for i in range(8)]
    samples = [hop * (t - 1) + 17 * i for i, t in enumerate(frames)]            # 1 + n // hop == t
    shapes = [("1x1000", [hop * 999]), ("8_ragged_128..1024", samples)]
    for name, counts in shapes:
        L = max(counts)
        audio = np.zeros((len(counts), L), dtype=np.float32)
        for b, n in enumerate(counts):
            audio[b, :n] = waveform(n, DEFAULT, seed=b)
        x = torch.from_numpy(audio).to(dev)
        lengths = None if len(counts) == 1 else torch.tensor(counts, dtype=torch.int32, device=dev)
        ours = lambda: fe.forward_device(x, lengths=lengths)
        theirs = lambda: ref(x)
        mel, got_frames = ours()
        want = theirs()
        diffs = []
        for b, n in enumerate(counts):
            t = 1 + n // hop
            assert int(got_frames[b]) == t
            if lengths is None:
                diffs.append(float((mel[b, :, :t] - want[b, :, :t]).abs().max()))
            else:                                               # the padded torch call sees zeros where the item ends: compare alone
                alone = ref(x[b:b + 1, :n])
                diffs.append(float((mel[b, :, :t] - alone[0]).abs().max()))
        for fn in (ours, theirs):
            time_ms(fn, 10, dev)
        a, b_ = [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
        rec = {"shape": name, "samples": counts, "frames": [1 + n // hop for n in counts], "iters": args.iters, "rounds": args.rounds,
               "device_ms": float(np.median(a)), "device_ms_min_max": [float(min(a)), float(max(a))],
               "torch_ms": float(np.median(b_)), "torch_ms_min_max": [float(min(b_)), float(max(b_))],
               "ratio_torch_over_device": float(np.median(b_) / np.median(a)), "launches": fe.launch_count(len(counts), L),
               "max_abs_diff_vs_torch_log_mel": max(diffs)}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/mel_frontend_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": fe.get_config(), "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
