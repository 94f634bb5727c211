#!/usr/bin/env python3
"""Times the device Griffin-Lim vocoder (iris.griffin_lim.GriffinLim.forward_device: 2 * n_iter + 2 launches) against the same
loop written with torch.istft / torch.stft and elementwise ops on the same GPU, from the same inverted magnitudes and the same
start phase.

    python tools/griffin_lim_bench.py [--iters 10] [--rounds 5] [--out profiles/griffin_lim_bench.json]
    python tools/griffin_lim_bench.py --ragged             # 8 utterances of 128 .. 1024 frames: ragged, per-item loop, dense padded
    python tools/griffin_lim_bench.py --phase device       # 1 x 1000 host-inclusive: host-drawn and uploaded phase against device-drawn

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


def _summary(name: str, samples) -> dict:
    return {f"{name}_ms": float(np.median(samples)), f"{name}_ms_min_max": [float(min(samples)), float(max(samples))]}


def _finish(args, dev, gl, results):
    out = {"tool": "tools/griffin_lim_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": gl.get_config(), "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


def ragged_main(args, dev):
    """8 utterances of 128 ... 1024 frames: ONE ragged call, the loop of one dense call per utterance (what a batch of unequal
    lengths cost before the ragged form), and the dense 8 x 1024 call that padding alone would run.  Device events; the three
    alternate in every round."""
    gl = GriffinLim()
    lengths = [128 * (i + 1) for i in range(8)]
    B, T = len(lengths), max(lengths)
    rng = np.random.default_rng(B * T)
    logmel = torch.from_numpy((-6.0 + 3.0 * rng.standard_normal((B, gl.n_mels, T))).astype(np.float32)).to(dev)
    packed = gl.draw_phase(B, T)
    ln = torch.tensor(lengths, dtype=torch.int32, device=dev)
    items = [(logmel[b:b + 1, :, :n].contiguous(), packed[b:b + 1, :n].contiguous()) for b, n in enumerate(lengths)]
    ragged = lambda: gl.forward_device(logmel, packed, lengths=ln)
    loop = lambda: [gl.forward_device(m, p) for m, p in items]
    dense = lambda: gl.forward_device(logmel, packed)
    got = ragged()
    same = all(torch.equal(got[b, :gl.samples_of(n)], w[0]) for b, (n, w) in enumerate(zip(lengths, loop())))
    fns = {"ragged": ragged, "per_item_loop": loop, "dense_padded": dense}
    for fn in fns.values():
        time_ms(fn, 2, dev)
    samples = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            samples[k].append(time_ms(fn, args.iters, dev))
    rec = {"shape": "ragged 8 x (128 .. 1024)", "frames": sum(lengths), "n_iter": gl.n_iter, "iters": args.iters, "rounds": args.rounds,
           "launches_ragged": gl.launch_count(B, T), "launches_loop": sum(gl.launch_count(1, n) for n in lengths),
           "items_equal_their_own_call": bool(same)}
    for k, v in samples.items():
        rec.update(_summary(k, v))
    rec["ratio_loop_over_ragged"] = rec["per_item_loop_ms"] / rec["ragged_ms"]
    print(json.dumps(rec))
    _finish(args, dev, gl, [rec])


def phase_main(args, dev):
    """1 x 1000 frames, host-inclusive: a host clock from ``forward_device(mel)`` on a device mel (no phase given) until the
    waveform is ready, with the start phase drawn on the host and uploaded, or drawn by the inversion kernel.  Both are timed
    in every run, alternating; ``--phase`` names the one the record is about."""
    import time
    models = {"host": GriffinLim(phase="host"), "device": GriffinLim(phase="device")}
    B, T = 1, 1000
    rng = np.random.default_rng(B * T)
    logmel = torch.from_numpy((-6.0 + 3.0 * rng.standard_normal((B, models["host"].n_mels, T))).astype(np.float32)).to(dev)

    def wall_ms(gl):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.iters):
            gl.forward_device(logmel)
            torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / args.iters

    for gl in models.values():
        gl.forward_device(logmel)
        wall_ms(gl)
    samples = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, gl in models.items():
            samples[k].append(wall_ms(gl))
    packed = models["host"].draw_phase(B, T)
    rec = {"shape": f"{B}x{T}", "phase": args.phase, "n_iter": models["host"].n_iter, "iters": args.iters, "rounds": args.rounds,
           "device_only_ms": float(np.median([time_ms(lambda: models["host"].forward_device(logmel, packed), args.iters, dev)
                                              for _ in range(args.rounds)])),
           "uploaded_bytes_host_phase": B * T * models["host"].n_bins * 2 * 4}
    for k, v in samples.items():
        rec.update(_summary(f"wall_{k}_phase", v))
    rec["host_draw_and_upload_ms"] = rec["wall_host_phase_ms"] - rec["wall_device_phase_ms"]
    print(json.dumps(rec))
    _finish(args, dev, models[args.phase], [rec])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true", help="8 utterances of 128 .. 1024 frames: ragged call, per-item loop, dense padded")
    ap.add_argument("--phase", choices=("host", "device"), default=None,
                    help="1 x 1000 frames timed host-inclusive with the start phase from the host or drawn on the device")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("griffin_lim_bench needs a GPU")
    dev = torch.device("cuda", 0)
    if args.ragged:
        return ragged_main(args, dev)
    if args.phase:
        return phase_main(args, dev)
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
    _finish(args, dev, gl, results)


if __name__ == "__main__":
    main()
