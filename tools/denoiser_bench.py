#!/usr/bin/env python3
"""Times the device bias denoiser (iris.denoiser.Denoiser.forward_device: 2 launches) against the same step written with
torch.stft -> subtract -> torch.istft on the same GPU, and, host-inclusive, against what a caller did before the stage existed:
copy the waveform out and run the loop in numpy.

    python tools/denoiser_bench.py [--iters 10] [--rounds 5] [--out profiles/denoiser_bench.json]
    python tools/denoiser_bench.py --chunked 256          # a DenoiserSession in 256-frame pushes against the whole-utterance call

Two shapes at the defaults (n_fft 1024, hop 256): 1 x 1000 and 32 x 500 mel frames of vocoder output.  Device events around
`iters` back-to-back calls, after a warm-up; the implementations alternate in every round and the median round is reported
with the spread.  The host-inclusive figures are a host clock from a device waveform until the denoised waveform is on the host
(device stage) or from the same device waveform through copy-out and numpy's rfft / irfft (host loop, fewer rounds: it is
slow).  Before timing, the two device results are compared.  Needs a GPU: there is no CPU fallback and no number without one.

--chunked CHUNK_FRAMES: 1 x 1000 frames only.  One session (``Denoiser.open_session``: pushes of CHUNK_FRAMES frames, then
``flush``) against ``forward_device`` of the same waveform in the same process, after checking that the two agree bit for bit.
Device events around `iters` whole sessions, the two alternating in every round; reported are the session's total, the total
divided by its windows (the per-push time) and the ratio total / whole with the spread over the rounds.
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
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tools")]

from iris.denoiser import Denoiser  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402


class TorchDenoiser:
    def __init__(self, dn: Denoiser, bias: torch.Tensor, dev):
        self.dn, self.bias = dn, bias[None, :, None]
        self.win = torch.hann_window(dn.win_length, periodic=True, dtype=torch.float32, device=dev)

    def __call__(self, wav, strength):
        d = self.dn
        a = torch.stft(wav, d.n_fft, hop_length=d.hop_length, win_length=d.win_length, window=self.win, center=True,
                       pad_mode="constant", return_complex=True)
        mag = a.abs()
        g = torch.clamp(mag - strength * self.bias, min=0.0)
        c = a * torch.where(mag > 0, g / mag, torch.zeros_like(mag))
        return torch.istft(c, d.n_fft, hop_length=d.hop_length, win_length=d.win_length, window=self.win, center=True,
                           length=wav.shape[1])


def numpy_denoise(wav: np.ndarray, bias: np.ndarray, strength: float, n_fft: int, hop: int) -> np.ndarray:
    """The host loop: frames, rfft, subtract, irfft, overlap-add (float32 in, float32 out; win_length == n_fft)."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
    B, L = wav.shape
    T = L // hop + 1
    y = np.pad(wav, ((0, 0), (n_fft // 2, n_fft // 2)))
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    a = np.fft.rfft(y[:, idx] * w, axis=2)
    mag = np.abs(a)
    g = np.maximum(mag - strength * bias[None, None, :], 0.0)
    c = a * np.where(mag > 0, g / np.maximum(mag, 1e-30), 0.0)
    fr = np.fft.irfft(c, n=n_fft, axis=2) * w
    out = np.zeros((B, n_fft + hop * (T - 1)), dtype=np.float64)
    wss = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, t]
        wss[t * hop:t * hop + n_fft] += w.astype(np.float64) ** 2
    out /= np.where(wss > 1e-30, wss, 1.0)
    return out[:, n_fft // 2:n_fft // 2 + L].astype(np.float32)


def _summary(name: str, samples) -> dict:
    return {f"{name}_ms": float(np.median(samples)), f"{name}_ms_min_max": [float(min(samples)), float(max(samples))]}


def chunked_main(args, dev):
    dn = Denoiser(strength=args.strength, device=dev)
    M, hop = 1000, dn.hop_length
    rng = np.random.default_rng(M)
    wav = torch.from_numpy((0.1 * rng.standard_normal((1, hop * M))).astype(np.float32)).to(dev)
    hum = torch.from_numpy((0.01 * rng.standard_normal((1, hop * 88))).astype(np.float32)).to(dev)
    dn.set_bias(dn.estimate_bias(hum))
    step = hop * args.chunked
    pieces = [wav[:, at:at + step].contiguous() for at in range(0, wav.shape[1], step)]

    def session():
        s = dn.open_session()
        out = [s.push(p) for p in pieces]
        out.append(s.flush())
        return out

    whole = lambda: dn.forward_device(wav)
    got = session()
    if not torch.equal(torch.cat(got, dim=1), whole()):
        sys.exit("the chunked session differs from the whole-utterance forward")
    windows = sum(1 for p in got if p.shape[1])
    for fn in (whole, session):
        time_ms(fn, 2, dev)
    a, b_ = [], []
    for _ in range(args.rounds):
        a.append(time_ms(whole, args.iters, dev))
        b_.append(time_ms(session, args.iters, dev))
    halo = dn.open_session().halo
    rec = {"shape": f"1x{M}", "chunk_frames": args.chunked, "pushes": len(pieces), "windows": windows, "halo_samples": list(halo),
           "iters": args.iters, "rounds": args.rounds, **_summary("whole", a), **_summary("chunked_total", b_),
           "per_push_ms": float(np.median(b_) / windows), "ratio_total_over_whole": float(np.median(b_) / np.median(a)),
           "ratio_min_max": [float(min(b_) / max(a)), float(max(b_) / min(a))], "bit_identical": True}
    print(json.dumps(rec))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        out = {"tool": "tools/denoiser_bench.py --chunked", "gpu": torch.cuda.get_device_name(dev), "config": dn.get_config(), "results": [rec]}
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds of the host-inclusive comparison (numpy is slow)")
    ap.add_argument("--strength", type=float, default=0.1)
    ap.add_argument("--chunked", type=int, default=0, metavar="CHUNK_FRAMES",
                    help="time a DenoiserSession in pushes of CHUNK_FRAMES frames against the whole-utterance call (1 x 1000 frames)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.chunked < 0:
        ap.error("--chunked takes a positive frame count")
    if not torch.cuda.is_available():
        sys.exit("denoiser_bench needs a GPU")
    dev = torch.device("cuda", 0)
    if args.chunked:
        return chunked_main(args, dev)
    dn = Denoiser(strength=args.strength, device=dev)
    results = []
    for B, M in ((1, 1000), (32, 500)):
        rng = np.random.default_rng(B * M)
        L = dn.hop_length * M
        wav = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
        hum = torch.from_numpy((0.01 * rng.standard_normal((1, dn.hop_length * 88))).astype(np.float32)).to(dev)
        bias = dn.estimate_bias(hum)
        dn.set_bias(bias)
        ref = TorchDenoiser(dn, bias, dev)
        ours = lambda: dn.forward_device(wav)
        theirs = lambda: ref(wav, args.strength)
        interior = slice(dn.n_fft, L - dn.n_fft)             # torch.istft refuses nothing here, but its edges divide by a small wss
        diff = float((ours()[:, interior] - theirs()[:, interior]).abs().max())
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_ = [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))

        def wall_ms(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        bias_host = bias.cpu().numpy()
        device_route = lambda: dn.forward_device(wav).cpu().numpy()
        host_route = lambda: numpy_denoise(wav.cpu().numpy(), bias_host, args.strength, dn.n_fft, dn.hop_length)
        wd, wh = [], []
        for _ in range(args.host_rounds):
            wd.append(wall_ms(device_route))
            wh.append(wall_ms(host_route))
        rec = {"shape": f"{B}x{M}", "samples": B * L, "iters": args.iters, "rounds": args.rounds, "launches": dn.launch_count(B, L),
               **_summary("device", a), **_summary("torch", b_), "ratio_torch_over_device": float(np.median(b_) / np.median(a)),
               "host_rounds": args.host_rounds, **_summary("wall_device_stage", wd), **_summary("wall_copy_out_numpy", wh),
               "ratio_numpy_over_device_stage": float(np.median(wh) / np.median(wd)), "waveform_bytes": 4 * B * L,
               "max_abs_diff_vs_torch_interior": diff}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/denoiser_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": dn.get_config(), "results": results}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
