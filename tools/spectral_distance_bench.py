#!/usr/bin/env python3
"""Times the device spectral-distance stage (iris.metrics.SpectralDistance.forward_device: 11 launches at the default three
resolutions, no read-back) beside
(a) the same sums in torch ops on the same GPU -- torch.stft of both batches per resolution, abs, a mask over each item's own
    frames, the three float64 reductions, and the sample-domain sums -- with no read-back, and
(b) the host route it replaces: copy both batches out and take the sums in numpy per item
    (tests/spectral_distance_restatement.py, float64 FFT),
and records how far bf16, the split-product mode (``f32s``) and Griffin-Lim lie from the fp32 forward of the seeded V1 generator.

    python tools/spectral_distance_bench.py [--iters 10] [--rounds 5] [--out profiles/spectral_distance.json]

Two shapes of vocoder output at hop 256 (``row_scale = 256``): 1 x 1000 mel frames, and 8 utterances of 128 .. 1024.  Every item
is seeded noise plus three sinusoids (tests/spectral_distance_cases.py); the candidate is the reference turned down with other
noise on it.  Device events around ``iters`` back-to-back calls after a warm-up (a host clock for the host route, which ends on
the host); the three alternate in every round and the median round is reported with the spread.  Before timing, the three
routes' sums are compared.  torch.stft frames an item by the PADDED length, so its last frames see the neighbour's padding where
the device sees silence: the torch route is given batches whose padding is zero, where the two agree.
The dtype distances come from SEEDED weights: such a generator emits noise-like output, so the figures illustrate what the
stage reports and are not perceptual statements about a trained checkpoint.  Needs a GPU: there is no CPU fallback.
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
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tools"), str(REPO / "tests"), str(REPO)]

from iris.metrics import DEFAULT_RESOLUTIONS, SpectralDistance  # noqa: E402
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict  # noqa: E402
from vae_decoder_bench import time_ms  # noqa: E402
import spectral_distance_cases as C  # noqa: E402
import spectral_distance_restatement as R  # noqa: E402

HOP = 256


def batches(frames):
    """``(ref, test) [B, HOP * max(frames)]`` float32, zero behind every item's own samples."""
    L = HOP * max(frames)
    ref, test = np.zeros((len(frames), L), np.float32), np.zeros((len(frames), L), np.float32)
    for b, m in enumerate(frames):
        ref[b, :HOP * m], test[b, :HOP * m] = C.pair(100 + b, HOP * m)
    return ref, test


class TorchSums:
    """The stage's sums in torch ops; nothing comes back to the host."""

    def __init__(self, device):
        self.windows = []
        for n_fft, hop, win in DEFAULT_RESOLUTIONS:
            w = torch.zeros(n_fft, dtype=torch.float32, device=device)
            lpad = (n_fft - win) // 2
            w[lpad:lpad + win] = torch.hann_window(win, periodic=True, dtype=torch.float32, device=device)
            self.windows.append(w)

    def __call__(self, ref, test, lengths):
        own = lengths.to(torch.int64) * HOP
        spec = []
        for (n_fft, hop, _), w in zip(DEFAULT_RESOLUTIONS, self.windows):
            A = torch.stft(ref, n_fft, hop_length=hop, window=w, center=True, pad_mode="constant", return_complex=True).abs()
            Bm = torch.stft(test, n_fft, hop_length=hop, window=w, center=True, pad_mode="constant", return_complex=True).abs()
            Tb = torch.where(own > 0, 1 + own // hop, torch.zeros_like(own))
            mask = (torch.arange(A.shape[2], device=ref.device)[None, :] < Tb[:, None])[:, None, :]
            a, c = A.double(), Bm.double()
            l1 = (torch.log(a.clamp_min(R.FLOOR)) - torch.log(c.clamp_min(R.FLOOR))).abs()
            spec.append(torch.stack([((a - c).square() * mask).sum(dim=(1, 2)), (a.square() * mask).sum(dim=(1, 2)),
                                     (l1 * mask).sum(dim=(1, 2))], dim=1))
        keep = torch.arange(ref.shape[1], device=ref.device)[None, :] < own[:, None]
        d = (ref.double() - test.double()) * keep
        wave = torch.stack([d.square().sum(dim=1), (ref.double() * keep).square().sum(dim=1),
                            ((ref - test).abs() * keep).amax(dim=1).double()], dim=1)
        return torch.stack(spec, dim=1), wave


def host_route(ref, test, frames):
    """Copy-out and the float64 restatement per item: what a caller did before the stage existed."""
    x, y = ref.cpu().numpy(), test.cpu().numpy()
    return [R.sums(x[b, :HOP * m], y[b, :HOP * m], DEFAULT_RESOLUTIONS) for b, m in enumerate(frames)]


def host_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _summary(name: str, samples) -> dict:
    return {f"{name}_ms": float(np.median(samples)), f"{name}_ms_min_max": [float(min(samples)), float(max(samples))]}


def dtype_distances(sd: SpectralDistance, dev) -> dict:
    from iris._engine import GeneratorEngine
    from iris.griffin_lim import GriffinLim
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg), dev)
    T = 200
    mel = torch.from_numpy(seeded_mel(3, 2, T, log_mel=True)).to(dev)
    out = {"mel": f"seeded_mel(3, 2, {T}, log_mel=True)", "weights": "seeded_state_dict(GeneratorConfig())",
           "note": "seeded weights: illustrative figures, not perceptual ones"}
    keys = ("spectral_convergence", "log_stft_l1", "mr_spectral_convergence", "mr_log_stft_l1", "snr_db", "emax")
    for other in ("bf16", "f32s"):
        rec = sd.compare_dtypes(eng, mel, "f32", other)
        out[other] = {k: np.asarray(rec[k]).tolist() for k in keys}
    ya = eng.forward(mel, dtype="f32")
    gl = GriffinLim(n_iter=60).forward_device(mel)                   # [B, hop (T - 1)]
    rec = sd.measure(ya[:, :gl.shape[1]].contiguous(), gl)
    out["griffin_lim"] = {k: np.asarray(rec[k]).tolist() for k in keys}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectral_distance_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sd = SpectralDistance(device=dev)
    torch_sums = TorchSums(dev)
    results = []
    for name, frames in (("1 x 1000", [1000]), ("8 x 128..1024", [128 * (i + 1) for i in range(8)])):
        ref_h, test_h = batches(frames)
        ref, test = torch.from_numpy(ref_h).to(dev), torch.from_numpy(test_h).to(dev)
        lengths = torch.tensor(frames, dtype=torch.int32, device=dev)
        B, L = ref.shape
        ours = lambda: sd.forward_device(ref, test, lengths=lengths, row_scale=HOP)
        theirs = lambda: torch_sums(ref, test, lengths)
        host = lambda: host_route(ref, test, frames)
        spec, wave, _ = [t.cpu().numpy() for t in ours()]
        t_spec, t_wave = [t.cpu().numpy() for t in theirs()]
        h = host()
        h_spec, h_wave = np.stack([s["spec"] for s in h]), np.stack([s["wave"] for s in h])
        d_dev = float(max(np.abs(spec / h_spec - 1.0).max(), np.abs(wave / h_wave - 1.0).max()))
        d_torch = float(max(np.abs(t_spec / h_spec - 1.0).max(), np.abs(t_wave / h_wave - 1.0).max()))
        if d_dev > 1e-5 or d_torch > 1e-5:                           # two fp32 transforms against a float64 one
            sys.exit(f"{name}: the three routes disagree: device {d_dev:.3e}, torch {d_torch:.3e} off float64 numpy")
        for fn in (ours, theirs):
            time_ms(fn, 2, dev)
        a, b_, c_ = [], [], []
        for _ in range(args.rounds):
            a.append(time_ms(ours, args.iters, dev))
            b_.append(time_ms(theirs, args.iters, dev))
            c_.append(host_ms(host, max(1, args.iters // 5)))
        rec = {"shape": name, "B": B, "L": L, "samples_in": HOP * sum(frames), "iters": args.iters, "rounds": args.rounds,
               "launches": sd.launch_count(B, L), **_summary("forward_device", a), **_summary("torch_ops", b_),
               **_summary("host_numpy", c_), "ratio_torch_over_device": float(np.median(b_) / np.median(a)),
               "ratio_host_over_device": float(np.median(c_) / np.median(a)),
               "device_vs_float64_rel": d_dev, "torch_vs_float64_rel": d_torch, "routes_agree": True}
        print(json.dumps(rec))
        results.append(rec)
    out = {"tool": "tools/spectral_distance_bench.py", "gpu": torch.cuda.get_device_name(dev), "config": sd.get_config(),
           "results": results, "dtype_distances": dtype_distances(sd, dev)}
    print(json.dumps(out["dtype_distances"]))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
