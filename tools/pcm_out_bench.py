"""Host-inclusive time of 16-bit PCM output: converted on the device (forward_pcm16) against converted on the host.

For each configuration (fp32 at 1 x 1000 frames, bf16 at 32 x 500 frames), numpy mel in -> numpy int16 out, synchronous,
through pinned host buffers on both legs:
  host    H2D mel -> engine.forward -> D2H fp32 waveform -> synthesis_output.pcm16_from_float on the host   (today's path)
  device  H2D mel -> engine.forward_pcm16 -> D2H int16                                                      (the new path)
and the same pair with peak normalisation (host: pcm16_from_float(normalize=True); device: forward_pcm16(normalize=True)).
The parts of the host leg are timed apart as well (D2H copy, host conversion), and the device time of the forward alone
with and without the PCM epilogue (hipEvents around N back-to-back calls).  Each figure is the median of R rounds of N calls.
The two legs are checked to produce the same bytes before anything is timed.  Prints one JSON object.

usage: python tools/pcm_out_bench.py [--out FILE] [--rounds R]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "iris-tts_amd"))
from iris._engine import GeneratorEngine  # noqa: E402
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict  # noqa: E402
from iris.synthesis_output import pcm16_from_float  # noqa: E402

CONFIGS = [("f32", 1, 1000, 10), ("bf16", 32, 500, 5)]       # dtype, batch, frames, calls per round


def wall_ms(fn, n, rounds):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def device_ms(fn, n, rounds):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / n)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0), dev)
    hop = eng.hop_length
    result = {"tool": "tools/pcm_out_bench.py", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
              "note": "host-inclusive: numpy mel -> numpy int16, synchronous, pinned host buffers on both legs; "
                      "median of `rounds` rounds of `calls` back-to-back calls", "configs": []}
    for dtype, B, T, calls in CONFIGS:
        eng.prepare(dtype)
        mel_np = seeded_mel(1003, B, T, log_mel=True)
        mel_pin = torch.from_numpy(mel_np).pin_memory()
        mel_dev = torch.empty((B, cfg.in_channels, T), dtype=torch.float32, device=dev)
        wav_dev = torch.empty((B, hop * T), dtype=torch.float32, device=dev)
        pcm_dev = torch.empty((B, hop * T), dtype=torch.int16, device=dev)
        wav_pin = torch.empty((B, hop * T), dtype=torch.float32).pin_memory()
        pcm_pin = torch.empty((B, hop * T), dtype=torch.int16).pin_memory()

        def upload():
            mel_pin.numpy()[...] = mel_np                                   # the caller's numpy mel into the pinned buffer
            mel_dev.copy_(mel_pin, non_blocking=True)

        def host_leg(normalize=False):
            upload()
            eng.forward(mel_dev, out=wav_dev, dtype=dtype)
            wav_pin.copy_(wav_dev, non_blocking=True)
            torch.cuda.synchronize()
            return pcm16_from_float(wav_pin.numpy(), normalize=normalize)

        def device_leg(normalize=False):
            upload()
            eng.forward_pcm16(mel_dev, out=pcm_dev, dtype=dtype, normalize=normalize, wav=wav_dev if normalize else None)
            pcm_pin.copy_(pcm_dev, non_blocking=True)
            torch.cuda.synchronize()
            return pcm_pin.numpy().copy()

        same = bool(np.array_equal(host_leg(), device_leg()))
        same_n = bool(np.array_equal(host_leg(True), device_leg(True)))

        def d2h_f32():
            wav_pin.copy_(wav_dev, non_blocking=True)
            torch.cuda.synchronize()

        def d2h_i16():
            pcm_pin.copy_(pcm_dev, non_blocking=True)
            torch.cuda.synchronize()

        rec = {"dtype": dtype, "batch": B, "frames": T, "samples": B * T * hop, "calls": calls,
               "legs_give_identical_bytes": same, "legs_give_identical_bytes_normalised": same_n,
               "host_inclusive": {
                   "host_conversion": wall_ms(host_leg, calls, args.rounds),
                   "device_conversion": wall_ms(device_leg, calls, args.rounds),
                   "host_conversion_normalised": wall_ms(lambda: host_leg(True), calls, args.rounds),
                   "device_conversion_normalised": wall_ms(lambda: device_leg(True), calls, args.rounds)},
               "parts": {
                   "d2h_fp32": wall_ms(d2h_f32, calls, args.rounds),
                   "d2h_int16": wall_ms(d2h_i16, calls, args.rounds),
                   "pcm16_from_float_on_host": wall_ms(lambda: pcm16_from_float(wav_pin.numpy()), calls, args.rounds),
                   "pcm16_from_float_normalised_on_host": wall_ms(lambda: pcm16_from_float(wav_pin.numpy(), normalize=True),
                                                                  calls, args.rounds)},
               "device_forward": {
                   "fp32_waveform": device_ms(lambda: eng.forward(mel_dev, out=wav_dev, dtype=dtype), calls, args.rounds),
                   "pcm16": device_ms(lambda: eng.forward_pcm16(mel_dev, out=pcm_dev, dtype=dtype), calls, args.rounds),
                   "pcm16_normalised": device_ms(lambda: eng.forward_pcm16(mel_dev, out=pcm_dev, dtype=dtype, normalize=True,
                                                                          wav=wav_dev), calls, args.rounds)}}
        hi = rec["host_inclusive"]
        rec["speedup_host_inclusive"] = hi["host_conversion"]["median_ms"] / hi["device_conversion"]["median_ms"]
        rec["speedup_host_inclusive_normalised"] = (hi["host_conversion_normalised"]["median_ms"]
                                                    / hi["device_conversion_normalised"]["median_ms"])
        result["configs"].append(rec)
    eng.close()
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
