"""Cost of the device sample-rate conversion stage (iris.resample, csrc/resample.h) behind the vocoder.

For each configuration (fp32 at 1 x 1000 frames, bf16 at 32 x 500 frames) and each output rate (16 000 and 48 000 Hz):
  device   hipEvents around N back-to-back calls on the forward's own waveform: the resampler in its three output forms
           (fp32; int16; fp32 + peaks + pcm_normalize_kernel), and -- the yardstick, the parent's streaming pass of the same
           shape -- the output stage's conversion of that waveform (iris_hifigan_op_pcm16: ONE pcm_normalize_kernel launch,
           but the entry point synchronises the stream, so its figure carries one host round trip per call and is an upper
           bound; the per-kernel figures come from running this tool under a kernel trace)
  host-inclusive, numpy mel -> numpy int16 at the new rate, synchronous, pinned buffers:
           device leg   H2D mel -> engine.forward_resampled(pcm16=True) -> D2H int16
           host leg     H2D mel -> engine.forward -> D2H fp32 -> polyphase resampling on the host -> pcm16_from_float
           (scipy.signal.resample_poly when scipy is importable; otherwise the same designed bank applied per item with
           numpy in float32 -- `host_resampler` says which; neither is the bit-exact resample_host, which is far slower).
Each figure is the median of R rounds of N calls.  Prints one JSON object.

usage: python tools/resample_bench.py [--out FILE] [--rounds R]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "iris-tts_amd"))
sys.path.insert(0, str(REPO / "tools"))
from iris import _native  # noqa: E402
from iris._engine import GeneratorEngine  # noqa: E402
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict  # noqa: E402
from iris.resample import Resampler, design_bank, out_range  # noqa: E402
from iris.synthesis_output import pcm16_from_float  # noqa: E402
from pcm_out_bench import device_ms, wall_ms  # noqa: E402

CONFIGS = [("f32", 1, 1000, 10), ("bf16", 32, 500, 5)]       # dtype, batch, frames, calls per round
RATES = (16000, 48000)

try:
    from scipy.signal import resample_poly
    HOST_RESAMPLER = "scipy.signal.resample_poly"
except ImportError:
    resample_poly = None
    HOST_RESAMPLER = "numpy float32 polyphase with the designed bank (scipy is not importable)"


def host_resample(wav, rate_out, bank, up, down):
    if resample_poly is not None:
        return resample_poly(wav, up, down, axis=1).astype(np.float32)
    taps = bank.shape[1]
    hw = taps // 2
    L = wav.shape[1]
    n = out_range(up, down, 0, L)[1]
    q = np.arange(n, dtype=np.int64) * down
    idx = (q // up - hw + 1)[:, None] + np.arange(taps)[None, :]
    rows = bank[q % up]
    rows = np.where((idx >= 0) & (idx < L), rows, np.float32(0.0))
    idx = np.clip(idx, 0, L - 1)
    return np.stack([np.einsum("nt,nt->n", w[idx], rows) for w in wav])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _native.load()
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0), dev)
    hop = eng.hop_length
    result = {"tool": "tools/resample_bench.py", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
              "host_resampler": HOST_RESAMPLER, "configs": []}
    for dtype, B, T, calls in CONFIGS:
        eng.prepare(dtype)
        mel_np = seeded_mel(1003, B, T, log_mel=True)
        mel_pin = torch.from_numpy(mel_np).pin_memory()
        mel_dev = torch.empty((B, cfg.in_channels, T), dtype=torch.float32, device=dev)
        mel_dev.copy_(mel_pin)
        L = hop * T
        wav_dev = eng.forward(mel_dev, dtype=dtype).clone()
        wav_pin = torch.empty((B, L), dtype=torch.float32).pin_memory()
        pcm_in = torch.empty((B, L), dtype=torch.int16, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def upload():
            mel_pin.numpy()[...] = mel_np
            mel_dev.copy_(mel_pin, non_blocking=True)

        def yardstick():
            _native.check("iris_hifigan_op_pcm16", lib.iris_hifigan_op_pcm16(
                ctypes.c_void_p(wav_dev.data_ptr()), None, 1, ctypes.c_void_p(pcm_in.data_ptr()), None, B, L, 0,
                ctypes.c_float(0.95), ctypes.c_void_p(stream)))

        for rate in RATES:
            rs = Resampler(rate, device=dev)
            bank, up, down = design_bank(rate)
            n = rs.out_range(0, L)[1]
            pcm_pin = torch.empty((B, n), dtype=torch.int16).pin_memory()

            def device_leg():
                upload()
                pcm_pin.copy_(eng.forward_resampled(mel_dev, rs, dtype=dtype, pcm16=True), non_blocking=True)
                torch.cuda.synchronize()
                return pcm_pin.numpy()

            def host_leg():
                upload()
                eng.forward(mel_dev, dtype=dtype, out=wav_dev)
                wav_pin.copy_(wav_dev, non_blocking=True)
                torch.cuda.synchronize()
                return pcm16_from_float(host_resample(wav_pin.numpy(), rate, bank, up, down))

            diff = np.abs(device_leg().astype(np.int32) - host_leg().astype(np.int32))
            dm = {"resample_fp32": device_ms(lambda: rs.forward(wav_dev), calls, args.rounds),
                  "resample_pcm16": device_ms(lambda: rs.forward(wav_dev, pcm16=True), calls, args.rounds),
                  "resample_normalised_three_queue_items": device_ms(lambda: rs.forward(wav_dev, pcm16=True, normalize=True),
                                                                     calls, args.rounds),
                  "pcm_normalize_same_waveform_synchronous_entry_point": device_ms(yardstick, calls, args.rounds)}
            hi = {"device_resampling": wall_ms(device_leg, calls, args.rounds),
                  "host_resampling": wall_ms(host_leg, max(1, calls // 5), args.rounds)}
            rec = {"dtype": dtype, "batch": B, "frames": T, "samples_in": B * L, "rate_out": rate, "samples_out": B * n,
                   "up": up, "down": down, "taps": rs.taps, "calls": calls,
                   "legs_max_abs_diff_lsb": int(diff.max()), "legs_mean_abs_diff_lsb": float(diff.mean()),
                   "device": dm, "host_inclusive": hi,
                   "ratio_resample_fp32_over_pcm_normalize": dm["resample_fp32"]["median_ms"]
                   / dm["pcm_normalize_same_waveform_synchronous_entry_point"]["median_ms"],
                   "taps_over_4": rs.taps / 4,
                   "speedup_host_inclusive": hi["host_resampling"]["median_ms"] / hi["device_resampling"]["median_ms"]}
            result["configs"].append(rec)
            rs.close()
    eng.close()
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
