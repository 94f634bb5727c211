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

--chunked FRAMES measures the streamed form instead (no vocoder is built): a random waveform of 1 x 1000 frames of 256 samples to
--rate (8000 Hz) in --encoding (f32, pcm16, ulaw, alaw):
  whole_call      Resampler.forward of the whole waveform, device and wall time per call
  window          ONE Resampler.forward_window on the window a ResamplerSession holds after a push of FRAMES frames (the piece and
                  the samples kept from the window before), device and wall time per call: the cost a chunk pays
  session_pass    the whole waveform pushed through a ResamplerSession FRAMES frames at a time and flushed, wall time per pass and
                  per window (torch.cat of the held samples and the plan's two host calls included)

usage: python tools/resample_bench.py [--out FILE] [--rounds R] [--chunked FRAMES [--encoding E] [--rate HZ]]
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


def chunked(args, dev):
    hop, frames = 256, 1000
    L, step, enc = hop * frames, hop * args.chunked, args.encoding
    rs = Resampler(args.rate, device=dev)
    wav = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 1.0, (1, L)).astype(np.float32)).to(dev)
    n_next, origin = rs.window_plan(0, step, 0, False)          # what the first push emits and keeps
    window = wav[:, origin:2 * step].contiguous()
    n_hi = rs.window_plan(origin, window.shape[1], n_next, False)[0]

    def whole():
        return rs.forward(wav, encoding=enc)

    def one_window():
        return rs.forward_window(window, origin, n_next, False, encoding=enc)

    def session_pass():
        session = rs.open_session(enc)
        out = [session.push(wav[:, at:at + step]) for at in range(0, L, step)]
        return out + [session.flush()]

    assert torch.equal(torch.cat(session_pass(), dim=1), whole())
    windows = -(-L // step) + 1
    passes = wall_ms(session_pass, 3, args.rounds)
    result = {"tool": "tools/resample_bench.py --chunked", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
              "rate_out": args.rate, "encoding": enc, "samples_in": L, "samples_out": rs.out_range(0, L)[1], "chunk_frames": args.chunked,
              "window_samples_in": int(window.shape[1]), "window_samples_out": n_hi - n_next, "windows_per_pass": windows,
              "whole_call": {"device": device_ms(whole, 20, args.rounds), "wall": wall_ms(whole, 20, args.rounds)},
              "window": {"device": device_ms(one_window, 50, args.rounds), "wall": wall_ms(one_window, 50, args.rounds)},
              "session_pass": {"wall": passes, "wall_per_window_median_ms": passes["median_ms"] / windows}}
    rs.close()
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunked", type=int, default=None, metavar="FRAMES", help="measure the streamed form at FRAMES frames per push")
    ap.add_argument("--encoding", type=str, default="f32", choices=["f32", "pcm16", "ulaw", "alaw"], help="with --chunked")
    ap.add_argument("--rate", type=int, default=8000, help="with --chunked: the output rate")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.chunked is not None:
        if args.chunked < 1:
            ap.error("--chunked takes a positive number of frames")
        result = chunked(args, dev)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result))
        return 0
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
