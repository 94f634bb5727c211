"""First-audio latency of the PostNet -> vocoder pipeline with a live mel producer (diagnostic; configs[4] shape:
B = 1, 1024 frames, 256-frame chunks, 3 x 256 x k5 PostNet, fp32 and bf16 vocoder).

Two figures per vocoder dtype, taken alternately in one process (host clock around work that ends in a device synchronise):
  push    a ``MelToWavePipeline.session()`` holds the first 256 + hv + hp - 1 raw frames; timed is the push of the ONE frame that
          completes the first chunk's context, up to that chunk's audio being ready on the stream (one PostNet pass over
          the window + one vocoder forward of chunk + halo frames).  The producer is still 749 frames from the end.
  stream  ``MelToWavePipeline.stream`` on the COMPLETE mel up to its first chunk being ready: what a caller can do without
          pushed input, and it includes the PostNet pass over the whole utterance -- and can only start after the last frame.
Also the time of the whole utterance through a session (four pushes of 256 frames + flush), for the cost of the windows.

    python tools/pipeline_push_latency.py [--frames 1024] [--reps 50] [--warmup 5] [--out profiles/x.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "iris-tts_amd"), str(ROOT)]
from iris._engine import GeneratorEngine  # noqa: E402
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict  # noqa: E402
from iris.pipeline import MelToWavePipeline  # noqa: E402
from iris.postnet import PostNet  # noqa: E402

SAMPLE_RATE = 22050


def spread(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4),
            "max_ms": round(float(a[-1]), 4), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no HIP device: this measurement has no CPU path")
    dev = torch.device("cuda", 0)
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=3), dev)
    post = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    T, chunk = args.frames, args.chunk
    mel = torch.from_numpy(seeded_mel(9, 1, T, log_mel=True)).to(dev)
    result = {"shape": {"batch": 1, "frames": T, "chunk_frames": chunk, "postnet": "3x256xk5"},
              "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "dtypes": {}}
    for dtype in ("f32", "bf16"):
        eng.prepare(dtype)
        pipe = MelToWavePipeline(post, lambda m, d=dtype: eng.forward(m, dtype=d), device=dev, chunk_frames=chunk, config=cfg)
        probe = pipe.session()
        hv, hp = probe.halo_frames, probe.postnet_halo_frames
        need = chunk + hv + hp                      # frames_received that releases the first chunk
        if T < need:
            sys.exit(f"--frames must be at least {need}")
        push_ms, stream_ms, session_all_ms, stream_all_ms = [], [], [], []
        for rep in range(args.warmup + args.reps):
            # push: everything but the last frame of the first chunk's context is already in the session
            ses = pipe.session()
            assert ses.push(mel[:, :, :need - 1]) == []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (first,) = ses.push(mel[:, :, need - 1:need])
            torch.cuda.synchronize()
            t_push = time.perf_counter() - t0
            # stream: the complete mel, up to the first chunk
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it = pipe.stream(mel)
            first_s = next(it)
            torch.cuda.synchronize()
            t_stream = time.perf_counter() - t0
            for _ in it:
                pass
            torch.cuda.synchronize()
            t_stream_all = time.perf_counter() - t0
            # the whole utterance through a session, a chunk's worth of frames per push
            ses = pipe.session()
            t0 = time.perf_counter()
            n = 0
            for s in range(0, T, chunk):
                n += len(ses.push(mel[:, :, s:s + chunk]))
            n += len(ses.flush())
            torch.cuda.synchronize()
            t_all = time.perf_counter() - t0
            if rep == 0:
                assert torch.equal(first, first_s), "pushed and streamed first chunk differ"
                assert n == -(-T // chunk)
            if rep >= args.warmup:
                push_ms.append(1e3 * t_push)
                stream_ms.append(1e3 * t_stream)
                session_all_ms.append(1e3 * t_all)
                stream_all_ms.append(1e3 * t_stream_all)
        result["dtypes"][dtype] = {
            "vocoder_halo_frames": hv, "postnet_halo_frames": hp,
            "audio_latency_frames": hv + hp, "audio_latency_s": round((hv + hp) * cfg.hop_length / SAMPLE_RATE, 4),
            "push_to_first_chunk": spread(push_ms),
            "stream_complete_mel_to_first_chunk": spread(stream_ms),
            "session_whole_utterance": spread(session_all_ms),
            "stream_whole_utterance": spread(stream_all_ms),
        }
        r = result["dtypes"][dtype]
        print(f"{dtype}: push -> first chunk {r['push_to_first_chunk']['median_ms']:.3f} ms "
              f"[{r['push_to_first_chunk']['p10_ms']:.3f}, {r['push_to_first_chunk']['p90_ms']:.3f}]; "
              f"stream(complete mel) -> first chunk {r['stream_complete_mel_to_first_chunk']['median_ms']:.3f} ms "
              f"[{r['stream_complete_mel_to_first_chunk']['p10_ms']:.3f}, {r['stream_complete_mel_to_first_chunk']['p90_ms']:.3f}]; "
              f"whole utterance: session {r['session_whole_utterance']['median_ms']:.3f} ms, "
              f"stream {r['stream_whole_utterance']['median_ms']:.3f} ms", flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
