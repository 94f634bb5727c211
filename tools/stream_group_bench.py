"""N concurrent streamed utterances: ``iris.stream_group.StreamGroup`` against N independent ``PipelineSession``s stepped in turn
(diagnostic).  V1 generator, fp32, 1000-frame utterances pushed 256 frames at a time, chain: limiter, then 8 kHz mu-law bytes.

  --mode group      every member pushes its piece, then ONE ``group.step()``: one ragged vocoder forward, one limiter group call
                    and one resampler group call for all N; steps go on until every member has drained.
  --mode sessions   the same pieces into N ``pipeline.session()``s one after the other, each ``flush``ed behind its last piece:
                    the path a caller had before the group (this mode uses nothing newer, so it also runs from an older checkout).

Per N and repetition, the whole run -- every push of every member up to the last byte -- is timed on the host clock (around a
final device synchronise) and with device events on the stream; reported are the median and min .. max over the repetitions of
the run, of the run per step (a step: one piece per member) and of the run per member-chunk (N x 4 vocoder chunks).

    python tools/stream_group_bench.py --mode group [--members 1 8 32 64] [--reps 5] [--warmup 1] [--out profiles/x.json]
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
from iris.limiter import Limiter  # noqa: E402
from iris.pipeline import MelToWavePipeline  # noqa: E402
from iris.resample import Resampler  # noqa: E402


def spread(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4), "n": int(a.size)}


def run_group(pipe, mels, piece, chunk):
    from iris.stream_group import StreamGroup
    group = StreamGroup(pipe, chunk_frames=chunk)
    members = [group.open() for _ in mels]
    at, steps, n_bytes = 0, 0, 0
    while group.members:
        for m, mel in zip(members, mels):
            if not m._ended:
                m.push(mel[:, :, at:at + piece])
                if at + piece >= mel.shape[2]:
                    m.end()
        at += piece
        n_bytes += sum(int(p.shape[1]) for p in group.step().values())
        steps += 1
    return steps, n_bytes


def run_sessions(pipe, mels, piece, chunk):
    sessions = [pipe.session() for _ in mels]
    T, steps, n_bytes = mels[0].shape[2], 0, 0
    for at in range(0, T, piece):
        for ses, mel in zip(sessions, mels):
            out = ses.push(mel[:, :, at:at + piece])
            if at + piece >= T:
                out = out + ses.flush()
            n_bytes += sum(int(p.shape[1]) for p in out)
        steps += 1
    return steps, n_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("group", "sessions"), required=True)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--piece", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no HIP device: this measurement has no CPU path")
    dev = torch.device("cuda", 0)
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=3), dev, dtype="f32")
    lim = Limiter(22050, ceiling_dbtp=-1.0, lookahead_ms=1.5, device=dev)
    res = Resampler(8000, device=dev)
    pipe = MelToWavePipeline(None, eng.forward, device=dev, chunk_frames=args.piece, config=cfg, limiter=lim.chunked(),
                             output=res.chunked("ulaw"))
    run = run_group if args.mode == "group" else run_sessions
    result = {"mode": args.mode, "shape": {"frames": args.frames, "piece_frames": args.piece, "chain": "limiter, 8 kHz mu-law"},
              "device": torch.cuda.get_device_name(dev), "warmup": args.warmup, "members": {}}
    chunks_each = -(-args.frames // args.piece)
    for N in args.members:
        mels = [torch.from_numpy(seeded_mel(100 + i, 1, args.frames, log_mel=True)).to(dev) for i in range(N)]
        wall, device, steps, n_bytes = [], [], 0, 0
        for rep in range(args.warmup + args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            steps, n_bytes = run(pipe, mels, args.piece, args.piece)
            stop.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
                device.append(start.elapsed_time(stop))
        assert n_bytes == N * res.out_range(0, cfg.hop_length * args.frames)[1], "the run did not drain every utterance"
        per = lambda ms, d: spread([m / d for m in ms])                      # noqa: E731
        r = result["members"][str(N)] = {
            "steps": steps, "member_chunks": N * chunks_each,
            "run_wall": spread(wall), "run_device": spread(device),
            "per_step_wall": per(wall, steps), "per_step_device": per(device, steps),
            "per_member_chunk_wall": per(wall, N * chunks_each), "per_member_chunk_device": per(device, N * chunks_each)}
        print(f"{args.mode} N = {N}: {steps} steps; per step wall {r['per_step_wall']['median_ms']:.3f} ms, device "
              f"{r['per_step_device']['median_ms']:.3f} ms; per member-chunk wall {r['per_member_chunk_wall']['median_ms']:.3f} ms "
              f"[{r['per_member_chunk_wall']['min_ms']:.3f} .. {r['per_member_chunk_wall']['max_ms']:.3f}], device "
              f"{r['per_member_chunk_device']['median_ms']:.3f} ms", flush=True)
    print(json.dumps(result))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
