"""Ragged batch vs padded batch vs one forward per utterance, fp32 (iris_hifigan_forward_ragged).

For 32 utterances with lengths from a fixed seed (uniform in [100, 1000], and again in [50, 200]) times
  per_item  one GeneratorEngine.forward per utterance, back to back on one stream;
  padded    one forward of the batch padded to T_max (its short items are wrong near their ends: tests/test_ragged_batch.py);
  ragged    one forward of the same padded batch with lengths=.
Each is the median of R rounds of N back-to-back calls (wall clock around a synchronised stream, no profiling events).
samples/s counts VALID samples only (hop * sum of lengths), for all three.  Prints one JSON object.

usage: python tools/ragged_batch_bench.py [--out FILE] [--rounds R] [--seed S]
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

SAMPLE_RATE = 22050


def timed(fn, n, rounds):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return statistics.median(ts), min(ts)


def case(eng, lengths, rounds):
    B, T = len(lengths), int(max(lengths))
    dev = eng.device
    mel = torch.from_numpy(seeded_mel(7, B, T, log_mel=True)).to(dev)
    items = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths)]
    out = torch.empty((B, eng.hop_length * T), dtype=torch.float32, device=dev)
    lens = torch.tensor(lengths, dtype=torch.int32)
    valid = eng.hop_length * int(sum(lengths))
    n = max(3, min(50, int(200000 / (B * T))))
    runs = {
        "per_item": lambda: [eng.forward(x, dtype="f32") for x in items],
        "padded": lambda: eng.forward(mel, out=out, dtype="f32"),
        "ragged": lambda: eng.forward(mel, out=out, dtype="f32", lengths=lens),
    }
    rec = {"B": B, "T_max": T, "sum_lengths": int(sum(lengths)), "fill": sum(lengths) / (B * T),
           "lengths": [int(v) for v in lengths], "calls_per_round": n, "rounds": rounds}
    for name, fn in runs.items():
        med, best = timed(fn, n, rounds)
        rec[name] = {"ms": med, "ms_min": best, "valid_samples_per_s": valid / (med * 1e-3),
                     "rtf": (med * 1e-3) / (valid / SAMPLE_RATE)}
    rec["ragged_vs_padded"] = rec["ragged"]["ms"] / rec["padded"]["ms"]
    rec["ragged_vs_per_item"] = rec["ragged"]["ms"] / rec["per_item"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=2026)
    args = ap.parse_args()
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg), torch.device("cuda", 0))
    rng = np.random.default_rng(args.seed)
    res = {"tool": "tools/ragged_batch_bench.py", "dtype": "f32", "seed": args.seed,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for lo, hi in ((100, 1000), (50, 200)):
        lengths = [int(v) for v in rng.integers(lo, hi + 1, size=32)]
        rec = case(eng, lengths, args.rounds)
        rec["range"] = [lo, hi]
        res["cases"].append(rec)
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
