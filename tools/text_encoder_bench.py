#!/usr/bin/env python3
"""Times the device text stage (iris.encoder: phoneme encoder + duration head + length regulator) against the same graph
written in eager torch ops (same weights) on the same GPU.

    python tools/text_encoder_bench.py [--shapes 1x100 1x400 8x200] [--iters 100] [--rounds 5] [--out profiles/text_encoder_bench.json]

Device events around `iters` back-to-back runs, after a warm-up of every shape; the two implementations alternate in every
round and the median round is reported with the spread.  Two figures per implementation: the launches alone (encoder, head,
scan and a gather to a T_pad known beforehand) and the whole stage as `frame_conditioning` runs it, i.e. with the read-back
of the frame totals that sizes the output -- the difference is what that one synchronising copy costs.  Batches are ragged
(lengths from P / 2 to P).  Outputs are compared at the timed shape before timing.  Needs a GPU: there is no CPU fallback
and no number without one.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tests")]

from iris import encoder as E  # noqa: E402
from encoder_restatement import randomise  # noqa: E402


class TorchGraph:
    """The stage in eager torch ops; a ragged batch through a key mask and masked conv inputs."""

    def __init__(self, enc, head, dev):
        self.enc, self.head = enc, head
        self.w = {k: torch.from_numpy(a).to(dev) for k, a in {**enc.weights, **head.weights}.items()}

    def norm(self, x, p):
        return F.layer_norm(x, x.shape[-1:], self.w[f"{p}.gamma"], self.w[f"{p}.beta"], 1e-6)

    def encode(self, ids, mask):
        w, enc = self.w, self.enc
        B, P = ids.shape
        H, Dk = enc.num_heads, enc.embed_dim // enc.num_heads
        x = w["phoneme_embedding.embeddings"][ids.long()] + w["positional_embedding.position_embedding.embeddings"][:P]
        bias = torch.zeros(B, 1, 1, P, device=ids.device).masked_fill(~mask[:, None, None, :], float("-inf"))
        for i in range(enc.num_blocks):
            p = f"transformer_block_{i}"
            q, k, v = (torch.einsum("bpe,ehd->bhpd", x, w[f"{p}.attention.{n}.kernel"]) + w[f"{p}.attention.{n}.bias"][None, :, None, :]
                       for n in ("query", "key", "value"))
            a = torch.softmax((q * Dk ** -0.5) @ k.transpose(2, 3) + bias, dim=-1) @ v
            x = self.norm(x + torch.einsum("bhpd,hde->bpe", a, w[f"{p}.attention.output.kernel"]) + w[f"{p}.attention.output.bias"],
                          f"{p}.attention_norm")
            h = torch.relu(x @ w[f"{p}.ffn.0.kernel"] + w[f"{p}.ffn.0.bias"])
            x = self.norm(x + h @ w[f"{p}.ffn.2.kernel"] + w[f"{p}.ffn.2.bias"], f"{p}.ffn_norm")
        return self.norm(x, "encoder_output_norm") * mask[..., None]

    def durations(self, enc_out, mask):
        w, x = self.w, enc_out
        for i in range(self.head.num_layers):
            k = w[f"duration_conv_{i}.kernel"].permute(2, 1, 0)
            x = torch.relu(F.conv1d((x * mask[..., None]).transpose(1, 2), k, w[f"duration_conv_{i}.bias"], padding=k.shape[2] // 2))
            x = self.norm(x.transpose(1, 2), f"duration_norm_{i}")
        pred = F.softplus(x @ w["duration_output.kernel"][0] + w["duration_output.bias"])[..., 0]
        frames = torch.clamp(torch.round(torch.exp(pred) - 1.0), 1.0, 1e6).to(torch.int32) * mask
        return pred * mask, frames

    def regulate(self, enc_out, frames, T_pad):
        B, P, Ed = enc_out.shape
        ends = torch.cumsum(frames, dim=1)
        t = torch.arange(T_pad, device=enc_out.device)
        idx = torch.searchsorted(ends, t[None, :].expand(B, -1).contiguous(), right=True).clamp(max=P - 1)
        cond = torch.gather(enc_out, 1, idx[..., None].expand(-1, -1, Ed))
        return cond * (t[None, :] < ends[:, -1:])[..., None]


def time_ms(fn, iters, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x100", "1x400", "8x200"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "text_encoder_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    enc, head = E.PhonemeEncoder(vocab_size=80, seed=1), E.DurationPredictor(seed=2)
    randomise(enc, 303)
    randomise(head, 304)
    graph = TorchGraph(enc, head, dev)
    results = []
    for shape in args.shapes:
        B, P = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(B * 1000 + P)
        ids = torch.from_numpy(rng.integers(0, 80, (B, P)).astype(np.int32)).to(dev)
        lengths = np.linspace(P // 2, P, B).astype(np.int32) if B > 1 else np.array([P], np.int32)
        mask = torch.from_numpy(E.create_padding_mask(lengths, P)).to(dev)
        with torch.no_grad():
            cond, per_item = E.frame_conditioning(enc, head, ids, lengths=lengths)
            T_pad = int(cond.shape[1])

            def ours_launches():
                enc_out = enc.forward_device(ids, lengths)
                _, _, offsets, totals = head.forward_device(enc_out, lengths)
                return E.regulate_device(enc_out, offsets, totals, T_pad)

            def ours_stage():
                return E.frame_conditioning(enc, head, ids, lengths=lengths)[0]

            def theirs_launches():
                enc_out = graph.encode(ids, mask)
                return graph.regulate(enc_out, graph.durations(enc_out, mask)[1], T_pad)

            def theirs_stage():
                enc_out = graph.encode(ids, mask)
                frames = graph.durations(enc_out, mask)[1]
                total = int(frames.sum(dim=1).max())                       # the same read-back
                return graph.regulate(enc_out, frames, -(-total // 4) * 4)

            theirs = theirs_stage()
            same_shape = tuple(theirs.shape) == tuple(cond.shape)
            diff = float((cond - theirs).abs().max()) / max(1.0, float(theirs.abs().max())) if same_shape else None
            fns = (ours_launches, ours_stage, theirs_launches, theirs_stage)
            for _ in range(10):
                for fn in fns:
                    fn()
            rounds = [[time_ms(fn, args.iters, dev) for fn in fns] for _ in range(args.rounds)]
        r = np.array(rounds)
        med = np.median(r, axis=0)
        rec = {"shape": shape, "lengths": lengths.tolist(), "frames_per_item": per_item, "T_pad": T_pad,
               "device_launches_ms": float(med[0]), "device_stage_ms": float(med[1]), "device_readback_ms": float(med[1] - med[0]),
               "torch_ops_launches_ms": float(med[2]), "torch_ops_stage_ms": float(med[3]),
               "min_max_ms": {n: [float(r[:, i].min()), float(r[:, i].max())] for i, n in enumerate(
                   ("device_launches", "device_stage", "torch_ops_launches", "torch_ops_stage"))},
               "ratio_torch_over_device_stage": float(med[3] / med[1]),
               "launches": enc.launch_count(B, P) + head.launch_count(B, P) + 1,
               "same_frame_count_as_torch_ops": same_shape, "max_rel_diff_vs_torch_ops": diff, "iters": args.iters, "rounds": args.rounds,
               "timing": "device events around `iters` back-to-back runs (launch gaps and host work included), median of rounds"}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"gpu": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
