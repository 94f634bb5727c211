#!/usr/bin/env python3
"""Times the device VAE decoder (iris.vae.TextConditionedVAE.generate_device) against the same graph written in torch
ops (F.conv1d / F.linear, same weights) on the same GPU.

    python tools/vae_decoder_bench.py [--shapes 1x1024 8x1024] [--iters 200] [--rounds 5] [--out profiles/vae_decoder_bench.json]
    python tools/vae_decoder_bench.py --ragged [--iters 200] [--rounds 5] [--out profiles/vae_ragged_bench.json]

Device events around `iters` back-to-back forwards, after a warm-up of every shape; the two implementations alternate in
every round and the median round is reported with the spread.  Both produce mel and residual; outputs are compared at the
timed shape before timing.  Needs a GPU: there is no CPU fallback and no number without one.

--ragged times a batch of 8 utterances of 128, 256, ..., 1024 frames three ways, alternating in every round: ONE ragged call
(generate_device(..., lengths=)), eight batch-of-one calls at the items' own lengths (what a host loop over the items
costs), and the dense 8 x 1024 call (what the ragged call's launches cost when every block has work).  Before timing,
every item of the ragged call is compared with its batch-of-one call bit for bit.
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

from iris.vae import TextConditionedVAE  # noqa: E402
from vae_restatement import randomise  # noqa: E402


class TorchGraph:
    """generate() in eager torch ops, channels-first [B, C, T] as F.conv1d wants it."""

    def __init__(self, vae: TextConditionedVAE, dev):
        self.v = vae
        self.w = {}
        for k, a in vae.weights.items():
            t = torch.from_numpy(a).to(dev)
            if k.endswith(".kernel"):
                t = t.permute(2, 1, 0).contiguous() if t.dim() == 3 else t.t().contiguous()   # conv [out, in, k]; linear [out, in]
            self.w[k] = t

    def conv(self, x, p, stride=1, dil=1, pad=None):
        w = self.w[f"{p}.kernel"]
        k = w.shape[2]
        if pad is None:
            pad = (dil * (k - 1) // 2,) * 2
        return F.conv1d(F.pad(x, pad) if any(pad) else x, w, self.w[f"{p}.bias"], stride=stride, dilation=dil)

    def lin(self, x, p):                                  # x [B, C, T] -> Dense over channels
        return F.linear(x.transpose(1, 2), self.w[f"{p}.kernel"], self.w[f"{p}.bias"]).transpose(1, 2)

    def __call__(self, cond, z):
        v = self.v
        gelu = lambda t: F.gelu(t, approximate="tanh")
        h = self.conv(cond.transpose(1, 2), "down_cond_proj")
        for s in range(v.down_stages):
            h = gelu(self.conv(h, f"downsample.blocks.{s}", stride=2, pad=(1, 2)))
        lat = h
        z = z.transpose(1, 2)
        half = v.latent_dim // 2
        for j in reversed(range(v.flow_layers)):
            p = f"vpflow.ap_{j}"
            x1, x2 = z[:, :half], z[:, half:]
            ce = gelu(self.lin(lat, f"{p}.cond_proj"))
            t = self.conv(gelu(self.conv(x1 + ce, f"{p}.net_pre")), f"{p}.net_post")
            gb = self.lin(ce, f"{p}.film.proj")
            z = torch.cat([x1, x2 - (gb[:, :half] * t + gb[:, half:])], dim=1)
        d = self.lin(z, "latent_dec_proj")
        C = v.model_channels
        for i in range(v.decoder_blocks):
            p = f"dec_block_{i}"
            hh = gelu(self.conv(d, f"{p}.conv", dil=2 ** (i % 4)))
            gb = self.lin(lat, f"{p}.film.proj")
            d = d + self.conv(gb[:, :C] * hh + gb[:, C:], f"{p}.res_proj")
        for s in range(v.down_stages):
            d = gelu(self.conv(d.repeat_interleave(2, dim=2), f"upsample.refine.{s}"))
        return self.conv(d, "out_proj"), self.lin(d, "residual_proj").transpose(1, 2)


def time_ms(fn, iters, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end) / iters


def ragged_main(args, dev):
    vae = TextConditionedVAE(80, 256, seed=1)
    randomise(vae, 101)
    lengths = [128 * (i + 1) for i in range(8)]
    B, T, f = len(lengths), max(lengths), vae.downsample_factor
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
    cond = torch.randn(B, T, vae.cond_dim, generator=g).to(dev)
    z = torch.randn(B, T // f, vae.latent_dim, generator=g).to(dev)
    lengths_dev = torch.tensor(lengths, dtype=torch.int32, device=dev)
    items = [(cond[b:b + 1, :n].contiguous(), z[b:b + 1, :n // f].contiguous()) for b, n in enumerate(lengths)]
    ragged = lambda: vae.generate_device(cond, z, lengths=lengths_dev)

    def loop():
        return [vae.generate_device(c, zz) for c, zz in items]
    dense = lambda: vae.generate_device(cond, z)
    with torch.no_grad():
        (mel, res), singles = ragged(), loop()
        for b, n in enumerate(lengths):
            if not (torch.equal(mel[b, :, :n], singles[b][0][0]) and torch.equal(res[b, :n], singles[b][1][0])):
                raise SystemExit(f"item {b}: the ragged call differs from its batch-of-one call")
            if mel[b, :, n:].any() or res[b, n:].any():
                raise SystemExit(f"item {b}: rows past its length are not 0")
        for _ in range(20):
            ragged(); loop(); dense()
        rounds = [(time_ms(ragged, args.iters, dev), time_ms(loop, args.iters, dev), time_ms(dense, args.iters, dev))
                  for _ in range(args.rounds)]
    r = np.array(rounds)
    med = np.median(r, axis=0)
    keys = ("ragged_ms", "loop_of_8_ms", "dense_8x1024_ms")
    rec = {"lengths": lengths, "T": T}
    for i, k in enumerate(keys):
        rec[k] = float(med[i])
        rec[k + "_min_max"] = [float(r[:, i].min()), float(r[:, i].max())]
    rec.update({"ratio_loop_over_ragged": float(med[1] / med[0]), "ratio_ragged_over_dense": float(med[0] / med[2]),
                "launches_ragged": vae.launch_count(B, T), "launches_loop": sum(vae.launch_count(1, n) for n in lengths),
                "items_bit_for_bit_their_batch_of_one_calls": True, "iters": args.iters, "rounds": args.rounds,
                "timing": "device events around `iters` back-to-back calls (launch gaps included), median of rounds; "
                          "the three ways alternate in every round; lengths are a device tensor made once"})
    print(json.dumps(rec), flush=True)
    out = Path(args.out or REPO / "profiles" / "vae_ragged_bench.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"gpu": torch.cuda.get_device_name(dev), "results": [rec]}, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="time the ragged batch of 8 against the loop and the dense call")
    ap.add_argument("--shapes", nargs="+", default=["1x1024", "8x1024"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/vae_decoder_bench.json (vae_ragged_bench.json with --ragged)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_decoder_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    if args.ragged:
        return ragged_main(args, dev)
    vae = TextConditionedVAE(80, 256, seed=1)
    randomise(vae, 101)
    graph = TorchGraph(vae, dev)
    results = []
    for shape in args.shapes:
        B, T = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
        cond = torch.randn(B, T, vae.cond_dim, generator=g).to(dev)
        z = torch.randn(B, T // vae.downsample_factor, vae.latent_dim, generator=g).to(dev)
        ours = lambda: vae.generate_device(cond, z)
        theirs = lambda: graph(cond, z)
        with torch.no_grad():
            (m1, r1), (m2, r2) = ours(), theirs()
            scale = max(1.0, float(m2.abs().max()))
            diff = {"mel": float((m1 - m2).abs().max()) / scale,
                    "residual": float((r1 - r2).abs().max()) / max(1.0, float(r2.abs().max()))}
            for _ in range(20):
                ours(); theirs()
            rounds = []
            for _ in range(args.rounds):
                rounds.append((time_ms(ours, args.iters, dev), time_ms(theirs, args.iters, dev)))
        a, b = np.array([r[0] for r in rounds]), np.array([r[1] for r in rounds])
        rec = {"shape": shape, "device_ms": float(np.median(a)), "device_ms_min_max": [float(a.min()), float(a.max())],
               "torch_ops_ms": float(np.median(b)), "torch_ops_ms_min_max": [float(b.min()), float(b.max())],
               "ratio_torch_over_device": float(np.median(b) / np.median(a)), "launches": vae.launch_count(B, T),
               "max_rel_diff_vs_torch_ops": diff, "iters": args.iters, "rounds": args.rounds,
               "timing": "device events around `iters` back-to-back forwards (launch gaps included), median of rounds"}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = Path(args.out or REPO / "profiles" / "vae_decoder_bench.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"gpu": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
