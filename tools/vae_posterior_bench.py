#!/usr/bin/env python3
"""Times the device VAE posterior encoder (iris.vae.VAEPosteriorEncoder.encode_device) and the whole reconstruction
(iris.vae.reconstruct: encoder, forward flow, decoder) against the same graph written in torch ops (F.conv1d / F.linear,
same weights) on the same GPU.

    python tools/vae_posterior_bench.py [--shapes 1x1024 8x1024] [--iters 100] [--rounds 5] [--out profiles/vae_posterior_bench.json]
    python tools/vae_posterior_bench.py --ragged [--iters 100] [--rounds 5] [--out profiles/vae_posterior_ragged_bench.json]

Device events around `iters` back-to-back calls, after a warm-up of every shape; the implementations alternate in every
round and the median round is reported with the spread.  Outputs are compared at the timed shape before timing.  Needs a
GPU: there is no CPU fallback and no number without one.

--ragged times a validation pass over a batch of 8 recorded utterances of 128, 256, ..., 1024 frames three ways, alternating
in every round: ONE ragged reconstruct(..., lengths=, losses=True), eight batch-of-one reconstruct(..., losses=True) calls at
the items' own lengths (what a host loop over the items costs), and the dense 8 x 1024 reconstruct(..., losses=True) (what the
ragged call's launches cost when every block has work; its numbers are not the items').  Before timing, every item of the
ragged call is compared with its batch-of-one call bit for bit, the loss sums included.
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
sys.path[:0] = [str(REPO / "iris-tts_amd"), str(REPO / "tests"), str(REPO / "tools")]

from iris.vae import TextConditionedVAE, VAEPosteriorEncoder, reconstruct  # noqa: E402
from vae_decoder_bench import TorchGraph, time_ms  # noqa: E402
from vae_restatement import randomise  # noqa: E402


class TorchPosterior(TorchGraph):
    """call(training=False) in eager torch ops, channels-first [B, C, T] as F.conv1d wants it (the mel already is)."""

    def __init__(self, enc: VAEPosteriorEncoder, vae: TextConditionedVAE, dev):
        super().__init__(vae, dev)
        self.e = enc
        for k, a in enc.weights.items():
            t = torch.from_numpy(a).to(dev)
            if k.endswith(".kernel"):
                t = t.permute(2, 1, 0).contiguous() if t.dim() == 3 else t.t().contiguous()
            self.w[k] = t

    def encode(self, mel, cond):
        e = self.e
        gelu = lambda t: F.gelu(t, approximate="tanh")
        C = e.model_channels
        c = cond.transpose(1, 2)
        h = self.conv(mel, "in_proj")
        for i in range(e.num_wavenet_blocks):
            p = f"enc_block_{i}"
            a = gelu(self.conv(h, f"{p}.conv", dil=2 ** (i % 4)))
            gb = self.lin(c, f"{p}.film.proj")
            h = h + self.conv(gb[:, :C] * a + gb[:, C:], f"{p}.res_proj")
        for s in range(e.down_stages):
            h = gelu(self.conv(h, f"downsample.blocks.{s}", stride=2, pad=(1, 2)))
        return self.lin(h, "latent_mean_proj").transpose(1, 2), self.lin(h, "latent_logvar_proj").transpose(1, 2)

    def reconstruct(self, mel, cond):
        v = self.v
        gelu = lambda t: F.gelu(t, approximate="tanh")
        mean, logvar = self.encode(mel, cond)
        h = self.conv(cond.transpose(1, 2), "down_cond_proj")
        for s in range(v.down_stages):
            h = gelu(self.conv(h, f"downsample.blocks.{s}", stride=2, pad=(1, 2)))
        lat = h
        z = mean.transpose(1, 2)
        half = v.latent_dim // 2
        for j in range(v.flow_layers):
            p = f"vpflow.ap_{j}"
            x1, x2 = z[:, :half], z[:, half:]
            ce = gelu(self.lin(lat, f"{p}.cond_proj"))
            t = self.conv(gelu(self.conv(x1 + ce, f"{p}.net_pre")), f"{p}.net_post")
            gb = self.lin(ce, f"{p}.film.proj")
            z = torch.cat([x1, x2 + (gb[:, :half] * t + gb[:, half:])], dim=1)
        d = self.lin(z, "latent_dec_proj")
        C = v.model_channels
        for i in range(v.decoder_blocks):
            p = f"dec_block_{i}"
            hh = gelu(self.conv(d, f"{p}.conv", dil=2 ** (i % 4)))
            gb = self.lin(lat, f"{p}.film.proj")
            d = d + self.conv(gb[:, :C] * hh + gb[:, C:], f"{p}.res_proj")
        for s in range(v.down_stages):
            d = gelu(self.conv(d.repeat_interleave(2, dim=2), f"upsample.refine.{s}"))
        return self.conv(d, "out_proj"), (mean, logvar), self.lin(d, "residual_proj").transpose(1, 2)


def rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def make_models():
    vae = TextConditionedVAE(80, 256, seed=1)
    randomise(vae, 101)
    enc = VAEPosteriorEncoder(80, 256, seed=2)
    w = randomise(enc, 303, scale=0.5)                    # half-size kernels: 8 residual blocks at gamma ~ 1 stay O(10)
    w.update({k: v for k, v in vae.weights.items() if k.startswith("downsample.blocks.")})
    enc.set_weights_dict(w)
    return enc, vae


def ragged_main(args, dev):
    enc, vae = make_models()
    lengths = [128 * (i + 1) for i in range(8)]
    B, T, f = len(lengths), max(lengths), vae.downsample_factor
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
    mel = torch.randn(B, vae.n_mels, T, generator=g).to(dev)
    cond = torch.randn(B, T, vae.cond_dim, generator=g).to(dev)
    lengths_dev = torch.tensor(lengths, dtype=torch.int32, device=dev)
    items = [(mel[b:b + 1, :, :n].contiguous(), cond[b:b + 1, :n].contiguous()) for b, n in enumerate(lengths)]
    ragged = lambda: reconstruct(enc, vae, mel, cond, lengths=lengths_dev, losses=True)

    def loop():
        return [reconstruct(enc, vae, m, c, losses=True) for m, c in items]
    dense = lambda: reconstruct(enc, vae, mel, cond, losses=True)
    with torch.no_grad():
        (recon, (mean, logvar), res, loss), singles = ragged(), loop()
        for b, n in enumerate(lengths):
            r1, (m1, l1), s1, loss1 = singles[b]
            same = (torch.equal(recon[b, :, :n], r1[0]) and torch.equal(res[b, :n], s1[0]) and torch.equal(mean[b, :n // f], m1[0])
                    and torch.equal(logvar[b, :n // f], l1[0]) and torch.equal(loss[2][b], loss1[2][0]) and torch.equal(loss[3][b], loss1[3][0]))
            if not same:
                raise SystemExit(f"item {b}: the ragged call differs from its batch-of-one call")
            if recon[b, :, n:].any() or res[b, n:].any() or mean[b, n // f:].any() or logvar[b, n // f:].any():
                raise SystemExit(f"item {b}: rows past its length are not 0")
        for _ in range(20):
            ragged(); loop(); dense()
        rounds = [(time_ms(ragged, args.iters, dev), time_ms(loop, args.iters, dev), time_ms(dense, args.iters, dev))
                  for _ in range(args.rounds)]
    r = np.array(rounds)
    med = np.median(r, axis=0)
    keys = ("ragged_ms", "loop_of_8_ms", "dense_8x1024_ms")
    rec = {"lengths": lengths, "T": T, "recon_l1": float(loss[0]), "kl": float(loss[1])}
    for i, k in enumerate(keys):
        rec[k] = float(med[i])
        rec[k + "_min_max"] = [float(r[:, i].min()), float(r[:, i].max())]
    per_call = lambda Bn, Tn: enc.launch_count(Bn, Tn) + vae.launch_count(Bn, Tn) + 2     # + the two launches of the losses
    rec.update({"ratio_loop_over_ragged": float(med[1] / med[0]), "ratio_ragged_over_dense": float(med[0] / med[2]),
                "launches_ragged": per_call(B, T), "launches_loop": sum(per_call(1, n) for n in lengths),
                "items_bit_for_bit_their_batch_of_one_calls": True, "iters": args.iters, "rounds": args.rounds,
                "timing": "device events around `iters` back-to-back calls (launch gaps included), median of rounds; "
                          "the three ways alternate in every round; lengths are a device tensor made once"})
    print(json.dumps(rec), flush=True)
    out = Path(args.out or REPO / "profiles" / "vae_posterior_ragged_bench.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"gpu": torch.cuda.get_device_name(dev), "results": [rec]}, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="time the ragged batch of 8 against the loop and the dense call")
    ap.add_argument("--shapes", nargs="+", default=["1x1024", "8x1024"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/vae_posterior_bench.json (vae_posterior_ragged_bench.json with --ragged)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_posterior_bench needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    if args.ragged:
        return ragged_main(args, dev)
    enc, vae = make_models()
    graph = TorchPosterior(enc, vae, dev)
    results = []
    for shape in args.shapes:
        B, T = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
        mel = torch.randn(B, vae.n_mels, T, generator=g).to(dev)
        cond = torch.randn(B, T, vae.cond_dim, generator=g).to(dev)
        fns = {"encoder_device": lambda: enc.encode_device(mel, cond), "encoder_torch_ops": lambda: graph.encode(mel, cond),
               "reconstruct_device": lambda: reconstruct(enc, vae, mel, cond), "reconstruct_torch_ops": lambda: graph.reconstruct(mel, cond)}
        with torch.no_grad():
            (m1, l1), (m2, l2) = fns["encoder_device"](), fns["encoder_torch_ops"]()
            (r1, _, s1), (r2, _, s2) = fns["reconstruct_device"](), fns["reconstruct_torch_ops"]()
            diff = {"mean": rel(m1, m2), "logvar": rel(l1, l2), "recon": rel(r1, r2), "residual": rel(s1, s2)}
            for _ in range(10):
                for fn in fns.values():
                    fn()
            rounds = [[time_ms(fn, args.iters, dev) for fn in fns.values()] for _ in range(args.rounds)]
        r = np.array(rounds)
        med = np.median(r, axis=0)
        rec = {"shape": shape}
        for i, k in enumerate(fns):
            rec[k + "_ms"] = float(med[i])
            rec[k + "_ms_min_max"] = [float(r[:, i].min()), float(r[:, i].max())]
        rec.update({"ratio_torch_over_device_encoder": float(med[1] / med[0]), "ratio_torch_over_device_reconstruct": float(med[3] / med[2]),
                    "launches_encoder": enc.launch_count(B, T), "launches_reconstruct": enc.launch_count(B, T) + vae.launch_count(B, T),
                    "max_rel_diff_vs_torch_ops": diff, "iters": args.iters, "rounds": args.rounds,
                    "timing": "device events around `iters` back-to-back calls (launch gaps included), median of rounds; "
                              "the four alternate in every round"})
        print(json.dumps(rec), flush=True)
        results.append(rec)
    out = Path(args.out or REPO / "profiles" / "vae_posterior_bench.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"gpu": torch.cuda.get_device_name(dev), "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
