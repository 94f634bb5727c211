"""Every launch of the VAE decoder and the posterior encoder against its fmaf chain, on the launch's OWN input tensor
(oracle/vae_chain_cases.py: the restatements, the claims and the derivation of their bars).

After a forward the workspace still holds what its later launches did not overwrite (``_read_buffers``); a launch whose inputs
AND output survive is judged.  Read off ``vae_forward`` / ``enc_forward`` (``vae_chain_cases.expected_*``), N blocks, S stages:
    decoder  conditioning GEMM, flow, block 0 (N <= 2), block N - 1 (N >= 2), every up stage (S <= 2; S = 3: the last one only,
             stage 2 overwrites stage 0's output, which is stage 1's input), out_proj, residual_proj, down_cond_proj (S = 0).
             Not judged: down_cond_proj (S > 0) and the decoder's own down stages -- they go through p and q, which the up
             stages overwrite; the blocks in between -- da and db alternate.
    encoder  in_proj, FiLM GEMM, block 0 (N <= 2), block N - 1 (N >= 2), every down stage (S <= 2; S = 3: the last one),
             the heads.  Not judged: the blocks in between (ha, hb alternate); S = 3: stages 0 and 1 (d0 is written twice).
The stride-2 form is therefore judged through the encoder, which launches the same instantiation.  Every test asserts the
list of launches it judged.  The layout restatement is pinned: its total equals ``workspace_bytes`` at every shape, and the
offsets of latcond, d0, the last decoder output and the encoder's taps equal what the ``*_tap`` entry points report.

Configurations (``vae_chain_cases.CONFIGS``): "default", "small" (the existing two), "blocks1" .. "blocks4" (default widths,
the judged last block at dilation 1, 2, 4, 8), "wide" (C = 256: 8 waves; S = 0), "odd" (C = 20, n_mels = 6, k = 7, S = 3; the
encoder half with n_mels = 8), "bare" (no block, no coupling; decoder only).  ``create`` accepted each as the issue states
it.  Two weight seeds; dense B = 1 and 3, latent rows 1, 2, 9, 16, 17, 32, 33, 65; ragged (6, 264) on "default" and (4, 70)
on "small" through ``generate_device``, ``encode_device`` and ``decode_posterior_device``, the inputs NaN at and past each
item's length.

The flow's bar is 4 e32, e32 of ``flow_np`` on the device's own z and film, the largest over the forwards of a test (CPU
figures: tests/test_oracle_vae_chain.py, 1.2e-07 .. 2.2e-07).

"bare": with no block and no coupling the conditioning GEMM has no column; ``vae_forward`` queued it all the same and
``launch_gemm`` divided by its zero waves, in the ``launch_count`` dry run too.  Read from the code and fixed before this
configuration first ran (``vae_forward`` skips the launch, ``launch_gemm`` refuses C_out == 0).

Measured on the DEVICE (the first run on an MI355X), worst err / bar per claim kind over both seeds and batch sizes:
    config          GELU     FUSED    flow err / (4 e32)
    default         0.081    0.039    0.304
    small           0.075    0.064    0.236
    blocks1         0.083    0.024    0.381
    blocks2         0.080    0.026    0.301
    blocks3         0.082    0.027    0.334
    blocks4         0.081    0.039    0.304
    wide            -        0.019    0.307     (S = 0: no GELU launch)
    odd             0.076    0.103    0.315
    bare            0.081    -        0.250
    ragged default  0.076    0.027    0.371
    ragged small    0.075    0.045    0.311
and every launch without a GELU equal to its chain, bit for bit, dense and ragged, every output tail exactly 0: no launch
differed from its restatement, and no kernel changed.  The fp32 numpy GELU sits at 0.079 of bar_g on the CPU; the device's
tanhf is as close.  The whole file ran in 9 s.
Every test prints its worst err / bar per claim kind, the elements judged and its wall time (``pytest -s``).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import vae_restatement as vr
from iris import _native
from oracle import vae_chain_cases as vc

pytestmark = pytest.mark.gpu

_pairs = {}


def _pair(name, si):
    if (name, si) not in _pairs:
        _pairs[(name, si)] = vc.make_pair(name, vc.WEIGHT_SEEDS[si])
    return _pairs[(name, si)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tap(model, fn, which, B, T):
    lib = model._ensure()
    off, n = ctypes.c_uint64(), ctypes.c_uint64()
    _native.check(fn, getattr(lib, fn)(model._handle, B, T, which, ctypes.byref(off), ctypes.byref(n)))
    return off.value // 4


def _buffers(model, B, T):
    """The workspace buffers of the last forward, with the layout restatement held to the ABI."""
    bufs, total = model._read_buffers(B, T)
    assert total == model.workspace_bytes(B, T), (type(model).__name__, B, T, total)
    layout, _ = model._workspace_layout(B, T)
    if model._abi_name == "vae_decoder":
        N = model.decoder_blocks
        last = "d0" if N == 0 else ("db" if (N - 1) & 1 else "da")
        want = {_native.VAE_TAP_LAT_COND: "latcond", _native.VAE_TAP_DEC_IN: "d0", _native.VAE_TAP_DEC_OUT: last}
        fn = "iris_vae_decoder_tap"
    else:
        N, S = model.num_wavenet_blocks, model.down_stages
        h_out = "h0" if N == 0 else ("hb" if (N - 1) & 1 else "ha")
        want = {_native.VAE_ENC_TAP_H_IN: "h0", _native.VAE_ENC_TAP_H_OUT: h_out,
                _native.VAE_ENC_TAP_LAT_H: h_out if S == 0 else f"d{(S - 1) & 1}"}
        fn = "iris_vae_encoder_tap"
    for which, name in want.items():
        assert _tap(model, fn, which, B, T) == layout[name][0], (fn, which, name)
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _decode(vae, cond, z, lengths, posterior):
    """One decoder forward -> (plan, every tensor it left).  Ragged: cond and z are NaN at and past each item's length."""
    B, T = cond.shape[:2]
    if lengths is not None:
        cond, z = vc.nan_past(cond, lengths, 1), vc.nan_past(z, lengths, 1, vae.down_stages)
    run = vae.decode_posterior_device if posterior else vae.generate_device
    mel, residual = run(_dev(cond), _dev(z), lengths=lengths)
    torch.cuda.synchronize()
    plan = vc.decoder_plan(vae, posterior=posterior)
    t = vc.from_buffers(plan, vae, _buffers(vae, B, T), B, T)
    t.update(cond=cond, z=z, mel=mel.cpu().numpy(), residual=residual.cpu().numpy())
    return plan, t


def _encode(enc, mel, cond, lengths):
    B, T = cond.shape[:2]
    if lengths is not None:
        mel, cond = vc.nan_past(mel, lengths, 2), vc.nan_past(cond, lengths, 1)
    mean, logvar = enc.encode_device(_dev(mel), _dev(cond), lengths=lengths)
    torch.cuda.synchronize()
    plan = vc.encoder_plan(enc)
    t = vc.from_buffers(plan, enc, _buffers(enc, B, T), B, T)
    mean, logvar = mean.cpu().numpy(), logvar.cpu().numpy()
    t.update(mel_in=mel, cond=cond, heads=np.concatenate([mean, logvar], axis=-1))
    return plan, t, mean


class _Tally:
    def __init__(self):
        self.worst, self.flows, self.elements, self.t0 = {}, [], 0, time.perf_counter()

    def add(self, result, want_names):
        names, worst, flows, elements = result
        assert names == want_names, (names, want_names)
        for k, v in worst.items():
            self.worst[k] = max(self.worst.get(k, 0.0), v)
        self.flows += flows
        self.elements += elements

    def close(self, title):
        e32 = max((f[1] for f in self.flows), default=0.0)
        line = ", ".join(f"{k} err / bar {v:.3f}" for k, v in sorted(self.worst.items()))
        if self.flows:
            err, _, what = max(self.flows, key=lambda f: f[0])
            line += f", flow err {err:.2e} / (4 e32 = {4 * e32:.2e}) = {err / (4 * e32):.3f}"
            assert e32 > 0 and err <= 4 * e32, f"{what}: |got - fp64| / max(1, max |fp64|) = {err:.3e} > 4 e32 = {4 * e32:.3e}"
        print(f"vae chain {title}: {line}; {self.elements} elements judged in {time.perf_counter() - self.t0:.2f} s")


DENSE = [(name, si, B) for name in vc.CONFIGS for si in range(len(vc.WEIGHT_SEEDS)) for B in vc.DENSE_B]


@pytest.mark.parametrize("name,si,B", DENSE, ids=[f"{n}-w{si}-B{B}" for n, si, B in DENSE])
def test_vae_every_launch_is_its_chain_dense(name, si, B):
    enc, vae = _pair(name, si)
    want_dec = vc.expected_decoder(vae)
    tally = _Tally()
    for Tq in vc.DENSE_TQ:
        T = Tq << vae.down_stages
        cond, z, mel = vc.make_inputs(name, B, T)
        plan, t = _decode(vae, cond, z, None, False)
        tally.add(vc.judge_forward(plan, vae, t, T), want_dec)
        if enc is None:
            continue
        plan, t, mean = _encode(enc, mel, cond, None)
        tally.add(vc.judge_forward(plan, enc, t, T), vc.expected_encoder(enc))
        plan, t = _decode(vae, cond, mean, None, True)                       # the FORWARD flow, on the posterior mean
        tally.add(vc.judge_forward(plan, vae, t, T, only=("flow",)), ["flow"])
    tally.close(f"{name} w{si} B={B}")


RAGGED = [(ci, si) for ci in range(len(vc.RAGGED)) for si in range(len(vc.WEIGHT_SEEDS))]


@pytest.mark.parametrize("ci,si", RAGGED, ids=[f"{vc.RAGGED[ci][0]}-{vc.RAGGED[ci][1]}x{vc.RAGGED[ci][2]}-w{si}" for ci, si in RAGGED])
def test_vae_every_launch_is_its_chain_ragged(ci, si):
    name, B, T, lengths = vc.RAGGED[ci]
    enc, vae = _pair(name, si)
    cond, z, mel = vc.make_inputs(name, B, T, seed=7)
    tally = _Tally()
    plan, t = _decode(vae, cond, z, lengths, False)
    tally.add(vc.judge_forward(plan, vae, t, T, lengths), vc.expected_decoder(vae))
    plan, t, mean = _encode(enc, mel, cond, lengths)
    tally.add(vc.judge_forward(plan, enc, t, T, lengths), vc.expected_encoder(enc))
    # the device's own mean is 0 past an item's latent rows (judged above); decode_posterior must not read it there either
    plan, t = _decode(vae, cond, mean, lengths, True)
    tally.add(vc.judge_forward(plan, vae, t, T, lengths), vc.expected_decoder(vae))
    tally.close(f"ragged {name} {B}x{T} w{si}")


def test_bare_decoder_creates_counts_and_runs():
    """decoder_blocks = 0 and flow_layers = 0: no conditioning GEMM (it would have no column).  1 + 2 S + 1 + 2 launches:
    down_cond_proj, the down and the up stages, the flow (latent_dec_proj alone), out_proj and residual_proj."""
    _, vae = _pair("bare", 0)
    S = vae.down_stages
    B, T = 2, 9 << S
    assert vae.launch_count(B, T) == 1 + 2 * S + 1 + 2
    cond, z, _ = vc.make_inputs("bare", B, T)
    plan, t = _decode(vae, cond, z, None, False)
    assert [l["name"] for l in vc.judged(plan)] == ["flow", "upsample.refine.0", "upsample.refine.1", "out_proj", "residual_proj"]
    tally = _Tally()
    tally.add(vc.judge_forward(plan, vae, t, T), vc.expected_decoder(vae))
    tally.close(f"bare B={B} T={T}")
    want = vr.generate_np(vae.weights, vae.get_config(), cond, z)
    w32 = vr.generate_np(vae.weights, vae.get_config(), cond, z, dtype=np.float32)
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(1.0, np.abs(b).max()))
    e32 = max(rel(a, b) for a, b in zip(w32, want))
    err = max(rel(t["mel"], want[0]), rel(t["residual"], want[1]))
    print(f"vae chain bare: parity with generate_np {err:.2e}, e32 {e32:.2e}")
    assert err <= 4 * e32, (err, e32)
