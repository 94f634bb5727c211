"""The ragged posterior side (iris_vae_posterior_encode_ragged, iris_vae_decoder_forward_posterior_ragged; ``encode_device``,
``decode_posterior_device`` and ``reconstruct`` with ``lengths=``; ``MelToWavePipeline.resynthesize`` on a list) on the
MI355X: item b of a ragged call against the batch-of-one call on its own rows, bit for bit, and once against the float64
restatement (tests/vae_posterior_restatement.py).  Models are vae_posterior_cases.make_pair's; the shapes are those of
tests/test_gpu_vae_ragged.py, for its reasons.  Every test starts from a mel, a conditioning and a latent that hold NaN past
each item's length, and from a workspace and outputs that hold NaN.

The restatement bar is measured, not guessed.  For exactly the "default" inputs of this file (``inputs("default")``, item b
alone: ``mel[b:b+1, :, :len_b]``, ``cond[b:b+1, :len_b]``),
``e32 = max|reconstruct_np(fp32) - reconstruct_np(fp64)| / max(1, max|fp64|)`` on the CPU was
    item  frames   mean       logvar     recon      residual
    0     260      1.018e-06  1.658e-06  1.352e-06  1.136e-06
    1     132      8.640e-07  9.431e-07  1.357e-06  1.158e-06
    2     128      9.606e-07  1.234e-06  1.443e-06  1.240e-06
    3     36       9.844e-07  1.075e-06  1.160e-06  1.228e-06
    4     4        6.443e-07  9.095e-07  1.299e-06  1.803e-06
so the bar is 4 x 1.803e-06 = 7.21e-06 -- the factor 4 allows for another summation order and tanhf, as in
tests/test_gpu_vae_posterior.py -- inside the project's 1e-4 parity claim.
Observed on an MI355X over these items and tensors: 7.5e-07 ... 2.72e-06 (largest: residual, item 4).
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import vae as V
from iris.pipeline import MelToWavePipeline

import vae_posterior_restatement as P
from vae_posterior_cases import full_config, make_inputs, make_pair

pytestmark = pytest.mark.gpu

SHAPES = {"default": (260, (260, 132, 128, 36, 4, 0)), "small": (70, (70, 34, 6))}
E32_MAX = 1.803e-06                 # the largest e32 of the table above (residual, item 4, 4 frames)
BAR = 4 * E32_MAX
assert BAR <= 1e-4
DEV = torch.device("cuda", 0)
NAN = float("nan")

_pairs = {}


def pair_of(name):
    if name not in _pairs:
        _pairs[name] = make_pair(name)
    return _pairs[name]


def inputs(name, lengths=None):
    """(mel, cond, z) of shape `name` as numpy, seeded, with NaN past each item's length -- `lengths` defaults to the
    shape's own; another assignment of lengths to the items poisons the same numbers differently."""
    T, own = SHAPES[name]
    lengths = own if lengths is None else lengths
    enc, vae = pair_of(name)
    mel, cond = make_inputs(enc, len(own), T)
    z = np.random.default_rng(9000 + T).standard_normal((len(own), T // enc.downsample_factor, enc.latent_dim)).astype(np.float32)
    for b, n in enumerate(lengths):
        mel[b, :, n:] = np.nan
        cond[b, n:] = np.nan
        z[b, n // enc.downsample_factor:] = np.nan
    return mel, cond, z


def _dev(name, lengths=None):
    return [torch.from_numpy(a).to(DEV) for a in inputs(name, lengths)]


def _poison_ws(model, B, T):
    model._ensure()
    ws = model._ws(B, T)
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(NAN)


def _encode(name, mel, cond, lengths):
    enc, _ = pair_of(name)
    _poison_ws(enc, mel.shape[0], mel.shape[2])
    return enc.encode_device(mel, cond, lengths=lengths)


def _decode(name, cond, z, lengths, want_residual=True):
    _, vae = pair_of(name)
    _poison_ws(vae, cond.shape[0], cond.shape[1])
    return vae.decode_posterior_device(cond, z, want_residual, lengths=lengths)


@pytest.fixture(scope="module")
def single():
    """(name, b, n) -> dict of the batch-of-one results on item b's first n frames, computed once: ``mean``, ``logvar``,
    ``recon``, ``residual`` of ``reconstruct`` and ``mel_z``, ``res_z`` of ``decode_posterior_device(cond, z)``.  The
    numbers of item b do not depend on which lengths poisoned the rest."""
    cache = {}

    def get(name, b, n):
        if (name, b, n) not in cache:
            enc, vae = pair_of(name)
            T, own = SHAPES[name]
            mel, cond, z = inputs(name, [T] * len(own))                                 # nothing poisoned
            m = torch.from_numpy(mel[b:b + 1, :, :n]).to(DEV)
            c = torch.from_numpy(cond[b:b + 1, :n]).to(DEV)
            zz = torch.from_numpy(z[b:b + 1, :n // enc.downsample_factor]).to(DEV)
            mean, logvar = enc.encode_device(m, c)
            recon, (mean2, logvar2), residual = V.reconstruct(enc, vae, m, c)
            assert torch.equal(mean, mean2) and torch.equal(logvar, logvar2)
            mel_z, res_z = vae.decode_posterior_device(c, zz)
            out = {"mean": mean, "logvar": logvar, "recon": recon, "residual": residual, "mel_z": mel_z, "res_z": res_z}
            assert not any(torch.isnan(t).any() for t in out.values())
            cache[(name, b, n)] = {k: t[0].clone() for k, t in out.items()}
        return cache[(name, b, n)]
    return get


def _check_latent(name, mean, logvar, lengths, single):
    f = pair_of(name)[0].downsample_factor
    assert not torch.isnan(mean).any() and not torch.isnan(logvar).any()
    for b, n in enumerate(lengths):
        want = single(name, b, n)
        assert torch.equal(mean[b, :n // f], want["mean"]) and torch.equal(logvar[b, :n // f], want["logvar"]), (name, b, n)
        assert not mean[b, n // f:].any() and not logvar[b, n // f:].any(), (name, b, n)


def _check_frames(name, mel, res, lengths, single, keys=("recon", "residual")):
    assert not torch.isnan(mel).any()
    for b, n in enumerate(lengths):
        want = single(name, b, n)
        assert torch.equal(mel[b, :, :n], want[keys[0]]), (name, b, n)
        assert not mel[b, :, n:].any(), (name, b, n)
        if res is not None:
            assert torch.equal(res[b, :n], want[keys[1]]), (name, b, n)
            assert not res[b, n:].any() and not torch.isnan(res[b]).any(), (name, b, n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_items_equal_their_batch_of_one_calls(single, name):
    enc, vae = pair_of(name)
    T, lengths = SHAPES[name]
    B = len(lengths)
    mel, cond, z = _dev(name)
    assert torch.isnan(mel).any() and torch.isnan(cond).any() and torch.isnan(z).any()
    mean, logvar = _encode(name, mel, cond, lengths)
    assert tuple(mean.shape) == tuple(logvar.shape) == (B, T // enc.downsample_factor, enc.latent_dim)
    _check_latent(name, mean, logvar, lengths, single)
    out_mel, out_res = _decode(name, cond, z, lengths)
    assert tuple(out_mel.shape) == (B, vae.n_mels, T) and tuple(out_res.shape) == (B, T, vae.cond_dim)
    _check_frames(name, out_mel, out_res, lengths, single, ("mel_z", "res_z"))
    mel2, none = _decode(name, cond, z, lengths, want_residual=False)
    assert none is None and torch.equal(mel2, out_mel)
    # end to end, device tensors and numpy
    _poison_ws(enc, B, T); _poison_ws(vae, B, T)
    recon, (m, lv), residual = V.reconstruct(enc, vae, mel, cond, lengths=lengths)
    assert torch.equal(m, mean) and torch.equal(lv, logvar)
    _check_frames(name, recon, residual, lengths, single)
    mel_np, cond_np, _ = inputs(name)
    r_np, (m_np, lv_np), s_np = V.reconstruct(enc, vae, mel_np, cond_np, lengths=np.asarray(lengths))
    assert np.array_equal(r_np, recon.cpu().numpy()) and np.array_equal(s_np, residual.cpu().numpy())
    assert np.array_equal(m_np, mean.cpu().numpy()) and np.array_equal(lv_np, logvar.cpu().numpy())
    m_host, lv_host = enc.encode(mel_np, cond_np, lengths=list(lengths))
    assert np.array_equal(m_host, m_np) and np.array_equal(lv_host, lv_np)
    # the default call keeps its arity; losses=True appends one entry
    assert len(V.reconstruct(enc, vae, mel, cond, lengths=lengths, losses=True)) == 4


@pytest.mark.parametrize("name", list(SHAPES))
def test_full_lengths_are_the_dense_call_and_device_lengths_the_host_list(name):
    enc, vae = pair_of(name)
    T, lengths = SHAPES[name]
    B = len(lengths)
    mel, cond, z = _dev(name, [T] * B)
    dense = V.reconstruct(enc, vae, mel, cond)
    full = V.reconstruct(enc, vae, mel, cond, lengths=[T] * B)
    assert torch.equal(full[0], dense[0]) and torch.equal(full[1][0], dense[1][0]) and torch.equal(full[1][1], dense[1][1])
    assert torch.equal(full[2], dense[2])
    dz, fz = vae.decode_posterior_device(cond, z), vae.decode_posterior_device(cond, z, lengths=[T] * B)
    assert torch.equal(dz[0], fz[0]) and torch.equal(dz[1], fz[1])
    mel, cond, z = _dev(name)
    lengths_dev = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    host = V.reconstruct(enc, vae, mel, cond, lengths=list(lengths))
    dev = V.reconstruct(enc, vae, mel, cond, lengths=lengths_dev)
    assert torch.equal(host[0], dev[0]) and torch.equal(host[1][0], dev[1][0]) and torch.equal(host[1][1], dev[1][1])
    assert torch.equal(host[2], dev[2])
    hz, vz = vae.decode_posterior_device(cond, z, lengths=list(lengths)), vae.decode_posterior_device(cond, z, lengths=lengths_dev)
    assert torch.equal(hz[0], vz[0]) and torch.equal(hz[1], vz[1])
    bad = torch.tensor(lengths, dtype=torch.int64, device=DEV)
    for call in (lambda: enc.encode_device(mel, cond, lengths=bad), lambda: vae.decode_posterior_device(cond, z, lengths=bad),
                 lambda: V.reconstruct(enc, vae, mel, cond, lengths=bad)):
        with pytest.raises(ValueError, match="int32"):
            call()


def test_lengths_overwritten_in_place_between_two_calls(single):
    name = "default"
    enc, vae = pair_of(name)
    T, first = SHAPES[name]
    second = (36, 0, 260, 4, 132, 128)                                                 # a permutation of `first`
    assert sorted(second) == sorted(first) and all(a != b for a, b in zip(first, second))
    lengths_dev = torch.tensor(first, dtype=torch.int32, device=DEV)
    ptr = lengths_dev.data_ptr()
    mel, cond, _ = _dev(name, first)
    out1 = V.reconstruct(enc, vae, mel, cond, lengths=lengths_dev)
    lengths_dev.copy_(torch.tensor(second, dtype=torch.int32))
    assert lengths_dev.data_ptr() == ptr
    mel, cond, _ = _dev(name, second)
    out2 = V.reconstruct(enc, vae, mel, cond, lengths=lengths_dev)
    for out, lengths in ((out1, first), (out2, second)):
        _check_latent(name, out[1][0], out[1][1], lengths, single)
        _check_frames(name, out[0], out[2], lengths, single)


def _p(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _nan_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)                         # every float of it a NaN


def _c_encode(enc, mel, cond, lengths_dev, T=None, ws_short=0, mean=None, logvar=None):
    """iris_vae_posterior_encode_ragged itself, on a workspace of its own; returns (status, mean, logvar)."""
    lib = enc._ensure()
    B, Tp = mel.shape[0], mel.shape[2]
    T = Tp if T is None else T
    n = ctypes.c_uint64()
    _native.check("workspace_bytes", lib.iris_vae_encoder_workspace_bytes(enc._handle, B, Tp, ctypes.byref(n)))
    ws = _nan_bytes(n.value)
    mean = torch.full((B, Tp // enc.downsample_factor, enc.latent_dim), NAN, device=DEV) if mean is None else mean
    logvar = torch.full_like(mean, NAN) if logvar is None else logvar
    status = lib.iris_vae_posterior_encode_ragged(enc._handle, _p(mel), _p(cond), B, T, _p(lengths_dev), _p(mean), _p(logvar), _p(ws),
                                                 ctypes.c_uint64(n.value - ws_short), _stream())
    torch.cuda.synchronize(DEV)
    return status, mean, logvar


def _c_decode(vae, cond, z, lengths_dev, T=None, ws_short=0, mel=None, res=None):
    """iris_vae_decoder_forward_posterior_ragged itself, on a workspace of its own; returns (status, mel, residual)."""
    lib = vae._ensure()
    B, Tp = cond.shape[0], cond.shape[1]
    T = Tp if T is None else T
    n = ctypes.c_uint64()
    _native.check("workspace_bytes", lib.iris_vae_decoder_workspace_bytes(vae._handle, B, Tp, ctypes.byref(n)))
    ws = _nan_bytes(n.value)
    mel = torch.full((B, vae.n_mels, Tp), NAN, device=DEV) if mel is None else mel
    res = torch.full((B, Tp, vae.cond_dim), NAN, device=DEV) if res is None else res
    status = lib.iris_vae_decoder_forward_posterior_ragged(vae._handle, _p(cond), _p(z), B, T, _p(lengths_dev), _p(mel), _p(res),
                                                           _p(ws), ctypes.c_uint64(n.value - ws_short), _stream())
    torch.cuda.synchronize(DEV)
    return status, mel, res


@pytest.mark.parametrize("name", list(SHAPES))
def test_lengths_are_sanitised_on_the_device(single, name):
    enc, vae = pair_of(name)
    T, own = SHAPES[name]
    f = enc.downsample_factor
    # T + 7 -> T, -3 -> 0, len + 1 -> len (rounded down to the factor), for the shape's first three items
    raw = [T + 7, -3, own[2] + 1]
    clean = [T, 0, own[2]]
    assert own[2] % f == 0 and (own[2] + 1) % f
    lengths = clean + [0] * (len(own) - 3)
    mel, cond, z = _dev(name, lengths)
    raw_dev = torch.tensor(raw + [0] * (len(own) - 3), dtype=torch.int32, device=DEV)
    status, mean, logvar = _c_encode(enc, mel, cond, raw_dev)
    assert status == 0
    _check_latent(name, mean, logvar, lengths, single)
    status, out_mel, out_res = _c_decode(vae, cond, z, raw_dev)
    assert status == 0
    _check_frames(name, out_mel, out_res, lengths, single, ("mel_z", "res_z"))
    want = vae.decode_posterior_device(cond, z, lengths=lengths)
    assert torch.equal(out_mel, want[0]) and torch.equal(out_res, want[1])


def test_restatement_parity_of_each_item():
    name = "default"
    enc, vae = pair_of(name)
    T, lengths = SHAPES[name]
    mel, cond, _ = _dev(name)
    recon, (mean, logvar), residual = V.reconstruct(enc, vae, mel, cond, lengths=lengths)
    got = {"mean": mean.cpu().numpy(), "logvar": logvar.cpu().numpy(), "recon": recon.cpu().numpy(), "residual": residual.cpu().numpy()}
    mel_np, cond_np, _ = inputs(name)
    f = enc.downsample_factor
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        r, (m, lv), s = P.reconstruct_np(enc.weights, vae.weights, full_config(enc, vae), mel_np[b:b + 1, :, :n], cond_np[b:b + 1, :n])
        want = {"mean": (m, got["mean"][b:b + 1, :n // f]), "logvar": (lv, got["logvar"][b:b + 1, :n // f]),
                "recon": (r, got["recon"][b:b + 1, :, :n]), "residual": (s, got["residual"][b:b + 1, :n])}
        errs = {k: float(np.abs(g.astype(np.float64) - w).max() / max(1.0, np.abs(w).max())) for k, (w, g) in want.items()}
        print(f"item {b} ({n} frames):", {k: f"{v:.3e}" for k, v in errs.items()}, f"bar {BAR:.3e}")
        assert all(np.isfinite(v) and v <= BAR for v in errs.values()), (b, n, errs, BAR)


def test_abi_errors_leave_the_outputs_untouched():
    enc, vae = pair_of("default")
    lib = enc._ensure()
    vae._ensure()
    B, T = 2, 8
    mel = torch.zeros(B, enc.n_mels, T, device=DEV)
    cond = torch.zeros(B, T, enc.cond_dim, device=DEV)
    z = torch.zeros(B, T // 4, enc.latent_dim, device=DEV)
    lengths = torch.tensor([8, 4], dtype=torch.int32, device=DEV)
    sentinel = 12345.0
    mean, logvar = torch.full((B, T // 4, enc.latent_dim), sentinel, device=DEV), torch.full((B, T // 4, enc.latent_dim), sentinel, device=DEV)
    out_mel, out_res = torch.full((B, vae.n_mels, T), sentinel, device=DEV), torch.full((B, T, vae.cond_dim), sentinel, device=DEV)
    enc_call = lambda L, **kw: _c_encode(enc, mel, cond, L, mean=mean, logvar=logvar, **kw)[0]
    dec_call = lambda L, **kw: _c_decode(vae, cond, z, L, mel=out_mel, res=out_res, **kw)[0]
    for call in (enc_call, dec_call):
        assert call(None) == _native.STATUS_INVALID_ARGUMENT
        assert b"lengths_dev" in lib.iris_hifigan_last_error()
        assert call(lengths, ws_short=1) == _native.STATUS_WORKSPACE_TOO_SMALL
        assert call(lengths, T=6) == _native.STATUS_INVALID_ARGUMENT                    # S = 2
        assert b"multiple" in lib.iris_hifigan_last_error()
    for t in (mean, logvar, out_mel, out_res):
        assert bool((t == sentinel).all())
    # the plan is the dense call's: same launches, same workspace, before and after a ragged forward
    before = (enc.launch_count(B, T), enc.workspace_bytes(B, T), vae.launch_count(B, T), vae.workspace_bytes(B, T))
    assert before[0] == enc.launch_count(1, 1024) == 13 and before[2] == vae.launch_count(1, 1024) == 13
    assert enc_call(lengths) == 0 and dec_call(lengths) == 0
    for t in (mean, logvar, out_mel, out_res):
        assert not bool((t == sentinel).any())
    assert (enc.launch_count(B, T), enc.workspace_bytes(B, T), vae.launch_count(B, T), vae.workspace_bytes(B, T)) == before


def test_resynthesize_on_a_list_runs_reconstruct_once(monkeypatch):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    from iris.postnet import PostNet
    enc, vae = pair_of("default")
    cfg = GeneratorConfig()
    engine = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=1.0), DEV)
    postnet = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    pipe = MelToWavePipeline(postnet, engine.forward, device=DEV, acoustic=vae, posterior=enc)
    frames = (36, 8, 20)
    mel_np, cond_np = make_inputs(enc, 3, 36)
    mels = [torch.from_numpy(np.ascontiguousarray(mel_np[i, :, :n])).to(DEV) for i, n in enumerate(frames)]
    conds = [torch.from_numpy(np.ascontiguousarray(cond_np[i, :n])).to(DEV) for i, n in enumerate(frames)]
    singles = [pipe.resynthesize(m[None], c[None]).clone() for m, c in zip(mels, conds)]
    calls = []
    inner = V.reconstruct

    def counted(*a, **kw):
        calls.append(kw.get("lengths"))
        return inner(*a, **kw)
    monkeypatch.setattr(V, "reconstruct", counted)
    wavs = pipe.resynthesize(mels, conds)
    assert len(calls) == 1 and list(calls[0]) == list(frames)                          # the posterior side ran once
    assert isinstance(wavs, list) and len(wavs) == 3
    for i, n in enumerate(frames):
        assert tuple(wavs[i].shape) == (256 * n,) and torch.equal(wavs[i], singles[i][0]), i
    # numpy in: the same waveforms
    host = pipe.resynthesize([m.cpu().numpy() for m in mels], [c.cpu().numpy() for c in conds])
    assert all(torch.equal(a, b) for a, b in zip(host, wavs))
    with pytest.raises(ValueError, match="multiple of 2\\^down_stages"):
        pipe.resynthesize([mels[0][:, :34]], [conds[0][:34]])
