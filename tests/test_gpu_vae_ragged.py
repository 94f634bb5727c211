"""The ragged VAE decoder (iris_vae_decoder_forward_ragged, ``generate_device(..., lengths=)``) on the MI355X: item b of a
ragged call against the batch-of-one call on its own rows, bit for bit, and once against the numpy restatement
(tests/vae_restatement.py).  Configs and weights are vae_cases.make_vae's.

Two shapes.  "default": T = 260, lengths (260, 132, 128, 36, 4, 0) -- latent rows 65 (three 32-row tiles), 33 and 32 (an end
one past a tile edge and on one), 9 (the dilation-8 taps reach past the item's end into the next item's rows), 1 (every tap
but one is padding) and 0 (an empty item).  "small": T = 70, lengths (70, 34, 6) -- one down stage, channels that are no
multiples of 32.  Every test starts from ``cond`` and ``z_prior`` that hold NaN past each item's length.

The restatement bar is measured, not guessed.  For exactly the "default" inputs of this file (``inputs("default")``, item b
alone: ``cond[b:b+1, :len_b]``, ``z[b:b+1, :len_b / 4]``),
``e32 = max|generate_np(fp32) - generate_np(fp64)| / max(1, max|fp64|)`` of the mel on the CPU was
    item  frames   mel
    0     260      1.005e-06
    1     132      9.262e-07
    2     128      9.239e-07
    3     36       8.680e-07
    4     4        5.161e-07
so the bar is 4 x 1.005e-06 = 4.02e-06 -- the factor 4 allows for another summation order and tanhf, as in
tests/test_gpu_vae.py -- inside the project's 1e-4 parity claim.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.pipeline import MelToWavePipeline

import vae_restatement as R
from vae_cases import make_inputs, make_vae

pytestmark = pytest.mark.gpu

SHAPES = {"default": (260, (260, 132, 128, 36, 4, 0)), "small": (70, (70, 34, 6))}
E32_MAX = 1.005e-06                 # the largest e32 of the table above (item 0, 260 frames)
BAR = 4 * E32_MAX
assert BAR <= 1e-4
DEV = torch.device("cuda", 0)


_vaes = {}


def vae_of(name):
    if name not in _vaes:
        _vaes[name] = make_vae(name)
    return _vaes[name]


def inputs(name, lengths=None):
    """(cond, z) of shape `name` as numpy, seeded (vae_cases.make_inputs), with NaN past each item's length -- `lengths`
    defaults to the shape's own; another assignment of lengths to the items poisons the same numbers differently."""
    T, own = SHAPES[name]
    lengths = own if lengths is None else lengths
    vae = vae_of(name)
    cond, z = make_inputs(vae, len(own), T)
    for b, n in enumerate(lengths):
        cond[b, n:] = np.nan
        z[b, n // vae.downsample_factor:] = np.nan
    return cond, z


@pytest.fixture(scope="module")
def single():
    """(name, b, n) -> (mel [n_mels, n], residual [n, cond_dim]) of the batch-of-one call on item b's first n frames,
    computed once.  The numbers of item b do not depend on which lengths poisoned the rest."""
    cache = {}

    def get(name, b, n):
        if (name, b, n) not in cache:
            vae = vae_of(name)
            cond, z = inputs(name, [SHAPES[name][0]] * len(SHAPES[name][1]))           # nothing poisoned
            c = torch.from_numpy(cond[b:b + 1, :n]).to(DEV)
            zz = torch.from_numpy(z[b:b + 1, :n // vae.downsample_factor]).to(DEV)
            mel, res = vae.generate_device(c, zz)
            assert not torch.isnan(mel).any() and not torch.isnan(res).any()
            cache[(name, b, n)] = (mel[0].clone(), res[0].clone())
        return cache[(name, b, n)]
    return get


def _dev(name, lengths=None):
    cond, z = inputs(name, lengths)
    return torch.from_numpy(cond).to(DEV), torch.from_numpy(z).to(DEV)


def _check_items(name, mel, res, lengths, single):
    """Item b equals its batch-of-one call, everything past its length is exactly 0, nothing is NaN."""
    T = SHAPES[name][0]
    assert mel.shape[2] == T and not torch.isnan(mel).any()
    for b, n in enumerate(lengths):
        want_mel, want_res = single(name, b, n)
        assert torch.equal(mel[b, :, :n], want_mel), (name, b, n)
        assert not mel[b, :, n:].any(), (name, b, n)
        if res is not None:
            assert torch.equal(res[b, :n], want_res), (name, b, n)
            assert not res[b, n:].any() and not torch.isnan(res[b]).any(), (name, b, n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_items_equal_their_batch_of_one_calls(single, name):
    vae = vae_of(name)
    T, lengths = SHAPES[name]
    cond, z = _dev(name)
    assert torch.isnan(cond).any() and torch.isnan(z).any()
    mel, res = vae.generate_device(cond, z, lengths=lengths)
    assert tuple(mel.shape) == (len(lengths), vae.n_mels, T) and tuple(res.shape) == (len(lengths), T, vae.cond_dim)
    _check_items(name, mel, res, lengths, single)
    mel2, none = vae.generate_device(cond, z, want_residual=False, lengths=lengths)
    assert none is None and torch.equal(mel2, mel)
    # numpy in, numpy out
    mel_np, res_np = vae.generate(*inputs(name), lengths=np.asarray(lengths))
    assert np.array_equal(mel_np, mel.cpu().numpy()) and np.array_equal(res_np, res.cpu().numpy())


@pytest.mark.parametrize("name", list(SHAPES))
def test_full_lengths_are_the_dense_call_and_device_lengths_the_host_list(name):
    vae = vae_of(name)
    T, lengths = SHAPES[name]
    B = len(lengths)
    cond, z = _dev(name, [T] * B)
    dense_mel, dense_res = vae.generate_device(cond, z)
    mel, res = vae.generate_device(cond, z, lengths=[T] * B)
    assert torch.equal(mel, dense_mel) and torch.equal(res, dense_res)
    cond, z = _dev(name)
    host = vae.generate_device(cond, z, lengths=list(lengths))
    dev = vae.generate_device(cond, z, lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    assert torch.equal(host[0], dev[0]) and torch.equal(host[1], dev[1])
    with pytest.raises(ValueError, match="int32"):
        vae.generate_device(cond, z, lengths=torch.tensor(lengths, dtype=torch.int64, device=DEV))


def test_lengths_overwritten_in_place_between_two_calls(single):
    name = "default"
    vae = vae_of(name)
    T, first = SHAPES[name]
    second = (36, 0, 260, 4, 132, 128)                                                 # a permutation of `first`
    assert sorted(second) == sorted(first) and all(a != b for a, b in zip(first, second))
    lengths_dev = torch.tensor(first, dtype=torch.int32, device=DEV)
    ptr = lengths_dev.data_ptr()
    mel1, res1 = vae.generate_device(*_dev(name, first), lengths=lengths_dev)
    lengths_dev.copy_(torch.tensor(second, dtype=torch.int32))
    assert lengths_dev.data_ptr() == ptr
    mel2, res2 = vae.generate_device(*_dev(name, second), lengths=lengths_dev)
    _check_items(name, mel1, res1, first, single)
    _check_items(name, mel2, res2, second, single)


def _c_ragged(vae, cond, z, lengths_dev, T=None, ws_short=0, mel=None, res=None):
    """iris_vae_decoder_forward_ragged itself, on a workspace of its own; returns (status, mel, residual)."""
    lib = vae._ensure()
    B = cond.shape[0]
    T = cond.shape[1] if T is None else T
    n = ctypes.c_uint64()
    _native.check("workspace_bytes", lib.iris_vae_decoder_workspace_bytes(vae._handle, B, cond.shape[1], ctypes.byref(n)))
    ws = torch.full((n.value,), 0xFF, dtype=torch.uint8, device=DEV)               # every float of it a NaN
    mel = torch.empty((B, vae.n_mels, cond.shape[1]), device=DEV) if mel is None else mel
    res = torch.empty((B, cond.shape[1], vae.cond_dim), device=DEV) if res is None else res
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    status = lib.iris_vae_decoder_forward_ragged(
        vae._handle, ctypes.c_void_p(cond.data_ptr()), ctypes.c_void_p(z.data_ptr()), B, T,
        ctypes.c_void_p(lengths_dev.data_ptr() if lengths_dev is not None else None), ctypes.c_void_p(mel.data_ptr()),
        ctypes.c_void_p(res.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ctypes.c_uint64(n.value - ws_short), stream)
    torch.cuda.synchronize(DEV)
    return status, mel, res


@pytest.mark.parametrize("name", list(SHAPES))
def test_lengths_are_sanitised_on_the_device(single, name):
    vae = vae_of(name)
    T, own = SHAPES[name]
    f = vae.downsample_factor
    # T + 7 -> T, -3 -> 0, len + 1 -> len (rounded down to the factor), for the shape's first three items
    raw = [T + 7, -3, own[2] + 1]
    clean = [T, 0, own[2]]
    assert own[2] % f == 0 and (own[2] + 1) % f
    lengths = clean + [0] * (len(own) - 3)
    cond, z = _dev(name, lengths)
    raw_dev = torch.tensor(raw + [0] * (len(own) - 3), dtype=torch.int32, device=DEV)
    status, mel, res = _c_ragged(vae, cond, z, raw_dev)
    assert status == 0
    _check_items(name, mel, res, lengths, single)
    want = vae.generate_device(cond, z, lengths=lengths)
    assert torch.equal(mel, want[0]) and torch.equal(res, want[1])


def test_restatement_parity_of_each_item():
    name = "default"
    vae = vae_of(name)
    T, lengths = SHAPES[name]
    mel, _ = vae.generate_device(*_dev(name), lengths=lengths)
    mel = mel.cpu().numpy()
    cond, z = inputs(name)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        want, _ = R.generate_np(vae.weights, vae.get_config(), cond[b:b + 1, :n], z[b:b + 1, :n // vae.downsample_factor])
        err = float(np.abs(mel[b:b + 1, :, :n].astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))
        print(f"item {b} ({n} frames): mel {err:.3e} bar {BAR:.3e}")
        assert err <= BAR, (b, n, err, BAR)


def test_abi_errors_leave_the_outputs_untouched():
    vae = vae_of("default")
    lib = vae._ensure()
    B, T = 2, 8
    cond = torch.zeros(B, T, vae.cond_dim, device=DEV)
    z = torch.zeros(B, T // 4, vae.latent_dim, device=DEV)
    lengths = torch.tensor([8, 4], dtype=torch.int32, device=DEV)
    sentinel = 12345.0
    mel = torch.full((B, vae.n_mels, T), sentinel, device=DEV)
    res = torch.full((B, T, vae.cond_dim), sentinel, device=DEV)
    assert _c_ragged(vae, cond, z, None, mel=mel, res=res)[0] == _native.STATUS_INVALID_ARGUMENT
    assert b"lengths_dev" in lib.iris_hifigan_last_error()
    assert _c_ragged(vae, cond, z, lengths, ws_short=1, mel=mel, res=res)[0] == _native.STATUS_WORKSPACE_TOO_SMALL
    assert _c_ragged(vae, cond, z, lengths, T=6, mel=mel, res=res)[0] == _native.STATUS_INVALID_ARGUMENT      # S = 2
    assert b"multiple" in lib.iris_hifigan_last_error()
    assert bool((mel == sentinel).all()) and bool((res == sentinel).all())
    # the plan is the dense call's: same launches, same workspace, before and after a ragged forward
    n, ws = vae.launch_count(B, T), ctypes.c_uint64()
    lib.iris_vae_decoder_workspace_bytes(vae._handle, B, T, ctypes.byref(ws))
    before = ws.value
    assert n == vae.launch_count(1, 1024) == 13
    assert _c_ragged(vae, cond, z, lengths, mel=mel, res=res)[0] == 0
    assert not bool((mel == sentinel).any()) and not bool((res == sentinel).any())
    lib.iris_vae_decoder_workspace_bytes(vae._handle, B, T, ctypes.byref(ws))
    assert vae.launch_count(B, T) == n and ws.value == before


def test_phonemes_to_waveforms_with_one_vae_call():
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    from iris.postnet import PostNet
    from iris.encoder import frame_conditioning
    from encoder_cases import make_ids, make_models
    enc, head = make_models("default")
    vae = make_vae("default")
    cfg = GeneratorConfig()
    engine = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=1.0), DEV)
    postnet = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    pipe = MelToWavePipeline(postnet, engine.forward, device=DEV, acoustic=vae, text=(enc, head))
    ids = make_ids("default", 3, 37)[:, :6]
    lengths = np.array([6, 1, 3])
    calls = []
    inner = vae.generate_device

    def counted(*a, **kw):
        calls.append(kw.get("lengths"))
        return inner(*a, **kw)
    vae.generate_device = counted
    rng = np.random.default_rng(8)
    singles, zs = [], []
    for i in range(3):
        own = ids[i:i + 1, :lengths[i]]
        _, n_i = frame_conditioning(enc, head, own, factor=4)                          # the item's frame total
        zs.append(torch.from_numpy(rng.standard_normal((1, -(-n_i[0] // 4), vae.latent_dim)).astype(np.float32)).to(DEV))
        singles.append(pipe.infer_from_phonemes(own, z_prior=zs[i]))
    del calls[:]
    batch, frames = pipe.infer_from_phonemes(ids, lengths=lengths, z_prior=zs)
    assert len(calls) == 1 and list(calls[0]) == [-(-n // 4) * 4 for n in frames]      # the VAE stage ran once
    assert isinstance(batch, list) and frames == [s[1][0] for s in singles] and len(set(frames)) > 1
    for i in range(3):
        assert tuple(batch[i].shape) == (256 * (-(-frames[i] // 4) * 4),)
        assert torch.equal(batch[i], singles[i][0][0]), i
