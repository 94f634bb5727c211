"""Ragged batches (iris_hifigan_forward_ragged): items of different lengths in one fp32 forward.

The property under test: item b of a ragged forward is, bit for bit, the forward of mel[b, :, :lengths[b]] alone; the
frames past its length are never read and its waveform past hop * lengths[b] is 0.  The GPU cases are chosen so that every
fp32 kernel family of the forward is reached (asserted on the host-side launch plan, as tests/test_planner_sweep.py does).
"""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.batching import pack_mels, split_waveforms
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
from oracle import hifigan_oracle as orc

HOP = 256


def _lengths(seed, B, lo, hi, T):
    """Seeded lengths in [lo, hi] with 0, 1, T - 1 and T among them (B >= 4)."""
    ls = np.random.default_rng(seed).integers(lo, hi + 1, size=B)
    ls[:4] = [0, 1, T - 1, T]
    return [int(v) for v in np.random.default_rng(seed + 1).permutation(ls)]


# (B, T_max, lengths, kernel families the plan of (B, T_max) must contain)
CASES = [
    (1, 100, [37], {"mrf_small_f32_kernel"}),
    (3, 100, [100, 0, 1], {"mrf_conv_mfma_f32_kernel", "mrf_pair_f32_kernel"}),
    (4, 500, [500, 13, 499, 250], {"mrf_pair_f32_kernel", "mrf_pair_f32_pf_kernel"}),
    (8, 1000, _lengths(81, 8, 1, 1000, 1000), {"mrf_conv_mfma_f32_kernel"}),
    (32, 500, _lengths(325, 32, 1, 500, 500), {"mrf_pair_f32_pf_kernel"}),
    (70, 1000, _lengths(701, 70, 1, 1000, 1000), {"mrf_pair_f32_pf_kernel"}),
]
ALWAYS = {"conv_mfma_f32_kernel", "convt_mfma_f32_kernel", "conv_post_rows_kernel", "mrf_conv_mfma_f32_kernel"}


def _families(plan):
    return {l["kernel"].split("<")[0] for l in plan["launches"]}


# ---- CPU ------------------------------------------------------------------------------------------
def test_cases_reach_every_fp32_kernel_family():
    cfg = GeneratorConfig()
    seen = set()
    for B, T, lengths, want in CASES:
        assert len(lengths) == B and all(0 <= l <= T for l in lengths)
        plan = _native.describe_plan(cfg, B, T)
        fams = _families(plan)
        assert want | ALWAYS <= fams, (B, T, fams)
        seen |= fams
        if (B, T) == (70, 1000):
            assert plan["passes"] == 2            # B * T > 65,536 frames: two sub-batch passes
    # the persistent MRF kernel in each of its job orders, and with the dynamic tile counter (B * T >= 2000, tall tiles)
    names = {l["kernel"] for B, T, _, _ in CASES for l in _native.describe_plan(cfg, B, T)["launches"]}
    assert any(n.endswith("false, 2>") for n in names)       # snake-ordered (tile, branch) jobs
    assert any(n.endswith("false, 1>") for n in names)       # one branch per block
    assert any(n.endswith("true, 0>") for n in names)        # summing launch
    assert any(n.endswith("false, 0, 2, true>") for n in names)   # 128-row tiles
    assert {"mrf_small_f32_kernel", "mrf_pair_f32_kernel", "mrf_pair_f32_pf_kernel"} <= seen


def test_cabi_declares_forward_ragged():
    assert "iris_hifigan_forward_ragged" in _native.SYMBOLS
    lib = _native.load()
    assert hasattr(lib, "iris_hifigan_forward_ragged")


def test_pack_and_split_round_trip():
    rng = np.random.default_rng(5)
    mels = [rng.standard_normal((80, n)).astype(np.float32) for n in (37, 512, 1, 0, 200)]
    padded, lengths = pack_mels(mels)
    assert isinstance(padded, np.ndarray) and padded.dtype == np.float32 and padded.shape == (5, 80, 512)
    assert lengths.dtype == np.int32 and lengths.tolist() == [37, 512, 1, 0, 200]
    for m, p, n in zip(mels, padded, lengths):
        assert np.array_equal(p[:, :n], m) and not p[:, n:].any()
    # tensors in -> tensor out; a fill value for the padding
    pt, lt = pack_mels([torch.from_numpy(m) for m in mels[:2]], fill=7.0)
    assert isinstance(pt, torch.Tensor) and pt.shape == (2, 80, 512) and lt.tolist() == [37, 512]
    assert torch.all(pt[0, :, 37:] == 7.0) and torch.equal(pt[0, :, :37], torch.from_numpy(mels[0]))
    # waveforms: one [hop * T_i] view per item
    wav = rng.standard_normal((5, 512 * HOP)).astype(np.float32)
    parts = split_waveforms(wav, lengths, HOP)
    assert [p.shape for p in parts] == [(HOP * n,) for n in lengths]
    for b, p in enumerate(parts):
        assert np.array_equal(p, wav[b, :HOP * lengths[b]])
    tparts = split_waveforms(torch.from_numpy(wav), torch.from_numpy(lengths), HOP)
    assert all(torch.equal(t, torch.from_numpy(p)) for t, p in zip(tparts, parts))


def test_pack_and_split_validation():
    with pytest.raises(ValueError):
        pack_mels([])
    with pytest.raises(ValueError):
        pack_mels([np.zeros((80, 4)), np.zeros((79, 4))])        # mel channels differ
    with pytest.raises(ValueError):
        pack_mels([np.zeros((80, 4, 1))])                        # not [n_mels, T]
    wav = np.zeros((2, 10 * HOP), np.float32)
    with pytest.raises(ValueError):
        split_waveforms(wav, [1, 2, 3], HOP)                     # one length per item
    with pytest.raises(ValueError):
        split_waveforms(wav, [1, 11], HOP)                       # longer than the waveform
    with pytest.raises(ValueError):
        split_waveforms(wav, [-1, 2], HOP)
    with pytest.raises(ValueError):
        split_waveforms(wav[0], [1], HOP)                        # not a batch
    with pytest.raises(ValueError):
        split_waveforms(wav, [1.5, 2.0], HOP)


def test_padded_batch_is_wrong_near_a_short_items_end():
    """Why the feature exists, on the CPU oracle: padding a short item to the batch's length changes its last frames
    (the generator sees ~13 frames ahead, and conv_pre's bias makes even zero padding nonzero one layer in)."""
    cfg = GeneratorConfig()
    folded = orc.to_torch_folded(seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0))
    n, T = 30, 48
    mel = seeded_mel(77, 1, n, log_mel=True)
    alone = orc.generator_forward_torch(folded, mel).numpy()[0, 0]
    padded = np.zeros((1, 80, T), np.float32)
    padded[:, :, :n] = mel
    in_batch = orc.generator_forward_torch(folded, padded).numpy()[0, 0, :HOP * n]
    tail = slice(HOP * (n - 13), HOP * n)
    assert np.abs(in_batch[tail] - alone[tail]).max() > 1e-3
    # far from the end the padding is out of reach: the item's own frames decide
    head = slice(0, HOP * (n - 14))
    assert np.abs(in_batch[head] - alone[head]).max() <= 1e-5
    # cut to its own length, the item computes its stand-alone output again
    again = orc.generator_forward_torch(folded, np.ascontiguousarray(padded[:, :, :n])).numpy()[0, 0]
    assert np.array_equal(again, alone)


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), torch.device("cuda", 0))
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,lengths", [c[:3] for c in CASES], ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_ragged_equals_each_item_alone(engine, B, T, lengths):
    dev = engine.device
    mel = torch.from_numpy(seeded_mel(100 + B, B, T, log_mel=True)).to(dev)
    singles = []
    for b, n in enumerate(lengths):
        singles.append(engine.forward(mel[b:b + 1, :, :n].contiguous(), dtype="f32")[0].clone() if n else None)
    outs = []
    for fill in (float("nan"), 1e30):
        m = mel.clone()
        for b, n in enumerate(lengths):
            m[b, :, n:] = fill
        outs.append(engine.forward(m, dtype="f32", lengths=lengths).clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "the result depends on the padded frames"
    out = outs[0]
    assert out.shape == (B, HOP * T)
    for b, n in enumerate(lengths):
        if n:
            assert torch.equal(out[b, :HOP * n], singles[b]), f"item {b} (length {n}) differs from its stand-alone forward"
        assert not out[b, HOP * n:].any(), f"item {b}: waveform past its length is not 0"


@pytest.mark.gpu
def test_ragged_with_full_lengths_equals_plain_forward(engine):
    for B, T in ((3, 100), (8, 1000)):
        mel = torch.from_numpy(seeded_mel(7 + B, B, T, log_mel=True)).to(engine.device)
        plain = engine.forward(mel, dtype="f32").clone()
        ragged = engine.forward(mel, dtype="f32", lengths=torch.full((B,), T, dtype=torch.int32))
        assert torch.equal(ragged, plain)


@pytest.mark.gpu
def test_ragged_against_oracle():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    eng = GeneratorEngine(cfg, sd, torch.device("cuda", 0))
    lengths = [120, 57, 9]
    mel = seeded_mel(1003, 3, 120, log_mel=True)
    got = eng.forward(torch.from_numpy(mel).to(eng.device), dtype="f32", lengths=lengths).cpu().numpy()
    folded = orc.to_torch_folded(sd)
    for b, n in enumerate(lengths):
        want = orc.generator_forward_torch(folded, np.ascontiguousarray(mel[b:b + 1, :, :n])).numpy()[0, 0]
        assert np.abs(got[b, :HOP * n] - want).max() <= 1e-4
        assert not got[b, HOP * n:].any()
    eng.close()


@pytest.mark.gpu
def test_ragged_errors(engine):
    dev = engine.device
    mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(dev)
    for dtype in ("bf16", "f32s"):
        with pytest.raises(_native.NativeCallError) as err:
            engine.forward(mel, dtype=dtype, lengths=[40, 20])
        assert err.value.status == _native.STATUS_UNSUPPORTED
    for bad in ([40], [40, 20, 1], [[40, 20]], [-1, 20], [41, 20], [40.0, 20.0]):
        with pytest.raises(ValueError):
            engine.forward(mel, dtype="f32", lengths=bad)
    # a NULL lengths pointer through the C-ABI
    lib = _native.load()
    out = torch.empty((2, HOP * 40), dtype=torch.float32, device=dev)
    ws = torch.empty(engine.workspace_bytes(2, 40, "f32"), dtype=torch.uint8, device=dev)
    status = lib.iris_hifigan_forward_ragged(engine._handle, ctypes.c_void_p(mel.data_ptr()), 2, 40, None,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                             ctypes.c_uint64(ws.numel()), _native.DTYPE_F32,
                                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert status == _native.STATUS_INVALID_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_drop_in_batch_entry_points(tmp_path):
    from iris import hifigan_pretrained as hp
    from iris.vocoder import HiFiGANVocoder
    rng = np.random.default_rng(19)
    mels = [(rng.standard_normal((80, n)) * 2.0 - 5.0).astype(np.float32) for n in (37, 512, 1)]
    cfg = GeneratorConfig()
    ck = tmp_path / "generator.ckpt"
    torch.save({k: torch.from_numpy(v) for k, v in seeded_state_dict(cfg, seed=4).items()}, ck)
    batch = hp.infer_hifigan_batch(mels, checkpoint_path=ck)
    assert len(batch) == 3
    for m, w in zip(mels, batch):
        single = hp.infer_hifigan(m, checkpoint_path=ck)
        assert w.ndim == 1 and w.shape == (HOP * m.shape[1],) and np.array_equal(w, single)
    voc = HiFiGANVocoder()
    vb = voc.infer_batch(mels)
    for m, w in zip(mels, vb):
        single = voc.infer(m)
        assert w.ndim == 1 and np.array_equal(w, single)
    assert voc.infer_batch([]) == []
