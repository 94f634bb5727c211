"""Ragged PostNet batches (iris_postnet_forward_ragged) and MelToWavePipeline.infer_batch.

The property under test: item b of a ragged PostNet pass is, bit for bit, the pass over mel[b, :, :lengths[b]] alone -- the
'same' padding of every layer ends at the item's own length -- the frames past its length are never read, and the refined
mel past it is 0.  infer_batch chains that into the vocoder's ragged forward: one PostNet pass and one forward per list.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from iris import _native
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
from iris.postnet import PostNet
from oracle import hifigan_oracle as orc
from oracle import postnet_oracle as porc

REPO = Path(__file__).resolve().parent.parent
HOP = 256

# Row tiles of the layers of a 3 x 256 x k5 PostNet (pick_tile / launch_conv, csrc/conv_mfma_f32.h): C_out = 256 and
# C_out = 80 both take WT = 1 (one wave row, four waves across C_out), so a tile is WT * MT * 32 = 32 rows with MT = 1 and
# 64 rows with MT = 2.  launch_conv picks MT = 1 while the grid has fewer than two blocks per CU (512 blocks on 256 CUs):
# every small case below, and every item run alone.  (8, 2048) is the smallest round shape whose hidden layers reach 512
# blocks (ceil(2048 / 64) * 2 C_out blocks * 8 items) and run 64-row tiles, while its last layer (one C_out block) and
# every stand-alone reference still run 32-row ones: the lengths sit one below, at and one above both tile edges.
TILE_ROWS_MT1, TILE_ROWS_MT2 = 32, 64
CASES = [
    (1, 40, [17]),
    (4, 70, [70, 0, 1, 69]),
    (3, 300, [300, 5, 131]),
    (6, 70, [TILE_ROWS_MT1 - 1, TILE_ROWS_MT1, TILE_ROWS_MT1 + 1, TILE_ROWS_MT2 - 1, TILE_ROWS_MT2, TILE_ROWS_MT2 + 1]),
    (8, 2048, [2048, TILE_ROWS_MT2 - 1, TILE_ROWS_MT2, TILE_ROWS_MT2 + 1, 2 * TILE_ROWS_MT2 - 1, 2 * TILE_ROWS_MT2 + 1,
               TILE_ROWS_MT1 + 1, 1]),
]


def _randomise(pn: PostNet, seed: int) -> None:
    """Non-trivial BatchNorm statistics and biases, so that nothing the padded frames could reach is zero by accident."""
    rng = np.random.default_rng(seed)
    w = dict(pn.weights)
    for key, val in w.items():
        if key.endswith(".bias") or key.endswith(".beta") or key.endswith(".moving_mean"):
            w[key] = rng.normal(0, 0.3, val.shape).astype(np.float32)
        elif key.endswith(".gamma"):
            w[key] = rng.uniform(0.5, 1.5, val.shape).astype(np.float32)
        elif key.endswith(".moving_variance"):
            w[key] = rng.uniform(0.2, 2.0, val.shape).astype(np.float32)
    pn.set_weights_dict(w)


# ---- CPU ------------------------------------------------------------------------------------------
def test_cabi_declares_postnet_forward_ragged():
    header = (REPO / "include" / "iris_hifigan.h").read_text()
    assert re.search(r"\bint32_t\s+iris_postnet_forward_ragged\s*\(", header)
    assert "iris_postnet_forward_ragged" in _native.SYMBOLS
    # same arguments as the plain forward plus the lengths pointer
    plain, ragged = _native.SYMBOLS["iris_postnet_forward"], _native.SYMBOLS["iris_postnet_forward_ragged"]
    assert ragged[0] is plain[0] and len(ragged[1]) == len(plain[1]) + 1
    lib = _native.load()
    assert hasattr(lib, "iris_postnet_forward_ragged")
    assert _native.ABI_VERSION == 4 and lib.iris_hifigan_abi_version() == 4      # a backward-compatible addition


def test_receptive_field_frames():
    assert PostNet(n_mels=80, num_layers=3, kernel_size=5).receptive_field_frames == 6
    assert PostNet(n_mels=80, num_layers=4, kernel_size=5).receptive_field_frames == 8


def test_receptive_field_is_tight_on_the_oracle():
    """The figure the session's halo rests on, on the numpy restatement: a raw frame reaches exactly +-6 refined frames."""
    pn = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    _randomise(pn, 6)
    rf = pn.receptive_field_frames
    mel = seeded_mel(31, 1, 40, log_mel=True)
    base = porc.postnet_forward_np(pn.weights, mel, 3)
    poked = mel.copy()
    poked[:, :, 20] += 1.0
    changed = np.flatnonzero(np.abs(porc.postnet_forward_np(pn.weights, poked, 3) - base).max(axis=(0, 1)) > 0)
    assert changed.min() == 20 - rf and changed.max() == 20 + rf


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def postnet():
    pn = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, dropout=0.3, seed=5)
    _randomise(pn, 6)
    return pn


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,lengths", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_ragged_postnet_equals_each_item_alone(postnet, B, T, lengths):
    assert len(lengths) == B and all(0 <= n <= T for n in lengths)
    mel = torch.from_numpy(seeded_mel(200 + B, B, T, log_mel=True)).cuda()
    singles = [postnet.forward_device(mel[b:b + 1, :, :n].contiguous()).clone() if n else None for b, n in enumerate(lengths)]
    outs = []
    for fill in (float("nan"), 1e30):
        m = mel.clone()
        for b, n in enumerate(lengths):
            m[b, :, n:] = fill
        outs.append(postnet.forward_device(m, lengths=lengths).clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "the result depends on the padded frames"
    out = outs[0]
    assert out.shape == (B, 80, T) and torch.isfinite(out).all()
    for b, n in enumerate(lengths):
        if n:
            assert torch.equal(out[b:b + 1, :, :n], singles[b]), f"item {b} (length {n}) differs from its stand-alone pass"
        assert not out[b, :, n:].any(), f"item {b}: refined mel past its length is not 0"


@pytest.mark.gpu
def test_ragged_postnet_with_full_lengths_equals_plain(postnet):
    mel = torch.from_numpy(seeded_mel(9, 3, 70, log_mel=True)).cuda()
    plain = postnet.forward_device(mel).clone()
    assert torch.equal(postnet.forward_device(mel, lengths=torch.full((3,), 70, dtype=torch.int32)), plain)
    assert torch.equal(postnet.forward_device(mel, lengths=[70, 70, 70]), plain)


@pytest.mark.gpu
def test_ragged_postnet_errors(postnet):
    mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).cuda()
    for bad in ([40], [40, 20, 1], [[40, 20]], [-1, 20], [41, 20], [40.0, 20.0], torch.tensor([40.0, 20.0])):
        with pytest.raises(ValueError):
            postnet.forward_device(mel, lengths=bad)
    # a NULL lengths pointer through the C-ABI
    lib = postnet._ensure()
    n = ctypes.c_uint64()
    assert lib.iris_postnet_workspace_bytes(postnet._handle, 2, 40, ctypes.byref(n)) == 0
    ws = torch.empty(int(n.value), dtype=torch.uint8, device=mel.device)
    out = torch.empty_like(mel)
    status = lib.iris_postnet_forward_ragged(postnet._handle, ctypes.c_void_p(mel.data_ptr()), 2, 40, None,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                             ctypes.c_uint64(ws.numel()),
                                             ctypes.c_void_p(torch.cuda.current_stream(mel.device).cuda_stream))
    assert status == _native.STATUS_INVALID_ARGUMENT
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_ragged_postnet_against_oracle(postnet):
    lengths = [120, 57, 9]
    mel = seeded_mel(1003, 3, 120, log_mel=True)
    got = postnet.forward_device(torch.from_numpy(mel).cuda(), lengths=lengths).cpu().numpy()
    for b, n in enumerate(lengths):
        item = np.ascontiguousarray(mel[b:b + 1, :, :n])
        want = porc.postnet_forward_np(postnet.weights, item, 3)[0]
        # the bar tests/test_postnet.py sets for the plain forward: 4 x the reference's own fp32 error on this item, at most 2e-5
        e32 = porc.e32(postnet.weights, item, 3)
        err = np.abs(got[b, :, :n] - want).max() / max(1.0, np.abs(want).max())
        print(f"ragged postnet item {b} ({n} frames): err {err:.3e} e32 {e32:.3e} bar {min(2e-5, 4 * e32):.3e}")
        assert err <= min(2e-5, 4 * e32), (err, e32)
        assert not got[b, :, n:].any()


@pytest.mark.gpu
def test_infer_batch_equals_each_utterance_alone(postnet):
    from iris._engine import GeneratorEngine
    from iris.pipeline import MelToWavePipeline
    dev = torch.device("cuda", 0)
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0)
    eng = GeneratorEngine(cfg, sd, dev, dtype="f32")
    pipe = MelToWavePipeline(postnet, eng.forward, device=dev, chunk_frames=256)
    mels = [seeded_mel(40 + i, 1, n, log_mel=True)[0] for i, n in enumerate((37, 300, 1))]
    calls = {"postnet": 0, "vocode": 0}
    fwd_post, fwd_voc = postnet.forward_device, pipe.streamer.forward

    class CountingPostNet:
        receptive_field_frames = postnet.receptive_field_frames

        def forward_device(self, mel, lengths=None):
            calls["postnet"] += 1
            return fwd_post(mel, lengths=lengths)

    def counting_vocode(mel, **kw):
        calls["vocode"] += 1
        return fwd_voc(mel, **kw)

    counted = MelToWavePipeline(CountingPostNet(), counting_vocode, device=dev, chunk_frames=256, config=cfg)
    waves = [w.clone() for w in counted.infer_batch(mels)]
    assert calls == {"postnet": 1, "vocode": 1}                      # one pass and one forward for the whole list
    assert len(waves) == 3
    for m, w in zip(mels, waves):
        alone = pipe.infer(m[None])[0]
        assert w.shape == (HOP * m.shape[1],) and torch.equal(w, alone)
    assert pipe.infer_batch([]) == []
    # without a PostNet: the engine's ragged forward alone
    plain = MelToWavePipeline(None, eng.forward, device=dev).infer_batch(mels)
    for m, w in zip(mels, plain):
        assert torch.equal(w, eng.forward(torch.from_numpy(m[None]).to(dev))[0])
    # not only self-consistent: the 37-frame item against the CPU restatements, one shot
    refined = porc.postnet_forward_np(postnet.weights, mels[0][None], 3)
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), refined).numpy()[0, 0]
    assert np.abs(waves[0].cpu().numpy() - want).max() <= 1e-4
    # a vocoder dtype without a ragged forward keeps failing as engine.forward(lengths=...) does
    for dtype in ("bf16", "f32s"):
        other = MelToWavePipeline(postnet, lambda m, **kw: eng.forward(m, dtype=dtype, **kw), device=dev, config=cfg)
        with pytest.raises(_native.NativeCallError) as err:
            other.infer_batch(mels)
        assert err.value.status == _native.STATUS_UNSUPPORTED
    eng.close()
