"""CPU tests of iris.encoder (phoneme encoder, duration head, length regulator): packing, C-ABI sizes, argument checks and
the numpy restatement's own conventions.  The device arithmetic is tested in tests/test_gpu_encoder.py."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import encoder as E
from iris.encoder import DurationPredictor, PhonemeEncoder

import encoder_restatement as R
from encoder_cases import BAR, CASES, CONFIGS, E32_WORST, case_id, decided, e32, make_models, reference, valid_mask

REPO = Path(__file__).resolve().parents[1]


def test_native_symbols_are_declared_and_exported_with_abi_4():
    header = (REPO / "include" / "iris_hifigan.h").read_text()
    declared = set(re.findall(r"\b(iris_(?:phoneme_encoder|duration_predictor|length)_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.TEXT_SYMBOLS)
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION == 4
    assert ctypes.sizeof(_native.PhonemeEncoderConfig) == 24 and ctypes.sizeof(_native.DurationPredictorConfig) == 20


@pytest.mark.parametrize("name", ["default", "small"])
def test_weight_count_matches_the_blob(name):
    lib = _native.load()
    enc, head = make_models(name)
    n = ctypes.c_uint64()
    cfg = enc.native_config()
    assert lib.iris_phoneme_encoder_weight_count(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == enc.blob_size() == enc.blob().size
    c = enc.get_config()
    Ed, F = c["embed_dim"], c["ffn_dim"]
    assert n.value == (c["vocab_size"] + c["max_length"]) * Ed + c["num_blocks"] * (4 * (Ed * Ed + Ed) + 2 * Ed * F + F + Ed + 4 * Ed) + 2 * Ed
    dcfg = head.native_config()
    assert lib.iris_duration_predictor_weight_count(ctypes.byref(dcfg), ctypes.byref(n)) == 0
    assert n.value == head.blob_size() == head.blob().size


def test_unsupported_and_invalid_configurations():
    lib = _native.load()
    enc, head = make_models("small")
    n = ctypes.c_uint64()
    for field, value, status in (("num_heads", 5, _native.STATUS_UNSUPPORTED),       # 48 % 5
                                 ("num_heads", 4, _native.STATUS_UNSUPPORTED),       # key_dim 12
                                 ("ffn_dim", 82, _native.STATUS_UNSUPPORTED),
                                 ("embed_dim", 288, _native.STATUS_UNSUPPORTED),     # key_dim 96, but a row above 256
                                 ("vocab_size", 0, _native.STATUS_INVALID_ARGUMENT)):
        bad = enc.native_config()
        setattr(bad, field, value)
        assert lib.iris_phoneme_encoder_weight_count(ctypes.byref(bad), ctypes.byref(n)) == status, field
        assert lib.iris_hifigan_last_error()
    for field, value, status in (("kernel_size", 4, _native.STATUS_UNSUPPORTED), ("hidden_dim", 42, _native.STATUS_UNSUPPORTED),
                                 ("in_dim", 50, _native.STATUS_UNSUPPORTED), ("num_layers", -1, _native.STATUS_INVALID_ARGUMENT)):
        bad = head.native_config()
        setattr(bad, field, value)
        assert lib.iris_duration_predictor_weight_count(ctypes.byref(bad), ctypes.byref(n)) == status, field
    cfg = enc.native_config()
    for P, status in ((0, _native.STATUS_INVALID_ARGUMENT), (enc.max_length + 1, _native.STATUS_INVALID_ARGUMENT)):
        assert lib.iris_phoneme_encoder_workspace_bytes(ctypes.byref(cfg), 1, P, ctypes.byref(n)) == status


@pytest.mark.parametrize("name", ["default", "small"])
def test_workspace_and_launch_count_need_no_device(name):
    enc, head = make_models(name)
    c, d = enc.get_config(), head.get_config()
    for B, P in ((1, 1), (3, 37), (1, c["max_length"])):
        assert enc.launch_count(B, P) == 5 * c["num_blocks"] + 2
        assert head.launch_count(B, P) == d["num_layers"] + 2
        rows = B * P
        assert enc.workspace_bytes(B, P) >= 4 * rows * (7 * c["embed_dim"] + c["ffn_dim"])
        assert enc.workspace_bytes(B, P) % 256 == 0
        assert head.workspace_bytes(B, P) >= 4 * rows * 3 * d["hidden_dim"]
    assert enc.launch_count(1, 1000) == 22 if name == "default" else True


def test_blob_packing_round_trips():
    enc, head = make_models("small")
    blob, w, Ed = enc.blob(), enc.weights, enc.embed_dim
    V, L, F = enc.vocab_size, enc.max_length, enc.ffn_dim
    assert np.array_equal(blob[:V * Ed].reshape(V, Ed), w["phoneme_embedding.embeddings"])
    off = (V + L) * Ed
    qkv = blob[off:off + 3 * Ed * Ed].reshape(3 * Ed, Ed)
    H, Dk = enc.num_heads, Ed // enc.num_heads
    for j, part in enumerate(("query", "key", "value")):
        for h in (0, H - 1):
            for d in (0, Dk - 1):
                assert np.array_equal(qkv[j * Ed + h * Dk + d], w[f"transformer_block_0.attention.{part}.kernel"][:, h, d])
    off += 3 * Ed * Ed
    assert np.array_equal(blob[off:off + 3 * Ed], np.concatenate([w[f"transformer_block_0.attention.{p}.bias"].ravel()
                                                                  for p in ("query", "key", "value")]))
    off += 3 * Ed
    wo = blob[off:off + Ed * Ed].reshape(Ed, Ed)
    assert np.array_equal(wo[5], w["transformer_block_0.attention.output.kernel"].reshape(Ed, Ed)[:, 5])
    assert np.array_equal(blob[-2 * Ed:-Ed], w["encoder_output_norm.gamma"])
    hb = head.blob()
    k0 = w0 = head.weights["duration_conv_0.kernel"]
    n0 = k0.size
    assert np.array_equal(hb[:n0].reshape(head.hidden_dim, head.in_dim, head.kernel_size), w0.transpose(2, 1, 0))
    assert hb[-1] == head.weights["duration_output.bias"][0]
    assert np.array_equal(hb[-1 - head.hidden_dim:-1], head.weights["duration_output.kernel"].ravel())
    assert F == 80


def test_npz_round_trip_and_h5_is_rejected(tmp_path):
    enc, head = make_models("small")
    for model, fresh in ((enc, PhonemeEncoder(**CONFIGS["small"]["encoder"], seed=9)), (head, DurationPredictor(**CONFIGS["small"]["head"], seed=9))):
        path = tmp_path / f"{model.name}.npz"
        model.save_weights(str(path))
        assert not np.array_equal(fresh.blob(), model.blob())
        fresh.load_weights(str(path))
        assert np.array_equal(fresh.blob(), model.blob())
        for ext in (".weights.h5", ".keras"):
            with pytest.raises(NotImplementedError):
                fresh.load_weights(str(tmp_path / f"w{ext}"))
            with pytest.raises(NotImplementedError):
                fresh.save_weights(str(tmp_path / f"w{ext}"))
        with pytest.raises(KeyError):
            fresh.set_weights_dict({})
    assert enc.get_config() == dict(vocab_size=11, embed_dim=48, num_blocks=3, num_heads=3, ffn_dim=80, max_length=150, dropout=0.1)
    assert PhonemeEncoder(vocab_size=80).get_config()["ffn_dim"] == 1024
    assert E.create_encoder(80).get_config()["num_blocks"] == 4 and E.create_duration_predictor().get_config()["kernel_size"] == 3
    assert set(k for k in PhonemeEncoder(vocab_size=5, num_blocks=1).weights if "block_0" in k) == {
        f"transformer_block_0.{s}" for s in (
            "attention.query.kernel", "attention.query.bias", "attention.key.kernel", "attention.key.bias", "attention.value.kernel",
            "attention.value.bias", "attention.output.kernel", "attention.output.bias", "attention_norm.gamma", "attention_norm.beta",
            "ffn.0.kernel", "ffn.0.bias", "ffn.2.kernel", "ffn.2.bias", "ffn_norm.gamma", "ffn_norm.beta")}


def test_bad_arguments_raise_before_any_device_work():
    enc, head = make_models("small")
    ok = np.zeros((1, 5), np.int32)
    for bad in (np.full((1, 5), 11, np.int32), np.full((1, 5), -1, np.int32), np.zeros((1, 151), np.int32), np.zeros((5,), np.int32),
                np.zeros((1, 5), np.float32)):
        with pytest.raises(ValueError):
            enc(bad)
    with pytest.raises(ValueError, match="prefix"):
        enc(ok, mask=np.array([[True, False, True, False, False]]))
    with pytest.raises(ValueError):
        enc(ok, lengths=np.array([6]))
    with pytest.raises(NotImplementedError):
        enc(ok, training=True)
    with pytest.raises(NotImplementedError):
        head(np.zeros((1, 5, 48), np.float32), training=True)
    with pytest.raises(ValueError):
        head(np.zeros((1, 5, 40), np.float32))
    with pytest.raises(ValueError, match=">= 0"):
        E.frame_conditioning(enc, head, ok, durations=np.array([[1, 2, -1, 0, 3]]))
    with pytest.raises(ValueError, match="max_frames"):
        E.frame_conditioning(enc, head, ok, durations=np.array([[40, 40, 0, 0, 21]]), max_frames=100)
    with pytest.raises(ValueError, match="integer"):
        E.frame_conditioning(enc, head, ok, durations=np.ones((1, 5), np.float32))
    assert not hasattr(E, "compute_duration_loss")
    assert np.array_equal(E.create_padding_mask(np.array([1, 3]), 3), [[True, False, False], [True, True, True]])


@pytest.mark.skipif(torch.cuda.is_available(), reason="a HIP device is visible")
def test_no_device_error():
    enc, _ = make_models("small")
    with pytest.raises(RuntimeError, match="no HIP device"):
        enc(np.zeros((1, 5), np.int32))


# ---- the restatement's own conventions ----------------------------------------------------------
def test_attention_with_one_hot_values_is_a_convex_combination():
    enc, _ = make_models("small")
    w = {k: v.astype(np.float64) for k, v in enc.weights.items()}
    p = "transformer_block_0.attention"
    Ed, H, Dk, P = 48, 3, 16, 9
    # value = the position's one-hot code in every head; output = identity on head 0: the result is the probabilities
    w[f"{p}.value.kernel"] = np.zeros((Ed, H, Dk)); w[f"{p}.value.bias"] = np.zeros((H, Dk))
    x = np.random.default_rng(0).standard_normal((P, Ed))
    x[:, :P] = np.eye(P)
    for h in range(H):
        w[f"{p}.value.kernel"][:P, h, :P] = np.eye(P)
    w[f"{p}.output.kernel"] = np.zeros((H, Dk, Ed)); w[f"{p}.output.bias"] = np.zeros(Ed)
    w[f"{p}.output.kernel"][0, :P, :P] = np.eye(P)
    probs = []
    out = R.attention(x, w, p, H, probs)
    a = out[:, :P]
    assert np.all(a >= 0) and np.allclose(a.sum(axis=1), 1.0, atol=1e-12) and np.allclose(a, probs[0][0], atol=1e-12)
    assert np.all(out[:, P:] == 0)
    # the query scale applies after the bias: a bias-only query gives scores bq . k / sqrt(Dk)
    w[f"{p}.query.kernel"] = np.zeros((Ed, H, Dk))
    probs = []
    R.attention(x, w, p, H, probs)
    k = np.einsum("pe,ed->pd", x, w[f"{p}.key.kernel"][:, 0]) + w[f"{p}.key.bias"][0]
    s = k @ w[f"{p}.query.bias"][0] / 4.0
    assert np.allclose(probs[0][0][0], np.exp(s - s.max()) / np.exp(s - s.max()).sum(), atol=1e-12)


def test_length_regulate_reference_docstring_example_and_padding():
    e = np.arange(1, 4, dtype=np.float32)[None, :, None] * np.ones((1, 3, 4), np.float32)
    out = R.length_regulate(e, np.array([[2, 3, 1]]))
    assert out.shape == (1, 6, 4) and out[0, :, 0].tolist() == [1, 1, 2, 2, 2, 3]
    out = R.length_regulate(e, np.array([[2, 0, 1]]), factor=4)
    assert out.shape == (1, 4, 4) and out[0, :, 0].tolist() == [1, 1, 3, 0]
    # layer norm: biased variance
    x = np.array([[1.0, 3.0]])
    assert np.allclose(R.layer_norm(x, np.ones(2), np.zeros(2)), [[-1, 1]], atol=1e-5)
    # 'same' conv pads (k - 1) / 2 zeros on both sides
    y = R.conv1d_same(np.array([[1.0], [2.0], [3.0]]), np.array([1.0, 10.0, 100.0]).reshape(3, 1, 1), np.zeros(1))
    assert y[:, 0].tolist() == [210.0, 321.0, 32.0]
    assert R.predict_frames(np.log1p(np.array([[0.2, 0.5, 1.5, 2.5, 2.51]]))).tolist() == [[1, 1, 2, 2, 3]]   # half to even, clip at 1


def test_measured_bar_and_frame_spread():
    """The bar of tests/test_gpu_encoder.py is 4 x the restatement's own fp32 error, measured here; the randomised head makes
    frames from 1 (some clipped up from 0) to beyond 20; float32 and float64 restatements agree on every decided frame and
    at most 2 % of the positions are undecided."""
    worst, lo, hi, clipped, undecided, positions = 0.0, 10 ** 9, 0, 0, 0, 0
    for case in CASES:
        worst = max(worst, *e32(case).values())
        lengths = case[3]
        m, dec = valid_mask(case), decided(case)
        p64, p32 = reference(case, "float64")["pred"], reference(case, "float32")["pred"]
        f64, f32 = R.predict_frames(p64, lengths), R.predict_frames(p32, lengths)
        assert np.array_equal(f64[dec], f32[dec]), case_id(case)
        lo, hi = min(lo, f64[m].min()), max(hi, f64[m].max())
        clipped += int((np.round(R.raw_frames(p64))[m] < 1).sum())
        undecided += int((m & ~dec).sum()); positions += int(m.sum())
        assert np.all(f64[~m] == 0)
    assert worst <= E32_WORST and BAR == 4 * E32_WORST and BAR <= 1e-4, worst
    assert lo == 1 and hi >= 20 and clipped > 0
    assert undecided <= 0.02 * positions
