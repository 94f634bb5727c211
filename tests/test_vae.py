"""iris.vae.TextConditionedVAE without a GPU: constructor surface, weight I/O, argument checks, the blob the C side
expects, the numpy restatement's own conventions (tests/vae_restatement.py) and the pipeline's ``infer_from_cond``."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.pipeline import MelToWavePipeline
from iris.vae import TextConditionedVAE

import vae_restatement as R
from vae_cases import CASES, CONFIGS, make_inputs, make_vae


def test_constructor_config_and_shapes():
    vae = TextConditionedVAE(80, 256, seed=0)
    cfg = vae.get_config()
    assert cfg == {"n_mels": 80, "cond_dim": 256, "model_channels": 192, "latent_dim": 16, "num_wavenet_blocks": 8,
                   "decoder_blocks": 4, "wavenet_kernel_size": 5, "down_stages": 2, "flow_layers": 4, "flow_hidden": 64,
                   "dropout": 0.1}
    w = vae.weights
    assert w["down_cond_proj.kernel"].shape == (1, 256, 192)
    assert w["downsample.blocks.1.kernel"].shape == (5, 192, 192) and w["downsample.blocks.0.bias"].shape == (192,)
    assert w["vpflow.ap_0.net_pre.kernel"].shape == (3, 8, 64)
    assert w["vpflow.ap_2.cond_proj.kernel"].shape == (192, 8)
    assert w["vpflow.ap_2.film.proj.kernel"].shape == (8, 16)
    assert w["latent_dec_proj.kernel"].shape == (16, 192)
    assert w["dec_block_3.film.proj.kernel"].shape == (192, 384)
    assert w["dec_block_1.res_proj.kernel"].shape == (1, 192, 192) and w["dec_block_1.conv.kernel"].shape == (5, 192, 192)
    assert w["upsample.refine.0.kernel"].shape == (5, 192, 192)
    assert w["out_proj.kernel"].shape == (1, 192, 80) and w["residual_proj.kernel"].shape == (192, 256)
    for j in range(4):                                                      # zero-initialised, vae.py:172-178
        assert not w[f"vpflow.ap_{j}.net_post.kernel"].any() and not w[f"vpflow.ap_{j}.net_post.bias"].any()
    assert w["vpflow.ap_1.net_pre.kernel"].any()
    assert not any(k.startswith(("in_proj", "enc_block", "latent_mean", "latent_logvar")) for k in w)
    same = TextConditionedVAE(80, 256, seed=0).weights
    assert all(np.array_equal(w[k], same[k]) for k in w)
    with pytest.raises(ValueError, match="even"):
        TextConditionedVAE(80, 256, latent_dim=5)


def test_npz_round_trip_ignores_encoder_keys_and_rejects_h5(tmp_path):
    vae = make_vae("small")
    vae.save_weights(str(tmp_path / "vae.npz"))
    extra = dict(vae.weights)
    extra["in_proj.kernel"] = np.zeros((1, 20, 48), np.float32)             # encoder side: ignored
    extra["enc_block_0.conv.kernel"] = np.zeros((3, 48, 48), np.float32)
    np.savez(str(tmp_path / "full.npz"), **extra)
    for name in ("vae.npz", "full.npz"):
        other = TextConditionedVAE(**CONFIGS["small"], seed=5)
        other.load_weights(str(tmp_path / name))
        assert all(np.array_equal(other.weights[k], vae.weights[k]) for k in vae.weights)
        assert set(other.weights) == set(vae.weights)
    for suffix in (".weights.h5", ".keras"):
        with pytest.raises(NotImplementedError):
            vae.load_weights(str(tmp_path / f"vae{suffix}"))
        with pytest.raises(NotImplementedError):
            vae.save_weights(str(tmp_path / f"vae{suffix}"))
    bad = dict(vae.weights)
    bad["out_proj.kernel"] = np.zeros((1, 48, 21), np.float32)
    with pytest.raises(ValueError, match="out_proj.kernel"):
        vae.set_weights_dict(bad)
    del bad["out_proj.kernel"]
    with pytest.raises(KeyError):
        vae.set_weights_dict(bad)


def test_training_and_bad_lengths_are_rejected():
    vae = TextConditionedVAE(80, 256, seed=0)
    with pytest.raises(NotImplementedError):
        vae(np.zeros((1, 80, 8), np.float32), np.zeros((1, 8, 256), np.float32), training=True)
    with pytest.raises(NotImplementedError):
        vae.call(np.zeros((1, 80, 8), np.float32), np.zeros((1, 8, 256), np.float32))
    for T in (6, 7, 9):
        with pytest.raises(ValueError, match="multiple of 2\\^down_stages"):
            vae.generate(np.zeros((1, T, 256), np.float32))
    with pytest.raises(ValueError, match="frame_text_cond"):
        vae.generate(np.zeros((1, 8, 255), np.float32))


@pytest.mark.skipif(torch.cuda.is_available(), reason="a HIP device is visible")
def test_no_device_error():
    vae = TextConditionedVAE(**CONFIGS["small"], seed=0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        vae.generate(np.zeros((1, 4, 24), np.float32))


@pytest.mark.parametrize("name", ["default", "small"])
def test_blob_size_matches_the_c_side(name):
    lib = _native.load()
    vae = TextConditionedVAE(**CONFIGS[name], seed=0)
    n = ctypes.c_uint64()
    cfg = vae.native_config()
    assert lib.iris_vae_decoder_weight_count(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == vae.blob_size() == vae.blob().size
    c = vae.get_config()
    C, half, FH, k, S = c["model_channels"], c["latent_dim"] // 2, c["flow_hidden"], c["wavenet_kernel_size"], c["down_stages"]
    formula = (c["cond_dim"] * C + C) + 2 * S * (5 * C * C + C) + c["flow_layers"] * (
        (C * half + half) + (3 * half * FH + FH) + (FH * half + half) + (half * 2 * half + 2 * half)) + (2 * half * C + C) + \
        c["decoder_blocks"] * ((k * C * C + C) + (2 * C * C + 2 * C) + (C * C + C)) + (C * c["n_mels"] + c["n_mels"]) + \
        (C * c["cond_dim"] + c["cond_dim"])
    assert n.value == formula
    # configurations the kernels cannot take
    for field, value, status in (("model_channels", 50, _native.STATUS_UNSUPPORTED), ("cond_dim", 22, _native.STATUS_UNSUPPORTED),
                                 ("model_channels", 260, _native.STATUS_UNSUPPORTED),
                                 ("wavenet_kernel_size", 4, _native.STATUS_UNSUPPORTED),
                                 ("latent_dim", 5, _native.STATUS_INVALID_ARGUMENT)):
        bad = vae.native_config()
        setattr(bad, field, value)
        assert lib.iris_vae_decoder_weight_count(ctypes.byref(bad), ctypes.byref(n)) == status, field
        assert lib.iris_hifigan_last_error()


def test_native_symbols_are_declared_in_the_header():
    header = (Path(__file__).resolve().parents[1] / "include" / "iris_hifigan.h").read_text()
    import re
    declared = set(re.findall(r"\b(iris_vae_decoder_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.VAE_SYMBOLS)
    assert _native.load().iris_hifigan_abi_version() == 4


# ---- the restatement's own conventions ----------------------------------------------------------
def _flow_setup(random_post):
    vae = TextConditionedVAE(**CONFIGS["small"], seed=3)
    if random_post:
        R.randomise(vae, 7)
    rng = np.random.default_rng(0)
    z = rng.standard_normal((2, 9, 4))
    lat_cond = rng.standard_normal((2, 9, 48))
    w = {k: v.astype(np.float64) for k, v in vae.weights.items()}
    return vae.get_config(), w, z, lat_cond


def test_flow_at_zero_init_net_post():
    """net_post is zero at init (vae.py:172-178), so t = 0 before FiLM -- but FiLM then gives gamma * 0 + beta(ce), so the
    reverse flow subtracts the sum of the couplings' beta rows; it is the identity exactly when those are 0."""
    cfg, w, z, lat_cond = _flow_setup(random_post=False)
    betas = 0.0
    for j in range(cfg["flow_layers"]):
        p = f"vpflow.ap_{j}"
        ce = R.gelu(lat_cond @ w[f"{p}.cond_proj.kernel"] + w[f"{p}.cond_proj.bias"])
        betas = betas + (ce @ w[f"{p}.film.proj.kernel"] + w[f"{p}.film.proj.bias"])[..., 2:]
    out = R.flow(w, cfg, z, lat_cond, reverse=True)
    assert np.array_equal(out[..., :2], z[..., :2]) and np.abs(out[..., 2:] - (z[..., 2:] - betas)).max() <= 1e-12
    for j in range(cfg["flow_layers"]):
        w[f"vpflow.ap_{j}.film.proj.kernel"][:, 2:] = 0.0
    assert np.array_equal(R.flow(w, cfg, z, lat_cond, reverse=True), z)           # z == z_prior
    cfg, w, z, lat_cond = _flow_setup(random_post=True)
    for j in range(cfg["flow_layers"]):
        w[f"vpflow.ap_{j}.film.proj.kernel"][:, 2:] = 0.0
        w[f"vpflow.ap_{j}.film.proj.bias"][2:] = 0.0
    out = R.flow(w, cfg, z, lat_cond, reverse=True)                               # random net_post: not the identity
    assert np.array_equal(out[..., :2], z[..., :2]) and np.abs(out[..., 2:] - z[..., 2:]).max() > 1e-2


def test_reverse_flow_inverts_a_forward_flow_written_here():
    cfg, w, z, lat_cond = _flow_setup(random_post=True)
    y = z.copy()
    for j in range(cfg["flow_layers"]):                                      # forward: layers in order, x2 + t
        p = f"vpflow.ap_{j}"
        x1, x2 = y[..., :2], y[..., 2:]
        ce = R.gelu(lat_cond @ w[f"{p}.cond_proj.kernel"] + w[f"{p}.cond_proj.bias"])
        hp = np.pad(x1 + ce, ((0, 0), (1, 1), (0, 0)))
        h = sum(hp[:, kap:kap + 9] @ w[f"{p}.net_pre.kernel"][kap] for kap in range(3)) + w[f"{p}.net_pre.bias"]
        t = R.gelu(h) @ w[f"{p}.net_post.kernel"][0] + w[f"{p}.net_post.bias"]
        gb = ce @ w[f"{p}.film.proj.kernel"] + w[f"{p}.film.proj.bias"]
        y = np.concatenate([x1, x2 + (gb[..., :2] * t + gb[..., 2:])], axis=-1)
    assert np.abs(y - z).max() > 1e-2
    assert np.abs(R.flow(w, cfg, y, lat_cond, reverse=True) - z).max() <= 1e-12
    assert np.abs(R.flow(w, cfg, z, lat_cond, reverse=False) - y).max() <= 1e-12


def test_stride2_same_conv_is_pad_1_2_and_windows():
    rng = np.random.default_rng(1)
    x, k, b = rng.standard_normal((2, 10, 6)), rng.standard_normal((5, 6, 7)), rng.standard_normal(7)
    xp = np.pad(x, ((0, 0), (1, 2), (0, 0)))
    win = np.lib.stride_tricks.sliding_window_view(xp, 5, axis=1)[:, ::2]    # [B, 5, C_in, k]
    assert win.shape == (2, 5, 6, 5)
    want = np.einsum("bick,kco->bio", win, k) + b
    assert np.abs(R.conv1d_same(x, k, b, stride=2) - want).max() <= 1e-12
    assert R.same_pads(10, 5, 2, 1) == (1, 2, 5) and R.same_pads(10, 5, 1, 8) == (16, 16, 10) and R.same_pads(7, 1, 1, 1) == (0, 0, 7)


def test_upsample_is_repeat_then_same_conv():
    vae = TextConditionedVAE(**CONFIGS["small"], seed=3)
    R.randomise(vae, 9)
    w = {k: v.astype(np.float64) for k, v in vae.weights.items()}
    d = np.random.default_rng(2).standard_normal((2, 5, 48))
    rep = np.repeat(d, 2, axis=1)
    assert np.array_equal(R.upsample2x(d), rep)
    xp = np.pad(rep, ((0, 0), (2, 2), (0, 0)))
    want = sum(xp[:, kap:kap + 10] @ w["upsample.refine.0.kernel"][kap] for kap in range(5)) + w["upsample.refine.0.bias"]
    assert np.abs(R.upsample_np(w, vae.get_config(), d) - R.gelu(want)).max() <= 1e-12


def test_restatement_shapes_and_fp32_switch():
    vae = make_vae("small")
    cond, z = make_inputs(vae, 2, 70)
    taps = {}
    mel, res = R.generate_np(vae.weights, vae.get_config(), cond, z, taps=taps)
    assert mel.shape == (2, 20, 70) and res.shape == (2, 70, 24) and mel.dtype == np.float64
    assert taps["lat_cond"].shape == taps["dec_in"].shape == taps["dec_out"].shape == (2, 35, 48)
    mel32, res32 = R.generate_np(vae.weights, vae.get_config(), cond, z, dtype=np.float32)
    assert mel32.dtype == res32.dtype == np.float32
    assert 0 < np.abs(mel32 - mel).max() < 1e-4 * np.abs(mel).max()
    # batch items are independent in the restatement too
    one, _ = R.generate_np(vae.weights, vae.get_config(), cond[1:], z[1:])
    assert np.abs(one[0] - mel[1]).max() <= 1e-12
    assert ("small", 2, 70) in CASES


# ---- pipeline -----------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self, log):
        self.log = log

    def forward(self, mel, lengths=None):
        self.log.append(("forward", tuple(mel.shape)))
        return mel.sum(dim=1).repeat_interleave(2, dim=1)

    def forward_pcm16(self, mel, lengths=None, normalize=False):
        self.log.append(("forward_pcm16", tuple(mel.shape)))
        return (mel.sum(dim=1).repeat_interleave(2, dim=1) * 100).to(torch.int16)

    def forward_resampled(self, mel, resampler, lengths=None, pcm16=False, normalize=False):
        self.log.append(("forward_resampled", resampler, pcm16))
        return mel.sum(dim=1)


def test_infer_from_cond_chains_acoustic_postnet_vocoder():
    log = []

    def acoustic(cond, z_prior):
        log.append(("acoustic", tuple(cond.shape), None if z_prior is None else tuple(z_prior.shape)))
        return torch.ones(cond.shape[0], 4, cond.shape[1]) * cond.sum(dim=2)[:, None, :], "residual"

    def postnet(mel):
        log.append(("postnet", tuple(mel.shape)))
        return mel + 1.0

    eng = _StubEngine(log)
    pipe = MelToWavePipeline(postnet, eng.forward, hop_length=2, chunk_frames=64, acoustic=acoustic)
    cond, z = torch.arange(24, dtype=torch.float32).reshape(1, 8, 3), torch.zeros(1, 2, 4)
    wav = pipe.infer_from_cond(cond, z)
    assert [e[0] for e in log] == ["acoustic", "postnet", "forward"] and log[0] == ("acoustic", (1, 8, 3), (1, 2, 4))
    assert torch.equal(wav, pipe.infer(acoustic(cond, z)[0]))
    del log[:]
    pcm = pipe.infer_from_cond(cond, pcm16=True)
    assert [e[0] for e in log] == ["acoustic", "postnet", "forward_pcm16"] and log[0][2] is None and pcm.dtype == torch.int16
    del log[:]
    marker = object()
    pipe.infer_from_cond(cond, z, resampler=marker, pcm16=True)
    assert log[-1] == ("forward_resampled", marker, True)
    # a TextConditionedVAE-like object is asked for the mel alone
    class _Vae:
        def generate_device(self, cond, z_prior=None, want_residual=True):
            log.append(("generate_device", want_residual))
            return acoustic(cond, z_prior)[0], None
    del log[:]
    MelToWavePipeline(None, eng.forward, hop_length=2, chunk_frames=64, acoustic=_Vae()).infer_from_cond(cond, z)
    assert log[0] == ("generate_device", False)
    with pytest.raises(ValueError, match="acoustic"):
        MelToWavePipeline(None, eng.forward, hop_length=2).infer_from_cond(cond)
    # existing signature unchanged: positional arguments still mean what they meant
    assert MelToWavePipeline(None, eng.forward, None, 2).acoustic is None
