"""iris.vae.VAEPosteriorEncoder, ``reconstruct`` and ``MelToWavePipeline.resynthesize`` without a GPU: constructor surface,
weight I/O shared with TextConditionedVAE, argument checks, the blob the C side expects, and the numpy restatement of the
reference's ``call(training=False)`` (tests/vae_posterior_restatement.py) against ``generate_np``."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.pipeline import MelToWavePipeline
from iris.vae import TextConditionedVAE, VAEPosteriorEncoder, reconstruct

import vae_posterior_restatement as P
import vae_restatement as R
from vae_posterior_cases import CASES, CONFIGS, ENC_KEYS, full_config, make_inputs, make_pair


def test_constructor_config_shapes_and_zero_logvar_head():
    enc = VAEPosteriorEncoder(80, 256, seed=0)
    assert enc.get_config() == {"n_mels": 80, "cond_dim": 256, "model_channels": 192, "latent_dim": 16, "num_wavenet_blocks": 8,
                                "wavenet_kernel_size": 5, "down_stages": 2}
    w = enc.weights
    assert w["in_proj.kernel"].shape == (1, 80, 192) and w["in_proj.bias"].shape == (192,)
    assert w["enc_block_7.conv.kernel"].shape == (5, 192, 192) and "enc_block_8.conv.kernel" not in w
    assert w["enc_block_0.film.proj.kernel"].shape == (256, 384) and w["enc_block_0.film.proj.bias"].shape == (384,)
    assert w["enc_block_3.res_proj.kernel"].shape == (1, 192, 192)
    assert w["downsample.blocks.1.kernel"].shape == (5, 192, 192) and "downsample.blocks.2.kernel" not in w
    assert w["latent_mean_proj.kernel"].shape == w["latent_logvar_proj.kernel"].shape == (192, 16)
    assert w["latent_mean_proj.kernel"].any()
    assert not w["latent_logvar_proj.kernel"].any() and not w["latent_logvar_proj.bias"].any()      # vae.py:320-325
    assert not any(k.startswith(("down_cond_proj", "vpflow", "dec_block", "upsample", "out_proj", "residual_proj")) for k in w)
    same = VAEPosteriorEncoder(80, 256, seed=0).weights
    assert all(np.array_equal(w[k], same[k]) for k in w)
    assert enc.downsample_factor == 4


@pytest.mark.parametrize("name", ["default", "small"])
def test_blob_size_matches_the_c_side(name):
    lib = _native.load()
    cfg = CONFIGS[name]
    enc = VAEPosteriorEncoder(**{k: cfg[k] for k in ENC_KEYS if k in cfg}, seed=0)
    n = ctypes.c_uint64()
    c = enc.native_config()
    assert lib.iris_vae_encoder_weight_count(ctypes.byref(c), ctypes.byref(n)) == 0
    assert n.value == enc.blob_size() == enc.blob().size
    g = enc.get_config()
    C, k = g["model_channels"], g["wavenet_kernel_size"]
    formula = (g["n_mels"] * C + C) + g["num_wavenet_blocks"] * ((k * C * C + C) + (g["cond_dim"] * 2 * C + 2 * C) + (C * C + C)) + \
        g["down_stages"] * (5 * C * C + C) + 2 * (C * g["latent_dim"] + g["latent_dim"])
    assert n.value == formula
    for field, value in (("wavenet_kernel_size", 4), ("model_channels", 260), ("n_mels", 22), ("cond_dim", 22), ("model_channels", 50),
                         ("latent_dim", 6)):
        bad = enc.native_config()
        setattr(bad, field, value)
        assert lib.iris_vae_encoder_weight_count(ctypes.byref(bad), ctypes.byref(n)) == _native.STATUS_UNSUPPORTED, field
        assert lib.iris_hifigan_last_error()


def test_native_symbols_are_declared_in_the_header():
    header = (Path(__file__).resolve().parents[1] / "include" / "iris_hifigan.h").read_text()
    declared = set(re.findall(r"\b(iris_vae_encoder_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.VAE_ENCODER_SYMBOLS) and len(declared) == 7
    assert "iris_vae_decoder_forward_posterior" in set(re.findall(r"\b(iris_vae_decoder_[a-z0-9_]+)\s*\(", header))
    assert _native.VAE_SYMBOLS["iris_vae_decoder_forward_posterior"] == _native.VAE_SYMBOLS["iris_vae_decoder_forward"]
    lib = _native.load()
    assert lib.iris_vae_encoder_forward and lib.iris_vae_decoder_forward_posterior
    assert lib.iris_hifigan_abi_version() == 4


def test_one_checkpoint_loads_into_both_classes(tmp_path):
    enc, vae = make_pair("small")
    full = {**enc.weights, **vae.weights}
    assert set(enc.weights) & set(vae.weights) == {"downsample.blocks.0.kernel", "downsample.blocks.0.bias"}
    np.savez(str(tmp_path / "full.npz"), **full)
    cfg = CONFIGS["small"]
    enc2 = VAEPosteriorEncoder(**{k: cfg[k] for k in ENC_KEYS if k in cfg}, seed=9)
    vae2 = TextConditionedVAE(**cfg, seed=9)
    enc2.load_weights(str(tmp_path / "full.npz"))
    vae2.load_weights(str(tmp_path / "full.npz"))
    assert set(enc2.weights) == set(enc.weights) and set(vae2.weights) == set(vae.weights)
    assert all(np.array_equal(enc2.weights[k], enc.weights[k]) for k in enc.weights)
    assert all(np.array_equal(vae2.weights[k], vae.weights[k]) for k in vae.weights)
    enc2.save_weights(str(tmp_path / "enc.npz"))
    enc3 = VAEPosteriorEncoder(**{k: cfg[k] for k in ENC_KEYS if k in cfg}, seed=4)
    enc3.load_weights(str(tmp_path / "enc.npz"))
    assert np.array_equal(enc3.blob(), enc.blob())
    with pytest.raises(KeyError):                          # a decoder-only file lacks the encoder's tensors
        enc3.set_weights_dict(vae.weights)
    with pytest.raises(NotImplementedError):
        enc.load_weights(str(tmp_path / "vae.weights.h5"))


def test_reconstruct_rejects_halves_of_different_models():
    enc, vae = make_pair("small")
    mel, cond = make_inputs(enc, 1, 4)
    cfg = CONFIGS["small"]
    for field, value in (("n_mels", 24), ("cond_dim", 28), ("model_channels", 52), ("latent_dim", 8), ("down_stages", 2)):
        other = VAEPosteriorEncoder(**{**{k: cfg[k] for k in ENC_KEYS if k in cfg}, field: value}, seed=0)
        with pytest.raises(ValueError, match=field):
            reconstruct(other, vae, mel, cond)
    w = dict(enc.weights)
    w["downsample.blocks.0.bias"] = w["downsample.blocks.0.bias"].copy()
    w["downsample.blocks.0.bias"][3] += 1e-3
    enc.set_weights_dict(w)
    with pytest.raises(ValueError, match="downsample.blocks.0.bias"):
        reconstruct(enc, vae, mel, cond)


def test_bad_shapes_are_rejected():
    enc, vae = make_pair("default")
    cond = np.zeros((1, 8, 256), np.float32)
    for T in (6, 7, 9):
        with pytest.raises(ValueError, match="multiple of 2\\^down_stages"):
            enc.encode(np.zeros((1, 80, T), np.float32), np.zeros((1, T, 256), np.float32))
        with pytest.raises(ValueError, match="multiple of 2\\^down_stages"):
            reconstruct(enc, vae, np.zeros((1, 80, T), np.float32), np.zeros((1, T, 256), np.float32))
    with pytest.raises(ValueError, match="mels"):
        enc.encode(np.zeros((1, 8, 80), np.float32), cond)                     # channels-last mel
    with pytest.raises(ValueError, match="mels"):
        enc.encode(np.zeros((80, 8), np.float32), cond)
    with pytest.raises(ValueError, match="frame_text_cond"):
        enc.encode(np.zeros((1, 80, 8), np.float32), np.zeros((1, 12, 256), np.float32))
    with pytest.raises(ValueError, match="frame_text_cond"):
        enc.encode_device(torch.zeros(2, 80, 8), torch.zeros(1, 8, 256))
    with pytest.raises(ValueError, match="expected z"):
        vae.decode_posterior_device(torch.zeros(1, 8, 256), torch.zeros(1, 3, 16))
    with pytest.raises(NotImplementedError):                                   # the decoder class keeps raising
        vae(np.zeros((1, 80, 8), np.float32), cond)


def test_restatement_decoder_half_is_generate_np_after_two_forward_flows():
    """reconstruct_np decodes z_flow = flow_fwd(mean).  generate_np(z_prior) decodes flow_rev(z_prior), and flow_rev inverts
    flow_fwd, so z_prior = flow_fwd(flow_fwd(mean)) must give the same mel and residual up to fp64 round-off.

    The bar, from the magnitudes: inverting one coupling computes (x2 + t) - t', where t' is t recomputed from the same x1
    and lat_cond -- the same numbers, so t' == t -- and leaves at most 2 roundings of size eps/2 * max|z_prior|.  Over
    flow_layers couplings the latent differs by at most flow_layers * eps * max|z_prior|.  The decoder behind it is a
    chain of linear maps, GELUs (slope <= 1.13) and FiLM scalings fixed by cond, so it carries a latent perturbation to
    the output with at most the gain it has on the latent itself times a margin; with gain = max|out| / max|z_flow| and a
    margin of 1e3 for the directions a max-norm gain underestimates, the bar is
    1e3 * flow_layers * eps * max|z_prior| * max(1, max|out| / max|z_flow|) -- 1e-10 to 3e-10 here, against outputs of 1e2."""
    eps = np.finfo(np.float64).eps
    for name, B, T in (("small", 2, 70), ("default", 2, 36)):
        enc, vae = make_pair(name)
        cfg = full_config(enc, vae)
        mel, cond = make_inputs(enc, B, T)
        taps = {}
        recon, (mean, logvar), residual = P.reconstruct_np(enc.weights, vae.weights, cfg, mel, cond, taps=taps)
        f = vae.downsample_factor
        assert recon.shape == (B, enc.n_mels, T) and residual.shape == (B, T, enc.cond_dim) and recon.dtype == np.float64
        assert mean.shape == logvar.shape == (B, T // f, enc.latent_dim) and np.abs(logvar).max() > 0.1
        assert taps["h_in"].shape == taps["h_out"].shape == (B, T, enc.model_channels)
        assert taps["lat_h"].shape == (B, T // f, enc.model_channels)
        wd = {k: v.astype(np.float64) for k, v in vae.weights.items()}
        lat_cond = R.lat_cond_np(wd, cfg, cond.astype(np.float64))
        z_flow = R.flow(wd, cfg, mean, lat_cond, reverse=False)
        assert np.array_equal(z_flow, taps["z_flow"]) and np.abs(z_flow - mean).max() > 1e-2
        z_prior = R.flow(wd, cfg, z_flow, lat_cond, reverse=False)
        want_mel, want_res = R.generate_np(vae.weights, cfg, cond, z_prior)
        for got, want in ((recon, want_mel), (residual, want_res)):
            bar = 1e3 * cfg["flow_layers"] * eps * np.abs(z_prior).max() * max(1.0, np.abs(want).max() / np.abs(z_flow).max())
            err = np.abs(got - want).max()
            print(f"{name} ({B}, {T}): err {err:.3e} bar {bar:.3e} max|out| {np.abs(want).max():.3e}")
            assert err <= bar and bar <= 1e-8 * np.abs(want).max()
        # fp32 switch, and batch items are independent in the restatement too
        r32, (m32, _), _ = P.reconstruct_np(enc.weights, vae.weights, cfg, mel, cond, dtype=np.float32)
        assert r32.dtype == m32.dtype == np.float32 and 0 < np.abs(r32 - recon).max() < 1e-4 * np.abs(recon).max()
        one, (m1, _), _ = P.reconstruct_np(enc.weights, vae.weights, cfg, mel[1:], cond[1:])
        assert np.abs(one[0] - recon[1]).max() <= 1e-9 * np.abs(recon).max() and np.abs(m1[0] - mean[1]).max() <= 1e-9 * np.abs(mean).max()
    assert ("small", 2, 70) in CASES and ("default", 2, 36) in CASES


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


def test_resynthesize_chains_posterior_postnet_vocoder():
    log = []

    def posterior(mel, cond):
        log.append(("posterior", tuple(mel.shape), tuple(cond.shape)))
        return 0.5 * mel + cond.sum(dim=2)[:, None, :], ("mean", "logvar"), "residual"

    def postnet(mel):
        log.append(("postnet", tuple(mel.shape)))
        return mel + 1.0

    eng = _StubEngine(log)
    pipe = MelToWavePipeline(postnet, eng.forward, hop_length=2, chunk_frames=64, posterior=posterior)
    mel, cond = torch.arange(32, dtype=torch.float32).reshape(1, 4, 8), torch.ones(1, 8, 3)
    wav = pipe.resynthesize(mel, cond)
    assert [e[0] for e in log] == ["posterior", "postnet", "forward"] and log[0] == ("posterior", (1, 4, 8), (1, 8, 3))
    assert torch.equal(wav, pipe.infer(posterior(mel, cond)[0])) and not torch.equal(wav, pipe.infer(mel))
    del log[:]
    pcm = pipe.resynthesize(mel, cond, pcm16=True)
    assert [e[0] for e in log] == ["posterior", "postnet", "forward_pcm16"] and pcm.dtype == torch.int16
    with pytest.raises(ValueError, match="posterior"):
        MelToWavePipeline(None, eng.forward, hop_length=2).resynthesize(mel, cond)
    # a VAEPosteriorEncoder needs its decoder, and the pair is checked before any device work
    enc, vae = make_pair("small")
    with pytest.raises(ValueError, match="acoustic"):
        MelToWavePipeline(None, eng.forward, hop_length=2, posterior=enc).resynthesize(mel, cond)
    other = TextConditionedVAE(**{**CONFIGS["small"], "latent_dim": 8}, seed=0)
    with pytest.raises(ValueError, match="latent_dim"):
        MelToWavePipeline(None, eng.forward, hop_length=2, posterior=enc, acoustic=other).resynthesize(
            np.zeros((1, 20, 4), np.float32), np.zeros((1, 4, 24), np.float32))
    # existing signature unchanged
    assert MelToWavePipeline(None, eng.forward, None, 2).posterior is None
