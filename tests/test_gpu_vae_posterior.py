"""The device VAE posterior encoder and the forward-flow decode (iris.vae.VAEPosteriorEncoder, reconstruct; csrc/
iris_vae_encoder.hip, vae_decoder.h) on the MI355X against the float64 restatement of the reference's
``TextConditionedVAE.call(training=False)`` (tests/vae_posterior_restatement.py).  Every parameter is randomised.

The bar is measured, not guessed.  For exactly the inputs of vae_posterior_cases.CASES,
``e32 = max|reconstruct_np(fp32) - reconstruct_np(fp64)| / max(1, max|fp64|)`` on the CPU was
    config   (B, T)     mean       logvar     recon      residual   h_in       h_out      lat_h
    default  (1, 4)     1.121e-06  1.111e-06  1.235e-06  1.039e-06  2.909e-07  7.014e-07  9.365e-07
    default  (2, 36)    8.516e-07  1.063e-06  1.106e-06  1.319e-06  3.262e-07  8.909e-07  8.759e-07
    default  (3, 132)   9.655e-07  1.426e-06  1.176e-06  1.065e-06  3.544e-07  1.045e-06  9.276e-07
    default  (1, 260)   9.216e-07  1.280e-06  1.522e-06  1.545e-06  2.943e-07  9.364e-07  1.024e-06
    small    (3, 6)     2.567e-07  4.192e-07  4.546e-07  5.518e-07  1.331e-07  3.058e-07  2.878e-07
    small    (2, 70)    4.283e-07  3.072e-07  5.563e-07  5.095e-07  1.734e-07  4.773e-07  4.035e-07
so the bar is 4 x 1.545e-06 = 6.18e-06: the project's convention for the PostNet, VAE and text stages -- the device's fp32
summation order (MFMA fragments) and tanhf differ from numpy's by about that much.
Observed on an MI355X over these cases and tensors: 1.1e-07 ... 2.59e-06 (largest: recon, default (1, 260)).
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
from iris.vae import VAEPosteriorEncoder, reconstruct

import vae_posterior_restatement as P
from vae_posterior_cases import CASES, CONFIGS, ENC_KEYS, full_config, make_inputs, make_pair

pytestmark = pytest.mark.gpu

E32_MAX = 1.545e-06            # the largest e32 of the table above (residual, default (1, 260))
BAR = 4 * E32_MAX
assert BAR <= 1e-4

DEV = torch.device("cuda", 0)
TAPS = (("h_in", _native.VAE_ENC_TAP_H_IN), ("h_out", _native.VAE_ENC_TAP_H_OUT), ("lat_h", _native.VAE_ENC_TAP_LAT_H))


def _err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))


def _nan_ws(model, B, T):
    model._ensure()
    ws = model._ws(B, T)
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


def _encode(enc, mel, cond):
    """iris_vae_encoder_forward into a workspace and outputs that hold NaN."""
    lib = _native.load()
    B, T = mel.shape[0], mel.shape[2]
    ws = _nan_ws(enc, B, T)
    mean = torch.full((B, T // enc.downsample_factor, enc.latent_dim), float("nan"), device=DEV)
    logvar = torch.full_like(mean, float("nan"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.iris_vae_encoder_forward(enc._handle, p(mel), p(cond), B, T, p(mean), p(logvar), p(ws), ctypes.c_uint64(ws.numel()),
                                      ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, lib.iris_hifigan_last_error()
    return mean, logvar


def _decode(vae, cond, z, posterior=True):
    """iris_vae_decoder_forward_posterior (or _forward) into a workspace and outputs that hold NaN."""
    lib = _native.load()
    B, T = cond.shape[0], cond.shape[1]
    ws = _nan_ws(vae, B, T)
    mel = torch.full((B, vae.n_mels, T), float("nan"), device=DEV)
    res = torch.full((B, T, vae.cond_dim), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fn = lib.iris_vae_decoder_forward_posterior if posterior else lib.iris_vae_decoder_forward
    rc = fn(vae._handle, p(cond), p(z), B, T, p(mel), p(res), p(ws), ctypes.c_uint64(ws.numel()),
            ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, lib.iris_hifigan_last_error()
    return mel, res


@pytest.fixture(scope="module")
def pairs():
    return {name: make_pair(name) for name in CONFIGS}


@pytest.fixture(scope="module")
def reference(pairs):
    """case -> (mel, cond, recon64, mean64, logvar64, residual64, taps64), computed once."""
    cache = {}

    def get(name, B, T):
        if (name, B, T) not in cache:
            enc, vae = pairs[name]
            mel, cond = make_inputs(enc, B, T)
            taps = {}
            recon, (mean, logvar), res = P.reconstruct_np(enc.weights, vae.weights, full_config(enc, vae), mel, cond, taps=taps)
            cache[(name, B, T)] = (mel, cond, recon, mean, logvar, res, taps)
        return cache[(name, B, T)]
    return get


def _dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


@pytest.mark.parametrize("name,B,T", CASES)
def test_restatement_parity(pairs, reference, name, B, T):
    enc, vae = pairs[name]
    mel_np, cond_np, want_recon, want_mean, want_logvar, want_res, want_taps = reference(name, B, T)
    mel, cond = _dev(mel_np, cond_np)
    mean, logvar = _encode(enc, mel, cond)
    errs = {"mean": _err(mean.cpu().numpy(), want_mean), "logvar": _err(logvar.cpu().numpy(), want_logvar)}
    for key, which in TAPS:
        got = enc._read_tap(which, B, T).cpu().numpy()
        assert got.shape == want_taps[key].shape, key
        errs[key] = _err(got, want_taps[key])
    recon, res = _decode(vae, cond, mean)
    assert tuple(recon.shape) == want_recon.shape and tuple(res.shape) == want_res.shape
    errs["recon"], errs["residual"] = _err(recon.cpu().numpy(), want_recon), _err(res.cpu().numpy(), want_res)
    print(f"{name} ({B}, {T}):", {k: f"{v:.3e}" for k, v in errs.items()}, f"bar {BAR:.3e}")
    assert all(np.isfinite(v) and v <= BAR for v in errs.values()), (errs, BAR)


@pytest.mark.parametrize("name,B,T", [("default", 2, 36), ("small", 2, 70)])
def test_forward_flow_equals_reverse_flow_when_t_is_zero(pairs, name, B, T):
    """FiLM of every coupling zeroed: t = 0 * net + 0 = +0 in both directions, x2 + 0 == x2 - 0 == x2 (z holds no -0)."""
    from iris.vae import TextConditionedVAE
    _, src = pairs[name]
    vae = TextConditionedVAE(**CONFIGS[name], seed=1)
    w = dict(src.weights)
    for j in range(vae.flow_layers):
        for leaf in ("kernel", "bias"):
            w[f"vpflow.ap_{j}.film.proj.{leaf}"] = np.zeros_like(w[f"vpflow.ap_{j}.film.proj.{leaf}"])
    vae.set_weights_dict(w)
    rng = np.random.default_rng(5)
    cond_np = rng.standard_normal((B, T, vae.cond_dim)).astype(np.float32)
    z_np = rng.standard_normal((B, T // vae.downsample_factor, vae.latent_dim)).astype(np.float32)
    assert not np.signbit(z_np[z_np == 0]).any()
    cond, z = _dev(cond_np, z_np)
    vae._ensure()
    mel_f, res_f = _decode(vae, cond, z, posterior=True)
    mel_r, res_r = _decode(vae, cond, z, posterior=False)
    assert bool(torch.isfinite(mel_f).all()) and torch.equal(mel_f, mel_r) and torch.equal(res_f, res_r)
    mel_p, res_p = vae.decode_posterior_device(cond, z)
    mel_g, res_g = vae.generate_device(cond, z)
    assert torch.equal(mel_p, mel_g) and torch.equal(res_p, res_g) and torch.equal(mel_p, mel_f)
    # with the FiLM back the two directions differ: the instantiation is not the reverse one under another name
    mel_s, _ = src.decode_posterior_device(cond, z)
    mel_t, _ = src.generate_device(cond, z)
    assert not torch.equal(mel_s, mel_t)


def test_batch_independence_and_determinism(pairs, reference):
    enc, vae = pairs["default"]
    mel_np, cond_np, *_ = reference("default", 3, 132)
    mel, cond = _dev(mel_np, cond_np)
    mean, logvar = _encode(enc, mel, cond)
    mean2, logvar2 = _encode(enc, mel, cond)
    assert torch.equal(mean, mean2) and torch.equal(logvar, logvar2)
    recon, res = _decode(vae, cond, mean)
    recon2, res2 = _decode(vae, cond, mean)
    assert torch.equal(recon, recon2) and torch.equal(res, res2)
    for b in range(3):
        m_b, l_b = _encode(enc, mel[b:b + 1].contiguous(), cond[b:b + 1].contiguous())
        assert torch.equal(m_b[0], mean[b]) and torch.equal(l_b[0], logvar[b]), b
        r_b, s_b = _decode(vae, cond[b:b + 1].contiguous(), mean[b:b + 1].contiguous())
        assert torch.equal(r_b[0], recon[b]) and torch.equal(s_b[0], res[b]), b


def test_inputs_are_not_written(pairs, reference):
    enc, _ = pairs["small"]
    mel_np, cond_np, *_ = reference("small", 2, 70)
    mel, cond = _dev(mel_np, cond_np)
    mean, _ = enc.encode_device(mel, cond)
    assert mel.data_ptr() != mean.data_ptr()
    assert np.array_equal(mel.cpu().numpy(), mel_np) and np.array_equal(cond.cpu().numpy(), cond_np)


def test_plan_and_workspace(pairs):
    lib = _native.load()
    for name in CONFIGS:
        enc, vae = pairs[name]
        f = enc.downsample_factor
        assert enc.launch_count(2, 8 * f) == enc.num_wavenet_blocks + enc.down_stages + 3, name
        assert enc.launch_count(0, 8 * f) == 0
        # the posterior decode runs generate's plan: launch_count's dry run is the code both forwards execute
        c = vae.get_config()
        assert vae.launch_count(2, 8 * f) == 3 + 2 * c["down_stages"] + c["decoder_blocks"] + 2
    enc, vae = pairs["default"]
    assert enc.launch_count(1, 1024) == 13
    small, large = enc.workspace_bytes(1, 64), enc.workspace_bytes(2, 64)
    assert 0 < small < large < enc.workspace_bytes(2, 128) and large >= 2 * 64 * (8 * 2 * 192 + 3 * 192) * 4
    mel, cond = torch.zeros(1, 80, 8, device=DEV), torch.zeros(1, 8, 256, device=DEV)
    need = enc.workspace_bytes(1, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    sentinel = 12345.0
    mean, logvar = torch.full((1, 2, 16), sentinel, device=DEV), torch.full((1, 2, 16), sentinel, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def forward(T, ws_bytes):
        return lib.iris_vae_encoder_forward(enc._handle, p(mel), p(cond), 1, T, p(mean), p(logvar), p(ws), ctypes.c_uint64(ws_bytes), stream)
    assert forward(6, need) == _native.STATUS_INVALID_ARGUMENT and b"multiple" in lib.iris_hifigan_last_error()
    assert forward(8, need - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize(DEV)
    assert bool((mean == sentinel).all()) and bool((logvar == sentinel).all())
    assert forward(8, need) == 0
    torch.cuda.synchronize(DEV)
    assert not bool((mean == sentinel).any()) and not bool((logvar == sentinel).any())
    # the posterior decode takes generate's workspace, and not a byte less
    z, cond8 = torch.zeros(1, 2, 16, device=DEV), torch.zeros(1, 8, 256, device=DEV)
    vneed = vae.workspace_bytes(1, 8)
    vws = torch.empty(vneed, dtype=torch.uint8, device=DEV)
    out_mel, out_res = torch.full((1, 80, 8), sentinel, device=DEV), torch.full((1, 8, 256), sentinel, device=DEV)
    args = (vae._handle, p(cond8), p(z), 1, 8, p(out_mel), p(out_res), p(vws))
    assert lib.iris_vae_decoder_forward_posterior(*args, ctypes.c_uint64(vneed - 1), stream) == _native.STATUS_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize(DEV)
    assert bool((out_mel == sentinel).all())
    assert lib.iris_vae_decoder_forward_posterior(*args, ctypes.c_uint64(vneed), stream) == 0
    torch.cuda.synchronize(DEV)
    assert not bool((out_mel == sentinel).any()) and not bool((out_res == sentinel).any())


def test_create_time_refusals(pairs):
    lib = _native.load()
    enc, _ = pairs["default"]
    blob = enc.blob()
    fp = ctypes.POINTER(ctypes.c_float)
    h = ctypes.c_void_p()
    with torch.cuda.device(DEV):
        for field, value in (("wavenet_kernel_size", 4), ("model_channels", 260), ("n_mels", 22)):
            bad = enc.native_config()
            setattr(bad, field, value)
            assert lib.iris_vae_encoder_create(ctypes.byref(bad), blob.ctypes.data_as(fp), ctypes.c_uint64(blob.size),
                                               ctypes.byref(h)) == _native.STATUS_UNSUPPORTED, field
            assert not h.value and lib.iris_hifigan_last_error()
        cfg = enc.native_config()
        assert lib.iris_vae_encoder_create(ctypes.byref(cfg), blob.ctypes.data_as(fp), ctypes.c_uint64(blob.size - 1),
                                           ctypes.byref(h)) == _native.STATUS_INVALID_ARGUMENT
        assert b"weight blob" in lib.iris_hifigan_last_error() and not h.value


def test_chain(pairs, reference):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    from iris.postnet import PostNet
    enc, vae = pairs["default"]
    mel_np, cond_np, want_recon, want_mean, *_ = reference("default", 2, 36)
    mel, cond = _dev(mel_np, cond_np)
    mean, logvar = enc.encode_device(mel, cond)
    want, want_res = vae.decode_posterior_device(cond, mean)
    recon, (m, lv), res = reconstruct(enc, vae, mel, cond)
    assert torch.equal(recon, want) and torch.equal(res, want_res) and torch.equal(m, mean) and torch.equal(lv, logvar)
    assert recon.is_contiguous() and tuple(recon.shape) == (2, 80, 36)
    r_np, (m_np, _), _ = reconstruct(enc, vae, mel_np, cond_np)                     # numpy in -> numpy out
    assert isinstance(r_np, np.ndarray) and np.array_equal(r_np, recon.cpu().numpy()) and np.array_equal(m_np, mean.cpu().numpy())
    assert _err(r_np, want_recon) <= BAR and _err(m_np, want_mean) <= BAR
    m_host, _ = enc.encode(mel_np, cond_np)
    assert np.array_equal(m_host, m_np)
    cfg = GeneratorConfig()
    engine = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=1.0), DEV)
    postnet = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    pipe = MelToWavePipeline(postnet, engine.forward, device=DEV, acoustic=vae, posterior=enc)
    # one utterance, scaled into the vocoder's range
    one_mel, one_cond = mel[:1].contiguous(), cond[:1].contiguous()
    one = reconstruct(enc, vae, one_mel, one_cond)[0]
    want_wav = pipe.infer(one).clone()
    got = pipe.resynthesize(one_mel, one_cond)
    assert tuple(got.shape) == (1, 36 * 256) and torch.equal(got, want_wav)
    want_pcm = pipe.infer(one, pcm16=True).clone()
    assert torch.equal(pipe.resynthesize(one_mel, one_cond, pcm16=True), want_pcm)
