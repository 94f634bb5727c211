"""The Griffin-Lim vocoder without a GPU: the float64 restatement (tests/griffin_lim_restatement.py) against numpy's FFT and
against itself, the library's host-only design tables against the float64 formulas, the mel inversion against scipy's exact
non-negative least squares, the cases of the GPU test (tests/test_gpu_griffin_lim.py), and the host logic of the C-ABI and of
``MelToWavePipeline`` with a whole-utterance vocoder."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.griffin_lim import GriffinLim, pack_phase, start_phase
from iris.pipeline import MelToWavePipeline

import griffin_lim_cases as C
import griffin_lim_restatement as G
import mel_restatement as M


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("small", 3), ("small", 70), ("two_tap", 34), ("default", 5)])
def test_stft_is_rfft_of_the_windowed_zero_padded_frames(name, T):
    n_fft, hop, win = C.stft_args(name)
    y = np.random.default_rng(T).standard_normal(hop * (T - 1))
    padded = np.concatenate([np.zeros(n_fft // 2), y, np.zeros(n_fft // 2)])
    w = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    want = np.stack([np.fft.rfft(padded[t * hop:t * hop + n_fft] * w) for t in range(T)])
    got = G.stft(y, n_fft, hop, win)
    assert got.shape == (T, n_fft // 2 + 1)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(G.stft_direct(y, n_fft, hop, win) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name,T", [("small", 3), ("small", 70), ("two_tap", 34), ("default", 9)])
def test_istft_inverts_stft_where_the_window_sum_is_not_zero(name, T):
    n_fft, hop, win = C.stft_args(name)
    y = np.random.default_rng(100 + T).standard_normal(hop * (T - 1))
    back = G.istft(G.stft(y, n_fft, hop, win), n_fft, hop, win)
    wss = G.window_sumsquare(T, n_fft, hop, win)[n_fft // 2:n_fft // 2 + hop * (T - 1)]
    assert back.shape == y.shape and (wss > G.FLT_MIN).sum() >= len(y) - 1
    assert np.abs(back - y)[wss > G.FLT_MIN].max() <= 1e-10


def test_fp32_restatement_follows_the_float64_one():
    e = C.e32()
    assert all(0.0 < e[k] <= 1e-5 for k in ("S", 0, 1, 2))
    for case, peak in e["peak"].items():                          # the GPU test's bar (d) shows something
        assert 4 * e[2] <= 0.01 * peak, case


# ---- the library's design tables (host only) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_design_tables(name):
    cfg = C.CONFIGS[name]
    N, bins = cfg["n_fft"], cfg["n_fft"] // 2 + 1
    t = C.model(name).design()
    assert t["dft"].shape == t["idft"].shape == (2, bins, N) and t["fb"].shape == (cfg["n_mels"], bins) and t["wsq"].shape == (N,)
    assert all(v.dtype == np.float32 for v in t.values())
    w = M.window(N, cfg["win_length"])
    k, n = np.arange(bins)[:, None], np.arange(N)[None, :]
    ang = 2.0 * np.pi * ((k * n) % N) / N
    f = np.where((k == 0) | (2 * k == N), 1.0, 2.0) / N
    sin = np.where((k * n) % N * 2 % N == 0, 0.0, np.sin(ang))     # sin(0) and sin(pi) are exactly 0, not 1.2e-16
    assert np.array_equal(t["idft"][0], (w * f * np.cos(ang)).astype(np.float32))
    assert np.array_equal(t["idft"][1], (-(w * f * sin)).astype(np.float32))
    assert (t["idft"][1, 0] == 0).all() and (t["idft"][1, -1] == 0).all()
    assert np.array_equal(t["wsq"], (w * w).astype(np.float32))
    from iris.mel import MelFrontend
    dft, fb = MelFrontend(**cfg).design()
    assert np.array_equal(t["dft"], dft) and np.array_equal(t["fb"], fb)
    # the inverse table inverts the forward one: istft_f32(stft_f32(y)) == y to fp32 accuracy
    y = np.random.default_rng(3).standard_normal(cfg["hop_length"] * 8).astype(np.float32)
    re, im = G.stft_f32(y, t["dft"], N, cfg["hop_length"])
    back = G.istft_f32(re, im, t["idft"], t["wsq"], N, cfg["hop_length"])
    wss = G.window_sumsquare(9, N, cfg["hop_length"], cfg["win_length"])[N // 2:N // 2 + len(y)]
    assert np.abs(back - y)[wss > 1e-3].max() <= 1e-4
    P, step = C.model(name).inversion_tables()
    assert P.shape == (bins, cfg["n_mels"]) and P.dtype == np.float32
    assert np.array_equal(P, np.linalg.pinv(fb.astype(np.float64)).astype(np.float32))
    assert step == G.nnls_step(fb.astype(np.float64))


# ---- mel inversion -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_inversion_residual_against_exact_nnls(name):
    """For step 1 / lambda_max the projected-gradient residual never increases and never undercuts the exact optimum."""
    from scipy.optimize import nnls
    case = [c for c in C.CASES if c[0] == name][-1]
    fb = C.fb64(name)
    lm = C.logmel(case)[0]
    m = np.exp(np.clip(lm.astype(np.float64), G.LOG_LO, G.LOG_HI)).T
    floor = np.array([nnls(fb, frame)[1] for frame in m])
    prev = None
    for iters in (0, 8, 32):
        x = G.invert(lm, fb, iters)
        assert (x >= 0).all()
        res = np.linalg.norm(x @ fb.T - m, axis=1)
        assert (res >= floor - 1e-9 * np.linalg.norm(m, axis=1)).all()
        if prev is not None:
            assert (res <= prev * (1 + 1e-12) + 1e-15).all()
        prev = res


# ---- the GPU test's cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=[C.case_id(c) for c in C.CASES])
def test_cases_converge_on_the_restatement(case):
    S, wav = C.restated(case, (0, 32))
    args = C.stft_args(case[0])
    for b in range(case[1]):
        assert G.spectral_convergence(wav[32][b], S[b], *args) < G.spectral_convergence(wav[0][b], S[b], *args)
    if case[0] == "default":
        assert (C.logmel(case) > G.LOG_HI).any()                  # the clip is hit


# ---- host logic of the C-ABI -------------------------------------------------------------------------------------------
def test_launch_count_and_workspace_need_no_device():
    for n_iter in (0, 1, 60):
        gl = GriffinLim(n_iter=n_iter)
        assert gl.launch_count(1, 1000) == gl.launch_count(8, 33) == 2 * n_iter + 2
        assert gl.launch_count(0, 33) == 0
    gl = GriffinLim()
    assert gl.get_config()["n_iter"] == 60 and gl.get_config()["momentum"] == 0.99 and gl.samples_of(33) == 8192
    sizes = [gl.workspace_bytes(B, T) for B, T in ((1, 2), (1, 33), (2, 33), (8, 500))]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert C.model("small").launch_count(1, 3) == 2 * 60 + 2
    for B, T in ((1, 1), (1, 0), (-1, 10)):
        with pytest.raises(_native.NativeCallError) as e:
            gl.launch_count(B, T)
        assert e.value.status == _native.STATUS_INVALID_ARGUMENT


@pytest.mark.parametrize("kw,text", [
    (dict(n_fft=1024, hop_length=300), "does not divide"),
    (dict(n_fft=1024, win_length=1025), "win_length 1025 exceeds n_fft"),
    (dict(n_fft=8192, hop_length=2048, win_length=8192), "n_fft 8192 exceeds 4096"),
    (dict(n_fft=48, hop_length=12, win_length=48, n_mels=8, sample_rate=8000, fmax=None), "multiple of 32"),
    (dict(n_mels=600, fmax=None), "LDS"),
    (dict(n_fft=1024, hop_length=8), "frame window of n_fft 1024, hop_length 8"),      # the front-end and the inversion fit
    (dict(n_fft=2048, hop_length=16, win_length=2048), "frame window"),
])
def test_unsupported_configs(kw, text):
    gl = GriffinLim(**kw)
    lib = _native.load()
    cfg = gl.native_config(with_step=False)
    one = (ctypes.c_float * 1)()
    for call in (lambda: gl.launch_count(1, 33), lambda: gl.workspace_bytes(1, 33), gl.design,
                 lambda: _native.check("iris_griffin_lim_create", lib.iris_griffin_lim_create(ctypes.byref(cfg), one, 1, ctypes.byref(ctypes.c_void_p())))):
        with pytest.raises(_native.NativeCallError) as e:
            call()
        assert e.value.status == _native.STATUS_UNSUPPORTED and text in str(e.value)


def test_argument_errors():
    lib = _native.load()
    gl = GriffinLim()
    null = ctypes.c_void_p(None)
    assert lib.iris_griffin_lim_forward(null, null, null, 1, 33, null, null, 0, null) == _native.STATUS_INVALID_ARGUMENT
    cfg = gl.native_config(with_step=False)
    out = ctypes.c_uint64()
    assert lib.iris_griffin_lim_workspace_bytes(ctypes.byref(cfg), 1, 33, None) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_griffin_lim_create(ctypes.byref(cfg), None, 0, ctypes.byref(ctypes.c_void_p())) == _native.STATUS_INVALID_ARGUMENT
    for field, bad in (("momentum", 1.0), ("momentum", -0.1), ("nnls_step", 0.0), ("n_iter", -1), ("nnls_iters", -1)):
        cfg = gl.native_config(with_step=False)
        setattr(cfg, field, bad)
        assert lib.iris_griffin_lim_workspace_bytes(ctypes.byref(cfg), 1, 33, ctypes.byref(out)) == _native.STATUS_INVALID_ARGUMENT
    for kw in (dict(n_iter=-1), dict(momentum=1.0), dict(nnls_iters=2.5), dict(n_fft=0)):
        with pytest.raises(ValueError):
            GriffinLim(**kw)
    for bad in (np.zeros((80, 33), np.float32), np.zeros((1, 79, 33), np.float32), np.zeros((1, 80, 1), np.float32)):
        with pytest.raises(ValueError):
            gl.forward_device(bad)                                # raised before any device is asked for
    with pytest.raises(ValueError):
        gl.forward_device(np.zeros((1, 80, 33), np.float32), phase0=np.zeros((1, 513, 32)))


def test_config_layout_is_the_c_struct():
    """The offsets csrc/iris_griffin_lim.hip asserts of ``iris_griffin_lim_config``."""
    cfg = _native.GriffinLimConfig
    assert ctypes.sizeof(cfg) == 64
    assert [getattr(cfg, n).offset for n in ("sample_rate", "n_iter", "fmin", "fmax", "nnls_iters", "momentum", "nnls_step")] == \
        [0, 20, 24, 32, 40, 48, 56]
    c = GriffinLim(n_iter=7, momentum=0.5, nnls_iters=3).native_config(with_step=False)
    assert (c.n_iter, c.nnls_iters, c.momentum, c.nnls_step, c.n_fft, c.fmax) == (7, 3, 0.5, 1.0, 1024, 8000.0)


def test_start_phase_and_its_packing():
    phi = start_phase(2, 5, 3, seed=1337)
    assert np.array_equal(phi, 2.0 * np.pi * np.random.default_rng(1337).random((2, 5, 3)))
    packed = pack_phase(phi)
    assert packed.shape == (2, 3, 5, 2) and packed.dtype == np.float32 and packed.flags.c_contiguous
    assert packed[1, 2, 4, 0] == np.float32(np.cos(phi[1, 4, 2])) and packed[1, 2, 4, 1] == np.float32(np.sin(phi[1, 4, 2]))


# ---- CPU logic of the pipeline -----------------------------------------------------------------------------------------
class _Whole:
    """A stand-in with GriffinLim's call surface: hop (T - 1) samples, sample i of an item is the mean of frame i // hop."""
    whole_utterance = True
    hop_length = 4

    def forward_device(self, mel):
        return mel.mean(dim=1)[:, :-1].repeat_interleave(self.hop_length, dim=1)


def test_pipeline_takes_the_length_from_a_whole_utterance_vocoder():
    voc = _Whole()
    pipe = MelToWavePipeline(None, voc)
    assert pipe.streamer.hop_length == 4
    mel = torch.arange(2 * 3 * 6, dtype=torch.float32).reshape(2, 3, 6)
    out = pipe.infer(mel)
    assert out.shape == (2, 4 * 5) and torch.equal(out, voc.forward_device(mel))
    outs = pipe.infer_batch([mel[0], mel[1]])
    assert len(outs) == 2 and torch.equal(outs[1], out[1])
    with pytest.raises(NotImplementedError, match="one length"):
        pipe.infer_batch([mel[0], mel[1][:, :4]])
    with pytest.raises(NotImplementedError):
        next(pipe.stream(mel))
    with pytest.raises(NotImplementedError):
        pipe.session()
    with pytest.raises(ValueError, match="normalize=True goes with pcm16=True"):
        pipe.infer(mel, normalize=True)


class _Resampler:
    """A stand-in with ``Resampler.forward``'s call surface: every second sample."""

    def forward(self, wav, pcm16=False, normalize=False):
        out = wav[:, ::2]
        return (out * 100).to(torch.int16) if pcm16 else out


def test_pipeline_stages_around_a_whole_utterance_vocoder():
    """``infer_from_cond`` and ``resampler=``: the acoustic stage's mel goes through in one call and the resampler gets the
    waveform as it is, whatever its length."""
    voc = _Whole()
    acoustic = lambda cond, z: (cond.transpose(1, 2)[:, :3] + (0 if z is None else z),)
    pipe = MelToWavePipeline(lambda mel, lengths=None: mel + 1, voc, acoustic=acoustic)
    cond = torch.arange(2 * 6 * 5, dtype=torch.float32).reshape(2, 6, 5)
    wav = voc.forward_device(cond.transpose(1, 2)[:, :3] + 1)
    assert wav.shape == (2, 20) and torch.equal(pipe.infer_from_cond(cond), wav)
    rs = _Resampler()
    assert torch.equal(pipe.infer_from_cond(cond, resampler=rs), wav[:, ::2])
    assert torch.equal(pipe.infer(cond.transpose(1, 2)[:, :3], resampler=rs, pcm16=True), (wav[:, ::2] * 100).to(torch.int16))
    outs = pipe.infer_batch([cond[0].T[:3], cond[1].T[:3]], resampler=rs)
    assert len(outs) == 2 and torch.equal(outs[0], wav[0, ::2])
