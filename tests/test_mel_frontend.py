"""The mel front-end without a GPU: the float64 restatement (tests/mel_restatement.py) against the rules it is written from
and against a direct O(N^2) DFT, the library's host-only design tables against the restatement, the host logic of the C-ABI
(launch count, workspace, unsupported configs) and of ``iris.mel`` / ``MelToWavePipeline.resynthesize_from_audio``.
The device itself is held to the restatement in tests/test_gpu_mel_frontend.py."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.mel import MelFrontend
from iris.pipeline import MelToWavePipeline

import mel_cases as C
import mel_restatement as R


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_filterbank_shape_support_and_scale():
    fb = R.filterbank(22050, 1024, 80, 0.0, 8000.0)
    assert fb.shape == (80, 513) and fb.dtype == np.float64
    assert (fb >= 0.0).all()
    freqs = np.arange(513) * 22050 / 1024
    assert (fb[:, freqs > 8000.0] == 0.0).all() and (fb[:, 0] == 0.0).all()
    assert (fb.max(axis=1) > 0.0).all()                      # no empty filter at these sizes
    assert float(R.hz_to_mel(1000.0)) == 15.0
    assert np.allclose(R.mel_to_hz(R.hz_to_mel([0.0, 440.0, 1000.0, 4000.0, 8000.0])), [0.0, 440.0, 1000.0, 4000.0, 8000.0], rtol=1e-13)
    # logarithmic above 1000 Hz: 27 mels per factor 6.4
    assert np.isclose(float(R.hz_to_mel(6400.0)), 15.0 + 27.0, rtol=1e-13)
    f = R.mel_edges(80, 0.0, 8000.0)
    assert f.shape == (82,) and f[0] == 0.0 and np.isclose(f[-1], 8000.0, rtol=1e-13) and (np.diff(f) > 0).all()
    g = R.mel_edges(20, 50.0, 8000.0)
    assert np.isclose(g[0], 50.0, rtol=1e-13) and np.isclose(g[-1], 8000.0, rtol=1e-13)


def test_filterbank_rows_are_scaled_by_two_over_their_width():
    """Row i is the unit-height triangle over (f[i], f[i+1], f[i+2]) times 2 / (f[i+2] - f[i])."""
    sr, n_fft, n_mels = 22050, 1024, 80
    fb = R.filterbank(sr, n_fft, n_mels, 0.0, 8000.0)
    f = R.mel_edges(n_mels, 0.0, 8000.0)
    freqs = np.arange(n_fft // 2 + 1) * sr / n_fft
    for i in (0, 1, 17, 40, 79):
        tri = np.interp(freqs, [f[i], f[i + 1], f[i + 2]], [0.0, 1.0, 0.0], left=0.0, right=0.0)
        assert np.allclose(fb[i], tri * 2.0 / (f[i + 2] - f[i]), rtol=1e-9, atol=1e-15), i


def test_window_is_scipys_periodic_hann():
    from scipy.signal import get_window
    for win in (1024, 192, 7):
        assert np.allclose(R.window(win, win), get_window("hann", win, fftbins=True), rtol=0, atol=1e-15)
    w = R.window(256, 192)
    assert w.shape == (256,) and (w[:32] == 0).all() and (w[224:] == 0).all()
    assert np.allclose(w[32:224], get_window("hann", 192, fftbins=True), rtol=0, atol=1e-15)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024])
def test_frame_count(n):
    x = np.ones(n)
    assert R.frames(x, 1024, 256).shape == (1 + n // 256, 1024)
    assert R.mel_np(x).shape == (80, 1 + n // 256)


def test_padding_is_constant_not_reflect():
    """A DC signal: frame 0 sees n_fft / 2 zeros, an interior frame none, so its bin-0 magnitude is smaller (half);
    reflection would make them equal."""
    mag = R.magnitudes(np.ones(4096), 1024, 256, 1024)
    assert mag[0, 0] < 0.51 * mag[8, 0] and np.isclose(mag[8, 0], 512.0)
    fr = R.frames(np.arange(1, 2049, dtype=np.float64), 1024, 256)
    assert (fr[0, :512] == 0).all() and fr[0, 512] == 1.0 and (fr[-1, -512:] == 0).all()


def test_restatement_against_a_direct_dft():
    cfg = dict(n_fft=16, hop=4, win_length=12)
    x = np.random.default_rng(3).standard_normal(37)
    a, b = R.magnitudes(x, **cfg), R.magnitudes_direct(x, **cfg)
    assert a.shape == b.shape == (10, 9)
    assert np.abs(a - b).max() <= 1e-12


# ---- the library's design tables (host only) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "small"])
def test_design_tables(name):
    cfg = C.CONFIGS[name]
    dft, fb = MelFrontend(**cfg).design()
    N, bins = cfg["n_fft"], cfg["n_fft"] // 2 + 1
    assert dft.shape == (2, bins, N) and fb.shape == (cfg["n_mels"], bins) and dft.dtype == fb.dtype == np.float32
    w = R.window(N, cfg["win_length"])
    k, n = np.arange(bins)[:, None], np.arange(N)[None, :]
    ang = 2.0 * np.pi * ((k * n) % N) / N
    assert np.abs(dft[0] - w * np.cos(ang)).max() <= 2.0 ** -24
    assert np.abs(dft[1] - w * np.sin(ang)).max() <= 2.0 ** -24
    assert (dft[1, 0] == 0).all() and (dft[1, -1] == 0).all()          # Im of bins 0 and n_fft / 2
    fb64 = R.filterbank(cfg["sample_rate"], N, cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    ulp = np.spacing(np.abs(fb64).astype(np.float32)).astype(np.float64)
    assert (np.abs(fb.astype(np.float64) - fb64) <= ulp).all()
    assert ((fb == 0) == (fb64 == 0)).all()


def test_fp32_restatement_error_is_small():
    """e32 of the accuracy cases (the GPU test's bar is 4 x their largest): inside the project's 1e-4 claim."""
    worst = max(C.e32_of(name, x) for name, x in C.accuracy_cases())
    assert 0.0 < 4 * worst <= 1e-4


def test_cases_have_bins_on_both_sides_of_the_clip():
    for name, x in C.accuracy_cases():
        cfg = C.CONFIGS[name]
        zf = C.zero_frames(len(x), cfg)
        if len(x) < 4 * cfg["n_fft"]:
            continue
        want = R.mel_np(x, **cfg)
        assert len(zf) >= 2 and (want[:, zf] == np.log(1e-5)).all()
        rest = [t for t in range(want.shape[1]) if t not in zf]
        assert (want[:, rest] > np.log(1e-5)).any()


# ---- host logic of the C-ABI -------------------------------------------------------------------------------------------
def test_launch_count_and_workspace_need_no_device():
    fe = MelFrontend()
    assert fe.launch_count(1, 255744) == 1 and fe.launch_count(8, 8229) == 1 and fe.launch_count(0, 100) == 0
    assert fe.launch_count(1, 0) == 1
    sizes = [fe.workspace_bytes(B, L) for B, L in ((1, 0), (1, 256), (1, 8229), (2, 8229), (8, 262144))]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert MelFrontend(**C.SMALL).launch_count(3, 2085) == 1
    with pytest.raises(_native.NativeCallError) as e:
        fe.launch_count(-1, 10)
    assert e.value.status == _native.STATUS_INVALID_ARGUMENT


@pytest.mark.parametrize("kw,text", [
    (dict(n_fft=1024, hop_length=300), "does not divide"),
    (dict(n_fft=1020, hop_length=102, win_length=1020), "multiple of 4"),
    (dict(n_fft=1024, win_length=1025), "win_length 1025 exceeds n_fft"),
    (dict(n_fft=8192, hop_length=2048, win_length=8192), "n_fft 8192 exceeds 4096"),
    (dict(n_fft=4096, hop_length=1024, win_length=4096), "LDS"),
])
def test_unsupported_configs(kw, text):
    """Every function that takes the config reports it, create before it touches a device."""
    import ctypes
    fe = MelFrontend(**kw)
    lib = _native.load()
    cfg = fe.native_config()
    for call in (lambda: fe.launch_count(1, 4096), lambda: fe.workspace_bytes(1, 4096), fe.design,
                 lambda: _native.check("iris_mel_frontend_create", lib.iris_mel_frontend_create(ctypes.byref(cfg), ctypes.byref(ctypes.c_void_p())))):
        with pytest.raises(_native.NativeCallError) as e:
            call()
        assert e.value.status == _native.STATUS_UNSUPPORTED and text in str(e.value)


def test_mel_frontend_argument_errors():
    for kw in (dict(n_fft=0), dict(hop_length=-4), dict(n_mels=0), dict(sample_rate=2.5), dict(fmin=9000.0), dict(fmax=20000.0),
               dict(fmin=-1.0)):
        with pytest.raises(ValueError):
            MelFrontend(**kw)
    fe = MelFrontend()
    assert fe.frames_of(0) == 1 and fe.frames_of(255) == 1 and fe.frames_of(256) == 2 and fe.frames_of(8229) == 33
    assert fe.get_config() == C.DEFAULT
    for bad in (np.zeros((2, 3, 4), np.float32), np.zeros(7, np.float32), torch.zeros(2, 8, dtype=torch.float64)):
        with pytest.raises(ValueError):
            fe.forward_device(bad)                           # raised before any device is asked for
    assert MelFrontend(fmax=None).native_config().fmax == 0.0


# ---- CPU logic of the pipeline -----------------------------------------------------------------------------------------
HOP, FACTOR = 256, 4


class _Acoustic:
    downsample_factor = FACTOR


class _Frontend:
    """A stand-in with MelFrontend's call surface: 'mel' channel c of frame t is the item's sample t * hop, plus c."""
    hop_length = HOP

    def __init__(self):
        self.calls = []

    def forward_device(self, audio, lengths=None, max_frames=None):
        self.calls.append((tuple(audio.shape), audio.dtype, lengths, max_frames))
        B, L = audio.shape
        T = 1 + L // HOP
        x = torch.nn.functional.pad(audio.to(torch.float32), (0, T * HOP - L))[:, ::HOP][:, :T]
        mel = x[:, None, :] + torch.arange(3, dtype=torch.float32)[None, :, None]
        n = torch.tensor([L] * B if lengths is None else list(lengths))
        frames = 1 + n // HOP
        if max_frames is not None:
            frames = torch.minimum(frames, torch.tensor(list(max_frames)))
        for b in range(B):
            mel[b, :, int(frames[b]):] = 0
        return mel, frames.to(torch.int32)


def _posterior(mel, cond):
    return (mel + cond.transpose(1, 2)[:, :3],)


def _vocode(mel, lengths=None):
    wav = mel.mean(dim=1).repeat_interleave(HOP, dim=1)
    if lengths is not None:
        for b, n in enumerate(lengths):
            wav[b, HOP * int(n):] = 0
    return wav


def _pipe(frontend):
    return MelToWavePipeline(None, _vocode, hop_length=HOP, acoustic=_Acoustic(), posterior=_posterior, frontend=frontend)


def test_resynthesize_from_audio_cpu_logic():
    fe = _Frontend()
    pipe = _pipe(fe)
    rng = np.random.default_rng(5)
    a0, a1 = rng.standard_normal(6400).astype(np.float32), rng.standard_normal(3328).astype(np.float32)
    c0, c1 = rng.standard_normal((24, 5)).astype(np.float32), rng.standard_normal((12, 5)).astype(np.float32)
    # one item: the mel is cut at the conditioning's 24 frames (6400 samples give 26) and handed to resynthesize
    got = pipe.resynthesize_from_audio(a0, c0)
    assert fe.calls[-1] == ((1, 6400), torch.float32, None, [24])
    mel0 = fe.forward_device(torch.from_numpy(a0)[None])[0][:, :, :24]
    assert torch.equal(got, pipe.resynthesize(mel0, torch.from_numpy(c0)[None])) and got.shape == (1, 24 * HOP)
    assert torch.equal(pipe.mel_from_audio(a0), fe.forward_device(torch.from_numpy(a0)[None])[0])
    # lists: ONE front-end call over the padded batch with the items' samples and caps, then resynthesize on a list
    fe.calls.clear()
    outs = pipe.resynthesize_from_audio([a0, a1], [c0, c1])
    assert fe.calls == [((2, 6400), torch.float32, [6400, 3328], [24, 12])]
    mel1 = fe.forward_device(torch.from_numpy(a1)[None])[0][:, :, :12]
    want = pipe.resynthesize([mel0[0], mel1[0]], [c0, c1])
    assert [tuple(o.shape) for o in outs] == [(24 * HOP,), (12 * HOP,)]
    assert all(torch.equal(o, w) for o, w in zip(outs, want))
    assert pipe.resynthesize_from_audio([], []) == []
    # int16 samples reach the front-end as int16
    pipe.resynthesize_from_audio((a0 * 1000).astype(np.int16), c0)
    assert fe.calls[-1][1] == torch.int16


def test_resynthesize_from_audio_argument_errors():
    pipe = _pipe(_Frontend())
    a = np.zeros(6400, np.float32)
    with pytest.raises(ValueError, match="2 waveforms but 1 conditionings"):
        pipe.resynthesize_from_audio([a, a], [np.zeros((24, 5), np.float32)])
    with pytest.raises(ValueError, match="not a multiple of 2\\^down_stages = 4"):
        pipe.resynthesize_from_audio(a, np.zeros((22, 5), np.float32))
    with pytest.raises(ValueError, match="item 1: T = 10 is not a multiple"):
        pipe.resynthesize_from_audio([a, a], [np.zeros((24, 5), np.float32), np.zeros((10, 5), np.float32)])
    with pytest.raises(ValueError, match="6400 samples give 26 frames, the conditioning has 28"):
        pipe.resynthesize_from_audio(a, np.zeros((28, 5), np.float32))
    with pytest.raises(ValueError, match="one waveform"):
        pipe.resynthesize_from_audio(np.zeros((2, 6400), np.float32), np.zeros((24, 5), np.float32))
    with pytest.raises(ValueError, match="needs a mel front-end"):
        _pipe(None).resynthesize_from_audio(a, np.zeros((24, 5), np.float32))
    with pytest.raises(ValueError, match="needs a mel front-end"):
        _pipe(None).mel_from_audio(a)
