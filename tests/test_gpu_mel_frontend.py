"""The mel front-end (iris_mel_frontend_*, ``iris.mel``, ``MelToWavePipeline.resynthesize_from_audio``) on the MI355X, held
to the float64 restatement of librosa 0.11's rules (tests/mel_restatement.py; parity unpinned: librosa cannot be imported
here).  Inputs are tests/mel_cases.py's: three tones, noise and a stretch of exact zeros.

The bar is the project's: ``e32`` = the largest difference between the restatement run in fp32 on the library's own design
tables and itself in float64, relative to ``max(1, max|want|)``, over exactly the cases compared here
(``mel_cases.accuracy_cases()``); the device must stay within ``4 * e32`` -- the factor allows for another summation order
and the device log.  e32 is measured when this module is imported (it depends on the host BLAS's summation order); on the CPU it was
    config   n      e32
    default  0      2.753e-08
    default  255    2.160e-07
    default  256    1.250e-07
    default  1023   7.006e-06
    default  8229   1.236e-05
    default  8229'  1.625e-05   (the second item of the B = 2 call)
    small    2085   1.891e-06
so the bar is 4 x 1.625e-05 = 6.50e-05, inside the project's 1e-4 claim.
Observed on an MI355X over these cases: 2.75e-08 ... 1.46e-05 (largest: default, n = 8229).
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.mel import MelFrontend, compute_mel_spectrogram
from iris.pipeline import MelToWavePipeline

import mel_cases as C
import mel_restatement as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
LOG_CLIP = np.log(np.float32(1e-5))                  # float32

_state = {}


def bar() -> float:
    if "bar" not in _state:
        _state["e32"] = max(C.e32_of(name, x) for name, x in C.accuracy_cases())
        _state["bar"] = 4 * _state["e32"]
        assert 0.0 < _state["bar"] <= 1e-4
    return _state["bar"]


def frontend(name="default") -> MelFrontend:
    if name not in _state:
        _state[name] = MelFrontend(**C.CONFIGS[name])
    return _state[name]


def want_of(name, x):
    """The float64 restatement of one waveform, computed once."""
    key = (name, len(x), float(x.sum()))
    if key not in _state:
        _state[key] = R.mel_np(x, **C.CONFIGS[name])
    return _state[key]


def poison_ws(fe, B, L):
    fe._ensure()
    ws = fe._ws(B, L)
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(NAN)


def check(name, x, got):
    want = want_of(name, x)
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    print(f"{name} n={len(x)}: e_dev={err:.3e} bar={bar():.3e} e32={_state['e32']:.3e}")
    assert err <= bar(), (name, len(x), err, bar())
    zf = C.zero_frames(len(x), C.CONFIGS[name])
    if zf:                                                # all-zero frames: log(1e-5) to 1 ulp
        assert np.abs(got[:, zf] - LOG_CLIP).max() <= np.spacing(np.abs(LOG_CLIP))


@pytest.mark.parametrize("n", C.DENSE_LENGTHS)
def test_dense_default(n):
    fe = frontend()
    x = C.waveform(n, C.DEFAULT)
    poison_ws(fe, 1, n)
    mel, frames = fe.forward_device(x[None])
    assert mel.shape == (1, 80, 1 + n // 256) and frames.tolist() == [1 + n // 256]
    check("default", x, mel[0].cpu().numpy())


def test_dense_batch_of_two():
    fe = frontend()
    xs = [C.waveform(8229, C.DEFAULT), C.waveform(8229, C.DEFAULT, seed=1)]
    mel, _ = fe.forward_device(np.stack(xs))
    assert mel.shape == (2, 80, 33)
    for b in range(2):
        check("default", xs[b], mel[b].cpu().numpy())
        assert torch.equal(mel[b], fe.forward_device(xs[b][None])[0][0])


def test_small_config():
    fe = frontend("small")
    x = C.waveform(C.SMALL_LENGTH, C.SMALL)
    poison_ws(fe, 1, len(x))
    mel, frames = fe.forward_device(x[None])
    assert mel.shape == (1, 20, 33) and frames.tolist() == [33]
    check("small", x, mel[0].cpu().numpy())


def ragged_audio():
    """[4, 8229] with NaN in every sample at or past n_b, and the items' own samples."""
    L = C.RAGGED_L
    items = [C.waveform(n, C.DEFAULT, seed=10 + b) for b, n in enumerate(C.RAGGED_SAMPLES)]
    audio = np.full((len(items), L), np.nan, dtype=np.float32)
    for b, x in enumerate(items):
        audio[b, :len(x)] = x
    return audio, items


@pytest.fixture(scope="module")
def singles():
    """Item b's batch-of-one dense result, computed once."""
    fe = frontend()
    return [fe.forward_device(x[None])[0][0].clone() for x in ragged_audio()[1]]


def test_ragged_items_are_their_batch_of_one(singles):
    fe = frontend()
    audio, _ = ragged_audio()
    poison_ws(fe, 4, C.RAGGED_L)
    mel, frames = fe.forward_device(audio, lengths=list(C.RAGGED_SAMPLES))
    want_frames = [1 + n // 256 for n in C.RAGGED_SAMPLES]
    assert frames.dtype == torch.int32 and frames.tolist() == want_frames == [33, 17, 2, 1]
    assert mel.shape == (4, 80, 33) and not torch.isnan(mel).any()
    for b, t in enumerate(want_frames):
        assert torch.equal(mel[b, :, :t], singles[b]), b
        assert (mel[b, :, t:] == 0).all()


def test_ragged_max_frames(singles):
    fe = frontend()
    audio, _ = ragged_audio()
    mel, frames = fe.forward_device(audio, lengths=torch.tensor(C.RAGGED_SAMPLES, dtype=torch.int32, device=DEV),
                                    max_frames=list(C.RAGGED_CAPS))
    want_frames = [min(1 + n // 256, c) for n, c in zip(C.RAGGED_SAMPLES, C.RAGGED_CAPS)]
    assert frames.tolist() == want_frames == [16, 17, 1, 0]
    for b, t in enumerate(want_frames):
        assert torch.equal(mel[b, :, :t], singles[b][:, :t]), b
        assert (mel[b, :, t:] == 0).all()
    # lengths past L and negative ones are clamped on the device
    mel2, frames2 = fe.forward_device(audio[:1], lengths=[10 ** 6])
    assert frames2.tolist() == [33] and torch.equal(mel2[0], singles[0])
    mel3, frames3 = fe.forward_device(audio[:1], lengths=[-5])
    assert frames3.tolist() == [1] and torch.equal(mel3[0, :, :1], singles[3]) and (mel3[0, :, 1:] == 0).all()


def test_int16_input_is_the_fp32_call_on_x_over_32768():
    fe = frontend()
    x = C.waveform(8229, C.DEFAULT)
    pcm = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    a, _ = fe.forward_device(pcm[None])
    b, _ = fe.forward_device((pcm.astype(np.float32) / np.float32(32768.0))[None])
    assert torch.equal(a, b)
    audio, _ = ragged_audio()
    rag = np.where(np.isnan(audio), 12345, np.clip(np.rint(np.nan_to_num(audio) * 32767.0), -32768, 32767)).astype(np.int16)
    a, fa = fe.forward_device(rag, lengths=list(C.RAGGED_SAMPLES))
    b, fb = fe.forward_device(np.where(np.isnan(audio), np.float32(np.nan), rag.astype(np.float32) / np.float32(32768.0)),
                              lengths=list(C.RAGGED_SAMPLES))
    assert torch.equal(a, b) and torch.equal(fa, fb)


def test_calling_conventions():
    fe = frontend()
    x = torch.from_numpy(C.waveform(8229, C.DEFAULT)[None]).to(DEV)
    first = fe.forward_device(x)[0].clone()
    assert torch.equal(fe.forward_device(x)[0], first)                # two calls in a row: identical bits
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = fe.forward_device(x)[0]
    side.synchronize()
    assert torch.equal(other, first)
    # a too-small workspace: the status code and its message, nothing launched
    lib = _native.load()
    need = fe.workspace_bytes(1, 8229)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    mel = torch.full((1, 80, 33), NAN, dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = lib.iris_mel_frontend_forward(fe._handle, ctypes.c_void_p(x.data_ptr()), _native.MEL_SAMPLES_F32, 1, 8229,
                                       ctypes.c_void_p(mel.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ctypes.c_uint64(need - 1), stream)
    assert rc == _native.STATUS_WORKSPACE_TOO_SMALL
    assert f"workspace has {need - 1} bytes, need {need}" in lib.iris_hifigan_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(mel).all()
    rc = lib.iris_mel_frontend_forward(fe._handle, ctypes.c_void_p(x.data_ptr()), 7, 1, 8229, ctypes.c_void_p(mel.data_ptr()),
                                       ctypes.c_void_p(ws.data_ptr()), ctypes.c_uint64(need), stream)
    assert rc == _native.STATUS_INVALID_ARGUMENT


def test_compute_mel_spectrogram_is_the_drop_in():
    x = C.waveform(8229, C.DEFAULT)
    got = compute_mel_spectrogram(x)
    assert isinstance(got, np.ndarray) and got.shape == (80, 33) and got.dtype == np.float32
    assert np.array_equal(got, frontend().forward_device(x[None])[0][0].cpu().numpy())
    small = compute_mel_spectrogram(C.waveform(C.SMALL_LENGTH, C.SMALL), **C.SMALL)
    assert small.shape == (20, 33)


def test_resynthesize_from_audio_on_a_list():
    """Two recordings of 6400 and 3328 samples with conditionings of 24 and 12 frames: one ragged front-end call, then the
    list form of resynthesize -- bit for bit ``resynthesize`` fed the front-end's own mels."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    from iris.postnet import PostNet
    from vae_posterior_cases import make_inputs, make_pair
    enc, vae = make_pair("default")
    cfg = GeneratorConfig()
    engine = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=1.0), DEV)
    postnet = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    fe = frontend()
    pipe = MelToWavePipeline(postnet, engine.forward, device=DEV, acoustic=vae, posterior=enc, frontend=fe)
    samples, frames = (6400, 3328), (24, 12)
    audios = [C.waveform(n, C.DEFAULT, seed=20 + i) for i, n in enumerate(samples)]
    cond_np = make_inputs(enc, 2, 24)[1]
    conds = [torch.from_numpy(np.ascontiguousarray(cond_np[i, :t])).to(DEV) for i, t in enumerate(frames)]
    calls = []
    inner = fe.forward_device

    def counted(*a, **kw):
        calls.append(kw)
        return inner(*a, **kw)
    pipe.frontend = type("Counted", (), {"forward_device": staticmethod(counted), "hop_length": fe.hop_length})()
    outs = pipe.resynthesize_from_audio(audios, conds)
    assert len(calls) == 1 and calls[0] == {"lengths": list(samples), "max_frames": list(frames)}
    mels = [fe.forward_device(a[None])[0][0, :, :t].contiguous() for a, t in zip(audios, frames)]
    want = pipe.resynthesize(mels, conds)
    assert [tuple(o.shape) for o in outs] == [(t * 256,) for t in frames]
    for o, w in zip(outs, want):
        assert torch.isfinite(o).all() and torch.equal(o, w)
    one = pipe.resynthesize_from_audio(audios[1], conds[1])
    assert torch.equal(one[0], outs[1])
    engine.close()
