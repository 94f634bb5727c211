"""The bias denoiser (``iris.denoiser``, iris_denoiser_*, csrc/denoiser.h) without a GPU: the float64 restatement of its math
(tests/denoiser_restatement.py) holds the properties the stage promises, the cases of tests/denoiser_cases.py exercise both
branches of the clamp, and the host-only half of the C-ABI -- symbols, launch counts, workspace layout, refusals -- answers as
include/iris_hifigan.h says.  The device itself is tests/test_gpu_denoiser.py's."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import Denoiser
from iris.pipeline import MelToWavePipeline

import denoiser_cases as C
import denoiser_restatement as D
import griffin_lim_restatement as G

REPO = Path(__file__).resolve().parents[1]
CASE_IDS = [C.case_id(c) for c in C.CASES]


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_inputs_and_clamp_share(case):
    name, B, M = case
    n_fft, hop, win = C.stft_args(name)
    wav = C.waveform(case)
    assert wav.shape == (B, hop * M) and wav.dtype == np.float32 and np.abs(wav).max() <= C.PEAK
    bias = C.bias(case)
    assert bias.shape == (n_fft // 2 + 1,) and bias.dtype == np.float32 and np.isfinite(bias).all() and (bias >= 0).all()
    clamped = total = 0
    for y in wav:
        re, im = D.stft_parts(y, n_fft, hop, win)
        assert re.shape == (M + 1, n_fft // 2 + 1)
        cl = D.subtract(re, im, bias, C.STRENGTH)[2]
        clamped, total = clamped + int(cl.sum()), total + cl.size
    share = clamped / total
    print(f"{C.case_id(case)}: clamped share {share:.3f}")
    assert 0.2 <= share <= 0.8


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_strength_zero_is_the_identity(case):
    name, _, M = case
    n_fft, hop, win = C.stft_args(name)
    wss = G.window_sumsquare(M + 1, n_fft, hop, win)[n_fft // 2:n_fft // 2 + hop * M]
    for y in C.waveform(case):
        out = D.denoise(y, C.bias(case), 0.0, n_fft, hop, win)
        live = wss > G.FLT_MIN
        assert live.any()
        assert np.abs(out - y)[live].max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_magnitudes_shrink_and_phase_stays(case):
    n_fft, hop, win = C.stft_args(case[0])
    for y in C.waveform(case):
        re, im = D.stft_parts(y, n_fft, hop, win)
        cre, cim, clamped = D.subtract(re, im, C.bias(case), C.STRENGTH)
        a, c = re + 1j * im, cre + 1j * cim
        assert (np.abs(c) <= np.abs(a)).all()
        assert (c[clamped] == 0).all()
        live = np.abs(c) > 0
        assert live.any() and not live.all()
        # the same direction: c / |c| == a / |a|
        assert np.abs(c[live] / np.abs(c[live]) - a[live] / np.abs(a[live])).max() <= 1e-12


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_large_strength_gives_exact_zero(case, dtype):
    name = case[0]
    kw = dict(dtype=np.float32, tables=C.tables(name)) if dtype == np.float32 else {}
    bias = np.maximum(C.bias(case), np.float32(1e-3))
    mag = C.magnitudes64(case)
    strength = 2.0 * float((mag / bias[None, None, :]).max())
    for y in C.waveform(case):
        out = D.denoise(y, bias, strength, *C.stft_args(name), **kw)
        assert out.dtype == dtype and np.array_equal(out, np.zeros_like(out))


def test_bias_of_a_stationary_tone_peaks_at_its_bin():
    n_fft, hop, win = C.stft_args("small")
    k0 = 5
    y = 0.5 * np.sin(2.0 * np.pi * k0 * np.arange(hop * 40) / n_fft)
    for kw in ({}, dict(dtype=np.float32, tables=C.tables("small"))):
        bias = D.estimate_bias(y, n_fft, hop, win, **kw)
        assert bias.shape == (n_fft // 2 + 1,) and int(np.argmax(bias)) == k0
        # a Hann window of `win` samples gives the tone's bin about amplitude * win / 4
        assert abs(float(bias[k0]) - 0.5 * win / 4) <= 0.05 * 0.5 * win / 4
    lo, hi = D.interior(41, n_fft, hop)
    assert (lo, hi) == (2, 39)
    with pytest.raises(ValueError):
        D.estimate_bias(y[:hop * 2], n_fft, hop, win)


def test_e32_is_measurable():
    e = C.e32()
    print("e32:", {k: f"{e[k]:.3e}" for k in ("out", "bias")})
    assert 0.0 < e["out"] < 1e-4 and 0.0 < e["bias"] < 1e-4
    assert sum("bias" in row for row in e["per_case"].values()) == 4         # every case but the one with fewer frames than taps


# ---- the C-ABI, host only ----------------------------------------------------------------------------------------------
def test_symbols_declared_and_loadable():
    header = (REPO / "include" / "iris_hifigan.h").read_text()
    declared = set(re.findall(r"\b(iris_denoiser_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.DENOISER_SYMBOLS)
    assert {"iris_denoiser_create", "iris_denoiser_destroy", "iris_denoiser_set_bias", "iris_denoiser_estimate_bias",
            "iris_denoiser_forward", "iris_denoiser_workspace_bytes", "iris_denoiser_launch_count"} <= declared
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert len(_native.DENOISER_SYMBOLS["iris_denoiser_forward"][1]) == 10


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_launch_counts_and_workspace_layout(case):
    name, B, M = case
    n_fft, hop, win = C.stft_args(name)
    dn = Denoiser(n_fft, hop, win)
    L = hop * M
    assert dn.launch_count(B, L) == 2
    assert dn.launch_count(0, L) == 0 and dn.launch_count(B, 0) == 0
    if C.restated_bias(case) is not None:
        assert dn.estimate_launch_count(L) == 2
    layout, floats = dn._workspace_layout(B, L)
    qp = (n_fft + 2 + 7) // 8 * 8
    assert layout["c"] == (0, (B, M + 1, qp))
    assert layout["frames"][0] == (B * (M + 1) * qp + 63) // 64 * 64 and floats == layout["frames"][0] + 64
    assert dn.workspace_bytes(B, L) == 4 * floats
    # the estimator's magnitudes [T, Ks] fit the workspace of a forward of shape (1, L)
    assert (M + 1) * ((n_fft // 2 + 1 + 3) // 4 * 4) * 4 <= dn.workspace_bytes(1, L)


def _status(fn, *args):
    with pytest.raises(_native.NativeCallError) as err:
        fn(*args)
    return err.value.status


def test_host_only_refusals():
    dn = Denoiser()
    assert _status(dn.launch_count, 1, 256 * 10 + 1) == _native.STATUS_INVALID_ARGUMENT          # L is no multiple of hop
    assert _status(dn.workspace_bytes, 1, 255) == _native.STATUS_INVALID_ARGUMENT
    assert _status(dn.workspace_bytes, -1, 256) == _native.STATUS_INVALID_ARGUMENT
    assert _status(dn.launch_count, 1, -256) == _native.STATUS_INVALID_ARGUMENT
    assert _status(dn.launch_count, 65536, 256) == _native.STATUS_UNSUPPORTED
    assert dn.launch_count(65535, 256) == 2
    assert _status(dn.estimate_launch_count, 256 * 3) == _native.STATUS_INVALID_ARGUMENT         # T = 4: no interior frame
    assert dn.estimate_launch_count(256 * 4) == 2                                                # T = 5: frame 2
    # the front-end's unsupported configs and the Griffin-Lim stage's
    for bad in (Denoiser(1024, 300, 1024), Denoiser(1024, 254, 1024), Denoiser(1024, 256, 2048), Denoiser(8192, 256, 1024),
                Denoiser(48, 12, 48), Denoiser(4096, 4, 4096)):
        assert _status(bad.launch_count, 1, bad.hop_length * 8) == _native.STATUS_UNSUPPORTED, bad.get_config()
        assert _status(bad.workspace_bytes, 1, bad.hop_length * 8) == _native.STATUS_UNSUPPORTED
    lib = _native.load()
    n = ctypes.c_int32()
    assert lib.iris_denoiser_launch_count(None, 1, 256, ctypes.byref(n)) == _native.STATUS_INVALID_ARGUMENT
    cfg = dn.native_config()
    assert lib.iris_denoiser_launch_count(ctypes.byref(cfg), 1, 256, None) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_denoiser_workspace_bytes(ctypes.byref(cfg), 1, 256, None) == _native.STATUS_INVALID_ARGUMENT
    # a NULL handle is refused before anything else is looked at; nothing needs a device
    assert lib.iris_denoiser_forward(None, None, 1, 256, None, 0.1, None, None, 0, None) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_denoiser_estimate_bias(None, None, 256 * 8, None, None, 0, None) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_denoiser_set_bias(None, None, None) == _native.STATUS_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.iris_denoiser_create(ctypes.byref(cfg), None, None) == _native.STATUS_INVALID_ARGUMENT
    bad_bias = np.zeros(513, np.float32)
    bad_bias[7] = -1.0
    assert lib.iris_denoiser_create(ctypes.byref(cfg), bad_bias.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    ctypes.byref(h)) == _native.STATUS_INVALID_ARGUMENT
    assert not h.value


def test_python_argument_checks():
    with pytest.raises(ValueError):
        Denoiser(strength=-0.1)
    with pytest.raises(ValueError):
        Denoiser(strength=float("nan"))
    with pytest.raises(ValueError):
        Denoiser(bias=np.zeros(512, np.float32))
    with pytest.raises(ValueError):
        Denoiser(bias=np.full(513, np.inf, np.float32))
    with pytest.raises(ValueError):
        Denoiser(n_fft=0)
    dn = Denoiser(strength=0.25)
    assert dn.n_bins == 513 and dn.get_config()["strength"] == 0.25
    with pytest.raises(ValueError):                            # before any device work: L is no multiple of hop
        dn.forward_device(np.zeros((1, 1000), np.float32))
    with pytest.raises(ValueError):
        dn.forward_device(np.zeros((1, 1024), np.float32), strength=-1.0)
    with pytest.raises(ValueError):
        dn.forward_device(np.zeros((2, 1024), np.float32), lengths=[1, 5])
    with pytest.raises(ValueError):
        dn.estimate_bias(np.zeros((1, 256 * 3), np.float32))


# ---- the pipeline ------------------------------------------------------------------------------------------------------
class _Vocode:
    cfg = None

    def __init__(self):
        self.calls = []

    def forward(self, mel, lengths=None):
        self.calls.append(("forward", tuple(mel.shape), None if lengths is None else [int(n) for n in lengths]))
        out = mel.sum(dim=1).repeat_interleave(4, dim=1)
        if lengths is not None:
            for b, n in enumerate(lengths):
                out[b, 4 * int(n):] = 0
        return out


class _Doubler:
    def __init__(self):
        self.calls = []

    def forward_device(self, wav, lengths=None):
        self.calls.append((tuple(wav.shape), lengths))
        return 2.0 * wav


def test_pipeline_without_a_denoiser_is_unchanged_and_chunked_routes_refuse():
    import torch
    mel = torch.arange(2 * 3 * 10, dtype=torch.float32).reshape(2, 3, 10)
    voc = _Vocode()
    plain = MelToWavePipeline(None, voc.forward, hop_length=4, chunk_frames=4)
    assert plain.denoiser is None
    want = plain.infer(mel)
    calls = list(voc.calls)
    assert torch.equal(torch.cat(list(plain.stream(mel)), dim=1), want)
    assert plain.session() is not None
    voc.calls.clear()
    explicit = MelToWavePipeline(None, voc.forward, hop_length=4, chunk_frames=4, denoiser=None)
    assert torch.equal(explicit.infer(mel), want) and voc.calls == calls          # the same vocoder calls, one for one

    dn = _Doubler()
    pipe = MelToWavePipeline(None, voc.forward, hop_length=4, chunk_frames=4, denoiser=dn)
    assert torch.equal(pipe.infer(mel), 2.0 * want) and dn.calls == [((2, 40), None)]
    outs = pipe.infer_batch([mel[0], mel[1, :, :6]])
    assert dn.calls[-1] == ((2, 40), [10, 6])                                      # the ragged route carries the lengths
    assert torch.equal(outs[0], 2.0 * want[0]) and outs[1].shape == (24,)
    with pytest.raises(ValueError, match="denoiser"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="denoiser"):
        pipe.session()
    with pytest.raises(ValueError):
        pipe.infer(mel, normalize=True)
