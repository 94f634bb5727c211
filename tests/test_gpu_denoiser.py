"""The bias denoiser (iris_denoiser_*, ``iris.denoiser``, ``MelToWavePipeline(denoiser=)``) on the MI355X, held to the float64
restatement of the arithmetic it commits to (tests/denoiser_restatement.py).  Cases, inputs and biases are
tests/denoiser_cases.py's; tests/test_denoiser.py shows that every case has both branches of the clamp live.

Bars, the project's ``e32`` scheme (tests/test_gpu_griffin_lim.py): ``e32`` = the largest difference between the restatement
run in fp32 on the library's own tables and itself in float64, relative to ``max(1, max |want|)``, over the cases; the device
must stay within ``4 * e32`` (another summation order), for the denoised waveform and for the bias estimate.  It is measured when
the bars are first asked for (it depends on the host BLAS's summation order); on the CPU it was 3.779e-07 for the waveform
(bar 1.51e-06) and 7.340e-08 for the bias estimate (bar 2.94e-07).
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import Denoiser
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import pcm16_from_float
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
from oracle import dsp_chain_cases as O

import denoiser_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
CASE_IDS = [C.case_id(c) for c in C.CASES]

_state = {}


def bars() -> dict:
    if "bars" not in _state:
        e = C.e32()
        _state["bars"] = {k: 4 * e[k] for k in ("out", "bias")}
        print("e32:", {k: f"{e[k]:.3e}" for k in ("out", "bias")})
        assert all(v > 0.0 for v in _state["bars"].values())
    return _state["bars"]


def model(name: str) -> Denoiser:
    if name not in _state:
        _state[name] = Denoiser(*C.stft_args(name), strength=C.STRENGTH, device=DEV)
    return _state[name]


def rel_err(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def poison_workspace(dn: Denoiser, B: int, L: int) -> None:
    dn._ensure()
    dn._ws(B, L).view(torch.float32).fill_(NAN)


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_forward_matches_the_restatement(case):
    name, B, M = case
    dn = model(name)
    dn.set_bias(C.bias(case))
    wav = C.waveform(case)
    poison_workspace(dn, B, wav.shape[1])
    got = dn.forward_device(wav)
    assert got.shape == wav.shape and got.dtype == torch.float32 and got.device == DEV
    err = rel_err(got.cpu().numpy(), C.restated(case))
    print(f"{C.case_id(case)} out: e_dev={err:.3e} bar={bars()['out']:.3e}")
    assert err <= bars()["out"]
    assert torch.equal(dn.forward_device(wav), got)
    assert np.array_equal(dn(wav[0]), got[0].cpu().numpy())                          # numpy in, numpy out


@pytest.mark.parametrize("case", [c for c in C.CASES if c != ("small", 1, 2)], ids=[i for i in CASE_IDS if i != "small-B1-M2"])
def test_estimate_bias_matches_the_restatement(case):
    dn = model(case[0])
    wav = C.waveform(case)[:1]
    poison_workspace(dn, 1, wav.shape[1])
    got = dn.estimate_bias(wav)
    assert got.shape == (dn.n_bins,) and got.device == DEV
    err = rel_err(got.cpu().numpy(), C.restated_bias(case))
    print(f"{C.case_id(case)} bias: e_dev={err:.3e} bar={bars()['bias']:.3e}")
    assert err <= bars()["bias"]
    assert torch.equal(dn.estimate_bias(wav), got)
    # an estimate goes back in device to device
    dn.set_bias(got)
    assert torch.equal(dn.bias, got)
    with pytest.raises(ValueError):
        dn.estimate_bias(C.waveform(("small", 1, 2)) if case[0] == "small" else wav[:, :dn.hop_length])


# ---- the new launch's sums, held to their chain --------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_strength_zero_stores_the_chain_of_the_update_transform(case):
    name, B, M = case
    dn = model(name)
    dn.set_bias(C.bias(case))
    wav = C.waveform(case)
    L, T, half = wav.shape[1], M + 1, dn.n_fft // 2
    poison_workspace(dn, B, L)
    dn.forward_device(wav, strength=0.0)
    c = dn._read_c(B, L).cpu().numpy()
    cfg, tab, d = O.GL_CONFIGS[name], C.tables(name), O.Design(O.GL_CONFIGS[name])
    bins = np.arange(half)
    for b in range(B):
        acc = O.update_acc(wav[b], T, cfg, tab)
        re, sine = acc[:, d.dft_col(bins, 0)], acc[:, d.dft_col(bins, 1)]
        im = -sine
        im[:, 0] = 0
        nyq = sine[:, 0]
        want = np.zeros((T, d.q), np.float32)
        want[:, 0:2 * half:2], want[:, 1:2 * half:2], want[:, 2 * half] = re, im, nyq
        live = np.zeros((T, d.q), bool)                      # where re^2 + im^2 does not underflow to 0 in fp32
        ok = (re * re + im * im) > 0
        live[:, 0:2 * half:2], live[:, 1:2 * half:2], live[:, 2 * half] = ok, ok, (nyq * nyq) > 0
        live[:, 2 * half + 1] = True                         # the stored 0 behind the Nyquist value
        assert live.mean() > 0.99
        assert O.differing(np.ascontiguousarray(c[b, :, :d.q]), want, live) == 0, (C.case_id(case), b)


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_large_strength_gives_exact_zero(case):
    dn = model(case[0])
    bias = np.maximum(C.bias(case), np.float32(1e-3))
    dn.set_bias(bias)
    strength = 2.0 * float((C.magnitudes64(case) / bias[None, None, :]).max())
    out = dn.forward_device(C.waveform(case), strength=strength)
    assert torch.equal(out, torch.zeros_like(out))


# ---- ragged batches ------------------------------------------------------------------------------------------------------
RAGGED_M = 40
RAGGED_LENGTHS = (0, 1, 2, 31, 32, 33, 40)


def ragged_input(name: str):
    cfg = C.CONFIGS[name]
    hop = cfg["hop_length"]
    wav = np.stack([C.waveform_item(hop * RAGGED_M, cfg, seed=50 + b) for b in range(len(RAGGED_LENGTHS))])
    bias = C.bias((name, 2, 39) if name == "default" else (name, 1, 69))
    return torch.from_numpy(wav).to(DEV), bias, hop


@pytest.mark.parametrize("name", ("default", "small"))
def test_ragged_items_are_their_batch_of_one_calls(name):
    dn = model(name)
    wav, bias, hop = ragged_input(name)
    dn.set_bias(bias)
    B, L = wav.shape
    alone = []
    for b, m in enumerate(RAGGED_LENGTHS):
        alone.append(dn.forward_device(wav[b:b + 1, :hop * m].contiguous()).clone())
    padded = wav.clone()
    for b, m in enumerate(RAGGED_LENGTHS):
        padded[b, hop * m:] = NAN                            # NaN in every padded sample ...
    poison_workspace(dn, B, L)                               # ... and in the whole workspace
    for lengths in (list(RAGGED_LENGTHS), torch.tensor(RAGGED_LENGTHS, dtype=torch.int32, device=DEV)):
        out = dn.forward_device(padded, lengths=lengths)
        assert out.shape == (B, L)
        for b, m in enumerate(RAGGED_LENGTHS):
            assert torch.equal(out[b:b + 1, :hop * m], alone[b]), (name, b, m)
            assert torch.equal(out[b, hop * m:], torch.zeros(L - hop * m, device=DEV)), (name, b, m)
    # device lengths out of range are clamped: -5 acts as 0, M + 9 as M
    wild = torch.tensor([-5, RAGGED_M + 9] + list(RAGGED_LENGTHS[2:]), dtype=torch.int32, device=DEV)
    tame = [0, RAGGED_M] + list(RAGGED_LENGTHS[2:])
    assert torch.equal(dn.forward_device(wav, lengths=wild), dn.forward_device(wav, lengths=tame))


def test_graph_capture_replays_and_follows_device_lengths():
    name = "small"
    dn = model(name)
    wav, bias, hop = ragged_input(name)
    dn.set_bias(bias)
    lengths, other = list(RAGGED_LENGTHS), list(reversed(RAGGED_LENGTHS))
    eager = {tuple(L): dn.forward_device(wav, lengths=L).clone() for L in (lengths, other)}
    assert torch.equal(dn.forward_device(wav, lengths=lengths), eager[tuple(lengths)])            # two runs agree
    assert not torch.equal(eager[tuple(lengths)], eager[tuple(other)])
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        dn.forward_device(wav, lengths=ln)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dn.forward_device(wav, lengths=ln)
    for L in (lengths, other):
        ln.copy_(torch.tensor(L, dtype=torch.int32))
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[tuple(L)]), L


# ---- the pipeline --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0)
    made = {dt: GeneratorEngine(cfg, sd, DEV, dtype=dt) for dt in ("f32", "bf16")}
    yield made
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_pipeline_with_a_denoiser(engines, dtype):
    eng = engines[dtype]
    dn = Denoiser.from_vocoder(eng.forward, frames=24, device=DEV)
    bias = dn.bias.cpu().numpy()
    assert bias.shape == (513,) and np.isfinite(bias).all() and (bias >= 0).all() and bias.max() > 0
    plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64)
    pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, denoiser=dn)
    mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(DEV)
    want = dn.forward_device(plain.infer(mel))
    got = pipe.infer(mel)
    assert torch.equal(got, want) and not torch.equal(got, plain.infer(mel))
    pcm = pipe.infer(mel, pcm16=True)
    assert pcm.dtype == torch.int16 and np.array_equal(pcm.cpu().numpy(), pcm16_from_float(want.cpu().numpy()))
    npcm, peaks = pipe.infer(mel, pcm16=True, normalize=True)
    assert np.array_equal(npcm.cpu().numpy(), pcm16_from_float(want.cpu().numpy(), normalize=True))
    assert torch.equal(peaks, want.abs().amax(dim=1))
    with pytest.raises(ValueError, match="denoiser"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="denoiser"):
        pipe.session()
    if dtype != "f32":
        return
    mels = [mel[0], mel[1, :, :17], mel[0, :, :33]]
    outs = pipe.infer_batch(mels)
    pcms = pipe.infer_batch(mels, pcm16=True)
    for m, out, p in zip(mels, outs, pcms):
        one = pipe.infer(m[None])[0]
        assert out.shape == (256 * m.shape[1],) and torch.equal(out, one)
        assert np.array_equal(p.cpu().numpy(), pcm16_from_float(one.cpu().numpy()))


# ---- refusals through the live handle --------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    dn = model("default")
    dn.set_bias(C.bias(("default", 2, 32)))
    lib = dn._ensure()
    B, L = 2, 256 * 8
    wav = torch.from_numpy(C.waveform(("default", 2, 32))[:, :L].copy()).to(DEV)
    out = torch.full((B, L), 7.0, dtype=torch.float32, device=DEV)
    bias_out = torch.full((513,), 7.0, dtype=torch.float32, device=DEV)
    ws = dn._ws(B, L)
    need = dn.workspace_bytes(B, L)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    lib.hipGetLastError.restype = ctypes.c_int
    lib.hipGetLastError()

    def fwd(w=wav, b=B, n=L, strength=0.1, o=out, space=ws, nbytes=need):
        p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.iris_denoiser_forward(dn._handle, p(w), b, n, None, ctypes.c_float(strength), p(o), p(space), ctypes.c_uint64(nbytes), stream)

    def est(w=wav, n=L, o=bias_out, space=ws, nbytes=need):
        p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.iris_denoiser_estimate_bias(dn._handle, p(w), n, p(o), p(space), ctypes.c_uint64(nbytes), stream)

    INVALID, UNSUPPORTED, SHORT = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED, _native.STATUS_WORKSPACE_TOO_SMALL
    assert fwd(n=L - 1) == INVALID                                       # L is no multiple of hop
    for bad in (-0.5, float("nan"), float("inf")):
        assert fwd(strength=bad) == INVALID
    assert fwd(w=None) == INVALID and fwd(o=None) == INVALID and fwd(space=None) == INVALID
    assert fwd(o=wav) == INVALID                                         # out aliases wav
    assert fwd(b=-1) == INVALID and fwd(n=-256) == INVALID
    assert fwd(b=65536) == UNSUPPORTED
    assert fwd(nbytes=need - 1) == SHORT
    assert est(n=L - 1) == INVALID and est(n=256 * 3) == INVALID         # no interior frame at T = 4
    assert est(w=None) == INVALID and est(o=None) == INVALID and est(space=None) == INVALID
    assert est(nbytes=dn.workspace_bytes(1, L) - 1) == SHORT
    assert lib.iris_denoiser_set_bias(dn._handle, None, stream) == INVALID
    torch.cuda.synchronize()
    assert lib.hipGetLastError() == 0
    assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(bias_out, torch.full_like(bias_out, 7.0))
    assert fwd() == 0 and est() == 0                                     # and the same arguments, valid, run
    torch.cuda.synchronize()
    assert not torch.equal(out, torch.full_like(out, 7.0)) and torch.isfinite(out).all() and torch.isfinite(bias_out).all()
