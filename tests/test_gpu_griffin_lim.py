"""The Griffin-Lim vocoder (iris_griffin_lim_*, ``iris.griffin_lim``, ``MelToWavePipeline(vocode=GriffinLim())``) on the MI355X,
held to the float64 restatement of the arithmetic it commits to (tests/griffin_lim_restatement.py; parity unpinned: librosa
cannot be imported here).  Cases and inputs are tests/griffin_lim_cases.py's.

Exact-arithmetic bars, the project's ``e32`` scheme (tests/test_gpu_mel_frontend.py): ``e32`` = the largest difference between
the restatement run in fp32 on the library's own tables and itself in float64, relative to ``max(1, max |want|)``, over the
cases; the device must stay within ``4 * e32`` (another summation order).  Measured when this module's bars are first asked
for (it depends on the host BLAS's summation order); on the CPU it was
    S (inversion alone)      4.154e-07
    waveform, n_iter = 0     7.476e-07
    waveform, n_iter = 1     1.793e-06
    waveform, n_iter = 2     2.063e-06   -> bar 8.25e-06; the smallest peak amplitude of a case is 0.747, 1 % of it 7.5e-03
The full loop: the restatement's spectral convergence differed between its fp32 and float64 runs by at most 1.012e-06 over
four phase seeds (1337, 1, 2, 3), the five cases and n_iter 32 and 60, so the margin is ``SC_MARGIN`` = 2.03e-06.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.griffin_lim import GriffinLim, pack_phase
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import pcm16_from_float

import griffin_lim_cases as C
import griffin_lim_restatement as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SC_MARGIN = 2.03e-6
CASE_IDS = [C.case_id(c) for c in C.CASES]

_state = {}


def bars() -> dict:
    if "bars" not in _state:
        e = C.e32()
        _state["bars"] = {k: 4 * e[k] for k in ("S", 0, 1, 2)}
        print("e32:", {k: f"{e[k]:.3e}" for k in ("S", 0, 1, 2)})
        assert all(v > 0.0 for v in _state["bars"].values())
        for case, peak in e["peak"].items():                  # a bar above 1 % of the peak would show nothing
            assert _state["bars"][2] <= 0.01 * peak, (case, _state["bars"][2], peak)
    return _state["bars"]


def model(name: str, n_iter: int) -> GriffinLim:
    if (name, n_iter) not in _state:
        _state[(name, n_iter)] = C.model(name, n_iter=n_iter)
    return _state[(name, n_iter)]


def run(case, n_iter: int) -> torch.Tensor:
    return model(case[0], n_iter).forward_device(C.logmel(case), C.phase(case))


def rel_err(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_inversion_alone(case):
    gl = model(case[0], 0)
    gl._ensure()
    gl._ws(case[1], case[2]).view(torch.float32).fill_(float("nan"))
    run(case, 0)
    got = gl.magnitudes(case[1], case[2]).cpu().numpy().transpose(0, 2, 1)
    err = rel_err(got, C.restated(case, (0, 1, 2))[0])
    print(f"{C.case_id(case)} S: e_dev={err:.3e} bar={bars()['S']:.3e}")
    assert err <= bars()["S"]


@pytest.mark.parametrize("n_iter", [0, 1, 2])
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_waveform_after_n_iter(case, n_iter):
    """0: one inverse STFT of c0 (linear); 1: one pass; 2: the first pass that uses the momentum term."""
    name, B, T = case
    got = run(case, n_iter)
    assert got.shape == (B, C.CONFIGS[name]["hop_length"] * (T - 1))
    err = rel_err(got.cpu().numpy(), C.restated(case, (0, 1, 2))[1][n_iter])
    print(f"{C.case_id(case)} n_iter={n_iter}: e_dev={err:.3e} bar={bars()[n_iter]:.3e}")
    assert err <= bars()[n_iter]


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_full_loop_spectral_convergence(case):
    name, B, _ = case
    S, want = C.restated(case, (0, 32, 60))
    args = C.stft_args(name)
    sc = {n: [G.spectral_convergence(w.astype(np.float64), S[b], *args) for b, w in enumerate(run(case, n).cpu().numpy())]
          for n in (0, 32, 60)}
    for n in (32, 60):
        for b in range(B):
            ref = G.spectral_convergence(want[n][b], S[b], *args)
            print(f"{C.case_id(case)} item {b} n_iter={n}: SC_dev={sc[n][b]:.8f} SC_restatement={ref:.8f} diff={sc[n][b] - ref:+.3e}")
    for b in range(B):
        assert sc[32][b] < sc[0][b]
        for n in (32, 60):
            assert sc[n][b] <= G.spectral_convergence(want[n][b], S[b], *args) + SC_MARGIN, (n, b)


def test_determinism_and_batch_independence():
    case = C.CASES[1]                                            # default, B = 2, T = 40
    gl = model("default", 2)
    lm, phi = C.logmel(case), C.phase(case)
    first = gl.forward_device(lm, phi).clone()
    assert torch.equal(gl.forward_device(lm, phi), first)
    for b in range(2):
        assert torch.equal(gl.forward_device(lm[b:b + 1], phi[b:b + 1])[0], first[b]), b
    # the default start phase is the seeded one
    assert torch.equal(gl.forward_device(lm), first)
    assert not torch.equal(gl.forward_device(lm, seed=7), first)


def test_graph_capture_replays_the_eager_result():
    case = C.CASES[0]
    gl = model("default", 2)
    lm = torch.from_numpy(C.logmel(case)).to(DEV)
    packed = torch.from_numpy(pack_phase(C.phase(case))).to(DEV)
    eager = gl.forward_device(lm, packed).clone()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        gl.forward_device(lm, packed)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gl.forward_device(lm, packed)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_pipeline_with_griffin_lim_as_the_vocoder():
    case = C.CASES[0]
    gl = model("default", 2)
    lm = C.logmel(case)
    pipe = MelToWavePipeline(None, gl, device=DEV)
    want = gl.forward_device(lm)
    got = pipe.infer(lm)
    assert got.shape == (2, 256 * 32) and torch.equal(got, want)
    pcm = pipe.infer(lm, pcm16=True)
    assert pcm.dtype == torch.int16 and np.array_equal(pcm.cpu().numpy(), pcm16_from_float(want.cpu().numpy()))
    norm, peaks = pipe.infer(lm, pcm16=True, normalize=True)
    assert np.array_equal(norm.cpu().numpy(), pcm16_from_float(want.cpu().numpy(), normalize=True))
    assert torch.equal(peaks, want.abs().amax(dim=1))
    outs = pipe.infer_batch([lm[0], lm[1]])
    assert len(outs) == 2 and all(torch.equal(o, w) for o, w in zip(outs, want))
    with pytest.raises(NotImplementedError):
        pipe.infer_batch([lm[0], lm[1][:, :20]])
    with pytest.raises(NotImplementedError):
        next(pipe.stream(lm))
    host = gl(lm[0])
    assert isinstance(host, np.ndarray) and host.shape == (256 * 32,)
    assert np.array_equal(host, gl.forward_device(lm[:1])[0].cpu().numpy())


def test_refused_forwards_return_their_code_and_launch_nothing():
    case = C.CASES[0]
    _, B, T = case
    gl = model("default", 2)
    lib = _native.load()
    lm = torch.from_numpy(C.logmel(case)).to(DEV)
    packed = torch.from_numpy(pack_phase(C.phase(case))).to(DEV)
    want = gl.forward_device(lm, packed).clone()
    need = gl.workspace_bytes(B, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ws.view(torch.float32).fill_(float("nan"))
    wav = torch.full((B, 256 * (T - 1)), float("nan"), dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(h=gl._handle, a=lm, p=packed, B=B, T=T, out=wav, w=ws, n=need):
        ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.iris_griffin_lim_forward(h, ptr(a), ptr(p), B, T, ptr(out), ptr(w), ctypes.c_uint64(n), stream)

    assert call(n=need - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
    assert f"workspace has {need - 1} bytes, need {need}" in lib.iris_hifigan_last_error().decode()
    assert call(n=0) == _native.STATUS_WORKSPACE_TOO_SMALL
    for kw in (dict(a=None), dict(p=None), dict(out=None), dict(w=None), dict(h=None), dict(T=1), dict(T=0), dict(T=-3), dict(B=-1)):
        assert call(**kw) == _native.STATUS_INVALID_ARGUMENT, kw
    assert call(B=65536) == _native.STATUS_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(wav).all() and torch.isnan(ws.view(torch.float32)).all()      # nothing was launched
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(wav).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(wav, want)


def test_text_to_waveform_and_the_resampled_output():
    """Phoneme ids -> encoder, duration head, VAE decoder -> Griffin-Lim: no checkpoint; then the stand-alone resampling stage."""
    from encoder_cases import make_models, reference
    from iris import encoder as E
    from iris.resample import Resampler
    from vae_cases import make_vae
    enc, head = make_models("default")
    vae = make_vae("default")
    gl = model("default", 2)
    pipe = MelToWavePipeline(None, gl, device=DEV, acoustic=vae, text=(enc, head))
    ids = reference(("default", 1, 7, None))["ids"]
    cond, per_item = E.frame_conditioning(enc, head, ids, factor=vae.downsample_factor)
    T = cond.shape[1]
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((1, T // 4, vae.latent_dim)).astype(np.float32)).to(DEV)
    mel = vae.generate_device(cond, z, want_residual=False)[0].clone()
    want = gl.forward_device(mel).clone()
    assert torch.isfinite(want).all() and tuple(want.shape) == (1, 256 * (T - 1))
    got, frames = pipe.infer_from_phonemes(ids, z_prior=z)
    assert frames == per_item and torch.equal(got, want)
    assert torch.equal(pipe.infer_from_cond(cond, z), want)
    rs = Resampler(16000, device=DEV)
    assert torch.equal(pipe.infer(mel, resampler=rs), rs.forward(want))
    pcm = pipe.infer_from_cond(cond, z, resampler=rs, pcm16=True)
    assert pcm.dtype == torch.int16 and torch.equal(pcm, rs.forward(want, pcm16=True))
