"""Ragged Griffin-Lim batches (``iris_griffin_lim_forward_ragged``, ``GriffinLim.forward_device(lengths=)``) and the start phase
drawn on the device (``phase0="device"``, ``GriffinLim.draw_phase``) on the MI355X.

The claim of the ragged form is equality, not closeness: block tiling does not depend on ``T`` and only bounds change, so
item b of a ragged call has the chains of its batch-of-one call at ``T = T_b`` -- every comparison below is ``torch.equal``.
Configs and inputs are tests/griffin_lim_cases.py's; the shapes are the smallest that reach every guard: a length on a
32-frame block edge (32, 64), one past it (33), one below the tap count (2, 3), an empty item (0) and the full length.

The drawn phase is held to ``iris.griffin_lim.philox_phase_np``, which shares the fp32 angle with the device, so what is left
is the device's ``cosf`` / ``sinf``: the bar is 4 fp32 ulp at magnitude 1, ``4 * 2^-23`` absolute -- the OpenCL full-profile
bound for sin and cos, which the ROCm device library (ocml) is written to; its documentation states no other bound.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.griffin_lim import GriffinLim, pack_phase, philox_phase_np
from iris.pipeline import MelToWavePipeline

import griffin_lim_cases as C
import griffin_lim_restatement as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
# (config, T, lengths)
RAGGED = (("default", 40, (40, 33)), ("default", 40, (32, 2)), ("default", 40, (31, 0)), ("small", 70, (70, 3, 33, 64)),
          ("two_tap", 34, (34, 2)))
IDS = [f"{n}-T{T}-" + "_".join(str(v) for v in L) for n, T, L in RAGGED]
TRIG_BAR = 4 * 2.0 ** -23

_state = {}


def model(name: str, n_iter: int, **kw) -> GriffinLim:
    key = (name, n_iter, tuple(sorted(kw.items())))
    if key not in _state:
        _state[key] = C.model(name, n_iter=n_iter, **kw)
    return _state[key]


def inputs(rc):
    """``(logmel [B, n_mels, T] float32, phi [B, K, T] float64)``: fresh copies the caller may poison."""
    name, T, lengths = rc
    case = (name, len(lengths), T)
    return C.logmel(case).copy(), C.phase(case).copy()


def hop_of(name: str) -> int:
    return C.CONFIGS[name]["hop_length"]


def alone(gl, lm, phi, b, n):
    """Item b's batch-of-one dense call at ``T = n``."""
    return gl.forward_device(np.ascontiguousarray(lm[b:b + 1, :, :n]), phi[b:b + 1, :, :n])[0]


def poison_wav(B, Ly):
    """Leaves NaN in the block the next ``torch.empty((B, Ly))`` most likely gets, so a row's tail is 0 only if stored."""
    t = torch.full((B, Ly), NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    del t


def check_against_alone(gl, got, lm, phi, rc):
    name, T, lengths = rc
    hop = hop_of(name)
    assert tuple(got.shape) == (len(lengths), hop * (T - 1))
    for b, n in enumerate(lengths):
        own = hop * (n - 1) if n else 0
        assert (got[b, own:] == 0).all(), (b, n)
        if n:
            assert torch.equal(got[b, :own], alone(gl, lm, phi, b, n)), (b, n)


@pytest.mark.parametrize("n_iter", [0, 1, 2])
@pytest.mark.parametrize("rc", RAGGED, ids=IDS)
def test_item_is_bit_for_bit_its_stand_alone_call(rc, n_iter):
    name, T, lengths = rc
    gl = model(name, n_iter)
    lm, phi = inputs(rc)
    poison_wav(len(lengths), hop_of(name) * (T - 1))
    got = gl.forward_device(lm, phi, lengths=list(lengths))
    check_against_alone(gl, got.clone(), lm, phi, rc)


@pytest.mark.parametrize("rc", RAGGED, ids=IDS)
def test_nothing_past_an_item_is_read(rc):
    name, T, lengths = rc
    B = len(lengths)
    gl = model(name, 2)
    lm, phi = inputs(rc)
    want = gl.forward_device(lm, phi, lengths=list(lengths)).clone()
    packed = pack_phase(phi)
    for b, n in enumerate(lengths):
        lm[b, :, n:] = NAN
        packed[b, n:] = NAN
    gl._ws(B, T).view(torch.float32).fill_(NAN)
    poison_wav(B, hop_of(name) * (T - 1))
    got = gl.forward_device(lm, torch.from_numpy(packed).to(DEV), lengths=list(lengths))
    assert torch.equal(got, want)
    # and nothing past an item is written: S, c and r rows at t >= T_b are still NaN
    ks, qp = (gl.n_bins + 3) // 4 * 4, (gl.n_fft + 2 + 7) // 8 * 8
    ws = gl._workspace.view(torch.float32)
    S = ws[:B * T * ks].view(B, T, ks)
    off = (B * T * ks + 63) // 64 * 64
    c = ws[off:off + B * T * qp].view(B, T, qp)
    for b, n in enumerate(lengths):
        assert torch.isnan(S[b, n:]).all() and torch.isnan(c[b, n:]).all(), b
        if n:
            assert torch.isfinite(S[b, :n, :gl.n_bins]).all() and torch.isfinite(c[b, :n, :gl.n_fft + 2]).all(), b


def test_device_lengths_and_their_sanitising():
    rc = RAGGED[3]                                                # small, T = 70, B = 4
    name, T, lengths = rc
    gl = model(name, 2)
    lm, phi = inputs(rc)
    want = gl.forward_device(lm, phi, lengths=list(lengths)).clone()
    dev = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    assert torch.equal(gl.forward_device(lm, phi, lengths=dev), want)
    assert torch.equal(gl.forward_device(lm, phi, lengths=np.array(lengths, dtype=np.int64)), want)
    # -5, 1 and T + 9 behave as 0, 0 and T
    odd = torch.tensor([-5, 1, T + 9, 33], dtype=torch.int32, device=DEV)
    assert torch.equal(gl.forward_device(lm, phi, lengths=odd), gl.forward_device(lm, phi, lengths=[0, 0, T, 33]))
    with pytest.raises(ValueError, match="never read by the host"):
        gl.forward_device(lm, lengths=dev)
    with pytest.raises(ValueError, match="int32"):
        gl.forward_device(lm, phi, lengths=dev.to(torch.int64))
    # full lengths are the dense call
    assert torch.equal(gl.forward_device(lm, phi, lengths=[T] * 4), gl.forward_device(lm, phi))


def test_host_phase_of_a_ragged_call_is_the_stand_alone_draw():
    rc = RAGGED[0]                                                # default, T = 40, (40, 33)
    name, T, lengths = rc
    gl = model(name, 2)
    lm, _ = inputs(rc)
    got = gl.forward_device(lm, seed=5, lengths=list(lengths)).clone()
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :256 * (n - 1)], gl.forward_device(np.ascontiguousarray(lm[b:b + 1, :, :n]), seed=5)[0]), b


class _Raw:
    """The two forwards through ctypes on buffers the test owns."""

    def __init__(self, gl, B, T, hop):
        self.lib, self.gl, self.B, self.T = _native.load(), gl, B, T
        gl._ensure()
        self.need = gl.workspace_bytes(B, T)
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=DEV)
        self.wav = torch.empty((B, hop * (T - 1)), dtype=torch.float32, device=DEV)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        self.poison()

    def poison(self):
        self.ws.view(torch.float32).fill_(NAN)
        self.wav.fill_(NAN)

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(None if t is None else t.data_ptr())

    def ragged(self, a, p, lengths, seed=0, item0=0, **kw):
        h, B, T = kw.get("h", self.gl._handle), kw.get("B", self.B), kw.get("T", self.T)
        out, w, n = kw.get("out", self.wav), kw.get("w", self.ws), kw.get("n", self.need)
        return self.lib.iris_griffin_lim_forward_ragged(h, self.ptr(a), self.ptr(p), ctypes.c_uint64(seed), item0, B, T, self.ptr(lengths),
                                                        self.ptr(out), self.ptr(w), ctypes.c_uint64(n), self.stream)

    def dense(self, a, p):
        return self.lib.iris_griffin_lim_forward(self.gl._handle, self.ptr(a), self.ptr(p), self.B, self.T, self.ptr(self.wav),
                                                 self.ptr(self.ws), ctypes.c_uint64(self.need), self.stream)


def test_no_lengths_through_the_new_entry_is_the_dense_forward():
    case = C.CASES[0]                                             # default, B = 2, T = 33
    _, B, T = case
    gl = model("default", 2)
    lm = torch.from_numpy(C.logmel(case)).to(DEV)
    packed = torch.from_numpy(pack_phase(C.phase(case))).to(DEV)
    raw = _Raw(gl, B, T, 256)
    assert raw.dense(lm, packed) == 0
    want = raw.wav.clone()
    raw.poison()
    assert raw.ragged(lm, packed, None, seed=99, item0=7) == 0   # seed and item0 are ignored with a phase
    torch.cuda.synchronize()
    assert torch.equal(raw.wav, want) and torch.equal(gl.forward_device(lm, packed), want)


def test_refused_ragged_forwards_return_their_code_and_launch_nothing():
    rc = RAGGED[0]
    name, T, lengths = rc
    B = len(lengths)
    gl = model(name, 2)
    lm_h, phi = inputs(rc)
    want = gl.forward_device(lm_h, phi, lengths=list(lengths)).clone()
    lm = torch.from_numpy(lm_h).to(DEV)
    packed = torch.from_numpy(pack_phase(phi)).to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    raw = _Raw(gl, B, T, 256)
    lib, need = raw.lib, raw.need
    call = lambda a=lm, p=packed, item0=0, **kw: raw.ragged(a, p, ln, item0=item0, **kw)
    assert call(n=need - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
    assert f"workspace has {need - 1} bytes, need {need}" in lib.iris_hifigan_last_error().decode()
    assert call(n=0) == _native.STATUS_WORKSPACE_TOO_SMALL
    for kw in (dict(a=None), dict(out=None), dict(w=None), dict(h=None), dict(T=1), dict(T=0), dict(T=-3), dict(B=-1), dict(item0=-1)):
        assert call(**kw) == _native.STATUS_INVALID_ARGUMENT, kw
    assert call(B=65536) == _native.STATUS_UNSUPPORTED
    big = torch.empty((B, T, gl.n_bins, 2), dtype=torch.float32, device=DEV)
    big.fill_(NAN)
    draw = lambda **kw: lib.iris_griffin_lim_draw_phase(kw.get("h", gl._handle), ctypes.c_uint64(1), kw.get("item0", 0), kw.get("B", B),
                                                        kw.get("T", T), raw.ptr(kw.get("out", big)), raw.stream)
    for kw in (dict(h=None), dict(out=None), dict(T=1), dict(B=-1), dict(item0=-1)):
        assert draw(**kw) == _native.STATUS_INVALID_ARGUMENT, kw
    assert draw(B=65536) == _native.STATUS_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(raw.wav).all() and torch.isnan(raw.ws.view(torch.float32)).all() and torch.isnan(big).all()
    assert call(B=0) == 0 and draw(B=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(raw.wav).all() and torch.isnan(big).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.wav, want)                              # the tail of a NaN-filled row was stored as 0


def test_a_captured_graph_follows_new_lengths():
    rc = RAGGED[3]                                                # small, T = 70, B = 4
    name, T, lengths = rc
    gl = model(name, 2)
    lm_h, phi = inputs(rc)
    lm = torch.from_numpy(lm_h).to(DEV)
    packed = torch.from_numpy(pack_phase(phi)).to(DEV)
    other = (33, 70, 0, 2)
    eager = {L: gl.forward_device(lm, packed, lengths=list(L)).clone() for L in (lengths, other)}
    assert not torch.equal(eager[lengths], eager[other])
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        gl.forward_device(lm, packed, lengths=ln)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gl.forward_device(lm, packed, lengths=ln)
    for L in (lengths, other):
        ln.copy_(torch.tensor(L, dtype=torch.int32))
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[L]), L


# ---- the start phase drawn on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,T,seed,first", [("default", 2, 40, 1337, 0), ("small", 3, 70, (0xABCDEF01 << 32) | 0x12345678, 5),
                                                 ("two_tap", 1, 34, 7, 2 ** 31 - 2)])
def test_draw_phase_against_the_numpy_restatement(name, B, T, seed, first):
    gl = model(name, 0)
    got = gl.draw_phase(B, T, seed=seed, first_item=first)
    assert tuple(got.shape) == (B, T, gl.n_bins, 2) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    want = np.stack([philox_phase_np(seed, first + b, gl.n_bins, T) for b in range(B)])
    err = float(np.abs(got - want).max())
    print(f"{name} {B}x{T}: max |device (cosf, sinf) - float64 of the same fp32 angle| = {err:.3e} ({err * 2 ** 23:.2f} ulp at 1), "
          f"bar {TRIG_BAR:.3e}")
    assert err <= TRIG_BAR
    assert torch.equal(gl.draw_phase(B, T, seed=seed, first_item=first).cpu(), torch.from_numpy(got.astype(np.float32)))


@pytest.mark.parametrize("rc", [RAGGED[0], RAGGED[3]], ids=[IDS[0], IDS[3]])
def test_forward_with_a_device_phase_is_the_forward_on_the_drawn_tensor(rc):
    name, T, lengths = rc
    B = len(lengths)
    gl = model(name, 2)
    lm, _ = inputs(rc)
    drawn = gl.draw_phase(B, T, seed=21, first_item=3)
    dense = gl.forward_device(lm, "device", seed=21, first_item=3).clone()
    assert torch.equal(dense, gl.forward_device(lm, drawn))
    assert not torch.equal(dense, gl.forward_device(lm, "device", seed=22, first_item=3))
    ragged = gl.forward_device(lm, "device", seed=21, first_item=3, lengths=list(lengths)).clone()
    assert torch.equal(ragged, gl.forward_device(lm, drawn, lengths=list(lengths)))
    # item b is its batch-of-one call on stream first_item + b, dense and ragged
    hop = hop_of(name)
    for b, n in enumerate(lengths):
        assert torch.equal(dense[b], gl.forward_device(lm[b:b + 1], "device", seed=21, first_item=3 + b)[0]), b
        if n:
            one = gl.forward_device(np.ascontiguousarray(lm[b:b + 1, :, :n]), "device", seed=21, first_item=3 + b)[0]
            assert torch.equal(ragged[b, :hop * (n - 1)], one) and (ragged[b, hop * (n - 1):] == 0).all(), b
    # the constructor's default for phase0=None
    dev_default = model(name, 2, phase="device")
    assert torch.equal(dev_default.forward_device(lm, seed=21, first_item=3), dense)


def test_the_drawn_phase_is_a_usable_start():
    case = ("small", 1, 70)
    S, _ = C.restated(case, (0,))
    args = C.stft_args("small")
    lm = C.logmel(case)
    sc = {n: G.spectral_convergence(model("small", n).forward_device(lm, "device")[0].cpu().numpy().astype(np.float64), S[0], *args)
          for n in (0, 32)}
    print(f"spectral convergence from the device-drawn phase: n_iter 0 {sc[0]:.6f}, n_iter 32 {sc[32]:.6f}")
    assert sc[32] < sc[0]


# ---- the pipeline ------------------------------------------------------------------------------------------------------
def test_pipeline_infer_batch_of_unequal_lengths():
    from iris.resample import Resampler
    case = C.CASES[1]                                             # default, B = 2, T = 40
    gl = model("default", 2, ragged=True)
    pipe = MelToWavePipeline(None, gl, device=DEV)
    lm = C.logmel(case)
    mels = [lm[0], np.ascontiguousarray(lm[1][:, :20])]
    rs = Resampler(16000, device=DEV)
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, normalize=True), dict(resampler=rs), dict(resampler=rs, pcm16=True, normalize=True)):
        outs = pipe.infer_batch(mels, **kw)
        assert len(outs) == 2
        for i, m in enumerate(mels):
            want = pipe.infer(m[None], **kw)
            want = (want[0] if kw.get("normalize") else want)[0]
            assert outs[i].dtype == want.dtype and torch.equal(outs[i], want), (kw, i)
    assert tuple(pipe.infer_batch(mels)[1].shape) == (256 * 19,)
    # a device-drawn phase: item i is the stand-alone call on stream i
    gd = model("default", 2, ragged=True, phase="device")
    outs = MelToWavePipeline(None, gd, device=DEV).infer_batch(mels)
    for i, m in enumerate(mels):
        assert torch.equal(outs[i], gd.forward_device(m[None], first_item=i)[0]), i


def test_text_to_waveform_on_a_ragged_batch():
    """Phoneme ids -> encoder, duration head, VAE decoder -> Griffin-Lim for two utterances of different frame totals in one
    pass per stage; each is bit for bit its own ``B = 1`` call."""
    from encoder_cases import make_ids, make_models
    from vae_cases import make_vae
    enc, head = make_models("default")
    vae = make_vae("default")
    gl = model("default", 2, ragged=True)
    pipe = MelToWavePipeline(None, gl, device=DEV, acoustic=vae, text=(enc, head))
    ids, lengths = make_ids("default", 2, 7), [7, 4]
    durations = np.array([[2, 3, 1, 2, 2, 3, 2], [3, 2, 2, 2, 0, 0, 0]], dtype=np.int32)      # 15 and 9 frames: 16 and 12 padded
    rng = np.random.default_rng(3)
    zs = [torch.from_numpy(rng.standard_normal((1, t // 4, vae.latent_dim)).astype(np.float32)).to(DEV) for t in (16, 12)]
    singles = [pipe.infer_from_phonemes(ids[i:i + 1, :n], durations=durations[i:i + 1, :n], z_prior=zs[i]) for i, n in enumerate(lengths)]
    batch, frames = pipe.infer_from_phonemes(ids, lengths=lengths, durations=durations, z_prior=zs)
    assert frames == [15, 9] == [s[1][0] for s in singles]
    for i, t in enumerate((16, 12)):
        assert tuple(batch[i].shape) == (256 * (t - 1),) and torch.equal(batch[i], singles[i][0][0]), i
