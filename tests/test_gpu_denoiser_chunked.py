"""The chunked bias denoiser (iris_denoiser_forward_window, ``DenoiserSession``, ``MelToWavePipeline(denoiser=dn.chunked())``)
on the MI355X.  The oracle everywhere is ``torch.equal`` with ``Denoiser.forward_device`` of the whole waveform: a frame's sums
depend on its own n_fft samples and a sample's on its own frames, in a fixed order, so a seam has no error at all and no
tolerance appears in this file.  Inputs, biases and ``STRENGTH`` = 1 are tests/denoiser_cases.py's (both clamp branches live);
the finality rule itself is held on the host by tests/test_denoiser_chunked.py.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import ChunkedDenoiser, Denoiser
from iris.pipeline import MelToWavePipeline
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import denoiser_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")

# (config, M, piece schedule in frames; None: one piece, which an utterance below the halo hands back from flush alone)
SESSIONS = (("default", 12, (1,) * 12),              # every push below the halo
            ("default", 39, (31, 1, 7)),             # a seam next to the 32-frame block edge
            ("small", 69, (31, 1, 33, 4)),           # three blocks
            ("small", 2, None), ("small", 1, None),  # shorter than the halo: everything comes from flush
            ("two_tap", 33, (16, 17)))               # two taps
SESSION_IDS = [f"{name}-M{M}" for name, M, _ in SESSIONS]

_state = {}


def model(name: str) -> Denoiser:
    if name not in _state:
        _state[name] = Denoiser(*C.stft_args(name), strength=C.STRENGTH, device=DEV)
    return _state[name]


def setup(name: str, M: int):
    """The model with the case's bias, its waveform [2, hop M] on the device, and a workspace full of NaN."""
    case = (name, 2, M)
    dn = model(name)
    dn.set_bias(C.bias(case))
    wav = torch.from_numpy(C.waveform(case)).to(DEV)
    dn._ws(2, wav.shape[1]).view(torch.float32).fill_(NAN)
    return dn, wav, case


def run_session(dn: Denoiser, wav: torch.Tensor, schedule, strength=None):
    """Pushes `schedule` frames at a time, flushes, and returns the pieces (the flush's last)."""
    session, hop, at, pieces = dn.open_session(strength=strength), dn.hop_length, 0, []
    for m in schedule:
        pieces.append(session.push(wav[:, at:at + hop * m]))
        at += hop * m
        assert session.samples_received == at and session.samples_emitted == sum(p.shape[1] for p in pieces)
        assert session.samples_buffered <= sum(session.halo) + hop * m
    assert at == wav.shape[1]
    pieces.append(session.flush())
    assert session.samples_emitted == wav.shape[1]
    return pieces


# ---- a session against the whole-utterance forward -------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,schedule", SESSIONS, ids=SESSION_IDS)
def test_session_equals_the_whole_utterance(name, M, schedule):
    dn, wav, _ = setup(name, M)
    whole = dn.forward_device(wav).clone()
    assert not torch.equal(whole, wav) and torch.isfinite(whole).all()
    pieces = run_session(dn, wav, schedule or (M,))
    assert all(p.device == DEV and p.dtype == torch.float32 and p.shape[0] == 2 for p in pieces)
    assert torch.equal(torch.cat(pieces, dim=1), whole)
    right = (dn.n_fft // dn.hop_length - 1) * dn.hop_length
    if schedule is None:                                          # below the halo: nothing before the flush
        assert M * dn.hop_length <= right and [p.shape[1] for p in pieces] == [0, wav.shape[1]]
    else:
        assert pieces[-1].shape[1] == right                       # the flush returns the halo
    # push plus flush of the whole utterance in one piece
    assert torch.equal(torch.cat(run_session(dn, wav, (M,)), dim=1), whole)


@pytest.mark.parametrize("name,M,schedule", [s for s in SESSIONS if s[2]], ids=[i for i, s in zip(SESSION_IDS, SESSIONS) if s[2]])
def test_strength_extremes_hold_across_seams(name, M, schedule):
    dn, wav, case = setup(name, M)
    # strength = 0: scale == 1 exactly, the plain istft(stft(wav)) -- the same bits chunked
    assert torch.equal(torch.cat(run_session(dn, wav, schedule, strength=0.0), dim=1), dn.forward_device(wav, strength=0.0))
    # a strength above max(mag / bias): exact zeros, in every piece
    bias = np.maximum(C.bias(case), np.float32(1e-3))
    dn.set_bias(bias)
    strength = 2.0 * float((C.magnitudes64(case) / bias[None, None, :]).max())
    out = torch.cat(run_session(dn, wav, schedule, strength=strength), dim=1)
    assert torch.equal(out, torch.zeros_like(wav))


# ---- iris_denoiser_forward_window itself ---------------------------------------------------------------------------------
def test_forward_window_stores_exactly_its_range_and_refuses_without_launching():
    name, M, m0, Mw, GUARD = "default", 39, 5, 20, 512
    dn, wav, _ = setup(name, M)
    hop, B = dn.hop_length, 2
    whole = dn.forward_device(wav).clone()
    origin, Lw = hop * m0, hop * Mw
    lo, count = dn.window_range(origin, Lw, False)
    assert (lo, count) == (origin + 3 * hop, Lw - 6 * hop) and dn.window_launch_count(B, Lw, origin, False) == 2
    window = wav[:, origin:origin + Lw].contiguous()
    lib = dn._ensure()
    ws = dn._ws(B, Lw)
    need = dn.window_workspace_bytes(B, Lw)
    ws.view(torch.float32).fill_(NAN)
    flat = torch.full((GUARD + B * count + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    out = flat[GUARD:GUARD + B * count]
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    lib.hipGetLastError.restype = ctypes.c_int
    lib.hipGetLastError()

    def fwd(w=window, n=Lw, org=origin, final=0, strength=C.STRENGTH, o=out, space=ws, nbytes=need):
        p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.iris_denoiser_forward_window(dn._handle, p(w), B, n, ctypes.c_int64(org), final, ctypes.c_float(strength), p(o),
                                                p(space), ctypes.c_uint64(nbytes), stream)

    INVALID, SHORT = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_WORKSPACE_TOO_SMALL
    assert fwd(nbytes=need - 1) == SHORT
    assert fwd(w=None) == INVALID and fwd(o=None) == INVALID and fwd(space=None) == INVALID
    assert fwd(org=origin + 1) == INVALID and fwd(org=-hop) == INVALID           # the origin is no multiple of hop, or negative
    assert fwd(n=Lw - 1) == INVALID and fwd(strength=-1.0) == INVALID and fwd(strength=NAN) == INVALID
    assert fwd(o=window) == INVALID                                              # out aliases wav
    torch.cuda.synchronize()
    assert lib.hipGetLastError() == 0
    assert torch.equal(flat, torch.full_like(flat, 7.0))                         # nothing was launched
    assert fwd(n=2 * hop) == 0                                                   # a window that settles nothing: OK, no launch
    torch.cuda.synchronize()
    assert torch.equal(flat, torch.full_like(flat, 7.0))

    assert fwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, count), whole[:, lo:lo + count])              # the slice of the whole result, bit for bit
    guard = torch.full((GUARD,), 7.0, dtype=torch.float32, device=DEV)
    assert torch.equal(flat[:GUARD], guard) and torch.equal(flat[GUARD + B * count:], guard)
    first = out.clone()
    out.fill_(NAN)
    assert fwd() == 0                                                            # two identical calls agree bit for bit
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    assert torch.equal(dn.forward_window(window, origin, False), first.view(B, count))
    # the same window as the utterance's last: its right edge is final now, and only the left halo is lost
    tail = dn.forward_window(wav[:, origin:].contiguous(), origin, True)
    assert tail.shape == (B, hop * (M - m0) - 3 * hop) and torch.equal(tail, whole[:, lo:])


# ---- the pipeline --------------------------------------------------------------------------------------------------------
def test_pipeline_streams_with_a_chunked_denoiser():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        dn = Denoiser.from_vocoder(eng.forward, frames=24, device=DEV)
        chunked = dn.chunked()
        assert isinstance(chunked, ChunkedDenoiser) and torch.equal(chunked.bias, dn.bias)
        pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=8, denoiser=chunked)
        mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(DEV)
        want = pipe.infer(mel)
        plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=8)
        assert torch.equal(want, dn.forward_device(plain.infer(mel))) and not torch.equal(want, plain.infer(mel))
        pieces = list(pipe.stream(mel))
        assert [p.shape[1] for p in pieces] == [256 * 5] + [256 * 8] * 4 + [256 * 3]      # short by the halo; the last carries it
        assert torch.equal(torch.cat(pieces, dim=1), want)
        session = pipe.session()
        got, at = [], 0
        for t in (7, 20, 13):
            got += session.push(mel[:, :, at:at + t])
            at += t
        got += session.flush()
        assert all(p.shape[1] > 0 for p in got) and torch.equal(torch.cat(got, dim=1), want)
        with pytest.raises(ValueError, match="fp32"):
            MelToWavePipeline(None, eng.forward_pcm16, device=DEV, chunk_frames=8, denoiser=chunked)
        refusing = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=8, denoiser=dn)
        with pytest.raises(ValueError, match="denoiser"):
            next(iter(refusing.stream(mel)))
        with pytest.raises(ValueError, match="denoiser"):
            refusing.session()
    finally:
        eng.close()
