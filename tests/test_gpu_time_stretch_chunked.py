"""The chunked time stretch on the device: a ``StretchSession`` against ``forward_device`` of the whole utterance, the state after
every window against the one-shot's own ``acc`` and ``out_c``, what ``iris_time_stretch_forward_window`` stores and refuses, and a
pipeline that streams through a chunked denoiser and a chunked stretch.  Everything is ``torch.equal``: the phase is an exact
integer sum, a row's chain depends on its own samples and a sample's on its own frames (csrc/time_stretch.h, "Windows").
The rule itself and the bookkeeping are tests/test_time_stretch_chunked.py's.
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
from iris.time_stretch import ChunkedStretch, TimeStretch
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import time_stretch_cases as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")

# (case, schedule in mel frames)
SEMI = ("small", 1, 69, TC.SEMITONE_DOWN)
SESSIONS = (
    (SEMI, (5, 1, 0, 9, 2, 1, 30, 21)),                  # uneven, with pieces shorter than the halo (e = 2 frames)
    (SEMI, (1,) * 69),                                   # hop-sized pieces
    (SEMI, (69,)),                                       # one piece: a single final window is forward_device
    (("small", 1, 69, 0.25), (20, 3, 46)),
    (("small", 1, 69, 4.0), (20, 3, 46)),
    (("small", 1, 2, 0.8), (1, 1)),                      # fewer frames than taps
    (("small", 1, 1, 4.0), (1,)),
    (("default", 2, 32, 0.8), (7, 9, 16)),               # the crop is live in the final window
    (("default", 2, 39, 1.25), (12, 1, 26)),             # the tail rule is live
    (("two_tap", 1, 33, 1.5), (4, 1, 28)),
    (("two_tap", 1, 33, 4.0), (4, 1, 28)),               # on the boundary of the non-final cap
)
SESSION_IDS = [f"{TC.case_id(c)}-{len(s)}pieces" for c, s in SESSIONS]

_models: dict = {}


def model(name: str) -> TimeStretch:
    if name not in _models:
        _models[name] = TimeStretch(*TC.stft_args(name), device=DEV)
    return _models[name]


def setup(case):
    ts = model(case[0])
    wav = torch.from_numpy(TC.waveform(case).copy()).to(DEV)
    return ts, wav


@pytest.mark.parametrize("case,schedule", SESSIONS, ids=SESSION_IDS)
def test_session_equals_the_whole_utterance(case, schedule):
    ts, wav = setup(case)
    hop, rate = ts.hop_length, case[3]
    assert sum(schedule) == case[2]
    want = ts.forward_device(wav, rate)[0].clone()
    session = ts.open_session(rate)
    got, at = [], 0
    for m in schedule:
        got.append(session.push(wav[:, at:at + hop * m]))
        at += hop * m
    got.append(session.flush())
    assert session.samples_emitted == want.shape[1] == ts.out_samples(wav.shape[1], rate)
    assert torch.equal(torch.cat(got, dim=1), want)
    if len(schedule) == 1:                                    # the single final window, with and without a state
        assert torch.equal(ts.forward_window(wav, rate, 0, True, 0, None), want)


def windows_of(ts: TimeStretch, rate: float, L: int, schedule):
    """``[(origin, Lw, final, u, u_hi, lo, count)]`` of a session over ``schedule``: the plan alone, as the session keeps it."""
    hop = ts.hop_length
    base = total = u = 0
    out = []
    for m, final in [(m, False) for m in schedule] + [(0, True)]:
        total += hop * m
        u_hi, lo, count, keep = ts.window_plan(rate, base, total - base, final, u)
        if u_hi == u and count == 0:
            continue
        out.append((base, total - base, final, u, u_hi, lo, count))
        u, base = u_hi, max(base, min(keep, total))
    assert total == L
    return out


@pytest.mark.parametrize("case,schedule", [SESSIONS[0], SESSIONS[3], SESSIONS[4], SESSIONS[7], SESSIONS[10]],
                         ids=[SESSION_IDS[i] for i in (0, 3, 4, 7, 10)])
def test_state_after_every_window(case, schedule):
    ts, wav = setup(case)
    B, L, rate, taps = wav.shape[0], wav.shape[1], case[3], ts.n_fft // ts.hop_length
    ts.forward_device(wav, rate)
    one = ts._read_buffers(B, L, rate)                        # the one-shot's own acc, inc and out_c
    T_out = one["acc"].shape[1]
    past = (one["acc"][:, -1] + one["inc"][:, -1]) & 0xFFFFFFFF
    K = ts.n_bins
    state = ts.new_state(B)
    state.view(torch.int32).fill_(0x7FC00123)                 # a NaN pattern: nothing of it may be read at u == 0
    for origin, Lw, final, u, u_hi, lo, count in windows_of(ts, rate, L, schedule):
        ts.forward_window(wav[:, origin:origin + Lw].contiguous(), rate, origin, final, u, state)
        acc, tail = ts._state_views(state, B)
        if u_hi > u:
            want = one["acc"][:, u_hi] if u_hi < T_out else past
            assert torch.equal(acc[:, :K], want[:, :K]), (origin, u, u_hi)
        keep = min(taps - 1, u_hi)
        assert torch.equal(tail[:, taps - 1 - keep:, :2 * K], one["out_c"][:, u_hi - keep:u_hi, :2 * K]), (origin, u, u_hi)
        # the padding columns and the rows of negative frames are as they were
        assert bool((acc[:, K:] == 0x7FC00123).all()) and bool((tail[:, :, 2 * K:].view(torch.int32) == 0x7FC00123).all())
        assert bool((tail[:, :taps - 1 - keep].view(torch.int32) == 0x7FC00123).all())
    assert u_hi == T_out


def test_forward_window_stores_exactly_its_range_and_refuses_without_launching():
    case, GUARD = ("default", 2, 39, 1.25), 512
    ts, wav = setup(case)
    hop, B, rate = ts.hop_length, 2, case[3]
    whole = ts.forward_device(wav, rate)[0].clone()
    # the session's first two windows by hand: [0, 20 hop) from frame 0, then from its keep_from on
    L0 = 20 * hop
    u, lo0, n0, origin = ts.window_plan(rate, 0, L0, False, 0)
    Lw = wav.shape[1] - origin
    u_hi, lo, count, _ = ts.window_plan(rate, origin, Lw, True, u)
    assert (u, lo0, n0, origin) == (15, 0, 15 * hop - 512, 16 * hop) and lo == n0 and u_hi == ts.out_frames_samples(wav.shape[1], rate)[0]
    state = ts.new_state(B)
    head = ts.forward_window(wav[:, :L0].contiguous(), rate, 0, False, 0, state)
    assert torch.equal(head, whole[:, :n0])
    kept = state.clone()
    window = wav[:, origin:origin + Lw].contiguous()
    lib = ts._ensure()
    need = ts.window_workspace_bytes(B, Lw, rate)
    assert ts._workspace.numel() >= need and ts.window_launch_count(B, Lw, rate, origin, True, u) == 4
    ws = ts._workspace
    ws.view(torch.float32).fill_(NAN)
    flat = torch.full((GUARD + B * count + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    out = flat[GUARD:GUARD + B * count]
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    lib.hipGetLastError.restype = ctypes.c_int
    lib.hipGetLastError()

    def fwd(w=window, n=Lw, org=origin, fin=1, r=rate, frame=u, st=state, o=out, space=ws, nbytes=need):
        p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.iris_time_stretch_forward_window(ts._handle, p(w), B, n, ctypes.c_int64(org), fin, ctypes.c_double(r), ctypes.c_int64(frame),
                                                    p(st), p(o), p(space), ctypes.c_uint64(nbytes), stream)

    INVALID, SHORT, UNSUPPORTED = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_WORKSPACE_TOO_SMALL, _native.STATUS_UNSUPPORTED
    assert fwd(nbytes=need - 1) == SHORT
    assert fwd(w=None) == INVALID and fwd(o=None) == INVALID and fwd(space=None) == INVALID and fwd(st=None) == INVALID
    assert fwd(org=origin + 1) == INVALID and fwd(org=-hop) == INVALID and fwd(n=Lw - 1) == INVALID
    assert fwd(frame=-1) == INVALID and fwd(r=5.0) == INVALID and fwd(r=NAN) == INVALID
    assert fwd(frame=u - 1) == INVALID                                           # its first row left with the samples before keep_from
    assert fwd(org=0, n=L0, fin=0, frame=0, st=None) == INVALID                  # a window that is not final carries a state
    assert fwd(o=window) == INVALID                                              # out aliases wav
    assert fwd(org=hop * ((1 << 60) // hop + 1), frame=1 << 40) == UNSUPPORTED
    torch.cuda.synchronize()
    assert lib.hipGetLastError() == 0
    assert torch.equal(flat, torch.full_like(flat, 7.0)) and torch.equal(state, kept)          # nothing was launched
    assert bool(torch.isnan(ws.view(torch.float32)).all())
    assert fwd(org=0, n=2 * hop, fin=0, frame=0) == 0                            # a window that computes nothing: OK, no launch
    torch.cuda.synchronize()
    assert torch.equal(flat, torch.full_like(flat, 7.0)) and torch.equal(state, kept)

    assert fwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, count), whole[:, lo:lo + count])              # the slice of the whole result, bit for bit
    assert lo + count == whole.shape[1]
    guard = torch.full((GUARD,), 7.0, dtype=torch.float32, device=DEV)
    assert torch.equal(flat[:GUARD], guard) and torch.equal(flat[GUARD + B * count:], guard)
    # the workspace: every buffer holds the rows the window owns and poison behind them
    frames = wav.shape[1] // hop + 1 - (origin // hop + 2)                       # rows [m0 + e, T) of the final window
    layout = ts._window_workspace_layout(B, Lw, rate, frames, u_hi - u, 3)
    floats, bits = ws.view(torch.float32), ws.view(torch.int32)
    POISON = int(torch.tensor(NAN).view(torch.int32))          # inc and acc are integers: compare bit patterns
    for name, (off, shape, room) in layout.items():
        used = int(np.prod(shape))
        owned = bits[off:off + used].view(shape)[..., :2 * ts.n_bins if name in ("c", "out_c") else ts.n_bins]
        assert not bool((owned == POISON).any()), name
        assert bool((bits[off + used:off + (room + 63) // 64 * 64] == POISON).all()), name
    end = max(off + (room + 63) // 64 * 64 for off, _, room in layout.values())
    assert end * 4 == need and bool((bits[end:] == POISON).all())
    # the rows it carried in stand in front of the new ones; two identical calls from the same state agree bit for bit
    off, shape, _ = layout["out_c"]
    assert torch.equal(floats[off:off + int(np.prod(shape))].view(shape)[:, :3, :2 * ts.n_bins], ts._state_views(kept, B)[1][:, :, :2 * ts.n_bins])
    again = kept.clone()
    got = ts.forward_window(window, rate, origin, True, u, again)
    assert torch.equal(got, out.view(B, count)) and torch.equal(again, state)


def test_pipeline_streams_with_a_chunked_denoiser_and_a_chunked_stretch():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        dn = Denoiser.from_vocoder(eng.forward, frames=24, device=DEV)
        ts = model("default")
        stretch = ts.at(0.8).chunked()
        assert isinstance(stretch, ChunkedStretch)
        pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=16, denoiser=dn.chunked(), stretch=stretch)
        mel = torch.from_numpy(seeded_mel(3, 2, 48, log_mel=True)).to(DEV)
        want = pipe.infer(mel).clone()
        plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=16)
        assert torch.equal(want, ts.forward_device(dn.forward_device(plain.infer(mel)), 0.8)[0])
        assert want.shape[1] == ts.out_samples(256 * 48, 0.8) == 15360
        pieces = list(pipe.stream(mel))
        assert all(p.shape[1] > 0 for p in pieces) and torch.equal(torch.cat(pieces, dim=1), want)
        session = pipe.session()
        got, at = [], 0
        for t in (7, 25, 16):
            got += session.push(mel[:, :, at:at + t])
            at += t
        got += session.flush()
        assert all(p.shape[1] > 0 for p in got) and torch.equal(torch.cat(got, dim=1), want)
        with pytest.raises(ValueError, match="fp32"):
            MelToWavePipeline(None, eng.forward_pcm16, device=DEV, chunk_frames=16, stretch=stretch)
        refusing = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=16, denoiser=dn.chunked(), stretch=ts.at(0.8))
        with pytest.raises(ValueError, match=r"\.chunked\(\)"):
            next(iter(refusing.stream(mel)))
        with pytest.raises(ValueError, match=r"\.chunked\(\)"):
            refusing.session()
    finally:
        eng.close()
