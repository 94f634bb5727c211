"""The chunked bias denoiser without a GPU: ``iris_denoiser_window_range`` against a brute-force restatement of the finality
rule, the bookkeeping of ``DenoiserSession`` against a fake windowed denoiser, and the pipeline's chunked routes with a fake
vocoder.  The device itself is tests/test_gpu_denoiser_chunked.py's.

The rule, from the definition (include/iris_hifigan.h, "Windows"): with N = n_fft, H = hop, a window holds samples
[o, o + Lw) of an utterance, o = H m0, Lw = H Mw.  Frame t covers samples [t H - N / 2, t H + N / 2) and exists when t >= 0
and, only if the window is final, t <= m0 + Mw.  The utterance begins at sample 0 and ends at o + Lw if the window is final;
otherwise its end is not known, so every sample from o + Lw on may belong to it.  A frame is computable when every sample of
its span that lies inside the utterance lies inside the window.  Sample s, in row j = floor((s + N / 2) / H), is final when
each of frames j - N / H + 1 .. j is computable or does not exist.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import ChunkedDenoiser, Denoiser, DenoiserSession
from iris.pipeline import MelToWavePipeline

import denoiser_cases as C

CONFIG_NAMES = ("default", "small", "two_tap")


# ---- the finality rule -------------------------------------------------------------------------------------------------
def brute_force_range(n_fft: int, hop: int, m0: int, Mw: int, final: bool):
    """The final samples of the window as a sorted list, sample by sample and frame by frame from the definition above."""
    N, H, taps, half = n_fft, hop, n_fft // hop, n_fft // 2
    o, end = H * m0, H * (m0 + Mw)

    def exists(t):
        return t >= 0 and (not final or t <= m0 + Mw)

    computable = {}

    def is_computable(t):
        if t not in computable:
            s = np.arange(t * H - half, t * H + half)
            in_utterance = (s >= 0) & ((s < end) if final else True)
            in_window = (s >= o) & (s < end)
            computable[t] = bool(np.all(in_window[in_utterance]))
        return computable[t]

    out = []
    for s in range(o, end):
        j = (s + half) // H
        if all((not exists(t)) or is_computable(t) for t in range(j - taps + 1, j + 1)):
            out.append(s)
    return out


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_window_range_is_the_finality_rule(name):
    n_fft, hop, win = C.stft_args(name)
    dn = Denoiser(n_fft, hop, win)
    for m0 in (0, 1, 5):
        for Mw in range(13):
            for final in (False, True):
                want = brute_force_range(n_fft, hop, m0, Mw, final)
                lo, count = dn.window_range(hop * m0, hop * Mw, final)
                assert count == len(want), (name, m0, Mw, final)
                if want:
                    assert want == list(range(lo, lo + count)), (name, m0, Mw, final)       # one range, and this one
                else:
                    assert lo == hop * m0
                assert dn.window_launch_count(2, hop * Mw, hop * m0, final) == (2 if count else 0)
    # what an interior window loses on either side comes from the design: (n_fft / hop - 1) frames
    lo, count = dn.window_range(hop * 5, hop * 12, False)
    lost = (n_fft // hop - 1) * hop
    assert (lo - hop * 5, hop * 17 - (lo + count)) == (lost, lost)
    assert DenoiserSession(dn).halo == (lost, lost)
    assert dn.window_workspace_bytes(2, hop * 12) == dn.workspace_bytes(2, hop * 12)


def _status(fn, *args):
    with pytest.raises(_native.NativeCallError) as err:
        fn(*args)
    return err.value.status


def test_window_queries_refuse():
    dn = Denoiser()
    INVALID, UNSUPPORTED = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    assert _status(dn.window_range, 255, 256 * 8, False) == INVALID                   # origin is no multiple of hop
    assert _status(dn.window_range, 256, 256 * 8 + 4, False) == INVALID               # nor is Lw
    assert _status(dn.window_range, -256, 256 * 8, False) == INVALID
    assert _status(dn.window_range, 256, -256, True) == INVALID
    assert _status(dn.window_launch_count, 1, 256 * 8, 100, False) == INVALID
    assert _status(dn.window_launch_count, 65536, 256 * 8, 0, False) == UNSUPPORTED
    assert _status(Denoiser(1024, 300, 1024).window_range, 0, 300 * 8, False) == UNSUPPORTED
    assert dn.window_range(256 * (1 << 40), 256 * 8, False) == (256 * (1 << 40) + 768, 512)     # 64-bit origins
    lib = _native.load()
    cfg, lo, n = dn.native_config(), ctypes.c_int64(), ctypes.c_int32()
    assert lib.iris_denoiser_window_range(ctypes.byref(cfg), 0, 256, 0, None, ctypes.byref(lo)) == INVALID
    assert lib.iris_denoiser_window_range(None, 0, 256, 0, ctypes.byref(lo), ctypes.byref(lo)) == INVALID
    assert lib.iris_denoiser_window_launch_count(ctypes.byref(cfg), 1, 256, 0, 0, None) == INVALID
    # a NULL handle is refused before anything else is looked at; nothing needs a device
    assert lib.iris_denoiser_forward_window(None, None, 1, 256 * 8, 0, 0, 0.1, None, None, 0, None) == INVALID
    assert len(_native.DENOISER_SYMBOLS["iris_denoiser_forward_window"][1]) == 11


# ---- the session's bookkeeping, against a fake windowed denoiser ---------------------------------------------------------
class _FakeWindowed:
    """A windowed "denoiser" on the host whose sample s is a function of s itself and of the utterance at s - left, s and
    s + right - 1 (0 outside the utterance) -- all three inside the span of the sample's own frames, so a window that
    settles s must hold them.  It asserts that, and computes in integers held exactly by fp32.  ``window_range`` is the
    library's own (host only)."""

    def __init__(self, name: str):
        n_fft, hop, win = C.stft_args(name)
        self.real = Denoiser(n_fft, hop, win)
        self.hop_length, self.n_fft = hop, n_fft
        self.reach = (n_fft // hop - 1) * hop
        self.strength = 0.5
        self.windows = []

    def window_range(self, origin, Lw, final):
        return self.real.window_range(origin, Lw, final)

    def forward_window(self, wav, origin, final, strength=None):
        B, Lw = wav.shape
        lo, count = self.window_range(origin, Lw, final)
        assert count > 0, "a window that settles nothing must not be launched"
        self.windows.append((origin, Lw, bool(final), lo, count))
        end = origin + Lw

        def at(s):                                            # the utterance at global samples s [count]
            inside = (s >= 0) & ((s < end) if final else torch.ones_like(s, dtype=torch.bool))
            held = (s >= origin) & (s < end)
            assert bool((held | ~inside).all()), "the window lacks a sample that one of its final samples reads"
            idx = (s - origin).clamp(0, Lw - 1)
            return torch.where(inside, wav[:, idx], torch.zeros((), dtype=wav.dtype))

        s = torch.arange(lo, lo + count)
        scale = (1.0 if strength is None else float(strength))
        return scale * ((s % 7 + 1).float() * at(s) + 2.0 * at(s - self.reach) + 4.0 * at(s + self.reach - 1))

    def forward_device(self, wav, lengths=None, strength=None):
        assert lengths is None or all(int(n) * self.hop_length == wav.shape[1] for n in lengths)      # no ragged form here
        if wav.shape[1] == 0:
            return wav.clone()
        out = self.forward_window(wav, 0, True, strength=strength)
        self.windows.pop()
        assert out.shape == wav.shape
        return out

    def open_session(self, strength=None):
        return DenoiserSession(self, strength=strength)


def _utterance(B: int, n: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(5 + n).integers(-50, 50, (B, n)).astype(np.float32))


SCHEDULES = {"single frames": lambda M: [1] * M, "one piece": lambda M: [M],
             "mixed": lambda M: [3, 1, 0, 7, 1, 1, 2, M - 15] if M >= 16 else [M]}


@pytest.mark.parametrize("name", CONFIG_NAMES)
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_session_equals_the_one_shot_and_tiles_the_utterance(name, schedule):
    for M in (1, 2, 5, 21):
        fake = _FakeWindowed(name)
        hop = fake.hop_length
        wav = _utterance(2, hop * M)
        want = fake.forward_device(wav)
        session = fake.open_session()
        left, right = session.halo
        got, at = [], 0
        for m in SCHEDULES[schedule](M):
            piece = session.push(wav[:, at:at + hop * m])
            at += hop * m
            assert piece.shape[0] == 2 and session.samples_received == at
            assert session.samples_emitted == sum(p.shape[1] for p in got) + piece.shape[1]
            assert session.samples_buffered <= left + right + hop * m, (name, schedule, M)
            got.append(piece)
        got.append(session.flush())
        assert session.samples_emitted == hop * M and session.samples_buffered == 0
        assert torch.equal(torch.cat(got, dim=1), want), (name, schedule, M)
        # the windows' final ranges tile [0, L): no gap and no overlap.  The one exception is a window that still starts at
        # sample 0 because the next sample due lies within `left` of it: no later origin settles that sample, so the window
        # settles [0, ...) again and the session drops what it has emitted.  A push that settles nothing launched nothing.
        edge = 0
        for origin, Lw, final, lo, count in fake.windows:
            assert origin % hop == 0 and lo + count > edge, (name, schedule, M, fake.windows)
            if origin:
                assert lo == edge, (name, schedule, M, fake.windows)
            else:
                assert lo == 0 and edge < left + hop, (name, schedule, M, fake.windows)
            edge = lo + count
        assert edge == hop * M
        assert sum(1 for w in fake.windows if w[2]) == 1 and fake.windows[-1][2]
        assert session.flush().shape == (2, 0)


def test_a_short_utterance_comes_from_flush():
    fake = _FakeWindowed("small")                             # taps = 4: 3 frames on either side
    hop = fake.hop_length
    wav = _utterance(1, hop * 3)
    session = fake.open_session(strength=2.0)
    assert session.push(wav[:, :hop]).shape == (1, 0) and session.push(wav[:, hop:]).shape == (1, 0)
    assert fake.windows == []
    assert torch.equal(session.flush(), fake.forward_device(wav, strength=2.0))
    # nothing pushed at all
    assert fake.open_session().flush().shape[1] == 0


def test_session_refusals():
    fake = _FakeWindowed("small")
    hop = fake.hop_length
    session = fake.open_session()
    with pytest.raises(ValueError):
        session.push(torch.zeros(2, hop + 1))                 # no multiple of hop
    with pytest.raises(ValueError):
        session.push(torch.zeros(2, hop), lengths=[1, 1])     # ragged batches stay on the whole-utterance route
    with pytest.raises(ValueError):
        session.push(torch.zeros(2, hop, dtype=torch.int16))
    with pytest.raises(ValueError):
        session.push(torch.zeros(hop))
    session.push(torch.zeros(2, hop))
    with pytest.raises(ValueError):
        session.push(torch.zeros(3, hop))                     # a change of B
    session.flush()
    with pytest.raises(RuntimeError):
        session.push(torch.zeros(2, hop))
    with pytest.raises(ValueError):
        Denoiser().open_session(strength=-1.0)


def test_chunked_wrapper_forwards():
    fake = _FakeWindowed("small")
    wrapped = ChunkedDenoiser(fake)
    assert wrapped.chunked_sessions and wrapped.strength == 0.5 and wrapped.hop_length == fake.hop_length
    wav = _utterance(1, fake.hop_length * 6)
    assert torch.equal(wrapped.forward_device(wav), fake.forward_device(wav))
    assert isinstance(wrapped.open_session(), DenoiserSession)
    dn = Denoiser()
    assert isinstance(dn.chunked(), ChunkedDenoiser) and dn.chunked().dn is dn
    assert not getattr(dn, "chunked_sessions", False)         # a plain Denoiser is no opt-in


# ---- the pipeline ------------------------------------------------------------------------------------------------------
HOP = C.CONFIGS["small"]["hop_length"]


class _Vocode:
    cfg = None

    def forward(self, mel, lengths=None):
        return mel.sum(dim=1).repeat_interleave(HOP, dim=1)

    def forward_pcm16(self, mel, lengths=None):
        return self.forward(mel).to(torch.int16)


class _Int16Vocode:
    cfg = None

    def forward(self, mel, lengths=None):
        return mel.sum(dim=1).repeat_interleave(HOP, dim=1).to(torch.int16)


class _Doubler:
    def forward_device(self, wav, lengths=None):
        return 2.0 * wav


def _mel(T: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(T).integers(-9, 9, (2, 3, T)).astype(np.float32))


@pytest.mark.parametrize("chunk_frames", (2, 4, 16))
def test_pipeline_streams_through_a_chunked_denoiser(chunk_frames):
    fake = _FakeWindowed("small")
    voc = _Vocode()
    pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=chunk_frames, denoiser=ChunkedDenoiser(fake))
    mel = _mel(21)
    want = pipe.infer(mel)
    assert torch.equal(want, fake.forward_device(voc.forward(mel)))
    pieces = list(pipe.stream(mel))
    assert all(p.shape[1] > 0 for p in pieces)                # empty pieces are skipped ...
    n_chunks = -(-21 // chunk_frames)
    assert len(pieces) == n_chunks + 1 - (1 if chunk_frames == 2 else 0)     # ... and a 2-frame chunk is below the 3-frame halo
    assert pieces[0].shape[1] == max(HOP * chunk_frames - 3 * HOP, 0) or chunk_frames == 2
    assert pieces[-1].shape[1] == 3 * HOP                     # the last piece carries the halo
    assert torch.equal(torch.cat(pieces, dim=1), want)

    session = pipe.session()
    got, at = [], 0
    for t in (7, 1, 0, 9, 4):
        got += session.push(mel[:, :, at:at + t])
        at += t
    got += session.flush()
    assert all(p.shape[1] > 0 for p in got)
    assert torch.equal(torch.cat(got, dim=1), want)

    batch = pipe.infer_batch([mel[0], mel[1]])                # the whole-utterance routes go through the wrapper
    assert torch.equal(torch.stack(batch), want)


def test_pipeline_refusals():
    fake = _FakeWindowed("small")
    voc = _Vocode()
    mel = _mel(9)
    with pytest.raises(ValueError, match="fp32"):
        MelToWavePipeline(None, voc.forward_pcm16, hop_length=HOP, chunk_frames=4, denoiser=ChunkedDenoiser(fake))
    ints = MelToWavePipeline(None, _Int16Vocode().forward, hop_length=HOP, chunk_frames=4, denoiser=ChunkedDenoiser(fake))
    with pytest.raises(ValueError, match="fp32"):
        list(ints.stream(mel))
    # a plain denoiser and a duck-typed one keep refusing, with the message they had
    for plain in (Denoiser(*C.stft_args("small")), _Doubler()):
        pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, denoiser=plain)
        with pytest.raises(ValueError, match="no chunked denoiser is built"):
            next(iter(pipe.stream(mel)))
        with pytest.raises(ValueError, match="denoiser"):
            pipe.session()

    class _Whole:                                             # a whole-utterance vocoder stays refused
        whole_utterance, hop_length = True, HOP

        def forward_device(self, mel):
            return mel.sum(dim=1).repeat_interleave(HOP, dim=1)[:, HOP:]

    whole = MelToWavePipeline(None, _Whole(), denoiser=ChunkedDenoiser(fake))
    with pytest.raises(NotImplementedError):
        next(iter(whole.stream(mel)))
    with pytest.raises(NotImplementedError):
        whole.session()
