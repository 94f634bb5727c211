"""The chunked limiter without a GPU: ``iris_limiter_window_range`` against its closed form and the refusals of the host-only
queries, the bookkeeping of ``LimiterSession`` against a fake windowed limiter built on the numpy restatement
(tests/limiter_restatement.py: ``device_f32``), and the pipeline's chunked routes with fake stages.  The device itself is
tests/test_gpu_limiter_chunked.py's.

The rule (csrc/limiter.h, "Windows"): with ``R = 2A + 7``, a window holds samples ``[origin, origin + Lw)`` of an utterance, starts
it when ``origin == 0`` and ends it when ``final``; it settles

    out_lo = origin + (origin > 0 ? R : 0);  out_hi = origin + Lw - (final ? 0 : R);  count = max(0, out_hi - out_lo).

What the reach test found.  ``R`` is the tile kernel's halo and is one sample more than the rules read: ``out[n]`` reads ``g[n]``,
which reads ``r`` within ``2A``, which reads ``u[k - 1]`` and ``u[k]``, which read ``x[k - 6 .. k + 6]`` -- ``x`` within ``2A + 6``.  So
a fake whose reach is ``R - 1`` still reproduces the one-shot bits on every input, and the reach that must make the comparison
fail is ``R - 2``: ``test_the_reach_is_pinned`` asserts that for ``A = 1`` on an input built for it (an over-the-ceiling point
BETWEEN two samples six samples in front of a cut, and a spike right behind the cut), and asserts that ``R - 1`` does not.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.limiter import TILE as T, ChunkedLimiter, Limiter, LimiterSession
from iris.pipeline import MelToWavePipeline

import limiter_cases as C
import limiter_restatement as R

LOOKAHEADS = (1, 33, 256)
_tables = {}


def table_of(A):
    if A not in _tables:
        _tables[A] = Limiter(C.RATE, 0.0, float(A)).design()
    return _tables[A]


def reach_of(A):
    return 2 * A + 7


def closed_form(reach, origin, Lw, final):
    lo = origin + (reach if origin > 0 else 0)
    hi = origin + Lw - (0 if final else reach)
    return lo, max(0, hi - lo)


def schedules(A, L):
    """The piece schedules of the issue, each summing to ``L``: one push; pieces that give empty outputs, a first window that
    settles exactly one sample and origins off any multiple of 4; equal pieces of 257; the cut at ``T + 5``."""
    Rr = reach_of(A)
    odd = [1, Rr - 1, 1, Rr + 1, T - 1, 3]
    equal = [257] * (L // 257) + ([L % 257] if L % 257 else [])
    return {"one push": [L], "odd pieces": odd + [L - sum(odd)], "equal 257": equal, "cut at T + 5": [T + 5, L - T - 5]}


# ---- the finality rule and the host-only queries ---------------------------------------------------------------------------
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_window_range_is_the_closed_form(A):
    lim, Rr = Limiter(C.RATE, -3.0, float(A)), reach_of(A)
    for origin in (0, 1, Rr - 1, Rr, 4099):
        for Lw in (0, 1, Rr, 2 * Rr - 1, 2 * Rr, 2 * Rr + 1, 5000):
            for final in (False, True):
                lo, count = closed_form(Rr, origin, Lw, final)
                assert lim.window_range(origin, Lw, final) == (lo, count), (A, origin, Lw, final)
                for B in (0, 1, 6):
                    want = 0 if (count == 0 or B == 0) else 2
                    assert lim.window_launch_count(B, Lw, origin, final) == want, (A, B, origin, Lw, final)
            assert lim.window_workspace_bytes(6, Lw) == lim.workspace_bytes(6, Lw)
    assert LimiterSession(lim).halo == (Rr, Rr)
    assert lim.window_range((1 << 40) + 3, 5000, False) == ((1 << 40) + 3 + Rr, 5000 - 2 * Rr)       # 64-bit origins


def _status(fn, *args):
    with pytest.raises(_native.NativeCallError) as err:
        fn(*args)
    return err.value.status


def test_window_queries_refuse():
    lim = Limiter()
    INVALID, UNSUPPORTED = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    assert _status(lim.window_range, -1, 100, False) == INVALID
    assert _status(lim.window_range, 0, -1, True) == INVALID
    assert _status(lim.window_launch_count, 1, 100, -1, False) == INVALID
    assert _status(lim.window_launch_count, -1, 100, 0, False) == INVALID
    assert _status(lim.window_launch_count, 65536, 100, 0, False) == UNSUPPORTED                    # grid.y
    assert _status(lim.window_launch_count, 4096, 1 << 19, 0, False) == UNSUPPORTED                  # B Lw = 2^31
    assert _status(lim.window_workspace_bytes, 2, -1) == INVALID
    top = (1 << 63) - 1
    assert lim.window_range(top - 100, 100, True) == (top - 100 + 73, 27)                            # origin + Lw = 2^63 - 1: the last index
    assert _status(lim.window_range, top - 99, 100, True) == UNSUPPORTED                             # beyond int64 sample indexing
    assert _status(lim.window_launch_count, 1, 100, top - 99, False) == UNSUPPORTED
    lib = _native.load()
    cfg, lo, n, nbytes = lim.native_config(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_uint64()
    bad = _native.LimiterConfig(0.9, 0)
    assert lib.iris_limiter_window_range(ctypes.byref(cfg), 0, 256, 0, None, ctypes.byref(lo)) == INVALID
    assert lib.iris_limiter_window_range(ctypes.byref(cfg), 0, 256, 0, ctypes.byref(lo), None) == INVALID
    assert lib.iris_limiter_window_range(None, 0, 256, 0, ctypes.byref(lo), ctypes.byref(lo)) == INVALID
    assert lib.iris_limiter_window_range(ctypes.byref(bad), 0, 256, 0, ctypes.byref(lo), ctypes.byref(lo)) == INVALID
    assert lib.iris_limiter_window_launch_count(ctypes.byref(cfg), 1, 256, 0, 0, None) == INVALID
    assert lib.iris_limiter_window_launch_count(ctypes.byref(bad), 1, 256, 0, 0, ctypes.byref(n)) == INVALID
    assert lib.iris_limiter_window_workspace_bytes(ctypes.byref(cfg), 1, 256, None) == INVALID
    assert lib.iris_limiter_window_workspace_bytes(None, 1, 256, ctypes.byref(nbytes)) == INVALID
    # a NULL handle is refused before anything else is looked at; nothing needs a device
    assert lib.iris_limiter_forward_window(None, None, 1, 2048, 0, 0, None, 0, None, None, 0, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
    assert len(_native.LIMITER_SYMBOLS["iris_limiter_forward_window"][1]) == 12
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION == 4


# ---- the session's bookkeeping, against a fake built on the restatement ----------------------------------------------------
class _FakeWindowed:
    """A windowed limiter on the host: ``forward_window`` is ``R.device_f32`` of the window itself -- its edges taken for edges
    of an item, zeros and ``r = 1`` beyond them, as the kernel stages them -- cut to the range ``window_range`` names, with ``(max
    p, min g)`` over that range.  ``reach``: what ``window_range`` holds back, ``2A + 7`` unless a test asks for less."""

    def __init__(self, A, c=1.0, reach=None):
        self.A, self.c, self.table = A, c, table_of(A)
        self.reach = reach_of(A) if reach is None else reach
        self.windows = []

    def window_range(self, origin, Lw, final):
        return closed_form(self.reach, origin, Lw, final)

    def forward_window(self, wav, origin, final, pcm16=False):
        B, Lw = wav.shape
        lo, count = self.window_range(origin, Lw, final)
        assert count > 0, "a window that settles nothing must not be launched"
        self.windows.append((origin, Lw, bool(final), lo, count))
        a = lo - origin
        out, stats = np.zeros((B, count), np.float32), np.zeros((B, 2), np.float32)
        for b in range(B):
            res = R.device_f32(wav[b].numpy(), self.c, self.A, self.table)
            out[b] = res["out"][a:a + count]
            stats[b] = (res["p"][a:a + count].max(), res["g"][a:a + count].min())
        return torch.from_numpy(out), torch.from_numpy(stats)

    def whole(self, wav):
        """``(out [B, L], stats [B, 2])`` of the one-shot call, from the restatement."""
        res = [R.device_f32(row.numpy(), self.c, self.A, self.table) for row in wav]
        stats = np.array([[r["tp"], r["min_g"]] for r in res], np.float32).reshape(len(res), 2)
        return torch.from_numpy(np.stack([r["out"] for r in res])), torch.from_numpy(stats)


def _utterance(A, c=1.0):
    """Three items of ``2T + 3`` samples: one that is never limited, the placements' seam item, and the window-specific one --
    spikes at ``cut - 1`` and ``cut + R`` for the cut at ``T + 5``, so the first spike's gain ramp lies within ``R`` of a window edge
    on both sides of the cut."""
    n, cut = 2 * T + 3, T + 5
    items = [C.quiet(n, c, 700 + A), C.spiked(n, c, 701 + A, [T - 1, T]), C.spiked(n, c, 702 + A, [cut - 1, cut + reach_of(A)])]
    return torch.from_numpy(np.stack(items))


def _run_session(fake, wav, pieces, check_bound=True):
    session, got, at = LimiterSession(fake), [], 0
    Rr = fake.reach
    for n in pieces:
        piece = session.push(wav[:, at:at + n])
        at += n
        assert piece.shape[0] == wav.shape[0] and session.samples_received == at
        assert session.samples_emitted == sum(p.shape[1] for p in got) + piece.shape[1] == max(0, at - Rr)
        if check_bound:
            assert session.samples_buffered <= 2 * Rr + n, (pieces, at)
        got.append(piece)
    got.append(session.flush())
    assert session.samples_emitted == wav.shape[1] and session.samples_buffered == 0
    return session, torch.cat(got, dim=1)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("A", LOOKAHEADS)
def test_session_equals_the_one_shot_restatement(A):
    wav = _utterance(A)
    L = wav.shape[1]
    fake = _FakeWindowed(A)
    want, want_stats = fake.whole(wav)
    assert float(want_stats[0, 1]) == 1.0 and float(want_stats[1:, 1].max()) < 1.0           # one item untouched, two limited
    for name, pieces in schedules(A, L).items():
        assert sum(pieces) == L
        fake.windows = []
        session, got = _run_session(fake, wav, pieces)
        assert torch.equal(_bits(got), _bits(want)), (A, name)
        assert torch.equal(_bits(session.stats), _bits(want_stats)), (A, name)
        # the windows' settled ranges tile [0, L) -- but for a window that still starts at sample 0 and settles [0, ...) again
        edge = 0
        for origin, Lw, final, lo, count in fake.windows:
            assert lo + count > edge and (lo == edge if origin else lo == 0), (A, name, fake.windows)
            edge = lo + count
        assert edge == L and sum(1 for w in fake.windows if w[2]) == 1 and fake.windows[-1][2]
        assert session.flush().shape == (3, 0)
    # the first piece is short by R, or empty with no launch; flush returns the last R
    Rr = reach_of(A)
    session = LimiterSession(fake)
    fake.windows = []
    assert session.stats is None
    assert session.push(wav[:, :Rr]).shape == (3, 0) and fake.windows == []
    assert torch.equal(session.stats, torch.tensor([[0.0, 1.0]] * 3))                         # before any window: (0, 1)
    assert session.push(wav[:, Rr:Rr + 1]).shape == (3, 1)
    assert session.push(wav[:, Rr + 1:]).shape == (3, L - Rr - 1) and session.flush().shape == (3, Rr)


def test_empty_pushes_and_an_empty_utterance():
    fake = _FakeWindowed(1)
    wav = _utterance(1)[:, :300]
    want, want_stats = fake.whole(wav)
    session, got = _run_session(fake, wav, [0, 100, 0, 0, 200, 0])
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(session.stats), _bits(want_stats))
    # shorter than R: everything comes from flush, in one final window
    fake.windows = []
    session, got = _run_session(fake, wav[:, :5], [2, 3])
    assert torch.equal(_bits(got), _bits(fake.whole(wav[:, :5])[0])) and len(fake.windows) == 1
    # an utterance of no samples, and nothing pushed at all
    fake.windows = []
    session = LimiterSession(fake)
    assert session.push(wav[:, :0]).shape == (3, 0) and session.flush().shape == (3, 0) and fake.windows == []
    assert torch.equal(session.stats, torch.tensor([[0.0, 1.0]] * 3))
    idle = LimiterSession(fake, pcm16=True)
    assert idle.flush().shape[1] == 0 and idle.flush().dtype == torch.int16 and idle.stats is None


def test_session_refusals():
    fake = _FakeWindowed(1)
    session = LimiterSession(fake)
    with pytest.raises(ValueError, match="ragged batches stay on"):
        session.push(torch.zeros(2, 10), lengths=[1, 1])
    with pytest.raises(ValueError):
        session.push(torch.zeros(2, 10, dtype=torch.int16))
    with pytest.raises(ValueError):
        session.push(torch.zeros(10))
    session.push(torch.zeros(2, 10))
    with pytest.raises(ValueError):
        session.push(torch.zeros(3, 10))                      # a change of B
    session.flush()
    with pytest.raises(RuntimeError, match="flushed"):
        session.push(torch.zeros(2, 10))


def test_the_reach_is_pinned():
    """``A = 1``, ``R = 9``.  Samples k and k + 1 are 0.9 each, so the point between them (about 1.14) is over the ceiling 1.0 and
    ``p[k]`` is ``|u[k, 2]|``, a chain over ``x[k - 5 .. k + 6]``; a spike sits at ``k + 6`` and the first piece ends right in front of
    it.  A window that settles ``g[k - 2]`` (it reads ``r[k]``) without holding ``x[k + 6]`` gets other bits: that is a reach of 7 =
    ``R - 2``.  With a reach of ``R - 1`` = 8 the last sample settled is ``k - 3``, which reads ``r[k - 1]`` and so ``x`` up to ``k + 5``:
    the rules read ``x`` within ``2A + 6``, one less than the kernel's halo ``R``, so ``R - 1`` cannot fail on any input."""
    A, k, n = 1, 400, 900
    y = C.quiet(n, 1.0, 77)
    y[k] = y[k + 1] = 0.9
    y[k + 6] = 1.5
    wav = torch.from_numpy(y[None].copy())
    table = table_of(A)
    ref = R.plain_f64(y, 1.0, A, table)
    assert ref["p"][k] > 1.0 and abs(ref["u"][k + 1, 1]) == ref["p"][k] and abs(float(y[k])) < 1.0      # the point, not a sample
    want = _FakeWindowed(A).whole(wav)[0]
    pieces = [k + 6, n - k - 6]
    mismatches = {}
    for reach in (reach_of(A), reach_of(A) - 1, reach_of(A) - 2):
        _, got = _run_session(_FakeWindowed(A, reach=reach), wav, pieces, check_bound=False)
        mismatches[reach] = int((_bits(got) != _bits(want)).sum())
    print(f"A = 1: samples that differ from the one-shot restatement by the fake's reach: {mismatches}")
    assert mismatches[reach_of(A)] == 0
    assert mismatches[reach_of(A) - 2] > 0                    # two short of R: the comparison fails
    assert mismatches[reach_of(A) - 1] == 0                   # one short: R has a sample to spare (the docstring above)


def test_chunked_wrapper_forwards():
    class _Lim(_FakeWindowed):
        def __init__(self):
            super().__init__(1)

        def limit_device(self, wav, lengths=None, row_scale=1):
            return ("limit", lengths, row_scale)

        def true_peak_device(self, wav, lengths=None, row_scale=1):
            return ("peak", lengths, row_scale)

    wrapped = ChunkedLimiter(_Lim(), pcm16=True)
    assert wrapped.chunked_sessions and wrapped.pcm16
    assert wrapped.limit_device(None, lengths=[1], row_scale=4) == ("limit", [1], 4)
    assert wrapped.true_peak_device(None, lengths=[2], row_scale=2) == ("peak", [2], 2)
    session = wrapped.open_session()
    assert isinstance(session, LimiterSession) and session.pcm16
    lim = Limiter()
    assert isinstance(lim.chunked(), ChunkedLimiter) and lim.chunked().lim is lim and not lim.chunked().pcm16
    assert lim.chunked(pcm16=True).pcm16 and not lim.open_session().pcm16 and lim.open_session(pcm16=True).pcm16
    assert not getattr(lim, "chunked_sessions", False)        # a plain Limiter is no opt-in


# ---- the pipeline's plumbing, with fake stages -----------------------------------------------------------------------------
HOP = 4


class _HoldSession:
    """Applies ``fn`` sample by sample, holds the last ``hold`` samples back until ``flush``, and notes every call."""

    def __init__(self, log, name, fn, hold):
        self.log, self.name, self.fn, self.hold = log, name, fn, hold
        self.buf = None

    def push(self, piece):
        self.log.append((self.name, "push", int(piece.shape[1])))
        self.buf = piece if self.buf is None else torch.cat([self.buf, piece], dim=1)
        n = max(0, self.buf.shape[1] - self.hold)
        out, self.buf = self.buf[:, :n], self.buf[:, n:]
        return self.fn(out)

    def flush(self):
        self.log.append((self.name, "flush", 0 if self.buf is None else int(self.buf.shape[1])))
        out, self.buf = (torch.zeros((0, 0)) if self.buf is None else self.buf), None
        return self.fn(out)


class _Stage:
    """Stands in for a chunked denoiser (doubles), stretch (adds 1) or limiter (clips at 5): three maps that do not commute."""

    chunked_sessions = True
    hop_length = HOP
    FNS = {"denoiser": lambda w: w * 2.0, "stretch": lambda w: w + 1.0, "limiter": lambda w: w.clamp(-5.0, 5.0)}

    def __init__(self, log, name, hold):
        self.log, self.name, self.hold, self.fn = log, name, hold, self.FNS[name]

    def forward_device(self, wav, lengths=None):
        return self.fn(wav) if self.name == "denoiser" else (self.fn(wav), None)

    def out_samples(self, L):
        return L

    def limit_device(self, wav, lengths=None, row_scale=1):
        return self.fn(wav), torch.zeros((wav.shape[0], 2))

    def open_session(self):
        self.log.append((self.name, "open", 0))
        return _HoldSession(self.log, self.name, self.fn, self.hold)


class _PlainLimiter:
    def limit_device(self, wav, lengths=None, row_scale=1):
        return wav.clamp(-5.0, 5.0), torch.zeros((wav.shape[0], 2))


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


def _mel(frames):
    return torch.from_numpy(np.random.default_rng(frames).integers(-2, 3, (2, 3, frames)).astype(np.float32))


def test_pipeline_runs_the_limiter_session_last_and_flush_cascades():
    log, voc, mel = [], _Vocode(), _mel(10)
    stages = dict(denoiser=_Stage(log, "denoiser", 6), stretch=_Stage(log, "stretch", 2), limiter=_Stage(log, "limiter", 3))
    pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, **stages)
    want = pipe.infer(mel)
    assert torch.equal(want, (voc.forward(mel) * 2.0 + 1.0).clamp(-5.0, 5.0)) and float(want.abs().max()) == 5.0
    assert float((voc.forward(mel) * 2.0).clamp(-5.0, 5.0).add(1.0).max()) == 6.0             # another order gives another result
    assert log == []                                          # the whole-utterance route opens no session
    pieces = list(pipe.stream(mel))
    assert all(p.shape[1] > 0 for p in pieces) and torch.equal(torch.cat(pieces, dim=1), want)
    assert log[:3] == [("denoiser", "open", 0), ("stretch", "open", 0), ("limiter", "open", 0)]        # the order infer applies
    # chunks of 16, 16 and 8 samples: 10 leave the denoiser's session, 8 the stretch's, 5 the limiter's, and so on; then every
    # flush sends what it held through the sessions behind it before they are flushed themselves
    assert log[3:] == [("denoiser", "push", 16), ("stretch", "push", 10), ("limiter", "push", 8),
                       ("denoiser", "push", 16), ("stretch", "push", 16), ("limiter", "push", 16),
                       ("denoiser", "push", 8), ("stretch", "push", 8), ("limiter", "push", 8),
                       ("denoiser", "flush", 6), ("stretch", "push", 6), ("limiter", "push", 6),
                       ("stretch", "flush", 2), ("limiter", "push", 2), ("limiter", "flush", 3)]
    assert [p.shape[1] for p in pieces] == [5, 16, 8, 6, 2, 3]
    del log[:]
    session, got, at = pipe.session(), [], 0
    for t in (3, 0, 1, 5, 1):
        got += session.push(mel[:, :, at:at + t])
        at += t
    got += session.flush()
    assert all(p.shape[1] > 0 for p in got) and torch.equal(torch.cat(got, dim=1), want)
    assert [e for e in log if e[1] == "flush"] == [("denoiser", "flush", 6), ("stretch", "flush", 2), ("limiter", "flush", 3)]
    # the limiter alone, and the whole-utterance routes through the wrapper
    only = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, limiter=_Stage([], "limiter", 3))
    assert torch.equal(torch.cat(list(only.stream(mel)), dim=1), only.infer(mel))
    assert torch.equal(torch.stack(only.infer_batch([mel[0], mel[1]])), only.infer(mel))


def test_pipeline_refusals():
    voc, mel = _Vocode(), _mel(9)
    with pytest.raises(ValueError, match="a chunked limiter takes the vocoder's fp32 waveform"):
        MelToWavePipeline(None, voc.forward_pcm16, hop_length=HOP, chunk_frames=4, limiter=_Stage([], "limiter", 3))
    ints = MelToWavePipeline(None, _Int16Vocode().forward, hop_length=HOP, chunk_frames=4, limiter=_Stage([], "limiter", 3))
    with pytest.raises(ValueError, match="fp32"):
        list(ints.stream(mel))
    # a plain limiter and a duck-typed one keep refusing, and the message still matches what the existing tests look for
    for plain in (Limiter(), _PlainLimiter()):
        pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, limiter=plain)
        with pytest.raises(ValueError, match="limiter= cannot be streamed.*no chunked form is built"):
            next(iter(pipe.stream(mel)))
        with pytest.raises(ValueError, match=r"limiter=lim\.chunked\(\)"):
            pipe.session()
    # assemble= and loudness= beside a chunked limiter still refuse: their measures are the whole item's
    for kw in (dict(assemble=object()), dict(loudness=object())):
        pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, limiter=_Stage([], "limiter", 3), **kw)
        with pytest.raises(ValueError, match="no chunked form is built"):
            pipe.session()
