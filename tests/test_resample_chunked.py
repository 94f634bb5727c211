"""The chunked resampler without a GPU: the window rule (csrc/resample.h, ``struct Window``) in its closed form, the bookkeeping
of ``ResamplerSession`` against a fake windowed resampler built on the numpy restatement ``resample_host``, and the pipeline's
``output=`` routes with fake stages.  The device itself is tests/test_gpu_resample_chunked.py's.

The rule.  With ``Hw = half_width`` and ``i0(n) = floor(n * down / up)``, output ``n`` reads ``x[i0(n) - Hw + 1 .. i0(n) + Hw]``.  A
window holds samples ``[origin, origin + Lw)``, ``n_next`` is the first output not yet emitted, and it emits ``[n_next, n_hi)``:

    n_hi = ceil((origin + Lw) * up / down) if final else ceil(max(0, origin + Lw - Hw) * up / down)
    precondition: origin == 0 or i0(n_next) - Hw + 1 >= origin;   keep_from = max(0, i0(n_hi) - Hw + 1)

The fake's ``forward_window`` is ``resample_host`` of the window ALONE at its ``origin`` -- which takes everything outside the
window for zeros -- cut to ``[n_next, n_hi)``.  So a rule that emitted an output one tap early, or let go of a sample one tap
early, would read a zero where the utterance has a sample, and the comparison with ``resample_host`` of the whole, which is an
equality of bits, would fail: ``test_the_rule_is_tight`` shows that it does."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.pipeline import MelToWavePipeline
from iris.resample import ChunkedResampler, Resampler, ResamplerSession, design_bank, resample_host, window_plan
from iris.synthesis_output import alaw_from_pcm16, pcm16_from_float, ulaw_from_pcm16

RATES = (8000, 16000, 44100, 48000)
ENCODE = {"f32": lambda y: y, "pcm16": pcm16_from_float, "ulaw": lambda y: ulaw_from_pcm16(pcm16_from_float(y)),
          "alaw": lambda y: alaw_from_pcm16(pcm16_from_float(y))}
_fakes = {}


def ceil_div(a, b):
    return -((-a) // b)


class _FakeResampler:
    """A windowed resampler on the host.  Two ways in which ``window_plan`` can be made wrong on purpose (0 unless a test asks):
    ``emit_early`` settles outputs whose last ``emit_early`` taps the window does not hold, ``drop_early`` lets go of that many
    samples the next window still reads."""

    def __init__(self, rate_out, emit_early=0, drop_early=0):
        self.bank, self.up, self.down = design_bank(rate_out)
        self.rate_out, self.taps = rate_out, self.bank.shape[1]
        self.half_width = self.taps // 2
        self.emit_early, self.drop_early = emit_early, drop_early
        self.windows = []

    def out_range(self, origin, L):
        lo = ceil_div(origin * self.up, self.down)
        return lo, ceil_div((origin + L) * self.up, self.down) - lo

    def window_plan(self, origin, Lw, n_next, final):
        up, down, hw = self.up, self.down, self.half_width
        end = origin + Lw
        if origin and n_next * down // up - hw + 1 < origin - self.drop_early:
            raise ValueError("precondition")
        n_hi = ceil_div((end if final else max(0, end - hw + self.emit_early)) * up, down)
        return n_hi, max(0, n_hi * down // up - hw + 1 + self.drop_early)

    def forward_window(self, wav, origin, n_next, final, encoding="f32"):
        n_hi = self.window_plan(origin, wav.shape[1], n_next, final)[0]
        assert n_hi > n_next, "a window that emits nothing must not be launched"
        self.windows.append((origin, int(wav.shape[1]), n_next, n_hi, bool(final)))
        n_lo = self.out_range(origin, wav.shape[1])[0]
        assert n_lo <= n_next
        y = resample_host(wav.numpy(), self.bank, self.up, self.down, origin=origin)
        return torch.from_numpy(ENCODE[encoding](y[:, n_next - n_lo:n_hi - n_lo]).copy())

    def forward(self, wav, lengths=None, row_scale=1, origin=0, encoding="f32"):
        assert lengths is None
        return torch.from_numpy(ENCODE[encoding](resample_host(wav.numpy(), self.bank, self.up, self.down, origin=origin)).copy())


def fake_of(rate):
    if rate not in _fakes:
        _fakes[rate] = _FakeResampler(rate)
    return _fakes[rate]


def utterance(L, seed=0, B=2):
    return torch.from_numpy(np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, (B, L)).astype(np.float32))


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def run_session(fake, wav, pieces, encoding="f32"):
    """Pushes ``pieces`` (sizes summing to the length), flushes, and checks the counters on the way."""
    session, got, at = ResamplerSession(fake, encoding), [], 0
    hw, up, down = fake.half_width, fake.up, fake.down
    assert sum(pieces) == wav.shape[1]
    for n in pieces:
        piece = session.push(wav[:, at:at + n])
        at += n
        got.append(piece)
        assert piece.shape[0] == wav.shape[0] and session.samples_received == at
        assert session.samples_emitted == sum(p.shape[1] for p in got) == ceil_div(max(0, at - hw) * up, down)
        assert session.samples_buffered <= 2 * hw + ceil_div(down, up) + n, (pieces, at)
    got.append(session.flush())
    assert session.samples_emitted == ceil_div(wav.shape[1] * up, down) and session.samples_buffered == 0
    assert session.flush().shape[1] == 0
    return torch.cat(got, dim=1)


def schedules(hw, L):
    """The push sizes of the issue for an utterance of ``L`` samples (1 on its own: ``test_single_sample_pushes``)."""
    def equal(n):
        return [n] * (L // n) + ([L % n] if L % n else [])
    mix, left = [], L
    for n in (0, 1, hw + 1, 0, 0, 2 * hw + 1, 7, 0, hw - 1, 300):
        mix.append(min(n, left))
        left -= mix[-1]
    return {"Hw - 1": equal(hw - 1), "Hw": equal(hw), "Hw + 1": equal(hw + 1), "2 Hw + 1": equal(2 * hw + 1),
            "mix with empty pieces": mix + [left, 0], "one push then flush": [L]}


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_window_plan_is_the_closed_form(rate):
    fake = fake_of(rate)
    up, down, hw = fake.up, fake.down, fake.half_width
    if rate == 8000:
        assert (up, down, hw) == (160, 441, 45)
    for origin in (0, 1, hw, 4099, (1 << 40) - 5000):
        for Lw in (0, 1, hw - 1, hw, hw + 1, 2 * hw + 1, 5000):
            for final in (False, True):
                settled = origin + Lw if final else max(0, origin + Lw - hw)
                n_hi = ceil_div(settled * up, down)
                # the first output a window at this origin may begin with: the smallest n whose first tap is held
                n_min = 0 if origin == 0 else ceil_div((origin + hw - 1) * up, down)
                for n_next in sorted({n_min, n_min + 1, max(n_min, n_hi)}):
                    if n_next > ceil_div((origin + Lw) * up, down):
                        continue                              # (past the window's last output: refused, below)
                    got = window_plan(up, down, hw, origin, Lw, n_next, final)
                    assert got == (n_hi, max(0, n_hi * down // up - hw + 1)) == fake.window_plan(origin, Lw, n_next, final)
                    # what the rule promises: every emitted output's taps lie in the window or outside the utterance ...
                    if n_hi > n_next:
                        last = (n_hi - 1) * down // up + hw
                        assert final or last < origin + Lw
                        assert origin == 0 or n_next * down // up - hw + 1 >= origin
                    # ... the next output's last tap does not (or it would have been emitted), and keep_from holds its first
                    if not final:
                        assert n_hi * down // up + hw >= origin + Lw or origin + Lw < hw
                if origin and n_min > 0:
                    with pytest.raises(ValueError, match="reads from sample"):
                        window_plan(up, down, hw, origin, Lw + 2 * hw, n_min - 1, final)     # one output early: a tap is gone
    with pytest.raises(ValueError):
        window_plan(up, down, hw, -1, 10, 0, False)
    with pytest.raises(ValueError):
        window_plan(up, down, hw, 0, 10, ceil_div(10 * up, down) + 1, True)                   # past the window's outputs


@pytest.mark.parametrize("rate", RATES)
def test_session_equals_resample_host_of_the_whole(rate):
    fake = fake_of(rate)
    hw, up, down = fake.half_width, fake.up, fake.down
    L = 3001 if rate <= 16000 else 1201                       # (upsampling: 32 taps, 2.2 outputs per sample)
    wav = utterance(L, seed=rate)
    want = fake.forward(wav)
    assert want.shape == (2, ceil_div(L * up, down))
    for name, pieces in schedules(hw, L).items():
        fake.windows = []
        got = run_session(fake, wav, pieces)
        assert got.dtype == torch.float32 and torch.equal(bits(got), bits(want)), (rate, name)
        # the windows' outputs tile [0, N) and exactly one window is final
        edge = 0
        for origin, Lw, n_next, n_hi, final in fake.windows:
            assert n_next == edge and n_hi > n_next
            edge = n_hi
        assert edge == want.shape[1] and [w[4] for w in fake.windows].count(True) == 1 and fake.windows[-1][4]
    # the other store forms are the same samples, encoded
    for enc, dtype in (("pcm16", torch.int16), ("ulaw", torch.uint8), ("alaw", torch.uint8)):
        got = run_session(fake, wav, schedules(hw, L)["mix with empty pieces"], enc)
        assert got.dtype == dtype and torch.equal(got, fake.forward(wav, encoding=enc)), (rate, enc)


@pytest.mark.parametrize("rate", RATES)
def test_single_sample_pushes(rate):
    fake = fake_of(rate)
    wav = utterance(307, seed=rate + 1, B=1)
    assert torch.equal(bits(run_session(fake, wav, [1] * 307)), bits(fake.forward(wav)))


@pytest.mark.parametrize("rate", RATES)
def test_short_utterances_and_flush_with_nothing_pushed(rate):
    fake = fake_of(rate)
    hw = fake.half_width
    for L in (1, 2, hw - 1, hw, hw + 1, 2 * hw):
        wav = utterance(L, seed=L)
        want = fake.forward(wav)
        assert want.shape[1] == ceil_div(L * fake.up, fake.down) >= 1
        assert torch.equal(bits(run_session(fake, wav, [L])), bits(want))
        assert torch.equal(bits(run_session(fake, wav, [1] * L)), bits(want))
    fake.windows = []
    for enc, dtype in (("f32", torch.float32), ("ulaw", torch.uint8)):
        idle = ResamplerSession(fake, enc)
        out = idle.flush()
        assert out.shape[1] == 0 and out.dtype == dtype and idle.samples_emitted == idle.samples_buffered == 0
        empty = ResamplerSession(fake, enc)
        assert empty.push(torch.zeros(3, 0)).shape == (3, 0) and empty.flush().shape == (3, 0)
    assert fake.windows == []                                 # nothing was launched


def test_per_chunk_calls_at_a_running_origin_do_not_concatenate():
    """Why the window form is needed: ``forward(origin=running)`` partitions the outputs but takes the samples in front of its
    ``origin`` (and behind its chunk) for zeros."""
    fake = fake_of(8000)
    wav = torch.ones(1, 900)                                  # non-zero at every seam
    want = fake.forward(wav)
    got = torch.cat([fake.forward(wav[:, at:at + 300], origin=at) for at in (0, 300, 600)], dim=1)
    assert got.shape == want.shape                            # the ranges do partition the output ...
    differ = (bits(got) != bits(want))[0].nonzero()[:, 0]
    assert len(differ) > 0                                    # ... and the samples near a seam are other samples
    seams = np.array([300, 600]) * fake.up / fake.down
    assert all(np.abs(seams - int(n)).min() <= fake.half_width * fake.up / fake.down + 1 for n in differ)
    assert torch.equal(bits(run_session(fake, wav, [300, 300, 300])), bits(want))


def test_the_rule_is_tight():
    """A plan that emits one tap early, or lets go of a sample one tap early, no longer reproduces the whole."""
    rate = 8000
    wav = utterance(1500, seed=5, B=1)
    want = fake_of(rate).forward(wav)
    exact, hw = fake_of(rate), fake_of(rate).half_width
    # a first cut at which one more sample settles one more output (at 160 / 441 not every cut does)
    cut = next(n for n in range(500, 600) if ceil_div((n - hw + 1) * exact.up, exact.down) > ceil_div((n - hw) * exact.up, exact.down))
    pieces = [cut, 500, 1000 - cut]
    mismatches = {}
    for name, kw in (("exact", {}), ("emit one tap early", dict(emit_early=1)), ("drop one sample early", dict(drop_early=1))):
        fake = _FakeResampler(rate, **kw)
        session, got, at = ResamplerSession(fake), [], 0
        for n in pieces:
            got.append(session.push(wav[:, at:at + n]))
            at += n
        got = torch.cat(got + [session.flush()], dim=1)
        assert got.shape == want.shape
        mismatches[name] = int((bits(got) != bits(want)).sum())
    print(f"8000 Hz, pushes of {pieces}: outputs that differ from the whole: {mismatches}")
    assert mismatches["exact"] == 0 and mismatches["emit one tap early"] > 0 and mismatches["drop one sample early"] > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    fake = fake_of(8000)
    hw = fake.half_width
    # a violated precondition: output 0 reads from sample -Hw + 1 on, a window at origin 5 no longer holds it
    with pytest.raises(ValueError, match="reads from sample"):
        window_plan(fake.up, fake.down, hw, 5, 1000, 0, False)
    session = ResamplerSession(fake)
    session.push(torch.zeros(1, 400))
    session._base += 1                                        # a session that lost a sample is refused by the plan, not wrong
    session._buf = session._buf[:, 1:]
    with pytest.raises(ValueError, match="precondition"):
        session.push(torch.zeros(1, 400))
    # the library refuses before it looks at a device
    lib = _native.load()
    inv = _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_resampler_forward_window(None, None, 1, 100, 0, 0, 0, None, _native.OUT_F32, None) == inv
    assert b"handle" in lib.iris_hifigan_last_error()
    assert lib.iris_resampler_window_plan(None, 0, 100, 0, 0, None, None) == inv
    assert lib.iris_resampler_forward_g711(None, None, 1, 100, None, 1, 0, _native.OUT_ULAW, None, None) == inv
    assert lib.iris_hifigan_op_g711(None, 1, 100, None, 1, _native.OUT_ULAW, None, None) == inv
    assert set(_native.RESAMPLER_WINDOW_SYMBOLS) == {"iris_resampler_forward_g711", "iris_resampler_window_plan",
                                                     "iris_resampler_forward_window"}
    assert len(_native.RESAMPLER_WINDOW_SYMBOLS["iris_resampler_forward_window"][1]) == 10
    assert (_native.OUT_F32, _native.OUT_PCM16, _native.OUT_ULAW, _native.OUT_ALAW) == (0, 1, 3, 4)
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION == 4
    # the session's own
    with pytest.raises(ValueError, match="encoding must be one of"):
        ResamplerSession(fake, "mp3")
    session = ResamplerSession(fake)
    with pytest.raises(ValueError, match="ragged batches stay on"):
        session.push(torch.zeros(2, 10), lengths=[1, 1])
    with pytest.raises(ValueError):
        session.push(torch.zeros(2, 10, dtype=torch.int16))
    session.push(torch.zeros(2, 10))
    with pytest.raises(ValueError):
        session.push(torch.zeros(3, 10))
    session.flush()
    with pytest.raises(RuntimeError, match="flushed"):
        session.push(torch.zeros(2, 10))
    # normalize= with a G.711 encoding: refused before anything touches the device (no handle is needed to ask)
    blank = Resampler.__new__(Resampler)
    for enc in ("ulaw", "alaw"):
        with pytest.raises(ValueError, match="G.711 encoding has no normalised form"):
            Resampler.forward(blank, None, pcm16=True, normalize=True, encoding=enc)
    with pytest.raises(ValueError, match="encoding must be one of"):
        Resampler.forward(blank, None, encoding="mp3")
    with pytest.raises(ValueError, match="do not go with it"):
        ChunkedResampler(fake, "ulaw").forward(torch.zeros(1, 10), normalize=True)
    blank._handle = None                                      # (nothing to destroy)


# ---- the pipeline's plumbing, with fake stages ---------------------------------------------------------------------------------
HOP = 64


class _HoldSession:
    def __init__(self, log, name, fn, hold):
        self.log, self.name, self.fn, self.hold, self.buf = log, name, fn, hold, None

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


class _Limiter:
    """Stands in for a chunked limiter: clips at 0.5 and holds 9 samples back."""

    chunked_sessions = True

    def __init__(self, log, pcm16=False):
        self.log, self.pcm16 = log, pcm16

    def limit_device(self, wav, lengths=None, row_scale=1):
        return wav.clamp(-0.5, 0.5), torch.zeros((wav.shape[0], 2))

    def open_session(self):
        self.log.append(("limiter", "open", 0))
        return _HoldSession(self.log, "limiter", lambda w: w.clamp(-0.5, 0.5), 9)


class _Output(ChunkedResampler):
    def __init__(self, log, fake, encoding):
        super().__init__(fake, encoding)
        self.log = log

    def open_session(self):
        self.log.append(("output", "open", 0))
        inner = super().open_session()
        log = self.log

        class _Logged:
            def push(self, piece):
                log.append(("output", "push", int(piece.shape[1])))
                return inner.push(piece)

            def flush(self):
                log.append(("output", "flush", inner.samples_buffered))
                return inner.flush()
        return _Logged()


class _Vocode:
    cfg = None

    def forward(self, mel, lengths=None):
        return (mel.sum(dim=1) / 4.0).repeat_interleave(HOP, dim=1) * torch.linspace(0.5, 1.0, HOP).repeat(mel.shape[2])

    def forward_pcm16(self, mel, lengths=None):
        return self.forward(mel).to(torch.int16)


def _mel(frames):
    return torch.from_numpy(np.random.default_rng(frames).integers(-2, 3, (2, 3, frames)).astype(np.float32))


def _pushed(pipe, mel, steps):
    session, got, at = pipe.session(), [], 0
    for t in steps:
        got += session.push(mel[:, :, at:at + t])
        at += t
    return got + session.flush()


@pytest.mark.parametrize("enc,dtype", [("f32", torch.float32), ("pcm16", torch.int16), ("ulaw", torch.uint8), ("alaw", torch.uint8)])
def test_pipeline_runs_the_output_session_last(enc, dtype):
    log, voc, mel, fake = [], _Vocode(), _mel(10), fake_of(8000)
    kw = dict(hop_length=HOP, chunk_frames=4)
    pipe = MelToWavePipeline(None, voc.forward, limiter=_Limiter(log), output=_Output(log, fake, enc), **kw)
    want = pipe.infer(mel)
    limited = voc.forward(mel).clamp(-0.5, 0.5)
    assert float(voc.forward(mel).abs().max()) > 0.5          # the limiter acts, so the order of the two stages shows
    assert want.dtype == dtype and want.shape == (2, ceil_div(HOP * 10 * 160, 441))
    assert torch.equal(want, fake.forward(limited, encoding=enc)) and log == []
    pieces = list(pipe.stream(mel))
    assert all(p.shape[1] > 0 and p.dtype == dtype for p in pieces) and torch.equal(torch.cat(pieces, dim=1), want)
    assert log[:2] == [("limiter", "open", 0), ("output", "open", 0)]
    # chunks of 256, 256 and 128 samples: the limiter holds 9 back; its flush goes through the output's session before that is flushed
    assert log[2:] == [("limiter", "push", 256), ("output", "push", 247), ("limiter", "push", 256), ("output", "push", 256),
                       ("limiter", "push", 128), ("output", "push", 128), ("limiter", "flush", 9), ("output", "push", 9),
                       ("output", "flush", log[-1][2])]
    assert 45 <= log[-1][2] <= 2 * 45 + 3                     # what the last window still held: Hw .. 2 Hw + ceil(down / up)
    del log[:]
    got = _pushed(pipe, mel, (3, 0, 1, 5, 1))
    assert all(p.shape[1] > 0 for p in got) and torch.equal(torch.cat(got, dim=1), want)
    assert [e[:2] for e in log if e[1] in ("open", "flush")] == [("limiter", "open"), ("output", "open"), ("limiter", "flush"), ("output", "flush")]
    # directly behind the vocoder when no other session exists
    only = MelToWavePipeline(None, voc.forward, output=ChunkedResampler(fake, enc), **kw)
    want = only.infer(mel)
    assert torch.equal(want, fake.forward(voc.forward(mel), encoding=enc))
    assert torch.equal(torch.cat(list(only.stream(mel)), dim=1), want)
    assert torch.equal(torch.cat(_pushed(only, mel, (10,)), dim=1), want)
    # output=None: nothing changes
    plain = MelToWavePipeline(None, voc.forward, limiter=_Limiter([]), **kw)
    assert torch.equal(plain.infer(mel), limited) and torch.equal(torch.cat(list(plain.stream(mel)), dim=1), limited)


def test_pipeline_refusals():
    voc, mel, fake = _Vocode(), _mel(9), fake_of(8000)
    kw = dict(hop_length=HOP, chunk_frames=4)
    out = ChunkedResampler(fake, "ulaw")
    assert out.chunked_sessions and out.rate_out == 8000 and out.encoding == "ulaw" and isinstance(out.open_session(), ResamplerSession)
    pipe = MelToWavePipeline(None, voc.forward, output=out, **kw)
    for bad in (dict(pcm16=True), dict(pcm16=True, normalize=True), dict(resampler=fake)):
        with pytest.raises(ValueError, match="output=: it decides the rate and the encoding"):
            pipe.infer(mel, **bad)
        with pytest.raises(ValueError, match="output=: it decides the rate and the encoding"):
            pipe.infer_batch([mel[0]], **bad)
    with pytest.raises(ValueError, match=r"limiter=lim\.chunked\(\), not lim\.chunked\(pcm16=True\)"):
        MelToWavePipeline(None, voc.forward, limiter=_Limiter([], pcm16=True), output=out, **kw)
    with pytest.raises(ValueError, match="output= reads the fp32 waveform.*forward_pcm16"):
        MelToWavePipeline(None, voc.forward_pcm16, output=out, **kw)
    with pytest.raises(ValueError, match=r"output=res\.chunked\(encoding\)"):
        MelToWavePipeline(None, voc.forward, output=fake, **kw)                # a plain resampler is no opt-in
    with pytest.raises(ValueError, match="encoding must be one of"):
        ChunkedResampler(fake, "mp3")
    # the stages that cannot stream keep refusing beside it
    for extra in (dict(assemble=object()), dict(loudness=object())):
        with pytest.raises(ValueError, match="no chunked form is built"):
            MelToWavePipeline(None, voc.forward, output=out, **kw, **extra).session()
