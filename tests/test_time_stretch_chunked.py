"""The chunked time stretch without a GPU: ``iris_time_stretch_window_plan`` against a brute force written from the rule, the
fp32 restatement of the stage run window by window under that plan (carried ``acc`` and tail rows) against its whole-utterance
result, the bookkeeping of ``StretchSession`` against a fake windowed stretch, the pipeline's routes with a fake vocoder, and
the host-only refusals.  The device itself is tests/test_gpu_time_stretch_chunked.py's.

The rule, from the definition (include/iris_hifigan.h, "Windows" of the time stretch): N = n_fft, H = hop, taps = N / H,
e = ceil(N / 2 / H).  A window holds samples [o, o + Lw) of an utterance, o = H m0, Lw = H Mw; ``final`` says that o + Lw is the
utterance's end.  Input row r covers samples [r H - N / 2, r H + N / 2), exists when r >= 0 and, only if final, r <= m0 + Mw,
and is computable when every sample of its span inside the utterance lies inside the window: rows [f_lo, f_hi).  With
i(t) = floor(float(t) * rate), output frame t is computable iff i(t) >= f_lo and i(t) + 1 < f_hi (not final) or t < T_out and
i(t) >= f_lo (final); the window computes [u, u_hi), the longest such run, and i(u) < f_lo is refused.  keep_from =
H max(0, i(u_hi) - e).  Sample s, in row j = floor((s + N / 2) / H), is emitted when each of frames j - taps + 1 .. j lies in
[max(0, u - taps + 1), u_hi) or does not exist (negative, or -- only if final -- >= T_out), s < n_out (final) or
s < rint((o + Lw) / rate) (not final), and no earlier window emitted it: j >= u, since a row below u has all its frames below u
and left with the window that computed the last of them.  (Without that clause a row j < u <= taps - 1 whose first frames are
negative would be named twice: the ranges of a schedule could not tile.)
"""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.resample import fmaf32
from iris.time_stretch import ChunkedStretch, StretchSession, TimeStretch
from iris.pipeline import MelToWavePipeline

import griffin_lim_restatement as G
import time_stretch_cases as TC
import time_stretch_restatement as R

CONFIG_NAMES = ("small", "two_tap", "default")
RATES = (0.25, 0.8, 1.0, TC.SEMITONE_DOWN, 1.5, 32.0 / 9.0, 4.0)
M_MAX = 12
INVALID, UNSUPPORTED = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED


def _ts(name: str) -> TimeStretch:
    return TimeStretch(*TC.stft_args(name))


def src_row(t: int, rate: float) -> int:
    return math.floor(float(t) * rate)


# ---- the plan against the definition -----------------------------------------------------------------------------------
def brute_rows(n_fft: int, hop: int, m0: int, Mw: int, final: bool):
    """``(f_lo, f_hi)`` sample by sample; where no row is computable both are the first row a later window could compute."""
    H, half = hop, n_fft // 2
    o, end = H * m0, H * (m0 + Mw)
    rows = []
    for r in range(0, m0 + Mw + 2):
        if final and r > m0 + Mw:
            continue
        s = np.arange(r * H - half, r * H + half)
        inside = (s >= 0) & ((s < end) if final else True)
        if bool(np.all(((s >= o) & (s < end))[inside])):
            rows.append(r)
    e = -(-half // H)
    if not rows:
        return (m0 + e if m0 else 0,) * 2
    assert rows == list(range(rows[0], rows[-1] + 1))
    return rows[0], rows[-1] + 1


def brute_plan(n_fft: int, hop: int, rate: float, m0: int, Mw: int, final: bool, u: int):
    """``(u_hi, emitted samples as an array, keep_from)`` from the definition above, or None where u is refused."""
    H, half, taps = hop, n_fft // 2, n_fft // hop
    e, end = -(-half // H), H * (m0 + Mw)
    f_lo, f_hi = brute_rows(n_fft, hop, m0, Mw, final)
    if src_row(u, rate) < f_lo:
        return None
    T_out = (R.out_frames(m0 + Mw + 1, rate) if m0 + Mw else 0) if final else None

    def computable(t):
        i = src_row(t, rate)
        return (t < T_out and i >= f_lo) if final else (i >= f_lo and i + 1 < f_hi)

    u_hi = u
    while computable(u_hi):
        u_hi += 1
    cap = R.out_samples(end, rate)
    s = np.arange(cap)
    j = (s + half) // H
    ok = np.ones(cap, dtype=bool)
    for kap in range(taps):
        t = j - kap
        missing = (t < 0) | ((t >= T_out) if final else False)
        ok &= missing | ((t >= max(0, u - taps + 1)) & (t < u_hi))
    ok &= j >= u
    return u_hi, s[ok], H * max(0, src_row(u_hi, rate) - e)


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_window_plan_is_the_rule(name):
    n_fft, hop, _ = TC.stft_args(name)
    ts = _ts(name)
    checked = refused = 0
    for rate in RATES:
        for m0 in range(M_MAX + 1):
            for Mw in range(M_MAX + 1 - m0):
                for final in (False, True):
                    f_lo, _ = brute_rows(n_fft, hop, m0, Mw, final)
                    first = next(t for t in range(10 ** 6) if src_row(t, rate) >= f_lo)             # the least u the window takes
                    last = next(t for t in range(10 ** 6) if src_row(t, rate) > m0 + Mw + 1)        # a u past everything it holds
                    if final:                                    # a u past T_out names frames an utterance of this length has not
                        last = min(last, R.out_frames(m0 + Mw + 1, rate) if m0 + Mw else 0)
                    for u in range(max(first - 1, 0), last + 1):
                        want = brute_plan(n_fft, hop, rate, m0, Mw, final, u)
                        key = (name, rate, m0, Mw, final, u)
                        if want is None:
                            with pytest.raises(_native.NativeCallError) as err:
                                ts.window_plan(rate, hop * m0, hop * Mw, final, u)
                            assert err.value.status == INVALID, key
                            refused += 1
                            continue
                        u_hi, lo, count, keep = ts.window_plan(rate, hop * m0, hop * Mw, final, u)
                        assert (u_hi, keep, count) == (want[0], want[2], len(want[1])), key
                        if count:
                            assert want[1][0] == lo and want[1][-1] == lo + count - 1, key           # one range, and this one
                        checked += 1
    assert checked > 1000 and refused > 100


def schedules(M: int, rng) -> list:
    out = [[M], [1] * M]
    for _ in range(4):
        cuts = sorted(rng.integers(0, M + 1, size=int(rng.integers(1, 5))).tolist())
        out.append([b - a for a, b in zip([0] + cuts, cuts + [M])])
    return out


def run_schedule(ts: TimeStretch, rate: float, pieces, hop: int, on_window=None):
    """The session's bookkeeping in integers: ``[(origin, Lw, final, u, u_hi, lo, count)]`` of the windows that do anything."""
    base = total = u = emitted = 0
    windows = []
    for n, final in [(m, False) for m in pieces] + [(0, True)]:
        total += hop * n
        u_hi, lo, count, keep = ts.window_plan(rate, base, total - base, final, u)
        if u_hi == u and count == 0:
            continue
        assert count == 0 or lo == emitted, (rate, pieces, windows)
        windows.append((base, total - base, final, u, u_hi, emitted, count))
        if on_window:
            on_window(*windows[-1])
        emitted, u = emitted + count, u_hi
        base = max(base, min(keep, total))
    return windows, emitted, u


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_any_schedule_tiles_the_output(name):
    n_fft, hop, _ = TC.stft_args(name)
    ts = _ts(name)
    rng = np.random.default_rng(11)
    for rate in RATES:
        for M in range(0, M_MAX + 1):
            for pieces in schedules(M, rng):
                _, emitted, u = run_schedule(ts, rate, pieces, hop)
                T_out, n_out = ts.out_frames_samples(hop * M, rate)
                assert emitted == n_out and (u == T_out or M == 0), (name, rate, M, pieces)


# ---- the fp32 restatement, window by window ----------------------------------------------------------------------------
CASES = TC.CASES[1:] + (("small", 1, 69, 0.25), ("small", 1, 69, 4.0), ("two_tap", 1, 33, 4.0))
MASK = R.MASK


class WindowedRestatement:
    """``restated(case, f32=True)`` of one item run under the plan.  A matrix product keeps the whole-utterance call's shape --
    the rows a window does not have are 0 and unused -- so that a row's sum is the same BLAS chain in both."""

    def __init__(self, case, y: np.ndarray):
        name, _, M, self.rate = case
        self.n_fft, self.hop, self.win = TC.stft_args(name)
        self.tables = TC.tables(name)
        self.y, self.M = y, M
        self.K, self.taps = self.n_fft // 2 + 1, self.n_fft // self.hop
        self.T, self.T_out = M + 1, R.out_frames(M + 1, self.rate)
        self.acc = None                                        # the carried state: the phase at frame u ...
        self.tail = {}                                         # ... and out_c of the last taps - 1 frames, by frame
        self.taps_seen = {k: {} for k in ("mag", "inc", "acc", "out_re", "out_im")}
        self.out = []

    def rows(self, origin: int, Lw: int, final: bool):
        e, m0, Mw = -(-(self.n_fft // 2) // self.hop), origin // self.hop, Lw // self.hop
        f_lo = m0 + e if m0 else 0
        return f_lo, max(f_lo, m0 + Mw + 1 if final else m0 + Mw - e + 1)

    def window(self, origin, Lw, final, u, u_hi, lo, count):
        N, H, half, K = self.n_fft, self.hop, self.n_fft // 2, self.K
        piece = self.y[origin:origin + Lw]
        f_lo, f_hi = self.rows(origin, Lw, final)
        fr = np.zeros((self.T, N), dtype=np.float32)
        for r in range(f_lo, f_hi):                            # its samples outside the window lie outside the utterance
            s = np.arange(r * H - half, r * H + half) - origin
            held = (s >= 0) & (s < Lw)
            fr[r, held] = piece[s[held]]
        re, im = fr @ self.tables["dft"][0].T, -(fr @ self.tables["dft"][1].T)
        im[:, 0] = 0
        im[:, -1] = 0
        zero = np.zeros(K, dtype=np.float32)

        def row(a, r):
            if r >= self.T:
                assert final
                return zero
            assert f_lo <= r < f_hi, "the plan names a frame whose row the window cannot compute"
            return a[r]

        t_new = list(range(u, u_hi))
        if t_new:
            idx = [src_row(t, self.rate) for t in t_new]
            alpha = np.array([float(t) * self.rate - i for t, i in zip(t_new, idx)])
            re0, im0 = np.stack([row(re, i) for i in idx]), np.stack([row(im, i) for i in idx])
            re1, im1 = np.stack([row(re, i + 1) for i in idx]), np.stack([row(im, i + 1) for i in idx])
            m0_, m1_ = np.sqrt(re0 * re0 + im0 * im0), np.sqrt(re1 * re1 + im1 * im1)
            a = np.broadcast_to(alpha.astype(np.float32)[:, None], m0_.shape)
            mag = fmaf32(a, m1_, (np.float32(1) - a) * m0_)
            adv = R.advance(N, H)
            dphi = np.arctan2(im1, re1) * R.INV_2PI32 - np.arctan2(im0, re0) * R.INV_2PI32 - (adv.astype(np.float32) / np.float32(N))[None, :]
            dphi = dphi - np.rint(dphi)
            assert dphi.dtype == np.float32 and mag.dtype == np.float32
            inc = (R.advance_fixed(N, H)[None, :] + R.fixed(dphi)) & MASK
            if u == 0:
                assert f_lo == 0
                self.acc = R.fixed(np.arctan2(im[0], re[0]) * R.INV_2PI32)
            for n, t in enumerate(t_new):
                ang = np.float32(2.0 * np.pi) * R.unfixed(self.acc)
                self.tail[t] = (mag[n] * np.cos(ang), mag[n] * np.sin(ang))
                for k, v in (("mag", mag[n]), ("inc", inc[n]), ("acc", self.acc), ("out_re", self.tail[t][0]), ("out_im", self.tail[t][1])):
                    self.taps_seen[k][t] = v
                self.acc = (self.acc + inc[n]) & MASK
        g0 = max(0, u - self.taps + 1)
        assert sorted(self.tail) == list(range(g0, u_hi)), "the state holds the last taps - 1 frames and nothing else"
        if count:
            cre, cim = np.zeros((self.T_out, K), dtype=np.float32), np.zeros((self.T_out, K), dtype=np.float32)
            for t, (a, b) in self.tail.items():
                cre[t], cim[t] = a, b
            frames = cre @ self.tables["idft"][0] + cim @ self.tables["idft"][1]
            y = np.zeros(N + H * max(self.T_out - 1, u_hi), dtype=np.float32)
            wss = np.zeros_like(y)
            for t in range(g0, u_hi):
                y[t * H:t * H + N] += frames[t]
                wss[t * H:t * H + N] += self.tables["wsq"]
            nz = wss > np.float32(G.FLT_MIN)
            y[nz] /= wss[nz]
            y = np.concatenate([y[half:], np.zeros(max(0, lo + count - (len(y) - half)), dtype=np.float32)])
            self.out.append(y[lo:lo + count])
        for t in [t for t in self.tail if t < u_hi - (self.taps - 1)]:
            del self.tail[t]


def uneven(M: int) -> list:
    return [5, 2, 0, 9, 1, 1, M - 18] if M >= 19 else ([M // 2, M - M // 2] if M > 1 else [M])


@pytest.mark.parametrize("case", CASES, ids=TC.case_id)
def test_restatement_by_windows_equals_the_whole(case):
    name, B, M, rate = case
    hop = TC.stft_args(name)[1]
    ts = _ts(name)
    want, taps = TC.restated(case, f32=True)
    for pieces in (uneven(M), [1] * M, [M]):
        for b in range(B):
            run = WindowedRestatement(case, TC.waveform(case)[b])
            _, emitted, u = run_schedule(ts, rate, pieces, hop, on_window=run.window)
            assert u == run.T_out and emitted == want.shape[1]
            for k, seen in run.taps_seen.items():              # every launch's own taps first: they name the frame that differs
                got = np.stack([seen[t] for t in range(run.T_out)])
                assert np.array_equal(got, taps[b][k]), (case, pieces, b, k)
            assert np.array_equal(np.concatenate(run.out), want[b]), (case, pieces, b)


# ---- the session's bookkeeping, against a fake windowed stretch --------------------------------------------------------
class _FakeWindowed:
    """A windowed "stretch" on the host: sample s of row j reads the utterance at the centre of input row i(j), H i(j) -- a
    sample frame j's own first row covers, so a window that emits s must hold it or it lies at or past the utterance's end,
    where it reads 0 as a frame that does not exist does.  It asserts that, and that ``u`` and the state travel from window
    to window.  The plan is the library's own (host only)."""

    def __init__(self, name: str):
        n_fft, hop, win = TC.stft_args(name)
        self.real = TimeStretch(n_fft, hop, win)
        self.hop_length, self.n_fft = hop, n_fft
        self.windows = []

    def window_plan(self, rate, origin, Lw, final, u):
        return self.real.window_plan(rate, origin, Lw, final, u)

    def out_samples(self, L, rate):
        return self.real.out_samples(L, rate)

    def new_state(self, B):
        return torch.zeros(1, dtype=torch.int64)

    def forward_window(self, wav, rate, origin, final, u, state):
        B, Lw = wav.shape
        u_hi, lo, count, _ = self.window_plan(rate, origin, Lw, final, u)
        assert u_hi > u or count > 0, "a window that does nothing must not be launched"
        if state is not None:
            assert int(state[0]) == u, "the state is not the one the previous window left"
            state[0] = u_hi
        self.windows.append((origin, Lw, bool(final), u, u_hi, lo, count))
        s = torch.arange(lo, lo + count)
        j = (s + self.n_fft // 2) // self.hop_length
        src = self.hop_length * torch.tensor([src_row(int(t), rate) for t in j], dtype=torch.int64)
        end = origin + Lw
        inside = (src < end) if final else torch.ones_like(src, dtype=torch.bool)
        held = (src >= origin) & (src < end)
        assert bool((held | ~inside).all()), "the window lacks an input sample that one of its emitted samples reads"
        vals = torch.where(inside, wav[:, (src - origin).clamp(0, max(Lw - 1, 0))] if Lw else torch.zeros(B, count), torch.zeros(()))
        return (s % 7 + 1).float() * vals

    def forward_device(self, wav, rate, lengths=None):
        assert lengths is None
        out = self.forward_window(wav, rate, 0, True, 0, None)
        self.windows.pop()
        return out, torch.full((wav.shape[0],), out.shape[1], dtype=torch.int32)


def _utterance(B: int, n: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(5 + n).integers(-50, 50, (B, n)).astype(np.float32))


SCHEDULES = {"single frames": lambda M: [1] * M, "one piece": lambda M: [M],
             "mixed": lambda M: [3, 1, 0, 7, 1, 1, 2, M - 15] if M >= 16 else [M]}


@pytest.mark.parametrize("name", CONFIG_NAMES)
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_session_equals_the_one_shot_and_counts_add_up(name, schedule):
    for rate in (0.25, 0.8, 1.5, 4.0):
        for M in (1, 2, 5, 21):
            fake = _FakeWindowed(name)
            hop, e = fake.hop_length, -(-(fake.n_fft // 2) // fake.hop_length)
            wav = _utterance(2, hop * M)
            want = fake.forward_device(wav, rate)[0]
            assert want.shape[1] == fake.out_samples(hop * M, rate)
            session = StretchSession(fake, rate)
            got, at = [], 0
            for m in SCHEDULES[schedule](M):
                piece = session.push(wav[:, at:at + hop * m])
                at += hop * m
                assert piece.shape[0] == 2 and session.samples_received == at
                assert session.samples_emitted == sum(p.shape[1] for p in got) + piece.shape[1]
                assert session.samples_buffered <= 2 * e * hop + hop * m, (name, schedule, rate, M)
                got.append(piece)
            got.append(session.flush())
            assert session.samples_emitted == fake.out_samples(hop * M, rate) and session.samples_buffered == 0
            assert torch.equal(torch.cat(got, dim=1), want), (name, schedule, rate, M)
            edge = 0
            for origin, Lw, final, u, u_hi, lo, count in fake.windows:
                assert origin % hop == 0 and (count == 0 or lo == edge)
                edge += count
            assert sum(1 for w in fake.windows if w[2]) == 1 and fake.windows[-1][2]
            assert session.flush().shape == (2, 0)


def test_pieces_shorter_than_the_halo_emit_nothing():
    fake = _FakeWindowed("small")                             # taps = 4, e = 2: a row is computable two frames after it arrives
    hop = fake.hop_length
    wav = _utterance(1, hop * 3)
    session = StretchSession(fake, 0.8)
    assert session.push(wav[:, :hop]).shape == (1, 0) and session.push(wav[:, hop:2 * hop]).shape == (1, 0)
    assert fake.windows == [] and session.samples_emitted == 0 and session.samples_buffered == 2 * hop
    third = session.push(wav[:, 2 * hop:])
    rest = session.flush()                                    # flush emits the rest
    assert session.samples_emitted == fake.out_samples(3 * hop, 0.8) == 60 and rest.shape[1] > 0
    assert torch.equal(torch.cat([third, rest], dim=1), fake.forward_device(wav, 0.8)[0])
    # samples that are no whole frame wait for the rest of theirs; an utterance that ends inside a frame is refused
    session = StretchSession(fake, 1.0)
    session.push(wav[:, :hop + 3])
    assert session.samples_buffered == hop + 3
    with pytest.raises(ValueError, match="hop_length"):
        session.flush()
    assert StretchSession(fake, 1.0).flush().shape[1] == 0    # nothing pushed at all


def test_session_refusals():
    fake = _FakeWindowed("small")
    hop = fake.hop_length
    session = StretchSession(fake, 1.25)
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
    with pytest.raises(ValueError, match="rate"):
        TimeStretch().open_session(5.0)                       # the rate is the session's, checked once
    assert isinstance(TimeStretch().open_session(0.9), StretchSession)


# ---- the pipeline ------------------------------------------------------------------------------------------------------
HOP = TC.CONFIGS["small"]["hop_length"]


class _Vocode:
    cfg = None

    def forward(self, mel, lengths=None):
        return mel.sum(dim=1).repeat_interleave(HOP, dim=1)

    def forward_pcm16(self, mel, lengths=None):
        return self.forward(mel).to(torch.int16)


class _Shift:
    """A chunked "denoiser" that delays nothing and doubles: its session hands every piece on at once."""

    chunked_sessions = True

    def forward_device(self, wav, lengths=None):
        return 2.0 * wav

    def open_session(self):
        outer = self

        class _S:
            def push(self, piece):
                return outer.forward_device(piece)

            def flush(self):
                return torch.zeros(2, 0)

        return _S()


def _mel(T: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(T).integers(-9, 9, (2, 3, T)).astype(np.float32))


@pytest.mark.parametrize("chunk_frames", (2, 4, 16))
@pytest.mark.parametrize("denoiser", (None, "chunked"))
def test_pipeline_streams_through_a_chunked_stretch(chunk_frames, denoiser):
    fake = _FakeWindowed("small")
    voc = _Vocode()
    dn = _Shift() if denoiser else None
    pipe = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=chunk_frames, denoiser=dn, stretch=fake_at(fake, 0.8).chunked())
    mel = _mel(21)
    want = pipe.infer(mel)
    assert torch.equal(want, fake.forward_device((2.0 if dn else 1.0) * voc.forward(mel), 0.8)[0])
    pieces = list(pipe.stream(mel))
    assert all(p.shape[1] > 0 for p in pieces)                # empty pieces are skipped
    assert torch.equal(torch.cat(pieces, dim=1), want)
    # the last piece carries the halo: what the final window alone could settle
    assert pieces[-1].shape[1] == fake.windows[-1][6] and fake.windows[-1][2]

    session = pipe.session()
    got, at = [], 0
    for t in (7, 1, 0, 9, 4):
        got += session.push(mel[:, :, at:at + t])
        at += t
    got += session.flush()
    assert all(p.shape[1] > 0 for p in got)
    assert torch.equal(torch.cat(got, dim=1), want)


def fake_at(fake, rate):
    from iris.time_stretch import StretchAt
    return StretchAt(fake, rate)


def test_pipeline_refusals():
    fake = _FakeWindowed("small")
    voc = _Vocode()
    mel = _mel(9)
    plain = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, stretch=fake_at(fake, 0.8))
    with pytest.raises(ValueError, match=r"\.chunked\(\)"):
        next(iter(plain.stream(mel)))
    with pytest.raises(ValueError, match=r"\.chunked\(\)"):
        plain.session()
    assert not getattr(TimeStretch().at(0.9), "chunked_sessions", False)      # a plain ts.at(rate) is no opt-in
    chunked = TimeStretch().at(0.9).chunked()
    assert isinstance(chunked, ChunkedStretch) and chunked.chunked_sessions and chunked.rate == 0.9 and chunked.hop_length == 512
    with pytest.raises(ValueError, match="fp32"):
        MelToWavePipeline(None, voc.forward_pcm16, hop_length=HOP, chunk_frames=4, stretch=fake_at(fake, 0.8).chunked())
    # a plain denoiser beside a chunked stretch still refuses
    class _Doubler:
        def forward_device(self, wav, lengths=None):
            return 2.0 * wav
    both = MelToWavePipeline(None, voc.forward, hop_length=HOP, chunk_frames=4, denoiser=_Doubler(), stretch=fake_at(fake, 0.8).chunked())
    with pytest.raises(ValueError, match="denoiser"):
        both.session()


# ---- host-only refusals and the launch counts ----------------------------------------------------------------------------
def _status(fn, *args):
    with pytest.raises(_native.NativeCallError) as err:
        fn(*args)
    return err.value.status


def test_window_queries_refuse_and_count():
    ts = TimeStretch(1024, 256, 1024)
    H = 256
    assert _status(ts.window_plan, 1.0, 255, H * 8, False, 0) == INVALID              # origin is no multiple of hop
    assert _status(ts.window_plan, 1.0, H, H * 8 + 4, False, 3) == INVALID            # nor is Lw
    assert _status(ts.window_plan, 1.0, -H, H * 8, False, 0) == INVALID
    assert _status(ts.window_plan, 1.0, 0, -H, True, 0) == INVALID
    assert _status(ts.window_plan, 1.0, 0, H * 8, False, -1) == INVALID
    assert _status(ts.window_plan, 5.0, 0, H * 8, False, 0) == INVALID                # the forward's rate rule
    assert _status(ts.window_plan, 1.0, H * 4, H * 8, False, 5) == INVALID            # frame 5 reads row 5, the window holds rows from 6 on
    assert ts.window_plan(1.0, H * 4, H * 8, False, 6) == (10, 6 * H - 512, 4 * H, 8 * H)
    assert _status(ts.window_plan, 1.0, H * ((1 << 60) // H + 1), H * 8, False, 1 << 58) == UNSUPPORTED
    assert _status(ts.window_plan, 1.0, 0, H * 8, True, (1 << 61) // H + 1) == UNSUPPORTED
    assert _status(TimeStretch(256, 256, 256).window_plan, 1.0, 0, 256 * 8, False, 0) == UNSUPPORTED     # frames that do not overlap
    assert _status(TimeStretch(1024, 300, 1024).window_plan, 1.0, 0, 300 * 8, False, 0) == UNSUPPORTED
    assert _status(ts.window_launch_count, 65536, H * 8, 1.0, 0, False, 0) == UNSUPPORTED
    assert _status(ts.window_workspace_bytes, 1, H * 8 + 1, 1.0) == INVALID
    m0 = (1 << 40)                                                                       # 64-bit origins and frames
    assert ts.window_plan(1.0, H * m0, H * 8, False, m0 + 2) == (m0 + 6, H * (m0 + 2) - 512, 4 * H, H * (m0 + 4))
    # launches: the forward's 4; 3 while frames advance under no whole row of samples; 0 for an empty plan
    assert ts.window_launch_count(2, H * 8, 1.0, 0, False, 0) == 4 == ts.launch_count(2, H * 8, 1.0)
    assert ts.window_launch_count(2, H * 8, 1.0, H * 4, True, 6) == 4
    assert ts.window_plan(1.0, 0, H * 3, False, 0) == (1, 0, 0, 0) and ts.window_launch_count(1, H * 3, 1.0, 0, False, 0) == 3
    assert ts.window_plan(1.0, 0, H * 2, False, 0) == (0, 0, 0, 0) and ts.window_launch_count(1, H * 2, 1.0, 0, False, 0) == 0
    assert ts.window_launch_count(0, H * 8, 1.0, 0, False, 0) == 0
    # a final window with samples left and no frame: rate 4, 7 mel frames, both frames computed before the end is known
    assert ts.window_plan(4.0, 0, H * 7, False, 0)[0] == 2 == ts.out_frames_samples(H * 7, 4.0)[0]
    keep = ts.window_plan(4.0, 0, H * 7, False, 0)[3]
    u_hi, lo, count, _ = ts.window_plan(4.0, keep, H * 7 - keep, True, 2)
    assert u_hi == 2 and count > 0 and lo + count == ts.out_samples(H * 7, 4.0)
    assert ts.window_launch_count(1, H * 7 - keep, 4.0, keep, True, 2) == 2
    # sizes: the state is acc [B, Ks] and tail [B, taps - 1, Qp], each on 256 bytes
    assert ts.state_bytes(2) == 4 * ((2 * 516 + 63) // 64 * 64 + (2 * 3 * 1032 + 63) // 64 * 64)
    lib = _native.load()
    cfg, v, n = ts.native_config(), ctypes.c_int64(), ctypes.c_int32()
    r = ctypes.byref(v)
    assert lib.iris_time_stretch_window_plan(ctypes.byref(cfg), 1.0, 0, H, 0, 0, None, r, r, r) == INVALID
    assert lib.iris_time_stretch_window_plan(None, 1.0, 0, H, 0, 0, r, r, r, r) == INVALID
    assert lib.iris_time_stretch_state_bytes(ctypes.byref(cfg), 1, None) == INVALID
    assert lib.iris_time_stretch_window_launch_count(ctypes.byref(cfg), 1, H, 1.0, 0, 0, 0, None) == INVALID
    # a NULL handle is refused before anything else is looked at; nothing needs a device
    assert lib.iris_time_stretch_forward_window(None, None, 1, H * 8, 0, 0, 1.0, 0, None, None, None, 0, None) == INVALID
    assert len(_native.TIME_STRETCH_SYMBOLS["iris_time_stretch_forward_window"][1]) == 13
