"""Groups of limiter windows on the device (``iris_limiter_forward_windows``): every row of a group call against
``forward_window(B = 1)`` of the same item -- samples and stats, fp32 and 16-bit PCM, bit for bit -- with rows that start at odd
element offsets so that both store paths run, the padding behind every row's own count, the launch counts, the refusals with an
untouched output, and three utterances of different lengths driven through group calls in lockstep against ``limit_device`` of
the whole.  Every comparison is an equality of bits."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.limiter import TILE as T, Limiter, LimiterSession

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RATE = 22050
_state = {}


def model(A) -> Limiter:
    if A not in _state:
        _state[A] = Limiter(RATE, -1.0, A * 1000.0 / RATE, device=DEV)
        assert _state[A].lookahead == A
    return _state[A]


def utterance(L, seed):
    """Random samples with peaks above the ceiling (0.891): the limiter acts on them."""
    return np.random.default_rng(seed).uniform(-1.4, 1.4, L).astype(np.float32)


def same(x: torch.Tensor, y: torch.Tensor) -> bool:
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def the_items(A):
    """The four rows of the issue: a window that crosses a tile seam, a final window from an interior origin, one that settles
    nothing at R = 15 (and little at the default), and a whole short utterance."""
    Rr = 2 * A + 7
    return [(0, T + 2 * Rr + 5, False), (1000, 300, True), (7, 20, False), (0, 37, True)]


@pytest.mark.parametrize("A", [4, 33])
@pytest.mark.parametrize("pcm16", [False, True])
def test_every_row_is_its_own_forward_window(A, pcm16):
    lim, items = model(A), the_items(A)
    in_stride = max(n for _, n, _ in items) + 3
    wav = torch.full((len(items), in_stride), float("nan"), device=DEV)          # behind a row's own Lw nothing is read
    for b, (_, n, _) in enumerate(items):
        wav[b, :n] = torch.from_numpy(utterance(n, 100 * A + b)).to(DEV)
    singles = [lim.forward_window(wav[b:b + 1, :n].contiguous(), o, f, pcm16=pcm16) for b, (o, n, f) in enumerate(items)]
    counts = [lim.window_range(o, n, f)[1] for o, n, f in items]
    assert counts[0] > T and counts[2] == 0 and counts[3] == 37
    for out_stride in (max(counts), max(counts) + 1, max(counts) + 2 + 2 * T):   # even and odd: rows on and off 16 / 8 bytes; a long tail
        out, stats, got_counts = lim.forward_windows(wav, items, pcm16=pcm16, out_stride=out_stride)
        torch.cuda.synchronize()
        assert got_counts == counts and out.shape == (len(items), out_stride)
        for b, (single, single_stats) in enumerate(singles):
            assert same(out[b:b + 1, :counts[b]], single), (A, pcm16, out_stride, b)
            assert int(torch.count_nonzero(out[b, counts[b]:])) == 0, (A, pcm16, out_stride, b)        # the padding: sample 0
            if counts[b]:
                assert same(stats[b:b + 1], single_stats), (A, pcm16, out_stride, b)
            else:
                assert stats[b].tolist() == [0.0, 1.0]
    assert float(torch.stack([s[1][0, 1] for s in singles if s[0].shape[1]]).min()) < 1.0            # some row is limited
    assert lim.windows_launch_count(items) == 2
    assert lim.windows_launch_count([(7, 2 * A + 7, False), (0, 3, False)]) == 0 and lim.windows_launch_count([]) == 0


def test_refusals_leave_the_output_untouched():
    lim = model(4)
    lib, INVALID, UNSUPPORTED = _native.load(), _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    wav = torch.from_numpy(np.stack([utterance(400, 1), utterance(400, 2)])).to(DEV)
    out = torch.full((2, 400), 7.0, device=DEV)
    stats = torch.full((2, 2), 7.0, device=DEV)
    ws = torch.zeros(lim.windows_workspace_bytes(2, 400), dtype=torch.uint8, device=DEV)
    lim.forward_windows(wav, [(0, 400, True), (0, 400, True)])                  # builds the handle
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(items, B=2, in_stride=400, out_ptr=None, out_stride=400, ws_bytes=None, wav_ptr=None):
        arr = lim._window_items(items)
        return lib.iris_limiter_forward_windows(
            lim._handle, ctypes.c_void_p(wav.data_ptr() if wav_ptr is None else wav_ptr), B, in_stride, arr,
            ctypes.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), out_stride, 0, ctypes.c_void_p(stats.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), ctypes.c_uint64(ws.numel() if ws_bytes is None else ws_bytes), stream)

    good = [(0, 400, True), (50, 300, False)]
    assert call([(0, 400, True), (-1, 300, False)]) == INVALID                   # a negative origin
    assert call([(0, 400, True), (50, -1, False)]) == INVALID
    assert call([(0, 401, True), (50, 300, False)]) == INVALID                   # Lw above in_stride
    assert call(good, out_stride=399) == INVALID                                 # a count above out_stride
    assert call(good, out_ptr=out.data_ptr() + 2) == INVALID                     # out_dev off 4 bytes
    assert call(good, out_ptr=wav.data_ptr() + 16) == INVALID                    # overlap
    assert call(good, wav_ptr=0) == INVALID
    assert call(good, ws_bytes=8) == _native.STATUS_WORKSPACE_TOO_SMALL
    assert call(good * 33, B=66) == UNSUPPORTED                                  # above IRIS_WINDOW_GROUP_MAX
    assert call([(0, 10, False), (5, 15, False)]) == 0                           # nothing settles: OK, and nothing is launched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7.0).all())
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_lockstep_sessions_equal_the_whole():
    """Three utterances cut into different piece sizes, one group call per step over whatever each session holds."""
    lim = model(33)
    lengths, piece_sizes = (6000, 2500, 9000), (700, 2500, 2311)
    waves = [torch.from_numpy(utterance(L, 40 + i)).to(DEV) for i, L in enumerate(lengths)]
    for pcm16 in (False, True):
        sessions = [LimiterSession(lim, pcm16=pcm16) for _ in waves]
        got, at, mixed = [[] for _ in waves], [0] * len(waves), False
        while any(not s._closed for s in sessions):
            rows = []
            for i, s in enumerate(sessions):
                if s._closed:
                    continue
                s._append(waves[i][None, at[i]:at[i] + piece_sizes[i]])
                at[i] += piece_sizes[i]
                plan = s._plan(at[i] >= lengths[i])
                rows.append((i, s, plan))
            live = [(i, s, p) for i, s, p in rows if p.launch]
            if live:
                packed = torch.nn.utils.rnn.pad_sequence([s._buf[0] for _, s, _ in live], batch_first=True)
                out, stats, counts = lim.forward_windows(packed, [(p.origin, p.Lw, p.final) for _, _, p in live], pcm16=pcm16)
                mixed = mixed or len({p.origin for _, _, p in live}) > 1          # rows at different origins in one call
                for k, (i, s, p) in enumerate(live):
                    got[i].append(s._keep(*s._take(p, (out[k:k + 1, :counts[k]], stats[k:k + 1]))))
            for i, s, p in rows:
                if not p.launch:
                    s._keep(*s._take(p, None))
                if p.final:
                    s._close()
        assert mixed
        for i, wav in enumerate(waves):
            want, want_stats = lim.limit_device(wav[None])
            if pcm16:
                from iris.synthesis_output import pcm16_on_device
                want = pcm16_on_device(want)
            assert same(torch.cat(got[i], dim=1), want), (pcm16, i)
            assert same(sessions[i].stats, want_stats), (pcm16, i)
            assert float(want_stats[0, 1]) < 1.0
