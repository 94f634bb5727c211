"""Groups of resampler windows on the device (``iris_resampler_forward_windows``): every row of a group call against
``forward_window(B = 1)`` of the same item in all four store forms, the padding behind every row's own count (the code of sample
0), an item that breaks the window precondition failing the whole call with the output untouched, and three utterances of
different lengths driven through group calls in lockstep against ``forward`` of the whole.  Every comparison is an equality of
bits."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.resample import Resampler, ResamplerSession, window_plan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENCODINGS = (("f32", torch.float32, 0), ("pcm16", torch.int16, 0), ("ulaw", torch.uint8, 0xFF), ("alaw", torch.uint8, 0xD5))
_state = {}


def model(rate) -> Resampler:
    if rate not in _state:
        _state[rate] = Resampler(rate, device=DEV)
    return _state[rate]


def utterance(L, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, L).astype(np.float32)


def same(x: torch.Tensor, y: torch.Tensor) -> bool:
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def the_items(rs):
    """Three rows: one that emits more than one kernel block of 1024 outputs from sample 0; an interior window that emits fewer
    than a block, its ``n_next`` and origin taken from ``window_plan`` of the window in front of it; and a final window."""
    up, down, hw = rs.up, rs.down, rs.half_width
    long_in = -(-(1024 + 300) * down // up) + hw + 7                              # more than 1324 outputs, not final
    n_next, keep_from = window_plan(up, down, hw, 0, 5000, 0, False)             # the window [0, 5000) in front of row 1
    return [(0, long_in, 0, False), (keep_from, 5000 - keep_from + 333, n_next, False), (0, 901, 0, True)]


@pytest.mark.parametrize("rate", [8000, 16000, 44100])
def test_every_row_is_its_own_forward_window(rate):
    rs = model(rate)
    items = the_items(rs)
    in_stride = max(n for _, n, _, _ in items) + 1                                # odd or even: rows on and off 16 bytes
    wav = torch.full((len(items), in_stride), float("nan"), device=DEV)           # behind a row's own Lw nothing is read
    for b, (_, n, _, _) in enumerate(items):
        wav[b, :n] = torch.from_numpy(utterance(n, rate + b)).to(DEV)
    assert rs.window_plan(*items[1])[1] >= 0 and items[1][0] > 0
    for enc, dtype, zero in ENCODINGS:
        singles = [rs.forward_window(wav[b:b + 1, :n].contiguous(), o, k, f, encoding=enc) for b, (o, n, k, f) in enumerate(items)]
        assert singles[0].shape[1] > 1024 and 0 < singles[1].shape[1] < 1024 and singles[2].shape[1] > 0
        most = max(s.shape[1] for s in singles)
        for out_stride in (most, most + 1, most + 2100):
            out, counts = rs.forward_windows(wav, items, encoding=enc, out_stride=out_stride)
            torch.cuda.synchronize()
            assert out.dtype == dtype and out.shape == (len(items), out_stride) and counts == [s.shape[1] for s in singles]
            for b, single in enumerate(singles):
                assert same(out[b:b + 1, :counts[b]], single), (rate, enc, out_stride, b)
                assert bool((out[b, counts[b]:] == zero).all()), (rate, enc, out_stride, b)             # the code of sample 0


def test_a_row_that_breaks_the_precondition_fails_the_whole_call():
    rs = model(8000)
    lib, INVALID, UNSUPPORTED = _native.load(), _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    wav = torch.from_numpy(np.stack([utterance(2000, 1), utterance(2000, 2)])).to(DEV)
    out = torch.full((2, 1000), 7.0, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(items, B=2, in_stride=2000, out_ptr=None, out_stride=1000, form=_native.OUT_F32):
        arr = (_native.ResamplerWindowItem * max(len(items), 1))()
        for b, (o, n, k, f) in enumerate(items):
            arr[b].origin, arr[b].Lw, arr[b].n_next, arr[b].final = o, n, k, int(f)
        return lib.iris_resampler_forward_windows(rs._handle, ctypes.c_void_p(wav.data_ptr()), B, in_stride, arr,
                                                  ctypes.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), out_stride, form, stream)

    good = (0, 2000, 0, True)
    assert call([good, (1000, 1000, 0, False)]) == INVALID                       # output 0 reads from sample -44 on, the window holds 1000 ..
    assert b"keep" in lib.iris_hifigan_last_error()
    assert call([good, (-1, 100, 0, False)]) == INVALID and call([good, (0, -1, 0, False)]) == INVALID
    assert call([good, (0, 2001, 0, False)]) == INVALID                          # Lw above in_stride
    assert call([good, (0, 100, 10**6, False)]) == INVALID                       # n_next outside the window's outputs
    assert call([good, good], out_stride=700) == INVALID                         # a count above out_stride
    assert call([good, good], out_ptr=out.data_ptr() + 2) == INVALID             # out_dev off 4 bytes
    assert call([good, good], form=2) == INVALID                                 # no normalised form in windows
    assert call([good] * 65, B=65) == UNSUPPORTED                                # above IRIS_WINDOW_GROUP_MAX
    assert call([(0, 10, 0, False), (0, 20, 0, False)]) == 0                     # nothing is final yet: OK, and nothing is launched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call([good, good]) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


@pytest.mark.parametrize("enc", ["f32", "ulaw"])
def test_lockstep_sessions_equal_the_whole(enc):
    """Three utterances cut into different piece sizes, one group call per step over whatever each session holds."""
    rs = model(8000)
    lengths, piece_sizes = (6000, 2500, 9000), (700, 2500, 2311)
    waves = [torch.from_numpy(utterance(L, 60 + i)).to(DEV) for i, L in enumerate(lengths)]
    sessions = [ResamplerSession(rs, enc) for _ in waves]
    got, at, mixed = [[] for _ in waves], [0] * len(waves), False
    while any(not s._closed for s in sessions):
        rows = []
        for i, s in enumerate(sessions):
            if s._closed:
                continue
            s._append(waves[i][None, at[i]:at[i] + piece_sizes[i]])
            at[i] += piece_sizes[i]
            rows.append((i, s, s._plan(at[i] >= lengths[i])))
        live = [(i, s, p) for i, s, p in rows if p.launch]
        if live:
            packed = torch.nn.utils.rnn.pad_sequence([s._buf[0] for _, s, _ in live], batch_first=True)
            out, counts = rs.forward_windows(packed, [(p.origin, p.Lw, p.n_next, p.final) for _, _, p in live], encoding=enc)
            mixed = mixed or len({p.origin for _, _, p in live}) > 1              # rows at different origins in one call
            for k, (i, s, p) in enumerate(live):
                got[i].append(s._keep(*s._take(p, out[k:k + 1, :counts[k]])))
        for i, s, p in rows:
            if not p.launch:
                s._keep(*s._take(p, None))
            if p.final:
                s._close()
    assert mixed
    for i, wav in enumerate(waves):
        assert same(torch.cat(got[i], dim=1), rs.forward(wav[None], encoding=enc)), (enc, i)
