"""``iris.stream_group.StreamGroup`` without a GPU: members at different places of different utterances, stepped together, against
fakes in the style of tests/test_resample_chunked.py.  Behind ``forward_windows`` stand the limiter's numpy restatement
(tests/limiter_restatement.py: ``device_f32``) and ``resample_host``, each applied to a row's window ALONE -- everything outside
the window is zeros to them, so a group that planned a member's window wrongly, or handed a row to the wrong member, would not
reproduce the whole-utterance bits.  The fake vocoder and the fake PostNet have a ragged form that is per item their dense form
(bounded by the item's own length, as the device's ragged forwards are).  Every comparison is an equality of bits.  The device is
tests/test_gpu_stream_group.py's."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.limiter import ChunkedLimiter, Limiter
from iris.pipeline import MelToWavePipeline
from iris.resample import ChunkedResampler, design_bank, resample_host
from iris.stream_group import GROUP_MAX, StreamGroup
from iris.synthesis_output import alaw_from_pcm16, pcm16_from_float, ulaw_from_pcm16

import limiter_cases as C
import limiter_restatement as R

HOP, N_MELS, CHUNK, A = 4, 3, 16, 1
ENCODE = {"f32": lambda y: y, "pcm16": pcm16_from_float, "ulaw": lambda y: ulaw_from_pcm16(pcm16_from_float(y)),
          "alaw": lambda y: alaw_from_pcm16(pcm16_from_float(y))}


def ceil_div(a, b):
    return -((-a) // b)


class _Vocode:
    """``wav[t * HOP + j] = (0.5 s[t - 1] + s[t] + 0.25 s[t + 1]) * (1 + j / 8)`` with ``s`` the sum over the mel bins and 0 outside
    the item's own frames: a receptive field of one frame, and a ragged form that is per item the dense form."""

    cfg = None

    def __init__(self):
        self.batches = []

    def forward(self, mel, lengths=None):
        B, _, T = mel.shape
        self.batches.append(B)
        out = torch.zeros((B, HOP * T), dtype=torch.float32)
        ramp = 1.0 + torch.arange(HOP, dtype=torch.float32) / 8.0
        for b in range(B):
            n = T if lengths is None else int(lengths[b])
            s = torch.nn.functional.pad(mel[b, :, :n].sum(dim=0), (1, 1))
            y = 0.5 * s[:-2] + s[1:-1] + 0.25 * s[2:]
            out[b, :HOP * n] = (y[:, None] * ramp[None, :]).reshape(-1)
        return out


class _PostNet:
    """``out[:, t] = mel[:, t] + 0.5 mel[:, t - 2] - 0.25 mel[:, t + 2]``, zeros outside the item's own frames."""

    receptive_field_frames = 2

    def __init__(self):
        self.batches = []

    def forward_device(self, mel, lengths=None):
        self.batches.append(int(mel.shape[0]))
        out = torch.zeros_like(mel)
        for b in range(mel.shape[0]):
            n = mel.shape[2] if lengths is None else int(lengths[b])
            x = torch.nn.functional.pad(mel[b, :, :n], (2, 2))
            out[b, :, :n] = x[:, 2:-2] + 0.5 * x[:, :-4] - 0.25 * x[:, 4:]
        return out


class _Limiter:
    """The windowed limiter of tests/test_limiter_chunked.py with a group form: row b of ``forward_windows`` is
    ``forward_window`` of that row's own ``Lw_b`` samples."""

    def __init__(self):
        self.c, self.table, self.reach = 1.0, Limiter(C.RATE, 0.0, float(A)).design(), 2 * A + 7
        self.group_rows, self.single_calls = [], 0

    def window_range(self, origin, Lw, final):
        lo = origin + (self.reach if origin > 0 else 0)
        return lo, max(0, origin + Lw - (0 if final else self.reach) - lo)

    def _row(self, x, origin, final):
        lo, count = self.window_range(origin, len(x), final)
        a = lo - origin
        res = R.device_f32(x, self.c, A, self.table)
        return res["out"][a:a + count], (res["p"][a:a + count].max(), res["g"][a:a + count].min())

    def forward_window(self, wav, origin, final, pcm16=False):
        self.single_calls += 1
        rows = [self._row(w.numpy(), origin, final) for w in wav]
        out = np.stack([r[0] for r in rows])
        return torch.from_numpy(pcm16_from_float(out) if pcm16 else out), torch.tensor([r[1] for r in rows], dtype=torch.float32)

    def forward_windows(self, wav, items, pcm16=False, out_stride=None):
        assert len(items) == wav.shape[0] <= GROUP_MAX
        self.group_rows.append(len(items))
        counts = [self.window_range(o, n, f)[1] for o, n, f in items]
        assert max(counts) > 0, "a group in which nothing settles must not be launched"
        out = np.zeros((len(items), max(counts)), np.float32)
        stats = np.tile(np.float32([0.0, 1.0]), (len(items), 1))
        for b, (o, n, f) in enumerate(items):
            if counts[b]:
                out[b, :counts[b]], stats[b] = self._row(wav[b, :n].numpy(), o, f)
        return torch.from_numpy(pcm16_from_float(out) if pcm16 else out), torch.from_numpy(stats), counts

    def limit_device(self, wav, lengths=None, row_scale=1):
        res = [R.device_f32(row.numpy(), self.c, A, self.table) for row in wav]
        return torch.from_numpy(np.stack([r["out"] for r in res])), None


class _Resampler:
    """The windowed resampler of tests/test_resample_chunked.py with a group form: row b of ``forward_windows`` is
    ``resample_host`` of that row's own window alone at its own origin, cut to ``[n_next_b, n_hi_b)``."""

    def __init__(self, rate_out):
        self.bank, self.up, self.down = design_bank(rate_out)
        self.rate_out, self.half_width = rate_out, self.bank.shape[1] // 2
        self.group_rows, self.single_calls = [], 0

    def out_range(self, origin, L):
        lo = ceil_div(origin * self.up, self.down)
        return lo, ceil_div((origin + L) * self.up, self.down) - lo

    def window_plan(self, origin, Lw, n_next, final):
        up, down, hw = self.up, self.down, self.half_width
        if origin and n_next * down // up - hw + 1 < origin:
            raise ValueError("precondition")
        n_hi = ceil_div((origin + Lw if final else max(0, origin + Lw - hw)) * up, down)
        return n_hi, max(0, n_hi * down // up - hw + 1)

    def _row(self, x, origin, n_next, final, encoding):
        n_hi = self.window_plan(origin, len(x), n_next, final)[0]
        n_lo = self.out_range(origin, len(x))[0]
        assert n_lo <= n_next
        y = resample_host(x[None], self.bank, self.up, self.down, origin=origin)[0]
        return ENCODE[encoding](y[n_next - n_lo:n_hi - n_lo])

    def forward_window(self, wav, origin, n_next, final, encoding="f32"):
        self.single_calls += 1
        return torch.from_numpy(np.stack([self._row(w.numpy(), origin, n_next, final, encoding) for w in wav]))

    def forward_windows(self, wav, items, encoding="f32", out_stride=None):
        assert len(items) == wav.shape[0] <= GROUP_MAX
        self.group_rows.append(len(items))
        rows = [self._row(wav[b, :n].numpy(), o, k, f, encoding) for b, (o, n, k, f) in enumerate(items)]
        counts = [len(r) for r in rows]
        assert max(counts) > 0, "a group in which nothing is final must not be launched"
        out = np.full((len(items), max(counts)), {"ulaw": 0xFF, "alaw": 0xD5}.get(encoding, 0), rows[0].dtype)
        for b, r in enumerate(rows):
            out[b, :len(r)] = r
        return torch.from_numpy(out), counts

    def forward(self, wav, lengths=None, row_scale=1, origin=0, encoding="f32"):
        assert lengths is None
        return torch.from_numpy(ENCODE[encoding](resample_host(wav.numpy(), self.bank, self.up, self.down, origin=origin)).copy())


def _mel(frames, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-0.6, 0.6, (N_MELS, frames)).astype(np.float32))


def _pipeline(postnet=True, limiter=True, output="ulaw", pcm16=False):
    voc = _Vocode()
    stages = {"voc": voc, "postnet": _PostNet() if postnet else None, "lim": _Limiter() if limiter else None,
              "res": _Resampler(8000) if output else None}
    pipe = MelToWavePipeline(stages["postnet"], voc.forward, hop_length=HOP, chunk_frames=CHUNK,
                             limiter=ChunkedLimiter(stages["lim"], pcm16=pcm16) if limiter else None,
                             output=ChunkedResampler(stages["res"], output) if output else None)
    return pipe, stages


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _calls(stages):
    return {"voc": len(stages["voc"].batches), "postnet": len(stages["postnet"].batches) if stages["postnet"] else 0,
            "lim": len(stages["lim"].group_rows) if stages["lim"] else 0, "res": len(stages["res"].group_rows) if stages["res"] else 0}


def _drive(group, stages, plan):
    """``plan``: ``[(opened at step, mel [n_mels, T], frames per push, an empty last push?)]``.  Every member pushes one piece per
    step from the step it is opened in and ends behind its last piece.  Returns the members' concatenated pieces."""
    members, at, got = [None] * len(plan), [0] * len(plan), [[] for _ in plan]
    shared = 0
    for step in range(200):
        for i, (start, mel, piece, empty_last) in enumerate(plan):
            if step == start:
                members[i] = group.open()
            m = members[i]
            if m is None or m._ended:
                continue
            if at[i] < mel.shape[1]:
                m.push(mel[:, at[i]:at[i] + piece] if i % 2 else mel[None, :, at[i]:at[i] + piece])     # [n_mels, t] and [1, n_mels, t]
                at[i] += piece
                if at[i] >= mel.shape[1] and not empty_last:
                    m.end()
            else:
                m.push(mel[:, :0])                              # an empty final push
                m.end()
        before = _calls(stages)
        pieces = group.step()
        after = _calls(stages)
        assert all(after[k] - before[k] in (0, 1) for k in after), (step, before, after)          # ONE call per stage and step
        if stages["voc"].batches and after["voc"] > before["voc"] and stages["voc"].batches[-1] > 1:
            shared += 1
        for m, piece in pieces.items():
            assert piece.shape[0] == 1 and piece.shape[1] > 0
            got[members.index(m)].append(piece)
        if all(m is not None and m.closed for m in members):
            break
    assert all(m.closed for m in members) and group.members == []
    assert shared > 0                                             # several members' windows were items of one forward
    return [torch.cat(g, dim=1) for g in got]


PLAN = [(0, _mel(40, 1), 5, True), (1, _mel(70, 2), 16, False), (3, _mel(23, 3), 23, False)]


@pytest.mark.parametrize("postnet,limiter,output,pcm16", [(True, True, "ulaw", False), (False, True, "ulaw", False),
                                                          (True, False, "alaw", False), (True, True, None, False),
                                                          (False, True, None, True), (False, False, None, False)])
def test_every_member_equals_the_whole_utterance_path(postnet, limiter, output, pcm16):
    pipe, stages = _pipeline(postnet, limiter, output, pcm16)
    got = _drive(StreamGroup(pipe, chunk_frames=CHUNK), stages, PLAN)
    for (_, mel, _, _), mine in zip(PLAN, got):
        want = pipe.infer(mel[None])
        if pcm16:                                                 # the limiter's own 16-bit store: the output stage's formula
            want = torch.from_numpy(pcm16_from_float(want.numpy()))
        assert mine.dtype == want.dtype and mine.shape == want.shape
        assert torch.equal(_bits(mine), _bits(want))
    if limiter:
        assert stages["lim"].single_calls == 0 and max(stages["lim"].group_rows) > 1
        raw = _Vocode().forward(PLAN[0][1][None])
        assert float(raw.abs().max()) > 1.0 and not torch.equal(stages["lim"].limit_device(raw)[0], raw)       # the limiter acts
    if output:
        assert stages["res"].single_calls == 0 and max(stages["res"].group_rows) > 1


def test_one_chunk_per_member_and_step():
    pipe, stages = _pipeline(False, True, "f32")
    group = StreamGroup(pipe, chunk_frames=CHUNK)
    m = group.open()
    m.push(_mel(70, 5))
    m.end()
    emitted = []
    while not m.closed:
        group.step()
        emitted.append(m.frames_emitted)
    assert emitted == [16, 32, 48, 64, 70] and stages["voc"].batches == [1] * 5
    with pytest.raises(RuntimeError, match="ended"):
        m.push(_mel(3, 0))
    # an utterance of no frames closes with nothing; a member that leaves is gone
    a, b = group.open(), group.open()
    a.end()
    b.push(_mel(40, 6))
    b.leave()
    assert group.step() == {} and a.closed and b.closed and group.members == []


def test_groups_above_64_members_are_split():
    pipe, stages = _pipeline(False, True, "ulaw")
    group = StreamGroup(pipe, chunk_frames=CHUNK)
    mels = [_mel(3, 10), _mel(4, 11)]
    members = [group.open() for _ in range(GROUP_MAX + 6)]
    for i, m in enumerate(members):
        m.push(mels[i % 2])
        m.end()
    pieces = group.step()
    assert stages["voc"].batches == [GROUP_MAX, 6] and stages["lim"].group_rows == [GROUP_MAX, 6] == stages["res"].group_rows
    want = [pipe.infer(mel[None]) for mel in mels]
    assert len(pieces) == len(members) and all(m.closed for m in members)
    for i, m in enumerate(members):
        assert torch.equal(pieces[m], want[i % 2])
    assert GROUP_MAX == _native.WINDOW_GROUP_MAX == 64


def test_refusals():
    voc = _Vocode()
    for name in ("denoiser", "stretch", "assemble", "loudness"):
        stage = type("S", (), {"chunked_sessions": True, "hop_length": HOP})()
        with pytest.raises(ValueError, match=f"{name}="):
            StreamGroup(MelToWavePipeline(None, voc.forward, hop_length=HOP, **{name: stage}))
    with pytest.raises(ValueError, match=r"limiter=lim\.chunked\(\)"):
        StreamGroup(MelToWavePipeline(None, voc.forward, hop_length=HOP, limiter=_Limiter()))
    half = type("V", (_Vocode,), {"default_dtype": "bf16"})()
    with pytest.raises(ValueError, match="fp32 engine.*bf16"):
        StreamGroup(MelToWavePipeline(None, half.forward, hop_length=HOP))
    whole = type("G", (), {"whole_utterance": True, "hop_length": HOP, "forward_device": lambda self, mel: mel})()
    with pytest.raises(ValueError, match="whole-utterance"):
        StreamGroup(MelToWavePipeline(None, whole))
    with pytest.raises(ValueError, match="receptive_field_frames"):
        StreamGroup(MelToWavePipeline(lambda mel, lengths=None: mel, voc.forward, hop_length=HOP))
    with pytest.raises(ValueError, match="chunk_frames"):
        StreamGroup(MelToWavePipeline(None, voc.forward, hop_length=HOP), chunk_frames=0)
    m = StreamGroup(MelToWavePipeline(None, voc.forward, hop_length=HOP)).open()
    with pytest.raises(ValueError, match="ONE utterance"):
        m.push(torch.zeros(2, N_MELS, 4))


def test_the_new_entry_points_are_bound_and_refuse_on_the_host():
    import ctypes
    lib = _native.load()
    INVALID, UNSUPPORTED = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    assert set(_native.WINDOW_GROUP_SYMBOLS) == {"iris_limiter_windows_workspace_bytes", "iris_limiter_windows_launch_count",
                                                 "iris_limiter_forward_windows", "iris_resampler_forward_windows"}
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION == 4        # a backward-compatible addition
    assert ctypes.sizeof(_native.LimiterWindowItem) == 16 and ctypes.sizeof(_native.ResamplerWindowItem) == 24
    lim = Limiter(22050, -1.0, 4 / 22.05)                                     # lookahead 4: R = 15
    R15 = 15
    assert lim.lookahead == 4
    items = [(0, 2048 + 2 * R15 + 5, False), (1000, 300, True), (7, 20, False), (0, 37, True)]
    assert lim.windows_launch_count(items) == 2
    assert lim.windows_launch_count([(7, 20, False), (0, R15, False)]) == 0 and lim.windows_launch_count([]) == 0
    assert lim.windows_workspace_bytes(4, 4096) == lim.window_workspace_bytes(4, 4096)
    for bad in ([(-1, 10, False)], [(0, -1, True)]):
        with pytest.raises(_native.NativeCallError) as err:
            lim.windows_launch_count(bad)
        assert err.value.status == INVALID
    with pytest.raises(_native.NativeCallError) as err:
        lim.windows_launch_count([(0, 100, True)] * (GROUP_MAX + 1))
    assert err.value.status == UNSUPPORTED
    with pytest.raises(_native.NativeCallError) as err:
        lim.windows_workspace_bytes(GROUP_MAX + 1, 100)
    assert err.value.status == UNSUPPORTED
    cfg, n = lim.native_config(), ctypes.c_int32()
    assert lib.iris_limiter_windows_launch_count(ctypes.byref(cfg), 1, None, ctypes.byref(n)) == INVALID
    assert lib.iris_limiter_windows_launch_count(ctypes.byref(cfg), 0, None, None) == INVALID
    # a NULL handle is refused before anything else is looked at; nothing needs a device
    assert lib.iris_limiter_forward_windows(None, None, 1, 100, None, None, 100, 0, None, None, 0, None) == INVALID
    assert lib.iris_resampler_forward_windows(None, None, 1, 100, None, None, 100, _native.OUT_F32, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
