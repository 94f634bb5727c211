"""The assemble stage on the device against its restatements (tests/assemble_restatement.py): the integer bounds equal librosa's
float64 ones, the energies and the joined samples equal the fp32 restatement bit for bit, every output element is stored and
nothing else is, an item does not depend on its neighbours, and the pipeline's route equals the stages applied by hand."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.assemble import Assembler
from iris.pipeline import MelToWavePipeline
from iris.resample import Resampler
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import assemble_cases as C
import assemble_restatement as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
ALL_CASES = C.CASES + C.WIDE_CASES
CASE_IDS = [C.case_id(c) for c in ALL_CASES]
WIDE = {c["name"] for c in C.WIDE_CASES}
GUARD = 256                       # bytes behind the workspace's stated size that must stay as they were
SENTINEL = -77
TOO_SMALL = 5                     # IRIS_HIFIGAN_WORKSPACE_TOO_SMALL

_state = {}


def model(c) -> Assembler:
    key = tuple(sorted(C.params(c).items(), key=lambda kv: kv[0]))
    if key not in _state:
        _state[key] = Assembler(**C.params(c), device=DEV)
    return _state[key]


def ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def poisoned(c) -> dict:
    """One raw call per case, kept: the row tails behind L_b hold NaN, and ``out``, both integer outputs and the workspace (with
    ``GUARD`` bytes behind it) are poisoned beforehand."""
    if c["name"] in _state:
        return _state[c["name"]]
    a = model(c)
    a._ensure()
    wav, lengths, row_scale = C.batch(c, fill=NAN)
    B, L = wav.shape
    cap, need = a.capacity(B, L), a.workspace_bytes(B, L)
    wav_d = torch.from_numpy(wav).to(DEV)
    len_d = None if lengths is None else torch.from_numpy(lengths).to(DEV)
    out = torch.full((cap,), NAN, dtype=torch.float32, device=DEV)
    offsets = torch.full((B + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    spans = torch.full((B, 2), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _native.check("iris_assemble_forward", _native.load().iris_assemble_forward(
            a._handle, ptr(wav_d), B, L, ptr(len_d), row_scale, ptr(out), ptr(spans), ptr(offsets), ptr(ws), ctypes.c_uint64(need),
            ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    _state[c["name"]] = dict(out=out, offsets=offsets, spans=spans, ws=ws.cpu().numpy(), need=need)
    return _state[c["name"]]


def batch_of_one_items(c):
    """The items compared with their batch-of-one calls: all of them in the first list; in a wide case at most 16 -- the first
    and the last, then the scan's thread and wave edges, then the neighbours of the long runs of empty items."""
    B = len(c["items"])
    if c["name"] not in WIDE or B <= 16:
        return list(range(B))
    lens = [len(y) for y in c["items"]]
    want = [0, B - 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
    for lo, hi in C.empty_runs(lens):
        if hi - lo >= 40:
            want += [lo - 1, hi]
    for lo, hi in C.empty_runs(lens):
        want += [lo - 1, hi]
    picked = []
    for b in want:
        if 0 <= b < B and lens[b] and b not in picked:
            picked.append(b)
    return picked[:16]


@pytest.mark.parametrize("c", ALL_CASES, ids=CASE_IDS)
def test_bounds_energies_and_samples_match_the_restatements(c):
    got, ref, a = poisoned(c), C.reference(c), model(c)
    B, L = len(c["items"]), c["L"]
    assert torch.equal(got["spans"].cpu(), torch.tensor(ref["spans"], dtype=torch.int32))                # librosa's, in float64
    assert torch.equal(got["offsets"].cpu(), torch.tensor(ref["offsets"], dtype=torch.int32))
    out = got["out"].cpu().numpy()
    assert not np.isnan(out).any()                                                                          # all of out[0, cap) was stored
    assert np.array_equal(out.view(np.uint32), ref["out"].view(np.uint32))                                  # pauses and the zero tail too
    # the workspace: mse rows up to T_b bit for bit, spans, and nothing else touched
    layout, words = a._workspace_layout(B, L)
    ws = got["ws"]
    assert got["need"] == max(256, 4 * words)
    touched = np.zeros(len(ws), dtype=bool)
    (o_m, (_, T)), (o_s, _) = layout["mse"], layout["spans"]
    mse = ws[4 * o_m:4 * (o_m + B * T)].view(np.float32).reshape(B, T)
    for b, m32 in enumerate(ref["mse32"]):
        assert np.array_equal(mse[b, :len(m32)].view(np.uint32), m32.view(np.uint32)), (b, np.abs(mse[b, :len(m32)] - m32).max())
        touched[4 * (o_m + b * T):4 * (o_m + b * T + len(m32))] = True
    assert np.array_equal(ws[4 * o_s:4 * (o_s + 2 * B)].view(np.int32).reshape(B, 2), np.array(ref["spans"], dtype=np.int32))
    touched[4 * o_s:4 * (o_s + 2 * B)] = True
    assert (ws[~touched] == 0xFF).all()                                                                     # row rests, padding, the guard


@pytest.mark.parametrize("c", ALL_CASES, ids=CASE_IDS)
def test_unpoisoned_call_repeats_and_items_are_their_batch_of_one_calls(c):
    got, a = poisoned(c), model(c)
    wav, lengths, row_scale = C.batch(c)
    first = a.join_device(wav, lengths=lengths, row_scale=row_scale)
    second = a.join_device(torch.from_numpy(wav).to(DEV), lengths=None if lengths is None else torch.from_numpy(lengths).to(DEV),
                           row_scale=row_scale)
    for x, y, z in zip(first, second, (got["out"], got["offsets"], got["spans"])):
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), z.view(torch.int32))                 # NaN tails change nothing
    offs = got["offsets"].cpu().tolist()
    for b in batch_of_one_items(c):
        y = c["items"][b]
        if len(y) == 0:
            continue
        one, one_offs, one_span = a.join_device(y[None].copy())
        s, e = got["spans"][b].cpu().tolist()
        assert one_span.cpu().tolist() == [[s, e]] and one_offs.cpu().tolist() == [0, e - s]
        assert torch.equal(one[:e - s], got["out"][offs[b]:offs[b] + e - s])
    trimmed, total_spans = a.join(wav, lengths=lengths, row_scale=row_scale)
    assert trimmed.shape == (offs[-1],) and torch.equal(trimmed, got["out"][:offs[-1]]) and torch.equal(total_spans, got["spans"])


@pytest.mark.parametrize("c", ALL_CASES, ids=CASE_IDS)
def test_trim_rows_are_the_joins_slices(c):
    a = model(c)
    wav, lengths, row_scale = C.batch(c, fill=NAN)
    B, L = wav.shape
    rows, counts = a.trim_device(wav, lengths=lengths, row_scale=row_scale)
    got = poisoned(c)
    spans, offs = got["spans"].cpu().numpy(), got["offsets"].cpu().tolist()
    assert rows.shape == (B, L) and torch.equal(counts.cpu(), torch.from_numpy(spans[:, 1] - spans[:, 0]))
    rows, out = rows.cpu(), got["out"].cpu()                                                  # (one copy each, not one per item)
    for b in range(B):
        n = int(spans[b, 1] - spans[b, 0])
        assert torch.equal(rows[b, :n], out[offs[b]:offs[b] + n]) and not rows[b, n:].any()


@pytest.mark.parametrize("name", ["gather_seams", "batch_257"])
def test_out_off_a_16_byte_boundary(name):
    """The gather stores 16 bytes at a time only where ``out`` lies on 16 bytes.  With ``out`` 4, 8 and 12 bytes past such an
    address both output forms give the aligned call's bits, store all of ``out`` and leave the words around it alone."""
    c = next(c for c in C.WIDE_CASES if c["name"] == name)
    a, aligned = model(c), poisoned(c)
    wav, lengths, row_scale = C.batch(c, fill=NAN)
    B, L = wav.shape
    need = a.workspace_bytes(B, L)
    wav_d, len_d = torch.from_numpy(wav).to(DEV), torch.from_numpy(lengths).to(DEV)
    rows_aligned, counts_aligned = a.trim_device(wav_d, lengths=len_d, row_scale=row_scale)
    lib, guard, mark = _native.load(), 64, 0x5EEDBEEF
    forms = ((lib.iris_assemble_forward, a.capacity(B, L), B + 1, aligned["out"], aligned["offsets"]),
             (lib.iris_assemble_trim_ragged, B * L, B, rows_aligned.reshape(-1), counts_aligned))
    for fn, cap, n_ints, want, want_ints in forms:
        assert want.data_ptr() % 16 == 0 and want.numel() == cap
        for shift in (1, 2, 3):
            buf = torch.full((guard + shift + cap + guard,), mark, dtype=torch.int32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            out = buf[guard + shift:guard + shift + cap].view(torch.float32)
            assert out.data_ptr() % 16 == 4 * shift
            out.fill_(NAN)
            ints = torch.full((n_ints,), SENTINEL, dtype=torch.int32, device=DEV)
            spans = torch.full((B, 2), SENTINEL, dtype=torch.int32, device=DEV)
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
            with torch.cuda.device(DEV):
                _native.check(fn.__name__, fn(a._handle, ptr(wav_d), B, L, ptr(len_d), row_scale, ptr(out), ptr(spans), ptr(ints), ptr(ws),
                                       ctypes.c_uint64(need), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
            torch.cuda.synchronize()
            assert not torch.isnan(out).any()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (fn.__name__, shift)
            assert torch.equal(ints, want_ints) and torch.equal(spans, aligned["spans"])
            assert (buf[:guard + shift] == mark).all() and (buf[guard + shift + cap:] == mark).all()


def test_refusals_behind_the_handle():
    c = C.CASES[0]
    a = model(c)
    a._ensure()
    lib, B, L = _native.load(), 2, 100
    buf = torch.zeros(B * L + a.capacity(B, L), dtype=torch.float32, device=DEV)
    ints = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(a.workspace_bytes(B, L), dtype=torch.uint8, device=DEV)
    call = lambda fn, wav, out, nbytes, scale=1, ints=ints: fn(a._handle, wav, B, L, None, scale, out, None, ptr(ints), ptr(ws), ctypes.c_uint64(nbytes), None)
    at = lambda i: ctypes.c_void_p(buf.data_ptr() + 4 * i)
    for fn in (lib.iris_assemble_forward, lib.iris_assemble_trim_ragged):
        assert call(fn, at(0), at(B * L - 1), ws.numel()) == 1                               # the last input sample is the first output
        assert call(fn, at(0), at(0), ws.numel()) == 1
        assert call(fn, None, at(B * L), ws.numel()) == 1 and call(fn, at(0), None, ws.numel()) == 1
        assert call(fn, at(0), at(B * L), ws.numel(), ints=None) == 1
        assert call(fn, at(0), at(B * L), ws.numel(), scale=0) == 1
        assert call(fn, at(0), at(B * L), ws.numel() - 1) == TOO_SMALL                               # a short workspace
    torch.cuda.synchronize()
    assert not buf.any()                                                                     # no refused call launched


def test_pipeline_returns_one_waveform_equal_to_the_stages_by_hand():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        kw = dict(frame_length=256, hop_length=64, top_db=25.0, pad=32, fade=16, pause=200)
        asm = Assembler(**kw, device=DEV)
        plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64)
        pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, assemble=asm)
        mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(DEV)
        mels = [mel[0], mel[1, :, :17], mel[0, :, :33]]
        rs = Resampler(16000, device=DEV)
        items = [w.cpu().numpy() for w in plain.infer_batch(mels)]
        spans = R.spans_f32(items, 256, 64, 25.0, None, 32)
        cap = asm.capacity(3, 256 * 40)
        joined, offs = R.join_f32(items, spans, 16, 200, cap)
        row = torch.from_numpy(joined).to(DEV)[None]
        n = rs.out_range(0, offs[-1])[1]
        want = rs.forward(row, lengths=[offs[-1]], row_scale=1, pcm16=True)[0, :n]
        got, got_spans = pipe.infer_batch(mels, resampler=rs, pcm16=True)
        assert got.dtype == torch.int16 and got.shape == (n,) and torch.equal(got, want)
        assert got_spans.cpu().tolist() == [list(s) for s in spans]
        wave, _ = pipe.infer_batch(mels)
        assert torch.equal(wave, row[0, :offs[-1]])
        one, one_span = pipe.infer(mel[:1])                                                    # one item: trimmed, a join of one
        assert one_span.cpu().tolist() == [list(spans[0])] and torch.equal(one, torch.from_numpy(R.faded_f32(items[0], spans[0], 16)).to(DEV))
    finally:
        eng.close()
