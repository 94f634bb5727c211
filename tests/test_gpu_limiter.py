"""The limiter on the device against its restatement with the kernel's own operations (tests/limiter_restatement.py:
``device_f32``): the samples, the statistics and the tiles' partials bit for bit, every output element stored and nothing else, an
item independent of its neighbours, ``measure`` equal to ``forward``'s statistics, ``out`` off a 16-byte boundary, the refusals
behind the handle, and the pipeline's route equal to the stages applied by hand."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.assemble import Assembler
from iris.limiter import TILE, Limiter
from iris.loudness import LoudnessNormalizer
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import pcm16_on_device
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import assemble_restatement as AR
import limiter_cases as C
import limiter_restatement as R
import loudness_restatement as LR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
CASE_IDS = [C.case_id(c) for c in C.CASES]
GUARD = 256                       # bytes behind the workspace's stated size that must stay as they were
TOO_SMALL = 5                     # IRIS_HIFIGAN_WORKSPACE_TOO_SMALL

_state = {}


def model(c) -> Limiter:
    key = (c["A"], c["c"])
    if key not in _state:
        _state[key] = Limiter(**C.params(c), device=DEV)
    return _state[key]


def ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def poisoned(c) -> dict:
    """One raw call per case, kept: the row tails behind L_b hold NaN, ``lengths`` is a device tensor, and ``out``, ``stats`` and
    the workspace (with ``GUARD`` bytes behind it) are poisoned beforehand."""
    if c["name"] in _state:
        return _state[c["name"]]
    a = model(c)
    a._ensure()
    wav, lengths, row_scale = C.batch(c, fill=NAN)
    B, L = wav.shape
    need = a.workspace_bytes(B, L)
    wav_d = torch.from_numpy(wav).to(DEV)
    len_d = None if lengths is None else torch.from_numpy(lengths).to(DEV)
    out = torch.full((B, L), NAN, dtype=torch.float32, device=DEV)
    stats = torch.full((B, 2), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _native.check("iris_limiter_forward_ragged", _native.load().iris_limiter_forward_ragged(
            a._handle, ptr(wav_d), B, L, ptr(len_d), row_scale, ptr(out), ptr(stats), ptr(ws), ctypes.c_uint64(need), stream()))
    torch.cuda.synchronize()
    _state[c["name"]] = dict(out=out, stats=stats, ws=ws.cpu().numpy(), need=need, wav=wav_d, lengths=len_d, row_scale=row_scale)
    return _state[c["name"]]


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_samples_stats_and_workspace_match_the_restatement(c):
    got, a = poisoned(c), model(c)
    table = a.design()
    assert np.float32(a.ceiling) == np.float32(c["c"]) and a.lookahead == c["A"]
    dev = C.device(c, table)
    want_stats, want_out = C.expected(c, table)
    B, L = len(c["items"]), c["L"]
    stats, out = got["stats"].cpu().numpy(), got["out"].cpu().numpy()
    print(f"{c['name']}: true peaks up to {stats[:, 0].max():.4f}, gains down to {stats[:, 1].min():.4f}, ceiling {c['c']}")
    assert not np.isnan(out).any()                                                            # all of out [B, L] was stored
    assert np.array_equal(bits(out), bits(want_out))                                          # the zeros behind L_b too
    assert np.array_equal(bits(stats), bits(want_stats))
    # the workspace: an item's own tiles bit for bit, and nothing else touched
    tiles = -(-L // TILE)
    ws = got["ws"]
    assert got["need"] == max(256, 4 * ((2 * B * tiles + 63) // 64 * 64))
    touched = np.zeros(len(ws), dtype=bool)
    for b, (y, r) in enumerate(zip(c["items"], dev)):
        want = R.tile_parts(r, len(y), TILE)
        lo = 4 * 2 * tiles * b
        touched[lo:lo + want.size * 4] = True
        assert np.array_equal(ws[lo:lo + want.size * 4].view(np.uint32), bits(want).reshape(-1)), b
    assert (ws[~touched] == 0xFF).all()                                                       # other tiles, padding, the guard


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_unpoisoned_call_repeats_and_measure_gives_the_same_stats(c):
    got, a = poisoned(c), model(c)
    wav, lengths, row_scale = C.batch(c)
    first = a.limit_device(wav, lengths=lengths, row_scale=row_scale)
    second = a.limit_device(torch.from_numpy(wav).to(DEV), lengths=got["lengths"], row_scale=row_scale)
    for x, y, z in zip(first, second, (got["out"], got["stats"])):
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), z.view(torch.int32))      # NaN tails change nothing
    # measure: the same statistics, and it writes nothing but them and the workspace
    B, L = wav.shape
    need = a.workspace_bytes(B, L)
    stats = torch.full((B, 2), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _native.check("iris_limiter_measure_ragged", _native.load().iris_limiter_measure_ragged(
            a._handle, ptr(got["wav"]), B, L, ptr(got["lengths"]), row_scale, ptr(stats), ptr(ws), ctypes.c_uint64(need), stream()))
    torch.cuda.synchronize()
    assert torch.equal(stats.view(torch.int32), got["stats"].view(torch.int32))
    assert np.array_equal(ws.cpu().numpy(), got["ws"])                                        # the same workspace, the same guard
    assert torch.equal(a.true_peak_device(wav, lengths=lengths, row_scale=row_scale).view(torch.int32), got["stats"].view(torch.int32))
    tp = got["stats"][:, 0].cpu().numpy()
    assert np.array_equal(np.isneginf(a.true_peak_dbtp(got["stats"])), tp == 0.0)


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_items_are_their_batch_of_one_calls(c):
    got, a = poisoned(c), model(c)
    B = len(c["items"])
    picked = list(range(B)) if B <= 9 else [0, 1, 2, 63, 64, 128, 254, 256]
    for b in picked:
        y = c["items"][b]
        if len(y) == 0:
            continue
        one, one_stats = a.limit_device(y[None].copy())
        assert torch.equal(one_stats.view(torch.int32), got["stats"][b:b + 1].view(torch.int32)), b
        assert torch.equal(one[0].view(torch.int32), got["out"][b, :len(y)].view(torch.int32)), b


@pytest.mark.parametrize("name", ["edge_lengths_A33", "ragged_256"])
def test_out_off_a_16_byte_boundary(name):
    """The tile kernel stores 16 bytes at a time only where a tile's first output lies on 16 bytes.  With ``out`` 4, 8 and 12 bytes
    past such an address it gives the aligned call's bits, stores all of ``out`` and leaves the words around it alone."""
    c = next(c for c in C.CASES if c["name"] == name)
    a, aligned = model(c), poisoned(c)
    B, L = aligned["out"].shape
    need = a.workspace_bytes(B, L)
    guard, mark = 64, 0x5EEDBEEF
    assert aligned["out"].data_ptr() % 16 == 0
    for shift in (1, 2, 3):
        buf = torch.full((guard + shift + B * L + guard,), mark, dtype=torch.int32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        out = buf[guard + shift:guard + shift + B * L].view(torch.float32)
        assert out.data_ptr() % 16 == 4 * shift
        out.fill_(NAN)
        stats = torch.full((B, 2), NAN, dtype=torch.float32, device=DEV)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        with torch.cuda.device(DEV):
            _native.check("iris_limiter_forward_ragged", _native.load().iris_limiter_forward_ragged(
                a._handle, ptr(aligned["wav"]), B, L, ptr(aligned["lengths"]), aligned["row_scale"], ptr(out), ptr(stats), ptr(ws),
                ctypes.c_uint64(need), stream()))
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        assert torch.equal(out.view(torch.int32), aligned["out"].reshape(-1).view(torch.int32)), shift
        assert torch.equal(stats.view(torch.int32), aligned["stats"].view(torch.int32))
        assert (buf[:guard + shift] == mark).all() and (buf[guard + shift + B * L:] == mark).all()


def test_refusals_behind_the_handle():
    a = model(C.CASES[0])
    a._ensure()
    lib, B, L = _native.load(), 2, 100
    buf = torch.zeros(2 * B * L, dtype=torch.float32, device=DEV)
    stats = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
    ws = torch.zeros(a.workspace_bytes(B, L), dtype=torch.uint8, device=DEV)
    call = lambda wav, out, nbytes, scale=1, st=stats, w=ws: lib.iris_limiter_forward_ragged(
        a._handle, wav, B, L, None, scale, out, ptr(st), w if isinstance(w, ctypes.c_void_p) else ptr(w), ctypes.c_uint64(nbytes), None)
    at = lambda i: ctypes.c_void_p(buf.data_ptr() + 4 * i)
    assert call(at(0), at(B * L - 1), ws.numel()) == 1                                       # the last input sample is the first output
    assert call(at(0), at(0), ws.numel()) == 1
    assert call(None, at(B * L), ws.numel()) == 1 and call(at(0), None, ws.numel()) == 1
    assert call(at(0), at(B * L), ws.numel(), st=None) == 1
    assert call(at(0), at(B * L), ws.numel(), scale=0) == 1
    assert call(at(0), at(B * L), ws.numel(), w=ctypes.c_void_p(ws.data_ptr() + 4)) == 1     # a workspace off 8 bytes
    assert call(at(0), at(B * L), ws.numel() - 1) == TOO_SMALL                               # a short workspace
    assert lib.iris_limiter_measure_ragged(a._handle, at(0), B, L, None, 1, ptr(stats), ptr(ws), ctypes.c_uint64(ws.numel() - 1), None) == TOO_SMALL
    assert lib.iris_limiter_measure_ragged(a._handle, at(0), B, L, None, 1, ctypes.c_void_p(stats.data_ptr() + 2), ptr(ws),
                                           ctypes.c_uint64(ws.numel()), None) == 1          # stats off 4 bytes
    torch.cuda.synchronize()
    assert not buf.any() and not stats.any() and not ws.any()                                # no refused call launched


def test_pipeline_levels_limits_joins_and_converts_as_the_stages_by_hand():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        kw = dict(frame_length=256, hop_length=64, top_db=25.0, pad=32, fade=16, pause=200)
        asm = Assembler(**kw, device=DEV)
        ld = LoudnessNormalizer(22050, target_lufs=-6.0, max_gain_db=60.0, peak_ceiling=None, device=DEV)
        lm = Limiter(22050, ceiling_dbtp=-1.0, lookahead_ms=1.5, device=DEV)
        plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64)
        pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, loudness=ld, limiter=lm, assemble=asm)
        mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(DEV)
        mels = [mel[0], mel[1, :, :17], mel[0, :, :36]]                 # 10240, 4352 (under 400 ms: no block) and 9216 samples
        items = [w.cpu().numpy() for w in plain.infer_batch(mels)]
        ld_table, lm_table = ld.design(), lm.design()
        levelled = [LR.scaled(y, LR.device_f64(y, 22050, ld_table)["gain"]) for y in items]
        limited = [R.device_f32(y, lm.ceiling, lm.lookahead, lm_table) for y in levelled]
        ceiling = np.float32(lm.ceiling)
        assert any(r["tp"] > ceiling and r["min_g"] < 1.0 for r in limited)                   # the levelled items exceed the ceiling
        held = [r["out"] for r in limited]
        spans = AR.spans_f32(held, 256, 64, 25.0, None, 32)
        joined, offs = AR.join_f32(held, spans, 16, 200, asm.capacity(3, 256 * 40))
        row = torch.from_numpy(joined).to(DEV)[None]
        want = pcm16_on_device(row)[0, :offs[-1]]
        got, got_spans = pipe.infer_batch(mels, pcm16=True)
        assert got.dtype == torch.int16 and got.shape == (offs[-1],) and torch.equal(got, want)
        assert got_spans.cpu().tolist() == [list(s) for s in spans]
        wave, _ = pipe.infer_batch(mels)
        assert torch.equal(wave, row[0, :offs[-1]])
        only = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, loudness=ld, limiter=lm).infer_batch(mels)
        for w, y in zip(only, held):
            assert torch.equal(w, torch.from_numpy(y).to(DEV)) and float(w.abs().max()) <= float(ceiling)
        with pytest.raises(ValueError, match="limiter= cannot be streamed.*no chunked form is built"):
            next(iter(MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, limiter=lm).stream(mel[:1])))
    finally:
        eng.close()
