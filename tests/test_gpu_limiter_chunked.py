"""The chunked limiter on the device: a ``LimiterSession`` over every piece schedule against the one-shot call and the numpy
restatement, in fp32 and as 16-bit PCM; raw ``iris_limiter_forward_window`` calls with poisoned buffers, packed rows off 16 bytes
and a guarded workspace; a window that is the whole utterance against ``forward_ragged``; and the pipeline's ``stream`` /
``session`` with ``limiter=lim.chunked()`` against ``infer``.  Every comparison is an equality of bits."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import Denoiser
from iris.limiter import TILE as T, Limiter
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import pcm16_on_device
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import limiter_cases as C
import limiter_restatement as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
GUARD = 256                       # bytes behind the workspace's stated size that must stay as they were
TOO_SMALL = 5                     # IRIS_HIFIGAN_WORKSPACE_TOO_SMALL
LOOKAHEADS = (1, 33, 256)
CUT = T + 5

_state = {}


def case_of(A):
    return next(c for c in C.CASES if c["name"] == f"placements_A{A}")


def reach_of(A):
    return 2 * A + 7


def model(A) -> Limiter:
    if ("model", A) not in _state:
        _state["model", A] = Limiter(**C.params(case_of(A)), device=DEV)
    return _state["model", A]


def cut_items(A):
    """The window-specific input: spikes at ``CUT - 1`` and ``CUT + R``, so the first spike's gain ramp lies within ``R`` of a
    window edge on both sides of a cut at ``CUT``; and an item that is never limited."""
    c = case_of(A)
    return [C.spiked(c["L"], c["c"], 800 + A, [CUT - 1, CUT + reach_of(A)]), C.quiet(c["L"], c["c"], 801 + A)]


def schedules(A, L):
    Rr = reach_of(A)
    odd = [1, Rr - 1, 1, Rr + 1, T - 1, 3]
    equal = [257] * (L // 257) + ([L % 257] if L % 257 else [])
    return {"one push": [L], "odd pieces": odd + [L - sum(odd)], "equal 257": equal, "cut at T + 5": [CUT, L - CUT]}


def one_shot(A, which) -> dict:
    """The inputs and the references of lookahead ``A``, computed once: ``which`` is "case" (the placements batch, B = 6) or "cut"
    (the window-specific batch, B = 2).  ``dev``: ``R.device_f32`` per item; ``out`` / ``stats`` / ``pcm``: the one-shot device call."""
    key = ("one_shot", A, which)
    if key not in _state:
        c, a = case_of(A), model(A)
        table = a.design()
        items = c["items"] if which == "case" else cut_items(A)
        dev = C.device(c, table) if which == "case" else [R.device_f32(y, c["c"], A, table) for y in items]
        wav = torch.from_numpy(np.stack(items)).to(DEV)
        out, stats = a.limit_device(wav)
        _state[key] = dict(items=items, dev=dev, wav=wav, out=out, stats=stats, pcm=pcm16_on_device(out),
                           want_out=np.stack([r["out"] for r in dev]),
                           want_stats=np.array([[r["tp"], r["min_g"]] for r in dev], dtype=np.float32))
    return _state[key]


def ptr(t):
    return t if isinstance(t, ctypes.c_void_p) else ctypes.c_void_p(None if t is None else t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(x: torch.Tensor, y: torch.Tensor) -> bool:
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ---- the inputs are not vacuous --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_a_seam_cuts_a_gain_ramp_and_an_item_is_never_limited(A):
    """In ``plain_f64`` alone: some schedule has a seam at sample s with ``g < 1`` somewhere in ``[s - R, s)`` and somewhere in ``[s,
    s + R)``; the placements case has an item that is limited and one that is not; the window-specific batch too."""
    c, a, Rr = case_of(A), model(A), reach_of(A)
    table = a.design()
    C.check_conditions(c, table)
    refs = {"case": C.reference(c, table), "cut": [R.plain_f64(y, c["c"], A, table) for y in cut_items(A)]}
    ceiling = float(np.float32(c["c"]))
    assert refs["cut"][0]["min_g"] < 1.0 and refs["cut"][1]["tp"] <= ceiling and refs["cut"][1]["min_g"] == 1.0
    assert any(r["tp"] <= ceiling and r["min_g"] == 1.0 for r in refs["case"])
    found = []
    for name, pieces in schedules(A, c["L"]).items():
        for s in np.cumsum(pieces)[:-1]:
            for which, ref in refs.items():
                for r in ref:
                    if (r["g"][max(0, s - Rr):s] < 1.0).any() and (r["g"][s:s + Rr] < 1.0).any():
                        found.append((name, int(s), which))
    print(f"A = {A}: {len(found)} (schedule, seam, batch) with the gain under 1 on both sides within R = {Rr}, e.g. {found[:3]}")
    assert found and any(f[0] == "cut at T + 5" and f[1] == CUT for f in found)


# ---- the session against the one-shot call and the restatement -------------------------------------------------------------
def run_session(a, wav, pieces, pcm16):
    session, got, at = a.open_session(pcm16=pcm16), [], 0
    Rr = 2 * a.lookahead + 7
    for n in pieces:
        piece = session.push(wav[:, at:at + n])
        at += n
        assert session.samples_emitted == max(0, at - Rr) and session.samples_buffered <= 2 * Rr + n
        got.append(piece)
    got.append(session.flush())
    assert session.samples_emitted == wav.shape[1] and session.samples_buffered == 0
    return session, torch.cat(got, dim=1)


@pytest.mark.parametrize("which", ["case", "cut"])
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_session_equals_the_one_shot_call_bit_for_bit(A, which):
    a, ref = model(A), one_shot(A, which)
    L = ref["wav"].shape[1]
    assert L == 2 * T + 3
    # the one-shot call is the restatement (and, for the placements batch, what the existing tests expect of it)
    assert np.array_equal(bits(ref["out"].cpu().numpy()), bits(ref["want_out"]))
    assert np.array_equal(bits(ref["stats"].cpu().numpy()), bits(ref["want_stats"]))
    if which == "case":
        want_stats, want_out = C.expected(case_of(A), a.design())
        assert np.array_equal(bits(ref["want_out"]), bits(want_out)) and np.array_equal(bits(ref["want_stats"]), bits(want_stats))
    for name, pieces in schedules(A, L).items():
        assert sum(pieces) == L
        session, got = run_session(a, ref["wav"], pieces, pcm16=False)
        assert got.dtype == torch.float32 and same_bits(got, ref["out"]), (A, which, name)
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref["want_out"])), (A, which, name)
        assert same_bits(session.stats, ref["stats"]), (A, which, name)
        session, pcm = run_session(a, ref["wav"], pieces, pcm16=True)
        assert pcm.dtype == torch.int16 and torch.equal(pcm, ref["pcm"]), (A, which, name)
        assert same_bits(session.stats, ref["stats"]), (A, which, name)
    print(f"A = {A}, {which}: gains down to {float(ref['stats'][:, 1].min()):.4f}, |pcm| up to {int(ref['pcm'].abs().max())}")


# ---- raw calls --------------------------------------------------------------------------------------------------------------
def raw_window(a, wav_d, origin, final, out, pcm16, stats, ws, nbytes):
    B, Lw = wav_d.shape
    with torch.cuda.device(DEV):
        return _native.load().iris_limiter_forward_window(
            a._handle, ptr(wav_d), B, Lw, ctypes.c_int64(origin), int(final), ptr(out), int(pcm16), ptr(stats), ptr(ws),
            ctypes.c_uint64(nbytes), stream())


@pytest.mark.parametrize("A", LOOKAHEADS)
def test_raw_window_stores_every_element_and_nothing_else(A):
    """A window of the placements batch at an odd origin, ending inside the utterance: packed rows ``[B, count]`` with ``count``
    odd, so rows start off 16 bytes.  ``out``, ``stats`` and the workspace (with ``GUARD`` bytes behind it) are poisoned beforehand."""
    a, ref, Rr = model(A), one_shot(A, "case"), reach_of(A)
    a._ensure()
    origin, Lw = 3, 2 * T - 41
    window = ref["wav"][:, origin:origin + Lw].contiguous()
    B = window.shape[0]
    lo, count = a.window_range(origin, Lw, False)
    assert (lo, count) == (origin + Rr, Lw - 2 * Rr) and count % 2 == 1 and count > T       # two tiles, odd packed rows
    need = a.window_workspace_bytes(B, Lw)
    tiles = -(-count // T)
    want_stats = np.array([[r["p"][lo:lo + count].max(), r["g"][lo:lo + count].min()] for r in ref["dev"]], dtype=np.float32)
    runs = []
    for _ in range(2):
        out = torch.full((B, count), NAN, dtype=torch.float32, device=DEV)
        stats = torch.full((B, 2), NAN, dtype=torch.float32, device=DEV)
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        _native.check("iris_limiter_forward_window", raw_window(a, window, origin, False, out, False, stats, ws, need))
        torch.cuda.synchronize()
        assert not torch.isnan(out).any() and not torch.isnan(stats).any()                     # every element was stored
        assert same_bits(out, ref["out"][:, lo:lo + count])
        assert np.array_equal(bits(stats.cpu().numpy()), bits(want_stats))
        host = ws.cpu().numpy()
        assert (host[need:] == 0xFF).all() and (host[4 * 2 * B * tiles:] == 0xFF).all()       # the guard, and all but the partials
        assert not np.isnan(host[:4 * 2 * B * tiles].view(np.float32)).any()
        runs.append((out, stats, host))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # out at every offset from 16 bytes, fp32 and PCM: the same bits, and the words around it stay
    mark = 0x5EED
    want_pcm = ref["pcm"][:, lo:lo + count]
    for pcm16, dtype in ((False, torch.float32), (True, torch.int16)):
        for shift in (0, 1, 2, 3):
            buf = torch.full((64 + shift + B * count + 64,), mark, dtype=torch.int16 if pcm16 else torch.int32, device=DEV)
            out = buf[64 + shift:64 + shift + B * count].view(dtype).view(B, count)
            assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == (2 if pcm16 else 4) * shift
            stats = torch.full((B, 2), NAN, dtype=torch.float32, device=DEV)
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
            _native.check("iris_limiter_forward_window", raw_window(a, window, origin, False, out, pcm16, stats, ws, need))
            torch.cuda.synchronize()
            if pcm16:
                assert torch.equal(out, want_pcm), (A, shift)
            else:
                assert same_bits(out, ref["out"][:, lo:lo + count]), (A, shift)
            assert np.array_equal(bits(stats.cpu().numpy()), bits(want_stats))
            assert (buf[:64 + shift] == mark).all() and (buf[64 + shift + B * count:] == mark).all(), (A, pcm16, shift)


def test_raw_window_refusals_and_a_window_that_settles_nothing():
    A = 33
    a, ref, Rr = model(A), one_shot(A, "case"), reach_of(A)
    a._ensure()
    origin, Lw = 3, 1000
    window = ref["wav"][:, origin:origin + Lw].contiguous()
    B = window.shape[0]
    count = a.window_range(origin, Lw, False)[1]
    need = a.window_workspace_bytes(B, Lw)

    def poisoned(n):
        return (torch.full((B, max(n, 1)), NAN, dtype=torch.float32, device=DEV), torch.full((B, 2), NAN, dtype=torch.float32, device=DEV),
                torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV))

    def untouched(out, stats, ws):
        torch.cuda.synchronize()
        return bool(torch.isnan(out).all() and torch.isnan(stats).all() and (ws == 0xFF).all())

    out, stats, ws = poisoned(count)
    assert raw_window(a, window, origin, False, out, False, stats, ws, need - 1) == TOO_SMALL          # one byte short
    assert raw_window(a, window, origin, False, out, True, stats, ws, need - 1) == TOO_SMALL
    assert raw_window(a, window, -1, False, out, False, stats, ws, need) == 1
    assert raw_window(a, window, origin, False, None, False, stats, ws, need) == 1
    assert raw_window(a, window, origin, False, out, False, None, ws, need) == 1
    assert raw_window(a, window, origin, False, out, False, stats, None, need) == 1
    assert raw_window(a, window, origin, False, window, False, stats, ws, need) == 1                   # out overlaps wav
    assert raw_window(a, window, origin, False, ctypes.c_void_p(out.data_ptr() + 2), False, stats, ws, need) == 1    # fp32 off 4 bytes
    with torch.cuda.device(DEV):
        assert _native.load().iris_limiter_forward_window(a._handle, None, B, Lw, origin, 0, ptr(out), 0, ptr(stats), ptr(ws), need, stream()) == 1
    assert untouched(out, stats, ws)                                                                   # no refused call launched
    # windows that settle nothing: shorter than 2R inside an utterance, shorter than R at its start, empty at its end
    for org, n, final in ((origin, 2 * Rr, False), (0, Rr, False), (origin, Rr, True), (origin, 0, True)):
        assert a.window_range(org, n, final)[1] == 0 and a.window_launch_count(B, n, org, final) == 0
        short = ref["wav"][:, org:org + n].contiguous()
        assert raw_window(a, short, org, final, out, False, stats, ws, need) == 0
        assert untouched(out, stats, ws), (org, n, final)
        got, got_stats = a.forward_window(short, org, final)
        assert got.shape == (B, 0) and torch.equal(got_stats.cpu(), torch.tensor([[0.0, 1.0]] * B))


@pytest.mark.parametrize("A", LOOKAHEADS)
def test_a_window_that_is_the_whole_utterance_equals_forward_ragged(A):
    a, ref = model(A), one_shot(A, "case")
    L = ref["wav"].shape[1]
    assert a.window_range(0, L, True) == (0, L)
    out, stats = a.forward_window(ref["wav"], 0, True)
    assert same_bits(out, ref["out"]) and same_bits(stats, ref["stats"])
    pcm, stats = a.forward_window(ref["wav"], 0, True, pcm16=True)
    assert torch.equal(pcm, ref["pcm"]) and same_bits(stats, ref["stats"])


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_pipeline_streams_what_infer_returns():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        lm = Limiter(22050, ceiling_dbtp=-12.0, lookahead_ms=1.5, device=DEV)
        mel = torch.from_numpy(seeded_mel(3, 1, 40, log_mel=True)).to(DEV)
        kw = dict(device=DEV, chunk_frames=16)
        plain = MelToWavePipeline(None, eng.forward, limiter=lm, **kw)
        want, want_pcm = plain.infer(mel), plain.infer(mel, pcm16=True)
        stats = lm.true_peak_device(MelToWavePipeline(None, eng.forward, **kw).infer(mel))
        print(f"vocoder output: true peak {float(stats[0, 0]):.4f} over the ceiling {lm.ceiling:.4f}, gain down to {float(stats[0, 1]):.4f}")
        assert float(stats[0, 1]) < 1.0 and float(want.abs().max()) <= lm.ceiling              # the limiter acts
        assert want.shape == (1, 256 * 40) and want_pcm.dtype == torch.int16

        def pushed(pipe):
            session, got, at = pipe.session(), [], 0
            for t in (7, 1, 0, 20, 12):
                got += session.push(mel[:, :, at:at + t])
                at += t
            return torch.cat(got + session.flush(), dim=1)

        pipe = MelToWavePipeline(None, eng.forward, limiter=lm.chunked(), **kw)
        pieces = list(pipe.stream(mel))
        assert len(pieces) == 4 and pieces[0].shape[1] == 256 * 16 - 73 and pieces[-1].shape[1] == 73
        assert same_bits(torch.cat(pieces, dim=1), want) and same_bits(pushed(pipe), want)
        assert same_bits(pipe.infer(mel), want) and torch.equal(pipe.infer(mel, pcm16=True), want_pcm)
        pipe16 = MelToWavePipeline(None, eng.forward, limiter=lm.chunked(pcm16=True), **kw)
        streamed = torch.cat(list(pipe16.stream(mel)), dim=1)
        assert streamed.dtype == torch.int16 and torch.equal(streamed, want_pcm) and torch.equal(pushed(pipe16), want_pcm)
        assert torch.equal(pipe16.infer(mel, pcm16=True), want_pcm) and same_bits(pipe16.infer(mel), want)
        # a chunked denoiser in front of it
        dn = Denoiser(1024, 256, 1024, strength=0.5, bias=np.full(513, 0.5, dtype=np.float32), device=DEV)
        both = MelToWavePipeline(None, eng.forward, denoiser=dn, limiter=lm, **kw).infer(mel)
        assert not same_bits(both, want)                                                        # the denoiser does something
        chained = MelToWavePipeline(None, eng.forward, denoiser=dn.chunked(), limiter=lm.chunked(), **kw)
        assert same_bits(torch.cat(list(chained.stream(mel)), dim=1), both) and same_bits(pushed(chained), both)
        with pytest.raises(ValueError, match="limiter= cannot be streamed.*no chunked form is built"):
            next(iter(plain.stream(mel)))
    finally:
        eng.close()
