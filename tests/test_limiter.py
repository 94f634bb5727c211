"""The limiter without a GPU and without a launch: the library's host-only answers and every refusal that needs no handle, the
design table against its float64 derivation, the restatement with the kernel's operations against the plain float64 one within a
bar derived from the chain lengths, the ceiling, the untouched item, ``g <= r``, where the clamp engages, the true peak of an
fs / 4 sine, and the pipeline's and the command line's argument handling (a short workspace and an overlapping output are refused
behind the handle check, so tests/test_gpu_limiter.py holds those)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.limiter import MAX_LOOKAHEAD, TILE, Limiter
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import build_parser, check_limit_dbtp, main

import limiter_cases as C
import limiter_restatement as R

CASE_IDS = [C.case_id(c) for c in C.CASES]
INVALID, UNSUPPORTED = 1, 4
_tables = {}


def table_of(c):
    if c["A"] not in _tables:
        _tables[c["A"]] = Limiter(C.RATE, 0.0, float(c["A"])).design()
    return _tables[c["A"]]


# ---- the library's host-only answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_host_only_answers(c):
    a = Limiter(**C.params(c))
    B, L = len(c["items"]), c["L"]
    assert a.lookahead == c["A"] and np.float32(a.ceiling) == np.float32(c["c"])
    assert a.launch_count(B, L) == 2 and a.launch_count(B, L, measure_only=True) == 2
    assert a.launch_count(0, L) == 0 and a.launch_count(B, 0) == 0
    tiles = -(-L // TILE)
    assert a.workspace_bytes(B, L) == max(256, 4 * ((2 * B * tiles + 63) // 64 * 64)) and a.workspace_bytes(0, 0) == 256
    assert a.get_config() == C.params(c) and a.design().shape == (36 + 2 * c["A"] + 1,)
    assert np.array_equal(a.design(), table_of(c))                       # the table does not depend on the ceiling


def _status(fn, cfg, *args):
    out = (ctypes.c_uint64 if fn.endswith("bytes") else ctypes.c_int32)()
    return getattr(_native.load(), fn)(ctypes.byref(cfg) if cfg is not None else None, *args, ctypes.byref(out))


def test_refusals_come_before_any_device_work():
    good = dict(ceiling=0.9, lookahead=33)
    cfg = lambda **kw: _native.LimiterConfig(**{**good, **kw})
    invalid = [dict(ceiling=0.0), dict(ceiling=-0.5), dict(ceiling=1.0001), dict(ceiling=float("nan")), dict(ceiling=float("inf")),
               dict(lookahead=0), dict(lookahead=-1), dict(lookahead=MAX_LOOKAHEAD + 1)]
    queries = (("iris_limiter_workspace_bytes", ()), ("iris_limiter_launch_count", (0,)), ("iris_limiter_launch_count", (1,)))
    for fn, extra in queries:
        assert _status(fn, cfg(), 2, 100, *extra) == 0
        for ok in (dict(ceiling=1.0), dict(ceiling=1e-6), dict(lookahead=1), dict(lookahead=MAX_LOOKAHEAD)):
            assert _status(fn, cfg(**ok), 2, 100, *extra) == 0, (fn, ok)                       # the limits themselves
        for kw in invalid:
            assert _status(fn, cfg(**kw), 2, 100, *extra) == INVALID, (fn, kw)
        assert _status(fn, None, 2, 100, *extra) == INVALID                                   # a NULL config
        assert getattr(_native.load(), fn)(ctypes.byref(cfg()), 2, 100, *extra, None) == INVALID  # a NULL result
        assert _status(fn, cfg(), -1, 100, *extra) == INVALID and _status(fn, cfg(), 2, -1, *extra) == INVALID
        assert _status(fn, cfg(), 65535, 100, *extra) == 0 and _status(fn, cfg(), 65536, 100, *extra) == UNSUPPORTED   # grid.y
        assert _status(fn, cfg(), 4096, 1 << 19, *extra) == UNSUPPORTED                       # B L = 2^31
        assert _status(fn, cfg(), 2, (1 << 30) - 1, *extra) == 0
        assert _status(fn, cfg(), 0, 100, *extra) == 0 and _status(fn, cfg(), 2, 0, *extra) == 0       # nothing to do
    lib, n = _native.load(), 36 + 2 * 33 + 1
    table = (ctypes.c_float * n)()
    assert lib.iris_limiter_design(ctypes.byref(cfg()), table, n) == 0
    assert lib.iris_limiter_design(ctypes.byref(cfg()), table, n - 1) == INVALID
    assert lib.iris_limiter_design(ctypes.byref(cfg()), None, n) == INVALID
    assert lib.iris_limiter_design(ctypes.byref(cfg(lookahead=0)), table, n) == INVALID
    assert lib.iris_limiter_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.iris_limiter_create(ctypes.byref(cfg()), None) == INVALID
    assert lib.iris_limiter_create(ctypes.byref(cfg(ceiling=2.0)), ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.iris_limiter_forward_ragged(None, None, 2, 100, None, 1, None, None, None, 0, None) == INVALID      # a NULL handle
    assert lib.iris_limiter_measure_ragged(None, None, 2, 100, None, 1, None, None, 0, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
    for kw, what in ((dict(lookahead_ms=0.01), "lookahead_ms"), (dict(lookahead_ms=12.0), "lookahead_ms"), (dict(ceiling_dbtp=0.5), "ceiling_dbtp"),
                     (dict(ceiling_dbtp=float("nan")), "ceiling_dbtp"), (dict(sample_rate=22050.5), "sample_rate"),
                     (dict(lookahead_ms=float("nan")), "lookahead_ms")):
        with pytest.raises(ValueError, match=what):
            Limiter(**kw)
    assert Limiter().lookahead == 33 and Limiter(22050, -1.0, 1.5).get_config()["ceiling_dbtp"] == -1.0
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION


# ---- the design table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 33, 256])
def test_design_is_its_float64_derivation_rounded_once(A):
    """Every value of the library's table is ONE fp32 rounding of the value derived here in float64 from numpy's own ``sinc``,
    ``i0`` and ``cos``, in the direction the rules name.  The bank is rounded to nearest: within half an ulp, 2^-24 relative.  The
    weights are rounded upward: not under the derived value and less than one ulp (at most 2^-23 relative) over it.  Either bar
    has 2^-20 of itself added for the two float64 evaluations' own error."""
    lib = Limiter(C.RATE, -3.0, float(A)).design().astype(np.float64)
    bank, w = R.design_f64(A)
    own = bank.reshape(-1)
    worst = float((np.abs(lib[:36] - own) / np.abs(own)).max())
    up = (lib[36:] - w) / w
    print(f"A = {A}: bank, largest relative distance to the float64 derivation {worst:.3e} (half an ulp: {2.0 ** -24:.3e}); "
          f"weights, lib / derived - 1 in [{up.min():.3e}, {up.max():.3e}] (an ulp: at most {2.0 ** -23:.3e}); "
          f"sum(w) - 1 = {lib[36:].sum() - 1.0:.3e}")
    assert np.all(np.abs(lib[:36] - own) <= 2.0 ** -24 * np.abs(own) * (1.0 + 2.0 ** -20))
    assert np.all(up >= -(2.0 ** -43)) and np.all(up <= 2.0 ** -23 * (1.0 + 2.0 ** -20))
    assert lib[36:].sum() >= 1.0                                                                         # what g <= r needs
    assert abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(lib[36:], lib[36:][::-1].copy())              # the shape is even
    assert np.all(np.abs(bank.sum(axis=1) - 1.0) < 1e-2)                                                 # unit gain at 0 Hz


# ---- the two restatements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_kernel_operations_agree_with_float64_within_the_derived_bar(c):
    table = table_of(c)
    C.check_conditions(c, table)
    worst = dict(p=0.0, g=0.0, out=0.0)
    bars = dict(p=0.0, g=0.0, out=0.0)
    for y, ref, dev in zip(c["items"], C.reference(c, table), C.device(c, table)):
        bar = R.error_bars(y, c["c"], c["A"], table)
        for k in ("p", "g", "out"):
            diff = np.abs(dev[k].astype(np.float64) - ref[k])
            if len(diff):
                worst[k], bars[k] = max(worst[k], float(diff.max())), max(bars[k], float(bar[k].max()))
            assert np.all(diff <= bar[k]), (c["name"], k)
        assert dev["out"].dtype == dev["g"].dtype == np.float32
    print(f"{c['name']}: largest |f32 - f64| (largest bar): " + ", ".join(f"{k} {worst[k]:.3e} ({bars[k]:.3e})" for k in worst))


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_output_stays_under_the_ceiling_and_a_quiet_item_is_untouched(c):
    table, ceiling = table_of(c), np.float32(c["c"])
    for y, ref, dev in zip(c["items"], C.reference(c, table), C.device(c, table)):
        assert np.all(np.abs(dev["out"]) <= ceiling)                                             # exactly, not within a bar
        if ref["tp"] <= float(ceiling) and dev["tp"] <= ceiling:
            assert np.array_equal(dev["out"].view(np.uint32), y.view(np.uint32)) and dev["min_g"] == 1.0
            assert np.all(dev["g"] == 1.0)


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_gain_is_at_most_the_required_gain_in_float64(c):
    """``g[n] <= r[n]`` in ``plain_f64``, as the rules state it for exact arithmetic: every m of the chain is at most r[n], so
    ``g[n] <= 1 - (1 - r[n]) sum(w)``, which is at most r[n] where the table's weights sum to 1 or more.  They are rounded to fp32
    upward for that reason (csrc/limiter.h); rounded to nearest they sum to 1 - 3.827e-9 at A = 33, and g passed r by up to
    2.551e-9 at the isolated peaks of these cases."""
    table = table_of(c)
    worst = -np.inf
    for ref in C.reference(c, table):
        if len(ref["g"]):
            worst = max(worst, float((ref["g"] - ref["r"]).max()))
    print(f"{c['name']}: largest g - r in float64 = {worst:.3e}; sum(w) - 1 = {float(table[36:].astype(np.float64).sum() - 1.0):.3e}")
    assert worst <= 0.0


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_clamp_engages_only_within_rounding(c):
    """Where the fp32 product ``x g`` passes the ceiling it does so by no more than the derived bar of the output, plus what the
    rounded weights' sum lacks of 1: ``|x| (1 - r) max(0, 1 - sum w)``, since ``|x| r <= p r <= c``."""
    table, ceiling = table_of(c), float(np.float32(c["c"]))
    lack = max(0.0, 1.0 - float(table[36:].astype(np.float64).sum()))
    engaged, worst = 0, 0.0
    for y, ref, dev in zip(c["items"], C.reference(c, table), C.device(c, table)):
        if not len(y):
            continue
        over = np.abs(dev["raw"].astype(np.float64)) - ceiling
        bar = R.error_bars(y, c["c"], c["A"], table)["out"] + np.abs(y.astype(np.float64)) * (1.0 - ref["r"]) * lack + 2.0 ** -52
        hit = over > 0.0
        engaged += int(hit.sum())
        if hit.any():
            worst = max(worst, float(over[hit].max()))
        assert np.all(over[hit] <= bar[hit]), c["name"]
    print(f"{c['name']}: the clamp engaged at {engaged} samples, by at most {worst:.3e}")


def test_true_peak_of_a_quarter_rate_sine_exceeds_its_sample_peak():
    amp, n = 0.9, 4096
    y = C.quarter_sine(n, 1.0, amp)
    table = Limiter(C.RATE, 0.0, 33.0).design()
    ref = R.plain_f64(y, 1.0, 33, table)
    mid = slice(64, n - 64)
    sample_peak, tp = float(np.abs(y).max()), float(ref["p"][mid].max())
    # a dense 64 x float64 sinc interpolation of the middle of the item
    t = 2048.0 + np.arange(4 * 64) / 64.0
    k = np.arange(n, dtype=np.float64)
    dense = float(np.abs(np.sinc(t[:, None] - k[None, :]) @ y.astype(np.float64)).max())
    print(f"fs / 4 sine of amplitude {amp}: sample peak {sample_peak:.4f}, 4 x true peak {tp:.4f}, 64 x sinc {dense:.4f}; "
          f"under-read {20.0 * np.log10(tp / dense):+.3f} dB (the samples alone: {20.0 * np.log10(sample_peak / dense):+.3f} dB)")
    assert abs(sample_peak - amp / np.sqrt(2.0)) < 1e-6 and tp > sample_peak * 1.2
    assert ref["tp"] <= 1.0 and np.array_equal(ref["out"], y.astype(np.float64))


# ---- the pipeline and the command line -----------------------------------------------------------------------------------
class _Stage:
    """Stands in for ``LoudnessNormalizer`` (doubles) or ``Limiter`` (clips at 1.5) and notes what it was handed."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def _note(self, wav, lengths, row_scale):
        self.log.append((self.name, float(wav.abs().max()), None if lengths is None else [int(v) for v in lengths], row_scale))

    def normalize_device(self, wav, lengths=None, row_scale=1):
        self._note(wav, lengths, row_scale)
        return wav * 2.0, torch.zeros((wav.shape[0], 2), dtype=torch.float64)

    def limit_device(self, wav, lengths=None, row_scale=1):
        self._note(wav, lengths, row_scale)
        return wav.clamp(-1.5, 1.5), torch.zeros((wav.shape[0], 2))

    def join_device(self, wav, lengths=None, row_scale=1):
        self._note(wav, lengths, row_scale)
        return wav.reshape(-1), torch.tensor([0] * wav.shape[0] + [wav.numel()], dtype=torch.int32), torch.zeros((wav.shape[0], 2), dtype=torch.int32)


def _vocode(mel, lengths=None):
    return torch.ones((mel.shape[0], 4 * mel.shape[2]), dtype=torch.float32)


def test_pipeline_limits_behind_the_level_and_in_front_of_the_join():
    log = []
    mels = [np.zeros((80, 8), np.float32), np.zeros((80, 5), np.float32)]
    plain = MelToWavePipeline(None, _vocode, hop_length=4)
    assert plain.limiter is None and [tuple(w.shape) for w in plain.infer_batch(mels)] == [(32,), (20,)]
    out = MelToWavePipeline(None, _vocode, hop_length=4, limiter=_Stage(log, "limiter")).infer_batch(mels)
    assert log == [("limiter", 1.0, [8, 5], 4)]                          # the batch's frames and the hop
    assert [tuple(w.shape) for w in out] == [(32,), (20,)] and all(float(w.max()) == 1.0 for w in out)
    del log[:]
    joined, _ = MelToWavePipeline(None, _vocode, hop_length=4, loudness=_Stage(log, "loudness"), limiter=_Stage(log, "limiter"),
                                  assemble=_Stage(log, "assemble")).infer_batch(mels)
    assert log == [("loudness", 1.0, [8, 5], 4), ("limiter", 2.0, [8, 5], 4), ("assemble", 1.5, [8, 5], 4)]
    assert joined.shape == (64,)
    del log[:]
    one = MelToWavePipeline(None, _vocode, hop_length=4, loudness=_Stage(log, "loudness"), limiter=_Stage(log, "limiter")).infer(
        np.zeros((1, 80, 6), np.float32))
    assert log == [("loudness", 1.0, None, 1), ("limiter", 2.0, None, 1)] and one.shape == (1, 24) and float(one.max()) == 1.5


def test_pipeline_refuses_to_stream_with_a_limiter():
    pipe = MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256, limiter=_Stage([], "limiter"))
    mel = np.zeros((1, 80, 8), np.float32)
    with pytest.raises(ValueError, match="no chunked form is built"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="no chunked form is built"):
        pipe.session()


def test_command_line_takes_a_true_peak_ceiling(tmp_path):
    args = build_parser().parse_args(["--mel", "m.npy", "--lufs", "-16", "--limit_dbtp", "-1"])
    assert args.limit_dbtp == -1.0 and build_parser().parse_args(["--mel", "m.npy"]).limit_dbtp is None
    assert check_limit_dbtp(-20) == -20.0 and check_limit_dbtp(0) == 0.0
    for bad in (0.5, -20.5, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="limit_dbtp"):
            check_limit_dbtp(bad)
    for bad in ("3", "-30", "nan"):
        with pytest.raises(SystemExit):
            main(["--mel", str(tmp_path / "absent.npy"), "--limit_dbtp", bad])
    with pytest.raises(SystemExit):
        main(["--mel", str(tmp_path / "absent.npy"), "--limit_dbtp", "-1", "--pcm16"])
