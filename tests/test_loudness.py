"""The loudness stage without a GPU: the K-weighting coefficients against the standard's table, the plain BS.1770 loop on a
full-scale sine, the restatement in the kernels' structure against the plain loop, the margin every block keeps from both gates,
the cases' reasons for being there, the library's host-only answers, every refusal that needs no handle, and the pipeline's and
the command line's argument handling (a short workspace and an overlapping output are refused behind the handle check, so
tests/test_gpu_loudness.py holds those)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.loudness import LoudnessNormalizer
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import build_parser, check_lufs, main

import loudness_cases as C
import loudness_restatement as R

CASE_IDS = [C.case_id(c) for c in C.CASES]
INVALID, UNSUPPORTED = 1, 4
# The two restatements differ by rounding order alone.  Their largest relative difference in ms_b over all items of all cases,
# measured on the CPU, is 3.4e-15; the bar is 16 times that.
MS_MEASURED, MS_BAR = 3.4e-15, 16 * 3.4e-15

TABLE_SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
TABLE_SHELF_A = (1.0, -1.69065929318241, 0.73248077421585)
TABLE_HP_A = (1.0, -1.99004745483398, 0.99007225036621)


# ---- the filters -------------------------------------------------------------------------------------------------------------
def test_coefficients_at_48000_are_the_standards_table():
    sb, sa, hb, ha = R.coefficients(48000)
    lib = LoudnessNormalizer(48000).design()
    assert lib.shape == (R.DESIGN,) == (_native.LOUDNESS_DESIGN_DOUBLES,)
    for got in ((sb, sa, hb, ha), (list(lib[0:3]), [1.0] + list(lib[3:5]), list(lib[5:8]), [1.0] + list(lib[8:10]))):
        assert np.abs(np.array(got[0]) - TABLE_SHELF_B).max() <= 1e-12 and np.abs(np.array(got[1]) - TABLE_SHELF_A).max() <= 1e-12
        assert list(got[2]) == [1.0, -2.0, 1.0] and np.abs(np.array(got[3]) - TABLE_HP_A).max() <= 1e-12


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 44100, 48000])
def test_library_design_is_the_restatements(rate):
    """The table the kernels read against the one derived here: the coefficients and thresholds to 1e-12 relative, the matrix
    powers to 1e-12 of their largest entry (the GPU tests hand the library's own table to ``device_f64``)."""
    kw = dict(target_lufs=-16.0, max_gain_db=20.0, peak_ceiling=0.9)
    lib, own = LoudnessNormalizer(rate, **kw).design(), R.design(rate, -16.0, 20.0, 0.9)
    assert np.all(np.abs(lib[:R.MATS] - own[:R.MATS]) <= 1e-12 * np.abs(own[:R.MATS]))
    assert own[R.ABS_THR] == R.ABS_GATE and own[R.CEILING] == float(np.float32(0.9)) and not own[14:16].any() and not lib[14:16].any()
    for k in range(R.SCAN_STEPS + 1):
        a, b = lib[R.MATS + 16 * k:R.MATS + 16 * k + 16], own[R.MATS + 16 * k:R.MATS + 16 * k + 16]
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    # P_0 is the transition of G steps with x = 0: a state pushed through the recurrence lands where the matrix says
    c = tuple(own[R.SHELF:R.SHELF + 5]) + tuple(own[R.HIGH_PASS:R.HIGH_PASS + 5])
    s = np.array([[0.3, -0.2, 0.1, 0.05]])
    want = own[R.MATS:R.MATS + 16].reshape(4, 4) @ s[0]
    for _ in range(R.G):
        R._step(c, s, np.zeros(1))
    assert np.abs(s[0] - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("rate,tol", [(48000, 0.01), (22050, 0.1), (8000, 0.1)])
def test_full_scale_sine_reads_minus_3_01(rate, tol):
    y = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * rate) / rate).astype(np.float32)
    ref = R.reference_f64(y, rate)
    dev = R.device_f64(y, rate, R.design(rate))
    print(f"{rate} Hz: {ref['lufs']:.4f} LUFS")
    assert abs(ref["lufs"] + 3.01) <= tol
    assert ref["rel_mask"].all() and np.array_equal(dev["rel_mask"], ref["rel_mask"]) and abs(dev["ms"] / ref["ms"] - 1.0) <= 1e-12
    assert LoudnessNormalizer.loudness_lufs(np.array([[ref["ms"], 1.0], [0.0, 1.0]])).tolist() == [ref["lufs"], -np.inf]


# ---- the two restatements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_every_block_keeps_the_margin_at_both_gates(c):
    """In the plain float64 loop, over every block of every item, none left out."""
    worst, blocks = np.inf, 0
    for r in C.reference(c):
        z = r["z"]
        blocks += len(z)
        if len(z):
            worst = min(worst, float(np.abs(z / R.ABS_GATE - 1.0).min()))
        if r["abs_mask"].any():
            worst = min(worst, float(np.abs(z / r["rel_thr"] - 1.0).min()))
    print(f"{c['name']}: {blocks} blocks, least |z / threshold - 1| = {worst:.3e}")
    assert blocks > 0 and worst >= C.MARGIN


@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_device_structure_agrees_with_the_plain_loop(c):
    worst = 0.0
    for y, r, v in zip(c["items"], C.reference(c), C.device(c)):
        assert np.array_equal(v["abs_mask"], r["abs_mask"]) and np.array_equal(v["rel_mask"], r["rel_mask"])
        assert len(v["z"]) == len(r["z"]) == R.blocks_of(len(y), c["rate"] // 10)
        assert (v["ms"] == 0.0) == (r["ms"] == 0.0) and v["peak"] == r["peak"]
        if r["ms"] > 0.0:
            worst = max(worst, abs(v["ms"] / r["ms"] - 1.0))
            assert abs(v["gain"] / r["gain"] - 1.0) <= MS_BAR
        else:
            assert v["gain"] == r["gain"] == 1.0
    print(f"{c['name']}: largest relative difference in ms_b = {worst:.3e} (bar {MS_BAR:.2e})")
    assert worst <= MS_BAR


def test_every_property_the_cases_are_chosen_for_holds():
    by = {c["name"]: c for c in C.CASES}
    ref = {n: C.reference(c) for n, c in by.items()}
    assert {c["rate"] for c in C.CASES} == {8000, 22050} and {c["row_scale"] for c in C.CASES} >= {None, 1, 256}
    assert {len(c["items"]) for c in C.CASES} >= {1, 5, 257}
    step = 800
    lens = [len(y) for y in by["edge_lengths"]["items"]]
    assert lens[:5] == [0, 1, 4 * step - 1, 4 * step, 4 * step + 1] and lens[5] % R.G and lens[5] % step
    assert [len(r["z"]) for r in ref["edge_lengths"]][:5] == [0, 0, 0, 1, 1]
    assert [r["gain"] == 1.0 for r in ref["edge_lengths"]][:5] == [True, True, True, False, False]
    three = ref["three_seconds"][0]
    n = len(by["three_seconds"]["items"][0])
    assert 2.9 * 22050 < n < 3.1 * 22050 and n % R.G and n % 2205 and -(-n // (R.G * R.CHUNK_SEGS)) == 9
    assert 0 < three["rel_mask"].sum() < three["abs_mask"].sum() < len(three["z"])          # both gates remove blocks
    cl, d = ref["clamps"], C.design(by["clamps"])
    assert len(cl[0]["z"]) > 0 and not cl[0]["abs_mask"].any() and cl[0]["ms"] == 0.0 and cl[0]["gain"] == 1.0   # all under -70
    assert cl[1]["rel_mask"].sum() < cl[1]["abs_mask"].sum() == len(cl[1]["z"])              # the relative gate alone
    assert cl[2]["gain"] == d[R.CEILING] / cl[2]["peak"] < d[R.MAX_GAIN] and cl[2]["peak"] == np.float32(0.9)   # the ceiling binds
    assert cl[3]["gain"] == d[R.MAX_GAIN] < d[R.CEILING] / cl[3]["peak"]                     # the cap binds
    assert cl[4]["gain"] < min(d[R.MAX_GAIN], d[R.CEILING] / cl[4]["peak"]) and cl[4]["gain"] != 1.0              # neither does
    wide = [len(y) for y in by["batch_257"]["items"]]
    assert len(wide) == 257 and wide[256] > 4 * step and {0, 1, 3199, 3200, 3201} <= set(wide)
    assert {r["ms"] > 0.0 for r in ref["batch_257"]} == {True, False}
    assert any(c["L"] % 4 and len(c["items"]) > 1 for c in C.CASES)                         # rows off 16 bytes


# ---- the library's host-only answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=CASE_IDS)
def test_host_only_answers(c):
    a = LoudnessNormalizer(**C.params(c))
    B, L = len(c["items"]), c["L"]
    assert a.launch_count(B, L) == 4 and a.launch_count(B, L, measure_only=True) == 3
    assert a.launch_count(0, L) == 0 and a.launch_count(B, 0) == 0
    layout, words = a._workspace_layout(B, L)
    assert a.workspace_bytes(B, L) == max(256, 4 * words) and a.workspace_bytes(0, 0) == 256
    assert layout["ends"][1] == (B, 128 * -(-L // 8192), 4) and layout["hops"][1] == (B, L // (c["rate"] // 10) + 1)
    assert a.get_config() == C.params(c)
    assert np.allclose(a.design()[:R.MATS], C.design(c)[:R.MATS], rtol=1e-12, atol=0)


def _status(fn, cfg, *args):
    out = (ctypes.c_uint64 if fn.endswith("bytes") else ctypes.c_int32)()
    return getattr(_native.load(), fn)(ctypes.byref(cfg) if cfg is not None else None, *args, ctypes.byref(out))


def test_refusals_come_before_any_device_work():
    good = dict(sample_rate=22050, target_lufs=-23.0, max_gain_db=30.0, peak_ceiling=0.0)
    cfg = lambda **kw: _native.LoudnessConfig(**{**good, **kw})
    invalid = [dict(sample_rate=7990), dict(sample_rate=48010), dict(sample_rate=22055), dict(sample_rate=0), dict(sample_rate=-22050),
               dict(target_lufs=0.5), dict(target_lufs=-71.0), dict(target_lufs=float("nan")), dict(target_lufs=float("-inf")),
               dict(max_gain_db=-1.0), dict(max_gain_db=121.0), dict(max_gain_db=float("nan")), dict(peak_ceiling=-0.1),
               dict(peak_ceiling=1.5), dict(peak_ceiling=float("nan"))]
    queries = (("iris_loudness_workspace_bytes", ()), ("iris_loudness_launch_count", (0,)), ("iris_loudness_launch_count", (1,)))
    for fn, extra in queries:
        assert _status(fn, cfg(), 2, 100, *extra) == 0
        for ok in (dict(sample_rate=8000), dict(sample_rate=48000), dict(target_lufs=0.0), dict(target_lufs=-70.0), dict(peak_ceiling=1.0)):
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
    lib = _native.load()
    table = (ctypes.c_double * R.DESIGN)()
    assert lib.iris_loudness_design(ctypes.byref(cfg()), table, R.DESIGN) == 0
    assert lib.iris_loudness_design(ctypes.byref(cfg()), table, R.DESIGN - 1) == INVALID
    assert lib.iris_loudness_design(ctypes.byref(cfg()), None, R.DESIGN) == INVALID
    assert lib.iris_loudness_design(ctypes.byref(cfg(sample_rate=22051)), table, R.DESIGN) == INVALID
    assert lib.iris_loudness_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.iris_loudness_create(ctypes.byref(cfg()), None) == INVALID
    assert lib.iris_loudness_create(ctypes.byref(cfg(sample_rate=22051)), ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.iris_loudness_normalize_ragged(None, None, 2, 100, None, 1, None, None, None, 0, None) == INVALID      # a NULL handle
    assert lib.iris_loudness_measure_ragged(None, None, 2, 100, None, 1, None, None, 0, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
    with pytest.raises(_native.NativeCallError, match="sample_rate"):
        LoudnessNormalizer(sample_rate=44101)
    with pytest.raises(ValueError, match="peak_ceiling"):
        LoudnessNormalizer(peak_ceiling=0.0)
    with pytest.raises(ValueError, match="sample_rate"):
        LoudnessNormalizer(sample_rate=22050.5)
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION


# ---- the pipeline and the command line -----------------------------------------------------------------------------------
class _Level:
    """Stands in for ``LoudnessNormalizer``: halves the waveform and notes what it was handed."""

    def __init__(self, log):
        self.log = log

    def normalize_device(self, wav, lengths=None, row_scale=1):
        self.log.append(("loudness", tuple(wav.shape), None if lengths is None else [int(v) for v in lengths], row_scale))
        return wav * 0.5, torch.zeros((wav.shape[0], 2), dtype=torch.float64)


class _Join:
    def __init__(self, log):
        self.log = log

    def join_device(self, wav, lengths=None, row_scale=1):
        self.log.append(("assemble", float(wav.abs().max()), None if lengths is None else [int(v) for v in lengths], row_scale))
        n = wav.numel()
        return wav.reshape(-1), torch.tensor([0] * wav.shape[0] + [n], dtype=torch.int32), torch.zeros((wav.shape[0], 2), dtype=torch.int32)


def _vocode(mel, lengths=None):
    return torch.ones((mel.shape[0], 4 * mel.shape[2]), dtype=torch.float32)


def test_pipeline_levels_in_front_of_the_join_and_hands_the_lengths_on():
    log = []
    mels = [np.zeros((80, 8), np.float32), np.zeros((80, 5), np.float32)]
    plain = MelToWavePipeline(None, _vocode, hop_length=4)
    assert plain.loudness is None and [tuple(w.shape) for w in plain.infer_batch(mels)] == [(32,), (20,)]
    pipe = MelToWavePipeline(None, _vocode, hop_length=4, loudness=_Level(log))
    out = pipe.infer_batch(mels)
    assert log == [("loudness", (2, 32), [8, 5], 4)]                      # the batch's frames and the hop
    assert [tuple(w.shape) for w in out] == [(32,), (20,)] and all(float(w.max()) == 0.5 for w in out)
    del log[:]
    joined, spans = MelToWavePipeline(None, _vocode, hop_length=4, loudness=_Level(log), assemble=_Join(log)).infer_batch(mels)
    assert [e[0] for e in log] == ["loudness", "assemble"] and log[1][1:] == (0.5, [8, 5], 4)     # levelled, then joined
    assert joined.shape == (64,)
    del log[:]
    one = pipe.infer(np.zeros((1, 80, 6), np.float32))
    assert log == [("loudness", (1, 24), None, 1)] and one.shape == (1, 24) and float(one.max()) == 0.5


def test_pipeline_refuses_to_stream_with_a_loudness_stage():
    pipe = MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256, loudness=_Level([]))
    mel = np.zeros((1, 80, 8), np.float32)
    with pytest.raises(ValueError, match="integrated loudness is the whole item's measure"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="integrated loudness is the whole item's measure"):
        pipe.session()


def test_command_line_takes_a_loudness_target(tmp_path):
    args = build_parser().parse_args(["--mel", "m.npy", "--lufs", "-16"])
    assert args.lufs == -16.0 and build_parser().parse_args(["--mel", "m.npy"]).lufs is None
    assert check_lufs(-23) == -23.0 and check_lufs(0) == 0.0
    for bad in (0.5, -70.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lufs"):
            check_lufs(bad)
    for bad in ("3", "-90", "nan"):
        with pytest.raises(SystemExit):
            main(["--mel", str(tmp_path / "absent.npy"), "--lufs", bad])
