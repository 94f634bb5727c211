"""The assemble stage without a GPU: the float64 restatement in librosa's log form against the product form the device uses, the
margin that makes the device's integer bounds exact, the cases' reasons for being there, the fp32 restatement's bounds, the
join's offsets against a loop, the library's host-only answers and every refusal that needs no handle (an overlapping output
and a short workspace are refused behind the handle check, so tests/test_gpu_assemble.py holds those two)."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.assemble import Assembler
from iris.pipeline import MelToWavePipeline
from iris.synthesis_output import build_parser, check_trim_db, main

import assemble_cases as C
import assemble_restatement as R

CASE_IDS = [C.case_id(c) for c in C.CASES]
ALL_CASES = C.CASES + C.WIDE_CASES
ALL_IDS = [C.case_id(c) for c in ALL_CASES]
INVALID, UNSUPPORTED = 1, 4


def frames(c):
    F, H = C.CONFIGS[c["cfg"]]
    return [(y, R.mse_f64(y, F, H)) for y in c["items"]]


# ---- the decision ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_log_form_and_product_form_agree_and_every_frame_keeps_the_margin(c):
    """A sum of F non-negative fp32 terms is within F * 2^-24 of exact, relatively: 1.2e-4 at F = 2048.  Every frame of every
    case stays eight times that away from the threshold, so the fp32 decision cannot differ; no frame is left out.  Eight
    times is 9.8e-4 at F = 2048, which the bar 1e-3 covers; at F = 8192 (``max_frame``) it is 3.9e-3 and the bar follows it."""
    bar = max(1e-3, 8 * C.CONFIGS[c["cfg"]][0] * 2.0 ** -24)
    assert bar == 1e-3 or c["cfg"] == "max_frame"
    worst = np.inf
    for y, mse in frames(c):
        ratio = R.ratio_f64(mse, c["top_db"], c["ref"])
        assert np.array_equal(ratio > 1.0, R.nonsilent_log_f64(mse, c["top_db"], c["ref"]))
        worst = min(worst, float(np.abs(ratio - 1.0).min()))
    print(f"{c['name']}: least |ratio - 1| = {worst:.3e} (bar {bar:.2e})")
    assert worst >= bar


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_fp32_restatement_bounds_equal_the_float64_ones(c):
    ref = C.reference(c)
    assert ref["spans32"] == ref["spans"]
    F, H = C.CONFIGS[c["cfg"]]
    for y, m32 in zip(c["items"], ref["mse32"]):
        m64 = R.mse_f64(y, F, H)
        assert m32.dtype == np.float32 and m32.shape == m64.shape
        assert np.all(np.abs(m32 - m64) <= F * 2.0 ** -24 * m64 + 1e-45)


# ---- the cases are what they claim to be ---------------------------------------------------------------------------------
def test_every_property_the_cases_are_chosen_for_holds():
    by = {c["name"]: c for c in C.CASES}
    ref = {n: C.reference(c) for n, c in by.items()}
    assert {c["cfg"] for c in C.CASES} == {"default", "small", "two_block"}
    assert {c["cfg"] for c in C.CASES + C.WIDE_CASES} == set(C.CONFIGS) == {"default", "small", "two_block", "hop1", "odd_hop", "max_frame"}
    assert C.CONFIGS["two_block"][0] // C.CONFIGS["two_block"][1] == 2
    assert {len(c["items"]) for c in C.CASES} >= {1, 2, 3, 5} and max(len(y) for c in C.CASES for y in c["items"]) <= 5000
    for n, c in by.items():
        if c["expect"]:
            for want, got in zip(c["expect"], ref[n]["spans"]):
                assert want is None or want == got, (n, want, got)
    assert ref["loud_throughout"]["spans"] == [(0, 1000)]                                       # nothing trimmed
    first, last = by["edge_samples"]["items"]
    assert np.argmax(np.abs(first)) == 0 and np.abs(first[1:]).max() <= C.FLOOR                  # only sample 0 is loud
    assert np.argmax(np.abs(last)) == len(last) - 1 and np.abs(last[:-1]).max() <= C.FLOOR       # only the last one
    for n in ("silence_ref_max", "silence_ref_abs"):
        assert not by[n]["items"][0].any() and len(by[n]["items"][0]) > 0                        # digital silence
    assert by["silence_ref_max"]["ref"] is None and ref["silence_ref_max"]["spans"][0] == (0, 200)       # keeps every frame
    assert by["silence_ref_abs"]["ref"] > 0 and ref["silence_ref_abs"]["spans"][0] == (0, 0)
    mid = by["empty_in_the_middle"]
    lens = [len(y) for y in mid["items"]]
    assert lens[1] == 0 and lens[0] > 0 and lens[-1] > 0 and mid["pause"] > 0                   # L_b == 0 between two items
    assert 0 < lens[2] < C.CONFIGS["small"][1] and R.frames_of(lens[2], 16) == 1                # one frame
    offs = ref["empty_in_the_middle"]["offsets"]
    kept = [e - s for s, e in ref["empty_in_the_middle"]["spans"]]
    assert offs[2] == kept[0] + mid["pause"] and offs[4] == kept[0] + kept[2] + 2 * mid["pause"]    # an empty item adds no pause
    assert any(len(y) % C.CONFIGS[c["cfg"]][1] for c in C.CASES for y in c["items"])          # L_b no multiple of H
    edge = C.RUN
    s0, s1, s2 = ref["run_edges"]["spans"]
    assert s0[0] < edge < s0[1] and s1[0] <= edge < s1[1] and s2[0] < s2[1]                     # across the edge, from the edge
    assert by["run_edges"]["items"][2][edge - 1] != 0 and np.abs(by["run_edges"]["items"][2][edge:1400]).max() <= C.FLOOR
    assert all(R.frames_of(len(y), 16) > R.KRUN_FRAMES for y in by["run_edges"]["items"])      # more than one run of frames
    assert {c["row_scale"] for c in C.CASES} >= {None, 1, 16}
    clip = by["pad_clips_both_ends"]
    raw = R.spans_f64(clip["items"], 64, 16, clip["top_db"], clip["ref"], 0)
    assert raw[0][0] < clip["pad"] and raw[0][1] + clip["pad"] > 300 and ref["pad_clips_both_ends"]["spans"][0] == (0, 300)
    fades = {(c["fade"] == 0, any(0 < 2 * c["fade"] < e - s for s, e in ref[n]["spans"]), any(c["fade"] > e - s > 0 for s, e in ref[n]["spans"]))
             for n, c in by.items()}
    assert any(f[0] for f in fades) and any(f[1] for f in fades) and any(f[2] for f in fades)
    assert {c["pause"] > 0 for c in C.CASES} == {True, False}
    assert any(c["L"] % 4 and len(c["items"]) > 1 for c in C.CASES) and any(c["L"] % 4 == 0 and len(c["items"]) > 1 for c in C.CASES)


def nonsilent_frames(c, b):
    """Indices of item b's non-silent frames, in float64."""
    F, H = C.CONFIGS[c["cfg"]]
    return np.flatnonzero(R.nonsilent_log_f64(R.mse_f64(c["items"][b], F, H), c["top_db"], c["ref"]))


def test_every_property_the_wide_cases_are_chosen_for_holds():
    by = {c["name"]: c for c in C.WIDE_CASES}
    ref = {n: C.reference(c) for n, c in by.items()}
    assert len(by) == len(C.WIDE_CASES) and not set(by) & {c["name"] for c in C.CASES}
    assert {len(c["items"]) for c in C.WIDE_CASES} >= {64, 65, 256, 257, 1000, 4096}
    # the batches: 0 / 16 / 32 / 48 samples, one burst each, long runs of empty items where the scan's ranges meet
    state = {63: set(), 64: set(), 65: set(), 255: set(), 256: set()}
    for B in C.WIDE_BATCHES:
        c = by[f"batch_{B}"]
        lens = [len(y) for y in c["items"]]
        assert len(lens) == B and set(lens) == {0, 16, 32, 48} and (c["cfg"], c["row_scale"], c["L"], c["pause"], c["fade"]) == ("two_block", 16, 48, 2, 4)
        kept = [e - s for s, e in ref[c["name"]]["spans"]]
        assert all((k > 0) == (n > 0) for k, n in zip(kept, lens))                              # an item is empty iff it has no sample
        long_runs = [(lo, hi) for lo, hi in C.empty_runs(lens) if hi - lo >= 40]
        assert long_runs, B
        if B >= 256:
            assert long_runs[0][0] == 0 and long_runs[-1][1] == B and len(long_runs) >= 3       # at the start, at the end, in the middle
        per = (B + 255) // 256
        if per > 1:                                                                             # a middle run across a wave's first item
            assert any(lo < 64 * per * w < hi - 1 for lo, hi in long_runs[1:-1] for w in (1, 2, 3)), B
        for i, seen in state.items():
            if i < B:
                seen.add(lens[i] > 0)
    assert all(seen == {True, False} for seen in state.values()), state                       # each both empty and not, by batch
    for trio in ((63, 64, 65), (255, 256)):                                                     # and all of them at once, either way
        together = {tuple(len(by[f"batch_{B}"]["items"][i]) > 0 for i in trio) for B in C.WIDE_BATCHES if B > trio[-1]}
        assert together >= {(True,) * len(trio), (False,) * len(trio)}
    lens = [len(y) for y in by["batch_4096"]["items"]]
    mid = [(lo, hi) for lo, hi in C.empty_runs(lens) if hi - lo >= 40][1]
    assert mid[0] < 1008 and mid[1] > 1024 + 16                  # thread 63's items 1008 .. 1023 whole, and on over item 1024 (wave 1's first)
    assert ref["batch_4096"]["cap"] == 204798 and ref["batch_64"]["offsets"][-1] > 0 and lens[0] == 0 and lens[-1] == 0
    assert len(by["batch_64"]["items"][63]) == 0 and len(by["batch_65"]["items"][64]) > 0      # lane 63 empty; wave 1's only item
    # many_frames
    c = by["many_frames"]
    H = C.CONFIGS["small"][1]
    assert c["cfg"] == "small" and c["row_scale"] == 1 and c["L"] % 2 == 1 and c["ref"] is None
    assert [R.frames_of(len(y), H) for y in c["items"]] == [256, 257, 513, 600]
    loud = [nonsilent_frames(c, b) for b in range(4)]
    assert any(f[0] >= 256 for f in loud)                                                                       # (a)
    assert any(f[-1] < 256 and R.frames_of(len(y), H) > 512 for f, y in zip(loud, c["items"]))                 # (b)
    y = c["items"][3]
    mse = R.mse_f64(y, 64, H)
    assert np.argmax(mse) >= 512                                                                                # (c)
    early = R.nonsilent_log_f64(mse[:512], c["top_db"], None)                  # the same frames under their own maximum
    assert early.any() and not R.nonsilent_log_f64(mse, c["top_db"], None)[:512].any()       # kept there, dropped by the loud frame
    assert any(f[0] % 256 >= 192 and f[-1] % 256 < 64 and f[-1] > f[0] for f in loud)                          # (d)
    assert any(f[0] % 256 < 64 <= f[-1] % 256 for f in loud)                                                    # and a burst over waves 0 | 1
    # the configs
    F, H = C.CONFIGS["hop1"]
    assert F // H > R.KRUN_FRAMES and by["hop1_long_frame"]["cfg"] == "hop1"
    assert [len(y) for y in by["hop1_long_frame"]["items"]] == [301, 77] and by["hop1_long_frame"]["L"] == 301
    F, H = C.CONFIGS["odd_hop"]
    assert H % 4 != 0 and F // H == 4 and by["odd_hop_unaligned"]["cfg"] == "odd_hop"
    assert [len(y) for y in by["odd_hop_unaligned"]["items"]] == [403, 199, 4] and R.frames_of(4, H) == 1 and 4 < H
    F, H = C.CONFIGS["max_frame"]
    c = by["max_frame_blocks"]
    status = ctypes.c_int64()
    cfg = lambda f: _native.AssembleConfig(frame_length=f, hop_length=f // 2, top_db=40.0, ref=0.0, pad_samples=0, fade_samples=0, pause_samples=0)
    assert _native.load().iris_assemble_out_capacity(ctypes.byref(cfg(F)), 2, 100, ctypes.byref(status)) == 0
    assert _native.load().iris_assemble_out_capacity(ctypes.byref(cfg(F + 2)), 2, 100, ctypes.byref(status)) == UNSUPPORTED   # F is the limit
    assert c["cfg"] == "max_frame" and F // H == 2 and -(-H // 256) == 16 and c["top_db"] == 40.0
    assert [len(y) for y in c["items"]] == [3 * 4096 + 5, 4095] and R.frames_of(4095, H) == 1 and 4095 % 4 == 3
    # gather_seams: a multiple of the gather block inside an up-ramp, a down-ramp and a pause, on an item's first position, in the tail
    c, r = by["gather_seams"], ref["gather_seams"]
    fade, pause, offs = c["fade"], c["pause"], r["offsets"]
    kept = [e - s for s, e in r["spans"]]
    assert c["cfg"] == "small" and fade >= 64 and pause >= 64 and all(k > 2 * fade for k in kept)
    seams = range(R.KGATHER_RUN, r["cap"], R.KGATHER_RUN)
    assert any(0 < m - o < fade - 1 for m in seams for o in offs[:-1])                                          # strictly inside an up-ramp
    assert any(0 < o + k - 1 - m < fade - 1 for m in seams for o, k in zip(offs, kept))                         # strictly inside a down-ramp
    assert any(o + k < m < o + k + pause - 1 for m in seams for o, k in zip(offs[:-2], kept))                   # strictly inside a pause
    assert any(m == o for m in seams for o in offs[1:-1])                                                       # an item's first position
    assert any(offs[-1] < m < r["cap"] for m in seams)                                                          # between total and cap


# ---- the wide cases bite where the eleven cannot -------------------------------------------------------------------------
def differs(c, mutation):
    """Which of the device's results the deviation changes on the case: a subset of spans, offsets, mse32, out."""
    clean, wrong = C.device_model(c), C.device_model(c, mutation)
    what = []
    if wrong["spans"] != clean["spans"]:
        what.append("spans")
    if wrong["offsets"] != clean["offsets"]:
        what.append("offsets")
    if any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(wrong["mse32"], clean["mse32"])):
        what.append("mse32")
    if not np.array_equal(wrong["out"].view(np.uint32), clean["out"].view(np.uint32)):
        what.append("out")
    return what


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_device_model_without_a_deviation_is_the_restatement(c):
    """``R.device_f32`` walks the launches as the kernels do (threads' item ranges, wave sums, the binary search, groups of four);
    with no deviation it must give what the plain restatement gives, or the mutation table below would mean nothing."""
    ref, dev = C.reference(c), C.device_model(c)
    assert dev["spans"] == ref["spans32"] == ref["spans"] and dev["offsets"] == ref["offsets"]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(dev["mse32"], ref["mse32"]))
    assert np.array_equal(dev["out"].view(np.uint32), ref["out"].view(np.uint32))


# deviations that by construction need B > 5, T_b > 256, R > 32 or H > 2048: no case of the first list can see them
NEEDS_WIDTH = ("scan_drops_wave_sums", "scan_per_rounds_down", "total_from_last_owner", "bounds_first_256", "ref_max_first_256",
               "first_last_wave0", "frame_sum_one_run", "accumulate_8_passes")


def test_every_deviation_is_caught_by_a_wide_case_and_the_width_ones_by_no_old_case():
    table = {m: {c["name"]: differs(c, m) for c in C.WIDE_CASES} for m in R.MUTATIONS}
    for m, row in table.items():
        print(f"{m}: " + (", ".join(f"{n} ({'/'.join(w)})" for n, w in row.items() if w) or "NOT CAUGHT"))
    assert len(R.MUTATIONS) == 11 and set(R.STAGE_OF) == set(R.MUTATIONS) and set(NEEDS_WIDTH) <= set(R.MUTATIONS)
    for m, row in table.items():
        assert any(row.values()), f"no wide case sees {m}"
    for c in C.WIDE_CASES:
        assert any(table[m][c["name"]] for m in R.MUTATIONS), f"{c['name']} catches no deviation"
    # each case catches the deviation in the path it is there for
    for B in (65, 256, 257, 1000, 4096):
        assert table["scan_drops_wave_sums"][f"batch_{B}"] and table["total_from_last_owner"][f"batch_{B}"]
    assert table["scan_per_rounds_down"]["batch_257"] and table["scan_per_rounds_down"]["batch_1000"]
    for m in ("bounds_first_256", "ref_max_first_256", "first_last_wave0"):
        assert "spans" in table[m]["many_frames"]
    assert "mse32" in table["frame_sum_one_run"]["hop1_long_frame"] and "spans" in table["frame_sum_one_run"]["hop1_long_frame"]
    assert "mse32" in table["accumulate_8_passes"]["max_frame_blocks"] and "spans" in table["accumulate_8_passes"]["max_frame_blocks"]
    assert table["ramp_block_local"]["gather_seams"] == ["out"]
    # the record that the gap existed: the eleven cases give the same bits under every one of these
    for m in NEEDS_WIDTH:
        for c in C.CASES:
            assert differs(c, m) == [], (m, c["name"])


# ---- the join ------------------------------------------------------------------------------------------------------------
def test_join_offsets_against_a_loop_over_items():
    rng = np.random.default_rng(5)
    for pause in (0, 1, 37):
        for _ in range(50):
            lens = [int(v) for v in rng.integers(0, 4, rng.integers(1, 9)) * rng.integers(0, 50)]
            timeline, starts = [], []
            for n in lens:                                   # brute force: write the items and pauses onto a timeline
                if n and timeline:
                    timeline += [-1] * pause
                starts.append(len(timeline))
                timeline += [len(starts)] * n
            offs = R.join_offsets(lens, pause)
            assert offs[-1] == len(timeline)
            for b, n in enumerate(lens):
                if n:
                    assert offs[b] == starts[b] and timeline[offs[b]:offs[b] + n] == [b + 1] * n


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_joined_reference_holds_each_item_once(c):
    ref = C.reference(c)
    out, offs, spans = ref["out"], ref["offsets"], ref["spans"]
    assert len(out) == ref["cap"] and offs[-1] <= ref["cap"] and not out[offs[-1]:].any()
    for y, (s, e), o in zip(c["items"], spans, offs):
        if c["fade"] == 0:
            assert np.array_equal(out[o:o + e - s], y[s:e])
        elif e - s > 2 * c["fade"]:
            assert np.array_equal(out[o + c["fade"]:o + e - s - c["fade"]], y[s + c["fade"]:e - c["fade"]])
            assert abs(out[o]) < abs(y[s]) or y[s] == 0


# ---- the library's host-only answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_host_only_answers(c):
    a = Assembler(**C.params(c))
    B, L = len(c["items"]), c["L"]
    H = a.hop_length
    assert a.capacity(B, L) == B * L + c["pause"] * (B - 1) == C.reference(c)["cap"]
    assert a.launch_count(B, L) == 3 and a.launch_count(0, L) == 0 and a.launch_count(B, 0) == 0
    up = lambda n: (n + 63) // 64 * 64
    assert a.workspace_bytes(B, L) == max(256, 4 * (up(B * (L // H + 1)) + up(2 * B))) == max(256, 4 * a._workspace_layout(B, L)[1])
    assert a.capacity(0, L) == 0 and a.capacity(1, L) == L


def _status(fn, cfg, *args):
    out = (ctypes.c_uint64 if fn.endswith("bytes") else ctypes.c_int64 if fn.endswith("capacity") else ctypes.c_int32)()
    return getattr(_native.load(), fn)(ctypes.byref(cfg) if cfg is not None else None, *args, ctypes.byref(out))


QUERIES = ("iris_assemble_out_capacity", "iris_assemble_workspace_bytes", "iris_assemble_launch_count")


def test_refusals_come_before_any_device_work():
    good = dict(frame_length=64, hop_length=16, top_db=60.0, ref=0.0, pad_samples=0, fade_samples=0, pause_samples=0)
    cfg = lambda **kw: _native.AssembleConfig(**{**good, **kw})
    invalid = [dict(frame_length=63), dict(frame_length=0), dict(hop_length=0), dict(hop_length=24), dict(hop_length=64), dict(top_db=0.0),
               dict(top_db=-3.0), dict(top_db=float("inf")), dict(top_db=float("nan")), dict(ref=-0.5), dict(pad_samples=-1),
               dict(fade_samples=-1), dict(pause_samples=-1)]
    unsupported = [dict(frame_length=8194, hop_length=1), dict(frame_length=16384, hop_length=512), dict(fade_samples=65537)]
    for fn in QUERIES:
        assert _status(fn, cfg(), 2, 100) == 0
        assert _status(fn, cfg(frame_length=8192, hop_length=512, fade_samples=65536), 4096, 100) == 0       # the limits themselves
        for kw in invalid:
            assert _status(fn, cfg(**kw), 2, 100) == INVALID, (fn, kw)
        for kw in unsupported:
            assert _status(fn, cfg(**kw), 2, 100) == UNSUPPORTED, (fn, kw)
        assert _status(fn, None, 2, 100) == INVALID                                                  # a NULL config
        assert getattr(_native.load(), fn)(ctypes.byref(cfg()), 2, 100, None) == INVALID             # a NULL result
        assert _status(fn, cfg(), -1, 100) == INVALID and _status(fn, cfg(), 2, -1) == INVALID
        assert _status(fn, cfg(), 4097, 100) == UNSUPPORTED                                          # offsets staged in LDS
        assert _status(fn, cfg(), 4096, 1 << 19) == UNSUPPORTED                                      # B L = 2^31
        assert _status(fn, cfg(), 2, (1 << 30) - 1) == 0
        assert _status(fn, cfg(pause_samples=2), 2, (1 << 30) - 1) == UNSUPPORTED                    # cap = 2^31
        assert _status(fn, cfg(), 0, 100) == 0 and _status(fn, cfg(), 2, 0) == 0                     # nothing to do
    lib = _native.load()
    assert lib.iris_assemble_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.iris_assemble_create(ctypes.byref(cfg()), None) == INVALID
    assert lib.iris_assemble_create(ctypes.byref(cfg(frame_length=63)), ctypes.byref(ctypes.c_void_p())) == INVALID
    for fn in (lib.iris_assemble_forward, lib.iris_assemble_trim_ragged):                            # a NULL handle
        assert fn(None, None, 2, 100, None, 1, None, None, None, None, 0, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
    with pytest.raises(_native.NativeCallError, match="frame_length"):
        Assembler(frame_length=2047)
    with pytest.raises(ValueError, match="ref"):
        Assembler(ref=0.0)
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION


# ---- the pipeline and the command line -----------------------------------------------------------------------------------
def test_pipeline_refuses_to_stream_with_an_assembler():
    pipe = MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256, assemble=Assembler(pause=100))
    assert pipe.assemble is not None and MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256).assemble is None
    mel = np.zeros((1, 80, 8), np.float32)
    with pytest.raises(ValueError, match="reference level is the whole item's maximum"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="reference level is the whole item's maximum"):
        pipe.session()


def test_command_line_takes_a_trim_threshold(tmp_path):
    args = build_parser().parse_args(["--mel", "m.npy", "--trim_db", "45"])
    assert args.trim_db == 45.0 and build_parser().parse_args(["--mel", "m.npy"]).trim_db is None
    assert check_trim_db(60) == 60.0
    for bad in (0.0, -10.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="trim_db"):
            check_trim_db(bad)
    for bad in ("0", "-5", "nan"):
        with pytest.raises(SystemExit):
            main(["--mel", str(tmp_path / "absent.npy"), "--trim_db", bad])
