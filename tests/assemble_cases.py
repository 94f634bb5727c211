"""Inputs of the assemble stage's tests: small ragged batches built from bursts of seeded noise at chosen levels over a floor.
A burst sample has magnitude in [level / 2, level], so a frame that holds even one of them is far from the threshold; the floor
lies far below it.  Each case names the property it is there for (``why``); tests/test_assemble.py asserts them.  ``CASES`` are
the small ones; ``WIDE_CASES`` reach the batch sizes, frame counts and configs at which the kernels' loops, scans and
reductions run more than once."""
import numpy as np

import assemble_restatement as R

CONFIGS = {"default": (2048, 512), "small": (64, 16), "two_block": (32, 16),      # (frame_length, hop_length)
           "hop1": (64, 1),              # R = 64 block sums a frame, more than an energy block's run of frames
           "odd_hop": (20, 5),           # R = 4, and no block behind the first starts on 16 bytes
           "max_frame": (8192, 4096)}    # the limit itself: 16 steps of a block's accumulate loop
FLOOR = 1e-5


def item(n, bursts, seed, floor=FLOOR):
    """``n`` samples of floor noise with ``bursts = [(lo, hi, level), ...]`` laid over it; ``floor=0`` gives digital zeros."""
    rng = np.random.default_rng(seed)
    y = (floor * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    for lo, hi, level in bursts:
        y[lo:hi] = (rng.choice([-1.0, 1.0], hi - lo) * rng.uniform(0.5, 1.0, hi - lo) * level).astype(np.float32)
    return y


def case(name, cfg, items, why, top_db=60.0, ref=None, pad=0, fade=0, pause=0, row_scale=None, L=None, expect=None):
    """``row_scale=None``: a dense batch (every item owns the whole row, ``lengths=None``); otherwise every item's length is a
    multiple of it.  ``L``: the row's width (the longest item by default).  ``expect``: spans worked out by hand, or None."""
    L = max(len(y) for y in items) if L is None else L
    if row_scale is None:
        assert all(len(y) == L for y in items)
    else:
        assert all(len(y) % row_scale == 0 and len(y) <= L for y in items)
    return dict(name=name, cfg=cfg, items=items, why=why, top_db=top_db, ref=ref, pad=pad, fade=fade, pause=pause,
                row_scale=row_scale, L=L, expect=expect)


RUN = R.KRUN_FRAMES * 16             # the first sample of an energy block's second run of frames at hop 16

CASES = [
    case("loud_throughout", "small", [item(1000, [(0, 1000, 0.5)], 1)], "nothing_trimmed", expect=[(0, 1000)]),
    case("edge_samples", "small", [item(700, [(0, 1, 0.9)], 2), item(333, [(332, 333, 0.9)], 3)], "only_first_and_only_last_sample",
         row_scale=1, L=701, expect=[(0, 48), (304, 333)]),
    case("silence_ref_max", "small", [item(200, [], 4, floor=0.0), item(300, [(100, 180, 0.3)], 5)], "digital_silence_keeps_all",
         row_scale=1, pause=7, expect=[(0, 200), None]),
    case("silence_ref_abs", "small", [item(200, [], 6, floor=0.0), item(300, [(100, 180, 0.3)], 7), item(240, [(60, 90, 3e-5)], 8)],
         "digital_silence_is_empty_under_an_absolute_ref", ref=0.1, row_scale=1, pause=11, expect=[(0, 0), None, (0, 0)]),
    case("empty_in_the_middle", "small", [item(400, [(120, 250, 0.5)], 9), item(0, [], 10), item(7, [(0, 7, 0.4)], 11),
                                           item(0, [], 12), item(523, [(300, 410, 0.2), (40, 60, 0.004)], 13)],
         "zero_length_and_one_frame_items", row_scale=1, L=525, fade=8, pause=50, expect=[None, (0, 0), (0, 7), (0, 0), None]),
    case("run_edges", "small", [item(1600, [(RUN - 12, RUN + 18, 0.5)], 14), item(1120, [(RUN, RUN + 88, 0.5)], 15),
                                item(1600, [(RUN - 112, RUN, 0.5), (1400, 1420, 2e-4)], 16)],
         "bursts_across_and_at_a_run_edge", row_scale=16, pause=3, fade=5),
    case("two_block_frames", "two_block", [item(777, [(500, 530, 0.5)], 17), item(650, [(RUN - 40, RUN, 0.25), (30, 40, 0.01)], 18),
                                           item(41, [(20, 30, 0.5)], 19)],
         "two_blocks_per_frame", row_scale=1, L=779, pad=5, pause=20),
    case("pad_clips_both_ends", "small", [item(300, [(40, 260, 0.5)], 20), item(300, [(140, 150, 0.5)], 21)], "pad_clips",
         pad=100, fade=16, expect=[(0, 300), None]),
    case("fade_longer_than_items", "small", [item(320, [(150, 170, 0.5)], 22), item(160, [(0, 160, 0.5)], 23)], "fade_exceeds_len",
         row_scale=16, fade=200, pause=9),
    case("default_ragged", "default", [item(5000, [(1500, 3200, 0.5), (4100, 4150, 0.002)], 24), item(3777, [(0, 900, 0.3)], 25),
                                       item(2600, [(2000, 2600, 0.4)], 26)],
         "default_config_ragged", top_db=40.0, row_scale=1, L=5001, fade=64, pause=300),
    case("default_dense", "default", [item(4096, [(1024, 2500, 0.5)], 27), item(4096, [(3000, 3300, 0.05)], 28)],
         "default_config_aligned_rows", fade=32, pause=128),
]


# ---- the widths the ABI admits: B up to 4096, more than 256 frames, R above a run, hops that are odd, 1 and 4096 ---------
WIDE_BATCHES = (64, 65, 256, 257, 1000, 4096)
# per batch size: the forced runs of empty items [lo, hi), then single items forced empty and forced non-empty
BATCH_LAYOUT = {
    64: dict(runs=[(24, 64)], empty=[], full=[0, 23]),                             # all of wave 0's lanes own an item; 63 empty
    65: dict(runs=[(0, 40)], empty=[], full=[63, 64]),                             # item 64 is wave 1's first
    256: dict(runs=[(0, 40), (100, 150), (216, 256)], empty=[], full=[63, 64, 65, 215]),
    257: dict(runs=[(0, 40), (50, 140), (217, 257)], empty=[], full=[49, 140, 216]),       # per = 2: item 128 is wave 1's first
    1000: dict(runs=[(0, 40), (490, 540), (960, 1000)], empty=[63, 64, 65], full=[255, 256, 257, 959]),   # per = 4
    4096: dict(runs=[(0, 40), (1000, 1060), (4056, 4096)], empty=[255, 256], full=[63, 64, 65, 999, 1060, 4055]),   # per = 16
}


def batch_items(B, seed):
    """``B`` items of 0, 16, 32 or 48 samples, a non-empty one holding one burst of at least four samples at a level of at least
    0.3; ``BATCH_LAYOUT[B]`` forces the long runs of empty items and the items at the scan's thread and wave edges."""
    rng = np.random.default_rng(seed)
    lay = BATCH_LAYOUT[B]
    lens = 16 * rng.integers(0, 4, B)
    lens[lay["full"]] = 16 * rng.integers(1, 4, len(lay["full"]))
    lens[lay["empty"]] = 0
    for lo, hi in lay["runs"]:
        lens[lo:hi] = 0
    items = []
    for b, n in enumerate(int(v) for v in lens):
        bursts = []
        if n:
            lo = int(rng.integers(0, n - 3))
            bursts = [(lo, int(rng.integers(lo + 4, n + 1)), float(rng.uniform(0.3, 0.9)))]
        items.append(item(n, bursts, 1000 * B + b))
    return items


def empty_runs(lens):
    """``[(lo, hi), ...]``: the maximal runs of zero-length items."""
    runs, lo = [], None
    for b, n in enumerate(list(lens) + [1]):
        if n == 0 and lo is None:
            lo = b
        if n and lo is not None:
            runs.append((lo, b))
            lo = None
    return runs


def _seam_item(i, k):
    """A burst over samples [16 a, 16 c): frames a - 1 .. c + 1 are non-silent, so with pad 5 the item keeps 16 k + 10 samples."""
    a = 4 + i
    c = a + k - 3
    return item(16 * (c + 2) + 5 + 37 + i, [(16 * a, 16 * c, 0.5)], 300 + i)


SEAM_BLOCKS = (248, 260, 246, 250, 60)       # kept lengths 16 k + 10: 3978, 4170, 3946, 4010, 970 (with pause 70, fade 64)

WIDE_CASES = [case(f"batch_{B}", "two_block", batch_items(B, 40 + B), "offset_scan_and_item_search_at_this_batch", pause=2, fade=4,
                   row_scale=16, L=48) for B in WIDE_BATCHES] + [
    case("many_frames", "small",
         [item(4085, [(900, 1100, 0.5)], 201),                                      # T = 256; frames 55 .. 70, across waves 0 | 1
          item(4100, [(3216, 4100, 0.4)], 202),                                     # T = 257; (d) first t = 200, last t = 256
          item(8200, [(1600, 1900, 0.6)], 203),                                     # T = 513; (b) last t < 256
          item(9599, [(8800, 8900, 0.9), (1000, 1040, 2e-4)], 204)],                # T = 600; (a), (c) loudest t >= 512 drops the burst at 1000
         "more_than_256_frames_per_item", row_scale=1, L=9601, pad=7, fade=10, pause=9),
    case("hop1_long_frame", "hop1", [item(301, [(100, 180, 0.5)], 205), item(77, [(30, 50, 0.4)], 206)],
         "R_above_a_run_of_frames", row_scale=1, L=301, pad=3, fade=8, pause=5),
    case("odd_hop_unaligned", "odd_hop", [item(403, [(150, 260, 0.5), (390, 403, 0.3)], 207), item(199, [(0, 33, 0.4)], 208),
                                          item(4, [(0, 4, 0.5)], 209)],
         "blocks_off_16_bytes", row_scale=1, L=403, pad=2, fade=6, pause=3),
    case("max_frame_blocks", "max_frame", [item(3 * 4096 + 5, [(6500, 8000, 0.5)], 210), item(4095, [(3000, 4095, 0.4)], 211)],
         "sixteen_accumulate_steps_and_a_partial_last_block", top_db=40.0, row_scale=1, L=3 * 4096 + 5, fade=16, pause=10),
    case("gather_seams", "small", [_seam_item(i, k) for i, k in enumerate(SEAM_BLOCKS)],
         "gather_block_edges_inside_ramps_a_pause_and_on_an_item_start", row_scale=1, pad=5, fade=64, pause=70),
]
for _c in CASES + WIDE_CASES:
    for _y in _c["items"]:
        _y.setflags(write=False)


def case_id(c):
    return c["name"]


def params(c):
    F, H = CONFIGS[c["cfg"]]
    return dict(frame_length=F, hop_length=H, top_db=c["top_db"], ref=c["ref"], pad=c["pad"], fade=c["fade"], pause=c["pause"])


def batch(c, fill=0.0):
    """``(wav [B, L] fp32, lengths or None, row_scale)``: the items in their rows, the rest of each row ``fill`` (NaN for the
    poison tests: nothing past an item's own samples is read)."""
    wav = np.full((len(c["items"]), c["L"]), fill, dtype=np.float32)
    for b, y in enumerate(c["items"]):
        wav[b, :len(y)] = y
    if c["row_scale"] is None:
        return wav, None, 1
    return wav, np.array([len(y) // c["row_scale"] for y in c["items"]], dtype=np.int32), c["row_scale"]


_ref_cache = {}


def reference(c):
    """Computed once per case and shared: float64 spans, fp32 mse per item, fp32 spans, and the fp32 join to ``cap``."""
    if c["name"] not in _ref_cache:
        F, H = CONFIGS[c["cfg"]]
        B, L = len(c["items"]), c["L"]
        spans64 = R.spans_f64(c["items"], F, H, c["top_db"], c["ref"], c["pad"])
        cap = B * L + c["pause"] * (B - 1)
        out, offs = R.join_f32(c["items"], spans64, c["fade"], c["pause"], cap)
        mse32 = [R.mse_f32(y, F, H) for y in c["items"]]
        spans32 = [R.span_from(R.nonsilent_f32(m, c["top_db"], c["ref"]), len(y), H, c["pad"]) for y, m in zip(c["items"], mse32)]
        _ref_cache[c["name"]] = dict(spans=spans64, spans32=spans32, mse32=mse32, out=out, offsets=offs, cap=cap)
    return _ref_cache[c["name"]]


_dev_cache = {}


def device_model(c, mutation=None):
    """``R.device_f32`` on the case: the three launches as the device runs them, with one deviation (``R.MUTATIONS``) or none."""
    key = (c["name"], mutation)
    if key not in _dev_cache:
        F, H = CONFIGS[c["cfg"]]
        clean = None if mutation is None else device_model(c)
        _dev_cache[key] = R.device_f32(c["items"], batch(c)[0], F, H, c["top_db"], c["ref"], c["pad"], c["fade"], c["pause"],
                                       reference(c)["cap"], mutation=mutation, clean=clean)
    return _dev_cache[key]
