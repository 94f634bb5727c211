"""Inputs of the assemble stage's tests: small ragged batches built from bursts of seeded noise at chosen levels over a floor.
A burst sample has magnitude in [level / 2, level], so a frame that holds even one of them is far from the threshold; the floor
lies far below it.  Each case names the property it is there for (``why``); tests/test_assemble.py asserts them."""
import numpy as np

import assemble_restatement as R

CONFIGS = {"default": (2048, 512), "small": (64, 16), "two_block": (32, 16)}      # (frame_length, hop_length)
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
for _c in CASES:
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
        _ref_cache[c["name"]] = dict(spans=spans64, spans32=R.spans_f32(c["items"], F, H, c["top_db"], c["ref"], c["pad"]),
                                     mse32=[R.mse_f32(y, F, H) for y in c["items"]], out=out, offsets=offs, cap=cap)
    return _ref_cache[c["name"]]
