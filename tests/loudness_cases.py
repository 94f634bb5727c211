"""Inputs of the loudness stage's tests: ragged batches of seeded uniform noise laid out in stretches at about -20, -45 and -80
dBFS (rms), at 8000 and 22050 Hz.  -80 dBFS lies under the absolute gate (-70 LUFS), -45 above it and, beside a -20 stretch,
under the relative one (-10 LU).  Each case names what it is there for (``why``); tests/test_loudness.py asserts it, and that
every block of every item keeps ``|z_j / threshold - 1| >= 1e-6`` at both gates in the plain float64 loop, none left out."""
import numpy as np

import loudness_restatement as R

LOUD, MID, QUIET = -20.0, -45.0, -80.0          # dBFS rms
MARGIN = 1e-6


def noise(n, parts, seed, spike=None):
    """``n`` samples; ``parts = [(lo, hi, dbfs), ...]`` are stretches of uniform noise with that rms, the rest is digital zero.
    ``spike = (index, value)`` sets one sample afterwards."""
    rng = np.random.default_rng(seed)
    y = np.zeros(n, dtype=np.float32)
    for lo, hi, db in parts:
        amp = 10.0 ** (db / 20.0) * np.sqrt(3.0)
        y[lo:hi] = (amp * rng.uniform(-1.0, 1.0, hi - lo)).astype(np.float32)
    if spike is not None:
        y[spike[0]] = spike[1]
    return y


def case(name, rate, items, why, target=-23.0, max_gain_db=30.0, ceiling=None, row_scale=None, L=None):
    """``row_scale=None``: a dense batch (``lengths=None``, every item owns the whole row); otherwise every item's length is a
    multiple of it.  ``L``: the row's width (the longest item by default)."""
    L = max(len(y) for y in items) if L is None else L
    if row_scale is None:
        assert all(len(y) == L for y in items)
    else:
        assert all(len(y) % row_scale == 0 and len(y) <= L for y in items)
    return dict(name=name, rate=rate, items=items, why=why, target=target, max_gain_db=max_gain_db, ceiling=ceiling,
                row_scale=row_scale, L=L)


def _wide_items():
    """257 short items at 8000 Hz: lengths around the first block, a few empty, levels drawn per item."""
    rng = np.random.default_rng(77)
    items = []
    for b in range(257):
        n = int(rng.choice([0, 1, 63, 64, 65, 800, 3199, 3200, 3201, 3264, 4000, 4096]))
        if b in (0, 255, 256):
            n = (4096, 3200, 4033)[(0, 255, 256).index(b)]
        db = float(rng.choice([LOUD, MID, QUIET]))
        items.append(noise(n, [(0, n, db)], 5000 + b))
    return items


S8, S22 = 800, 2205                              # a gating step at each rate

CASES = [
    # L_b of 0, 1, 4 step - 1, 4 step, 4 step + 1, and one that is a multiple of neither G nor step
    case("edge_lengths", 8000, [noise(0, [], 1), noise(1, [(0, 1, LOUD)], 2), noise(4 * S8 - 1, [(0, 4 * S8 - 1, LOUD)], 3),
                                noise(4 * S8, [(0, 4 * S8, LOUD)], 4), noise(4 * S8 + 1, [(0, 4 * S8 + 1, LOUD)], 5),
                                noise(7777, [(0, 7777, MID)], 6), noise(9001, [(100, 5000, LOUD), (5000, 9001, QUIET)], 7)],
         "lengths_around_one_block", row_scale=1, L=9003),
    # one dense item of 3 s: nine chunks, so the carry walks; the relative gate removes the -45 stretch, the absolute one the -80
    case("three_seconds", 22050, [noise(66151, [(0, 20000, LOUD), (20000, 40000, MID), (40000, 52000, QUIET), (52000, 66151, LOUD)], 8)],
         "carry_and_both_gates"),
    # five items, lengths in units of 256: nothing above the absolute gate; the relative gate removes blocks; the ceiling binds
    # (one sample at 0.9); the gain cap binds (-45 dBFS to -14 LUFS is over 12 dB); an ordinary one
    case("clamps", 22050, [noise(256 * 60, [(0, 256 * 60, QUIET)], 9),
                           noise(256 * 130, [(0, 15000, LOUD), (15000, 256 * 130, MID)], 10),
                           noise(256 * 90, [(0, 256 * 90, LOUD)], 11, spike=(12345, 0.9)),
                           noise(256 * 77, [(0, 256 * 77, MID)], 12),
                           noise(256 * 40, [(300, 256 * 40, LOUD)], 13)],
         "both_clamps_and_a_silent_item", target=-14.0, max_gain_db=12.0, ceiling=0.5, row_scale=256, L=256 * 130),
    # one more item than the gate kernel's block is wide
    case("batch_257", 8000, _wide_items(), "wide_batch", target=-16.0, ceiling=0.95, row_scale=1, L=4099),
]


def case_id(c):
    return c["name"]


def params(c):
    """Keyword arguments of ``LoudnessNormalizer`` for the case."""
    return dict(sample_rate=c["rate"], target_lufs=c["target"], max_gain_db=c["max_gain_db"], peak_ceiling=c["ceiling"])


def design(c):
    return R.design(c["rate"], c["target"], c["max_gain_db"], 0.0 if c["ceiling"] is None else c["ceiling"])


def batch(c, fill=0.0):
    """``(wav [B, L] float32, lengths [B] int32 or None, row_scale)``; everything behind an item holds ``fill``."""
    B, L = len(c["items"]), c["L"]
    wav = np.full((B, L), fill, dtype=np.float32)
    for b, y in enumerate(c["items"]):
        wav[b, :len(y)] = y
    if c["row_scale"] is None:
        return wav, None, 1
    return wav, np.array([len(y) // c["row_scale"] for y in c["items"]], dtype=np.int32), c["row_scale"]


_cache = {}


def reference(c):
    """Per item ``R.reference_f64`` (computed once)."""
    key = ("ref", c["name"])
    if key not in _cache:
        d = design(c)
        _cache[key] = [R.reference_f64(y, c["rate"], d) for y in c["items"]]
    return _cache[key]


def device(c, d=None):
    """Per item ``R.device_f64`` with the table ``d`` (the library's, or ``design(c)``), computed once per table."""
    d = design(c) if d is None else d
    key = ("dev", c["name"], d.tobytes())
    if key not in _cache:
        _cache[key] = [R.device_f64(y, c["rate"], d) for y in c["items"]]
    return _cache[key]


def expected(c, d=None):
    """``(stats [B, 2] float64, out [B, L] float32)`` as the device must give them."""
    dev = device(c, d)
    stats = np.array([[r["ms"], r["gain"]] for r in dev], dtype=np.float64).reshape(len(dev), 2)
    out = np.stack([R.scaled(y, r["gain"], c["L"]) for y, r in zip(c["items"], dev)])
    return stats, out
