"""Inputs of the limiter's tests: ragged batches of seeded uniform noise under the ceiling with single samples, or an fs / 4 sine,
set above it.  ``A`` is the lookahead in samples (1, 33, 256), ``c`` the ceiling (1.0, 0.5), ``T`` the kernel's tile.  The edge-length
cases hold items of 0, 1, 2, A, 2A + 1, T - 1, T, T + 1 and 2T + 3 samples; the others place peaks at sample 0, at ``L_b - 1``, on a
tile seam, on both sides of a seam less than ``A`` apart (``A = 1`` admits only neighbours) and between samples only.  The
conditions at the end of the file hold in ``plain_f64`` alone: every case but the edge-length ones has an item that is limited and
one that is not."""
import numpy as np

from iris.limiter import TILE as T

import limiter_restatement as R

RATE = 1000                                     # lookahead_ms = A at this rate


def quiet(n, c, seed, level=0.4):
    """``n`` samples of uniform noise within ``level * c``: its true peak stays under c (the bank's gain is under 1.5)."""
    return (level * c * np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(np.float32)


def spiked(n, c, seed, at, height=1.5):
    """``quiet`` with the samples ``at`` set to ``+- height * c`` (alternating signs)."""
    y = quiet(n, c, seed)
    for i, k in enumerate(at):
        if 0 <= k < n:
            y[k] = (height if i % 2 == 0 else -height) * c
    return y


def quarter_sine(n, c, amp=1.2):
    """An fs / 4 sine at 45 degrees: every sample is ``+- amp c / sqrt(2)`` (0.85 c, under the ceiling), the wave between them
    reaches ``amp c``."""
    return (amp * c * np.sin(0.5 * np.pi * np.arange(n) + 0.25 * np.pi)).astype(np.float32)


def case(name, A, c, items, edge=False, row_scale=None, L=None):
    """``row_scale=None``: a dense batch (``lengths=None``); otherwise every item's length is a multiple of it."""
    L = max(len(y) for y in items) if L is None else L
    if row_scale is None:
        assert all(len(y) == L for y in items)
    else:
        assert all(len(y) % row_scale == 0 and len(y) <= L for y in items)
    return dict(name=name, A=A, c=c, items=items, edge=edge, row_scale=row_scale, L=L)


def edge_lengths(A, c, seed):
    lens = sorted({0, 1, 2, A, 2 * A + 1, T - 1, T, T + 1, 2 * T + 3})
    # a peak at both ends of every item, and one inside the long ones
    items = [spiked(n, c, seed + i, [0, n - 1, n // 2] if n > 2 else [0]) for i, n in enumerate(lens)]
    return case(f"edge_lengths_A{A}", A, c, items, edge=True, row_scale=1, L=2 * T + 5)       # rows off 16 bytes


def placements(A, c, seed):
    n, h = 2 * T + 3, max(A // 4, 0)
    items = [quiet(n, c, seed),                                     # under the ceiling
             spiked(n, c, seed + 1, [0]),                           # at sample 0
             spiked(n, c, seed + 2, [n - 1]),                       # at L_b - 1
             spiked(n, c, seed + 3, [T - 1, T]),                    # on a tile seam, its last and first sample
             spiked(n, c, seed + 4, [T - 1 - h, T + h, 2 * T - 1 - h, 2 * T + h]),    # both sides of a seam, 2 (A // 4) + 1 apart
             quarter_sine(n, c)]                                    # between samples only
    return case(f"placements_A{A}", A, c, items)


def _ragged():
    c = 0.5
    return case("ragged_256", 33, c, [spiked(5 * 256, c, 31, [700, 1279]), quiet(16 * 256, c, 32),
                                      spiked(9 * 256, c, 33, [T - 3, T + 5], height=3.0)], row_scale=256, L=17 * 256)


def _wide():
    rng = np.random.default_rng(57)
    items = []
    for b in range(257):
        n = int(rng.integers(0, 64))
        if b in (0, 255, 256):
            n = (63, 0, 40)[(0, 255, 256).index(b)]
        items.append(spiked(n, 1.0, 900 + b, [int(rng.integers(0, max(n, 1)))]) if b % 3 else quiet(n, 1.0, 900 + b))
    return case("batch_257", 33, 1.0, items, row_scale=1, L=63)


CASES = [edge_lengths(1, 0.5, 100), edge_lengths(33, 1.0, 200), edge_lengths(256, 0.5, 300),
         placements(1, 1.0, 400), placements(33, 1.0, 500), placements(256, 0.5, 600), _ragged(), _wide()]


def case_id(c):
    return c["name"]


def params(c):
    """Keyword arguments of ``Limiter`` for the case: the ceiling as the library will see it is ``float32(10 ** (dbtp / 20))``."""
    return dict(sample_rate=RATE, ceiling_dbtp=20.0 * np.log10(c["c"]), lookahead_ms=float(c["A"]))


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


def _per_item(kind, fn, c, table):
    table = np.asarray(table, dtype=np.float32)
    key = (kind, c["name"], table.tobytes())
    if key not in _cache:
        _cache[key] = [fn(y, c["c"], c["A"], table) for y in c["items"]]
    return _cache[key]


def reference(c, table):
    """Per item ``R.plain_f64`` (computed once per table)."""
    return _per_item("ref", R.plain_f64, c, table)


def device(c, table):
    """Per item ``R.device_f32`` (computed once per table)."""
    return _per_item("dev", R.device_f32, c, table)


def expected(c, table):
    """``(stats [B, 2] float32, out [B, L] float32)`` as the device must give them."""
    dev = device(c, table)
    stats = np.array([[r["tp"], r["min_g"]] for r in dev], dtype=np.float32).reshape(len(dev), 2)
    out = np.zeros((len(dev), c["L"]), dtype=np.float32)
    for b, r in enumerate(dev):
        out[b, :len(r["out"])] = r["out"]
    return stats, out


def check_conditions(c, table):
    """In ``plain_f64`` alone: a case that is not an edge-length one has an item with ``tp > c`` and ``min g < 1``, and one with
    ``tp <= c``."""
    if c["edge"]:
        return
    ref = reference(c, table)
    ceiling = float(np.float32(c["c"]))
    assert any(r["tp"] > ceiling and r["min_g"] < 1.0 for r in ref), c["name"]
    assert any(r["tp"] <= ceiling for r in ref), c["name"]
