"""The limiter's rules (csrc/limiter.h) in plain numpy, twice: ``plain_f64`` in float64, and ``device_f32`` with the kernel's own
operations -- float32 ``fmaf`` chains in the stated order (``iris.resample.fmaf32``: one rounding), the fp64 division rounded to
fp32 -- which the device must equal bit for bit.  Both take the design table (``Limiter.design()``: 36 bank values, then the
``2A + 1`` weights); ``design_f64`` derives that table independently in float64.  One item ``x [n]`` float32 at a time."""
import numpy as np

from iris.resample import fmaf32

TAPS, PHASES, BANK = 12, 3, 36
BETA, ROLLOFF, HALF_WIDTH = 9.0, 0.945, 6       # csrc/resample.h: the defaults, and Hw for 6 zeros at s = 1
F32 = np.float32


def design_f64(A):
    """``(bank [3, 12], w [2A + 1])`` in float64, before any rounding to fp32: the Kaiser-windowed sinc at ``t = (j - 5) - q / 4``
    (numpy's ``sinc`` and ``i0``, not the library's series) and the Hann shape normalised to sum 1."""
    j = np.arange(TAPS, dtype=np.float64)[None, :]
    q = np.arange(1, PHASES + 1, dtype=np.float64)[:, None]
    t = (j - (HALF_WIDTH - 1)) - q / 4.0
    bank = ROLLOFF * np.sinc(ROLLOFF * t) * np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / HALF_WIDTH) ** 2, 0.0))) / np.i0(BETA)
    bank = np.where(np.abs(t) <= HALF_WIDTH, bank, 0.0)
    k = np.arange(-A, A + 1, dtype=np.float64)
    w = 0.5 * (1.0 + np.cos(np.pi * k / (A + 1)))
    return bank, w / w.sum()


def split(table, A):
    table = np.asarray(table)
    assert table.shape == (BANK + 2 * A + 1,)
    return table[:BANK].reshape(PHASES, TAPS), table[BANK:]


def _padded(x, pad, dtype):
    out = np.zeros(len(x) + 2 * pad, dtype=dtype)
    out[pad:pad + len(x)] = x
    return out


def _run(x, c, A, table, exact):
    """The rules once; ``exact``: float64 throughout, otherwise the kernel's float32 operations."""
    x = np.asarray(x, dtype=F32)
    n = len(x)
    dt = np.float64 if exact else F32
    bank, w = split(np.asarray(table, dtype=F32).astype(dt), A)
    c = dt(F32(c))
    one = dt(1.0)
    if n == 0:
        e = np.zeros(0, dtype=dt)
        return dict(u=np.zeros((1, PHASES), dtype=dt), p=e, tp=dt(0.0), r=e, m=e, g=e, min_g=one, raw=e, out=e)
    # u[g, q] for g = -1 .. n - 1 (row g + 1): x[g - 5 + j]
    xp = _padded(x, 6, dt)
    u = np.zeros((n + 1, PHASES), dtype=dt)
    for q in range(PHASES):
        acc = np.zeros(n + 1, dtype=dt)
        for j in range(TAPS):
            xv = xp[j:j + n + 1]                                    # x[g - 5 + j] = xp[g + 1 + j]
            acc = acc + xv * bank[q, j] if exact else fmaf32(xv, np.full(n + 1, bank[q, j], dtype=F32), acc)
        u[:, q] = acc
    au = np.abs(u).max(axis=1)
    p = np.maximum(np.abs(x.astype(dt)), np.maximum(au[:-1], au[1:]))
    with np.errstate(divide="ignore"):
        quot = c.astype(np.float64) / p.astype(np.float64)
    r = np.where(p > c, quot if exact else quot.astype(F32), one).astype(dt)
    # m[g] for g = -A .. n + A - 1 from r on -2A .. n + 2A - 1, 1 outside the item
    rp = np.ones(n + 4 * A, dtype=dt)
    rp[2 * A:2 * A + n] = r
    m = rp[:n + 2 * A].copy()
    for k in range(1, 2 * A + 1):
        m = np.minimum(m, rp[k:k + n + 2 * A])
    d = one - m
    acc = np.zeros(n, dtype=dt)
    for j in range(2 * A + 1):
        dv = d[j:j + n]                                             # d[n + j - A], stored from -A
        acc = acc + dv * w[j] if exact else fmaf32(dv, np.full(n, w[j], dtype=F32), acc)
    g = one - acc
    raw = x.astype(dt) * g
    out = np.minimum(np.maximum(raw, -c), c)
    return dict(u=u, p=p, tp=p.max(), r=r, m=m[A:A + n], g=g, min_g=g.min(), raw=raw, out=out)


def plain_f64(x, c, A, table):
    """Every rule in float64 (the table's fp32 values as they are).  ``u [n + 1, 3]`` (row 0 is ``u[-1]``), ``p``, ``tp``, ``r``,
    ``m``, ``g``, ``min_g``, ``raw`` (``x g`` in front of the clamp) and ``out``."""
    return _run(x, c, A, table, True)


def device_f32(x, c, A, table):
    """The same with the kernel's operations; every array float32."""
    return _run(x, c, A, table, False)


def tile_parts(res, n, tile):
    """``[ceil(n / tile), 2]`` float32: ``(max p, min g)`` over each tile of an item's own samples."""
    tiles = -(-n // tile)
    out = np.zeros((tiles, 2), dtype=F32)
    for t in range(tiles):
        out[t] = (res["p"][t * tile:(t + 1) * tile].max(), res["g"][t * tile:(t + 1) * tile].min())
    return out


def error_bars(x, c, A, table):
    """What ``device_f32`` may differ from ``plain_f64`` by, from the chain lengths alone (u = 2^-24, every quantity below in
    float64 from ``plain_f64``): a chain of n fmaf is off by at most ``n u sum|h||x|``; a maximum or minimum passes its inputs'
    largest error on; ``min(1, c / p)`` has slope at most ``1 / c`` and its fp32 rounding adds u (r <= 1); ``1 - m`` and ``1 - s``
    add u each; the smoothing passes ``sum |w| E_d`` on and adds ``(2A + 1) u sum|w||d|``; the product adds ``u |x g|`` and the clamp
    has slope 1.  Returns ``dict(p=, g=, out=)`` per sample."""
    u_ = 2.0 ** -24
    ref = plain_f64(x, c, A, table)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    bank, w = split(np.asarray(table, dtype=np.float32).astype(np.float64), A)
    if n == 0:
        e = np.zeros(0)
        return dict(p=e, g=e, out=e)
    xp = _padded(np.abs(x), 6, np.float64)
    e_u = np.zeros(n + 1)
    for q in range(PHASES):
        acc = np.zeros(n + 1)
        for j in range(TAPS):
            acc += xp[j:j + n + 1] * abs(bank[q, j])
        e_u = np.maximum(e_u, TAPS * u_ * acc)
    e_p = np.maximum(e_u[:-1], e_u[1:])
    e_r = e_p / float(np.float32(c)) + u_
    ep = np.zeros(n + 4 * A)
    ep[2 * A:2 * A + n] = e_r
    e_m = ep[:n + 2 * A].copy()
    for k in range(1, 2 * A + 1):
        e_m = np.maximum(e_m, ep[k:k + n + 2 * A])
    e_d = e_m + u_
    rp = np.ones(n + 4 * A)
    rp[2 * A:2 * A + n] = ref["r"]
    m = rp[:n + 2 * A].copy()
    for k in range(1, 2 * A + 1):
        m = np.minimum(m, rp[k:k + n + 2 * A])
    d = 1.0 - m
    e_s = np.zeros(n)
    for j in range(2 * A + 1):
        e_s += abs(w[j]) * (e_d[j:j + n] + (2 * A + 1) * u_ * np.abs(d[j:j + n]))
    e_g = e_s + u_
    e_out = np.abs(x) * e_g + u_ * np.abs(ref["raw"])
    return dict(p=e_p, g=e_g, out=e_out)
