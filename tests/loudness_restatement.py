"""The loudness stage (csrc/loudness.h) restated in numpy float64, twice.  ``reference_f64`` is the plain BS.1770-4 loop:
sequential biquads (scipy's ``lfilter``), 400 ms blocks every 100 ms, the two gates, the gain.  ``device_f64`` is the same in the
kernels' own structure -- segments of G samples from state 0, the scan inside a chunk, the carry, the start states, the rerun,
every sum in the header's order -- so the device's results equal it bit for bit.  Neither contracts a product into a sum: numpy
has no fused multiply-add, and the kernels are compiled without one."""
import math

import numpy as np
from scipy.signal import lfilter

G, CHUNK_SEGS, SCAN_STEPS = 64, 128, 7            # kSeg, kChunkSegs, kScanSteps
SHELF, HIGH_PASS, ABS_THR, TARGET_MS, MAX_GAIN, CEILING, MATS, DESIGN = 0, 5, 10, 11, 12, 13, 16, 16 + 16 * 8
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)


def coefficients(rate):
    """``(shelf b, shelf a, high-pass b, high-pass a)``, three values each with ``a[0] = 1``: the bilinear derivation with
    ``K = tan(pi f0 / fs)`` of libebur128 and pyloudnorm."""
    K, Q = math.tan(math.pi * 1681.974450955533 / rate), 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    sa = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K, Q = math.tan(math.pi * 38.13547087602444 / rate), 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return sb, sa, [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def mat_mul(X, Y):
    """4 x 4, terms ascending (``mat_mul`` of the header)."""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = X[i, 0] * Y[0, j]
            for m in range(1, 4):
                s = s + X[i, m] * Y[m, j]
            out[i, j] = s
    return out


def design(rate, target_lufs=-23.0, max_gain_db=30.0, peak_ceiling=0.0):
    """The table ``iris_loudness_design`` returns, derived here; ``target_lufs`` / ``max_gain_db`` / ``peak_ceiling`` are taken
    through float32 first, as the config carries them."""
    sb, sa, hb, ha = coefficients(rate)
    d = np.zeros(DESIGN)
    d[SHELF:SHELF + 5] = sb + sa[1:]
    d[HIGH_PASS:HIGH_PASS + 5] = hb + ha[1:]
    d[ABS_THR] = ABS_GATE
    d[TARGET_MS] = 10.0 ** ((float(np.float32(target_lufs)) + 0.691) / 10.0)
    d[MAX_GAIN] = 10.0 ** (float(np.float32(max_gain_db)) / 20.0)
    d[CEILING] = float(np.float32(peak_ceiling))
    a1, a2, (c0, c1, c2), d1, d2 = sa[1], sa[2], hb, ha[1], ha[2]
    A = np.array([[-a1, 1.0, 0.0, 0.0], [-a2, 0.0, 0.0, 0.0], [c1 - d1 * c0, 0.0, -d1, 1.0], [c2 - d2 * c0, 0.0, -d2, 0.0]])
    P = A.copy()
    for _ in range(G - 1):
        P = mat_mul(A, P)
    mats = [P]
    for _ in range(SCAN_STEPS):
        mats.append(mat_mul(mats[-1], mats[-1]))
    d[MATS:] = np.concatenate([m.reshape(-1) for m in mats])
    return d


def blocks_of(n, step):
    return (n - 4 * step) // step + 1 if n >= 4 * step else 0


def gain_of(ms, peak, d):
    """``g_b`` from ``ms_b`` and the item's peak (a float32 value), every operation one rounding."""
    if not ms > 0.0:
        return 1.0
    g = float(np.sqrt(np.float64(d[TARGET_MS]) / np.float64(ms)))
    g = min(g, float(d[MAX_GAIN]))
    if d[CEILING] > 0.0 and peak > 0.0:
        g = min(g, float(np.float64(d[CEILING]) / np.float64(peak)))
    return g


def scaled(y, g, L=None):
    """``out`` row of an item: one fp32 product per sample, 0 behind the item up to ``L``."""
    out = np.zeros(len(y) if L is None else L, dtype=np.float32)
    out[:len(y)] = y * np.float32(g)
    return out


# ---- the plain loop ----------------------------------------------------------------------------------------------------------
def reference_f64(y, rate, d=None):
    """One item ``y`` (float32) -> ``dict(z, abs_mask, rel_mask, ms, gain, peak, lufs)``: BS.1770-4 as the standard states it."""
    d = design(rate) if d is None else d
    sb, sa, hb, ha = coefficients(rate)
    step = rate // 10
    x = np.asarray(y, dtype=np.float64)
    v = lfilter(hb, ha, lfilter(sb, sa, x)) if len(x) else x
    J = blocks_of(len(x), step)
    sq = v * v
    z = np.array([sq[j * step:j * step + 4 * step].sum() / (4 * step) for j in range(J)])
    abs_mask = z > ABS_GATE
    rel_thr = 0.1 * z[abs_mask].mean() if abs_mask.any() else np.inf
    rel_mask = abs_mask & (z > rel_thr)
    ms = float(z[rel_mask].mean()) if rel_mask.any() else 0.0
    peak = float(np.abs(np.asarray(y, dtype=np.float32)).max()) if len(x) else 0.0
    with np.errstate(divide="ignore"):
        lufs = -0.691 + 10.0 * np.log10(ms)
    return dict(z=z, abs_mask=abs_mask, rel_mask=rel_mask, rel_thr=rel_thr, ms=ms, gain=gain_of(ms, peak, d), peak=peak, lufs=float(lufs))


# ---- the kernels' structure ----------------------------------------------------------------------------------------------------
def _step(c, s, x):
    """One sample of every segment at once; ``s`` is ``[n, 4]`` and changes in place.  Returns v."""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = c
    u = b0 * x + s[:, 0]
    s[:, 0] = (b1 * x - a1 * u) + s[:, 1]
    s[:, 1] = b2 * x - a2 * u
    v = c0 * u + s[:, 2]
    s[:, 2] = (c1 * u - d1 * v) + s[:, 3]
    s[:, 3] = c2 * u - d2 * v
    return v


def _matvec(P, v):
    """``v [n, 4]`` -> ``P v`` per row of v, terms ascending."""
    out = np.empty_like(v)
    for r in range(4):
        s = P[r, 0] * v[:, 0]
        for m in range(1, 4):
            s = s + P[r, m] * v[:, m]
        out[:, r] = s
    return out


def fixed_sum(values):
    """The header's block sum of ``values`` (already gated, in block order): 256 strided accumulators, then a tree."""
    acc = np.zeros(256)
    for t in range(min(256, len(values))):
        for z in values[t::256]:
            acc[t] = acc[t] + z
    o = 128
    while o >= 1:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return float(acc[0])


def _gated_sum(z, mask):
    """``fixed_sum`` over the blocks of ``mask``, each accumulator taking its own j = t, t + 256, ... ascending."""
    acc = np.zeros(256)
    for j in np.flatnonzero(mask):
        acc[j % 256] = acc[j % 256] + z[j]
    o = 128
    while o >= 1:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return float(acc[0])


def device_f64(y, rate, d):
    """One item ``y`` (float32) with the library's (or ``design``'s) table ``d`` -> ``dict(z, abs_mask, rel_mask, ms, gain, peak,
    ends, parts, hops, seg_peak)``, the last four as the workspace holds them for the item."""
    y = np.asarray(y, dtype=np.float32)
    n, step = len(y), rate // 10
    c = tuple(d[SHELF:SHELF + 5]) + tuple(d[HIGH_PASS:HIGH_PASS + 5])
    P = d[MATS:].reshape(SCAN_STEPS + 1, 4, 4)
    chunks = -(-n // (G * CHUNK_SEGS))
    segs = chunks * CHUNK_SEGS
    x = np.zeros(segs * G)
    x[:n] = y
    x = x.reshape(segs, G)
    first = np.arange(segs) * G
    whole = first + G <= n
    # local: every segment from 0, then the scan inside each chunk
    e = np.zeros((segs, 4))
    for i in range(G):
        _step(c, e, x[:, i])
    e[~whole] = 0.0
    e = e.reshape(chunks, CHUNK_SEGS, 4)
    for k in range(SCAN_STEPS):
        o = 1 << k
        new = e.copy()
        for ch in range(chunks):
            new[ch, o:] = _matvec(P[k], e[ch, :CHUNK_SEGS - o]) + e[ch, o:]
        e = new
    # rerun: the carry, the start states, the segments again
    start = np.zeros((chunks, CHUNK_SEGS, 4))
    C = np.zeros((1, 4))
    for ch in range(chunks):
        w = np.zeros((CHUNK_SEGS, 4))
        w[0] = C[0]
        for k in range(SCAN_STEPS):
            o = 1 << k
            w[o:2 * o] = _matvec(P[k], w[:o])
        start[ch, 0] = w[0]
        start[ch, 1:] = w[1:] + e[ch, :-1]
        C = _matvec(P[SCAN_STEPS], C) + e[ch, -1]
    s = start.reshape(segs, 4).copy()
    cnt = np.clip(n - first, 0, G)
    m = (first // step + 1) * step - first
    p0, p1 = np.zeros(segs), np.zeros(segs)
    for i in range(G):
        v = _step(c, s, x[:, i])
        q = v * v
        live = i < cnt
        p0 = np.where(live & (i < m), p0 + q, p0)
        p1 = np.where(live & (i >= m), p1 + q, p1)
    seg_peak = np.abs(x.astype(np.float32)).max(axis=1) if segs else np.zeros(0, np.float32)
    used = first < n
    # gate
    nh = n // step
    J = nh - 3 if nh >= 4 else 0
    S = np.zeros(nh)
    for h in range(nh):
        acc = 0.0
        for k in range(h * step // G, ((h + 1) * step - 1) // G + 1):
            acc = acc + (p0[k] if k * G // step == h else p1[k])
        S[h] = acc
    z = np.array([(((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) / float(4 * step) for j in range(J)])
    abs_mask = z > d[ABS_THR]
    rel_mask = np.zeros(J, dtype=bool)
    ms = 0.0
    if abs_mask.any():
        rel_thr = 0.1 * (_gated_sum(z, abs_mask) / float(abs_mask.sum()))
        rel_mask = abs_mask & (z > rel_thr)
        if rel_mask.any():
            ms = _gated_sum(z, rel_mask) / float(rel_mask.sum())
    peak = float(seg_peak[used].max()) if used.any() else 0.0
    return dict(z=z, abs_mask=abs_mask, rel_mask=rel_mask, ms=ms, gain=gain_of(ms, peak, d), peak=peak,
                ends=e.reshape(segs, 4), parts=np.stack([p0, p1], axis=1), hops=S, seg_peak=seg_peak, used=used)
