"""Restatements of the assemble stage (csrc/assemble.h) for its tests: librosa's trim loop in float64 and in its own form,
the join by its rule, and the device's arithmetic in fp32 in the header's sum order.  No GPU, no native library."""
import math

import numpy as np

AMIN = 1e-10                     # librosa's amin = 1e-5 on amplitudes, squared by amplitude_to_db
KRUN_FRAMES = 32                 # csrc/assemble.h kRunFrames: frames of one item an energy block owns


def frames_of(L, H):
    return L // H + 1


def k_of(top_db):
    """``k``: 10 ** (-top_db / 10) in double on the fp32 value of top_db, rounded to fp32 once (``as_validate``)."""
    return np.float32(10.0 ** (-float(np.float32(top_db)) / 10.0))


def ramp_of(fade):
    """``fill_ramp``: 0.5 - 0.5 cos(pi (j + 0.5) / fade) in double, rounded once."""
    return np.array([0.5 - 0.5 * math.cos(math.pi * (j + 0.5) / fade) for j in range(fade)], dtype=np.float32)


# ---- float64, librosa's own steps ---------------------------------------------------------------------------------------
def mse_f64(y, F, H):
    """``librosa.feature.rms(y=, frame_length=F, hop_length=H, center=True, pad_mode="constant") ** 2``: pad, frame, mean of squares."""
    y = np.asarray(y, dtype=np.float64)
    padded = np.pad(y, F // 2)
    T = frames_of(len(y), H)
    frames = np.stack([padded[t * H:t * H + F] for t in range(T)])
    return np.mean(frames ** 2, axis=1)


def nonsilent_log_f64(mse, top_db, ref):
    """``amplitude_to_db(rms, ref=, top_db=None) > -top_db``: 10 log10(max(amin, rms^2)) - 10 log10(max(amin, ref^2))."""
    rms = np.sqrt(mse)
    ref_value = np.max(rms) if ref is None else float(ref)
    db = 10.0 * np.log10(np.maximum(AMIN, rms ** 2)) - 10.0 * np.log10(max(AMIN, ref_value ** 2))
    return db > -float(np.float32(top_db))


def ratio_f64(mse, top_db, ref):
    """``max(mse, amin) / (max(ref_b, amin) k)`` per frame: above 1 is non-silent (the product form), and its distance from 1
    is the margin an fp32 sum has to stay inside."""
    ref_b = np.max(mse) if ref is None else float(np.float32(ref)) ** 2
    return np.maximum(mse, AMIN) / (max(ref_b, AMIN) * float(k_of(top_db)))


def span_from(nonsilent, L, H, pad):
    """``frames_to_samples`` of the first and last non-silent frame, the end clipped to L, then the kept margin."""
    idx = np.flatnonzero(nonsilent)
    if L == 0 or idx.size == 0:
        start = end = 0
    else:
        start, end = int(idx[0]) * H, min(L, (int(idx[-1]) + 1) * H)
    return max(0, start - pad), min(L, end + pad)


def spans_f64(items, F, H, top_db, ref, pad):
    return [span_from(nonsilent_log_f64(mse_f64(y, F, H), top_db, ref), len(y), H, pad) for y in items]


# ---- the join -----------------------------------------------------------------------------------------------------------
def join_offsets(lens, pause):
    """``(off_0 .. off_(B-1), total)`` by the rule: off_b = S_b + pause P_b, total = S_B + pause max(P_B - 1, 0)."""
    offs, S, P = [], 0, 0
    for n in lens:
        offs.append(S + pause * P)
        S += n
        P += n > 0
    return offs + [S + pause * max(P - 1, 0)]


# ---- fp32, the header's order -------------------------------------------------------------------------------------------
def block_sums_f32(y, H, passes=None):
    """``S[j]`` for the blocks that hold a sample: 256 accumulators over i = m, m + 256, ..., quads, then the 64-lane tree.
    ``passes``: a deviation (``MUTATIONS``), the accumulate loop stopped after that many steps of 256."""
    y = np.asarray(y, dtype=np.float32)
    n_blk = -(-len(y) // H)
    rows = -(-H // 256)
    x = np.zeros((n_blk, rows * 256), dtype=np.float32)
    for j in range(n_blk):
        seg = y[j * H:(j + 1) * H]
        x[j, :len(seg)] = seg
    x = x.reshape(n_blk, rows, 256)
    acc = np.zeros((n_blk, 256), dtype=np.float32)
    for r in range(rows if passes is None else min(rows, passes)):
        acc = acc + x[:, r] * x[:, r]
    v = ((acc[:, 0::4] + acc[:, 1::4]) + acc[:, 2::4]) + acc[:, 3::4]
    o = 32
    while o >= 1:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0]


def mse_f32(y, F, H, passes=None, blocks=None):
    """``blocks``: a deviation (``MUTATIONS``), a frame's sum cut to its first ``blocks`` block sums."""
    S, R, T = block_sums_f32(y, H, passes), F // H, frames_of(len(y), H)

    def blk(j):
        return S[j] if 0 <= j < len(S) else np.float32(0.0)

    out = np.zeros(T, dtype=np.float32)
    for t in range(T):
        s = blk(t - R // 2)
        for j in range(t - R // 2 + 1, t - R // 2 + (R if blocks is None else min(R, blocks))):
            s = np.float32(s + blk(j))
        out[t] = s / np.float32(F)
    return out


def nonsilent_f32(mse, top_db, ref):
    amin = np.float32(AMIN)
    ref_b = np.max(mse) if ref is None else np.float32(ref) * np.float32(ref)
    thr = np.float32(np.maximum(ref_b, amin) * k_of(top_db))
    return np.maximum(mse, amin) > thr


def spans_f32(items, F, H, top_db, ref, pad):
    return [span_from(nonsilent_f32(mse_f32(y, F, H), top_db, ref), len(y), H, pad) for y in items]


def faded_f32(y, span, fade):
    """The trimmed item: ``(y[start' + n] * a) * b2``, two fp32 products in that order."""
    seg = np.asarray(y, dtype=np.float32)[span[0]:span[1]].copy()
    n = len(seg)
    if fade and n:
        ramp, idx = ramp_of(fade), np.arange(n)
        a = np.where(idx < fade, ramp[np.minimum(idx, fade - 1)], np.float32(1.0)).astype(np.float32)
        back = n - 1 - idx
        b2 = np.where(back < fade, ramp[np.minimum(back, fade - 1)], np.float32(1.0)).astype(np.float32)
        seg = (seg * a) * b2
    return seg


def join_f32(items, spans, fade, pause, cap):
    """``(out [cap], offsets [B + 1])``: the trimmed items end to end, zeros in the pauses and the tail."""
    offs = join_offsets([e - s for s, e in spans], pause)
    out = np.zeros(cap, dtype=np.float32)
    for y, sp, o in zip(items, spans, offs):
        seg = faded_f32(y, sp, fade)
        out[o:o + len(seg)] = seg
    return out, offs


# ---- the three launches as the device runs them, with one named deviation ------------------------------------------------
KGATHER_RUN = 4096               # csrc/assemble.h kGatherRun: output positions of a gather block

MUTATIONS = {                    # each a wrong kernel a reviewer could plausibly write; None is the header's own
    "scan_drops_wave_sums": "gather scan: the sums of the waves in front are left out of the off of the items that waves 1-3 own",
    "scan_per_rounds_down": "gather scan: per = max(1, B / 256), so items past 256 per are owned by nobody (their off reads 0)",
    "total_from_last_owner": "gather scan: off[B] is the wave-level inclusive sum of the last thread that owns an item, not the run behind thread 255",
    "item_of_strict": "gather item_of: off[mid] < p for off[mid] <= p",
    "item_of_first_of_run": "gather item_of: the first of a run of equal offsets is returned, not the last",
    "bounds_first_256": "bounds: the frame loops make one pass (t < 256 only)",
    "ref_max_first_256": "bounds: the item's own maximum is taken over t < 256 only",
    "first_last_wave0": "bounds: first and last are taken from wave 0's candidates only (t mod 256 < 64)",
    "frame_sum_one_run": "energy: a frame adds min(R, kRunFrames) block sums, not R",
    "accumulate_8_passes": "energy: a block's accumulate loop stops after 8 steps of 256 (2048 samples)",
    "ramp_block_local": "gather sample: the ramps are looked up at the position inside the gather block's part of the item",
}


def energies_dev(items, F, H, mutation=None):
    """``energy_kernel``: mse per item, fp32."""
    passes = 8 if mutation == "accumulate_8_passes" else None
    blocks = KRUN_FRAMES if mutation == "frame_sum_one_run" else None
    return [mse_f32(y, F, H, passes=passes, blocks=blocks) for y in items]


def bounds_dev(mse, lens, H, top_db, ref, pad, mutation=None):
    """``bounds_kernel``: ``(start', end')`` per item.  Thread ``tid`` of 256 looks at t = tid, tid + 256, ...; wave w holds the
    frames with ``t mod 256`` in [64 w, 64 w + 64)."""
    amin, k, spans = np.float32(AMIN), k_of(top_db), []
    for m, Lb in zip(mse, lens):
        T = frames_of(Lb, H)
        assert len(m) == T
        seen = min(T, 256) if mutation == "bounds_first_256" else T
        if ref is None:
            ref_b = np.max(m[:min(T, 256) if mutation in ("bounds_first_256", "ref_max_first_256") else T], initial=np.float32(0.0))
        else:
            ref_b = np.float32(ref) * np.float32(ref)
        thr = np.float32(np.maximum(ref_b, amin) * k)
        loud = np.maximum(m, amin) > thr
        loud[seen:] = False
        if mutation == "first_last_wave0":
            loud &= np.arange(T) % 256 < 64
        idx = np.flatnonzero(loud)
        start = end = 0
        if idx.size:
            start, end = int(idx[0]) * H, min(Lb, (int(idx[-1]) + 1) * H)
        spans.append((max(0, start - pad), min(Lb, end + pad)))
    return spans


def scan_dev(lens, pause, mutation=None):
    """The gather's scan of ``w_b = len_b + (len_b > 0 ? pause : 0)`` into ``off[0 .. B]``: 256 threads own ``per`` items each, an
    inclusive scan inside each wave of 64, the sums of the waves in front added, ``off[B]`` the run behind thread 255.  A word
    no thread stores reads as 0 here (on the device it is whatever the LDS held)."""
    B = len(lens)
    w = [int(n) + (pause if n else 0) for n in lens]
    per = max(1, B // 256) if mutation == "scan_per_rounds_down" else (B + 255) // 256
    lo = [min(t * per, B) for t in range(256)]
    hi = [min(lo[t] + per, B) for t in range(256)]
    mine = [sum(w[lo[t]:hi[t]]) for t in range(256)]
    incl = [sum(mine[t - t % 64:t + 1]) for t in range(256)]
    wave_sum = [incl[64 * v + 63] for v in range(4)]
    off = [0] * (B + 1)
    for t in range(256):
        run = incl[t] - mine[t] + sum(wave_sum[:t // 64])
        lost = sum(wave_sum[:t // 64]) if mutation == "scan_drops_wave_sums" else 0     # from the items' off, not from the total
        for i in range(lo[t], hi[t]):
            off[i] = run - lost
            run += w[i]
        if t == 255:
            off[B] = run
    if mutation == "total_from_last_owner":
        off[B] = incl[max(t for t in range(256) if lo[t] < hi[t])] if B else 0
    return off


def gather_dev(wav, spans, off, fade, pause, cap, mutation=None):
    """``gather_kernel``, the join form: ``(out [cap] fp32, offsets [B + 1])``.  A group of four positions takes its first
    position's item where the whole group lies in front of the next item's start, and searches per position otherwise."""
    B = len(spans)
    off = np.asarray(off, dtype=np.int64)
    start = np.array([s for s, _ in spans], dtype=np.int64)
    length = np.array([e - s for s, e in spans], dtype=np.int64)
    ramp = ramp_of(fade) if fade else np.ones(1, dtype=np.float32)

    def item_of(p):
        lo, hi = np.zeros(len(p), dtype=np.int64), np.full(len(p), B, dtype=np.int64)
        while np.any(hi - lo > 1):
            go = hi - lo > 1
            mid = (lo + hi) >> 1
            left = off[mid] < p if mutation == "item_of_strict" else off[mid] <= p
            lo, hi = np.where(go & left, mid, lo), np.where(go & ~left, mid, hi)
        if mutation == "item_of_first_of_run":
            while True:
                back = (lo > 0) & (off[np.maximum(lo - 1, 0)] == off[lo])
                if not back.any():
                    break
                lo = lo - back
        return lo

    p = np.arange(cap, dtype=np.int64)
    first = item_of(p - p % 4)                                       # the group's own search
    nxt = np.where(first == B - 1, np.int64(0xffffffff), off[np.minimum(first + 1, B)])
    b = np.where(p - p % 4 + 3 < nxt, first, item_of(p))
    at, n = off[b], p - off[b]
    inside = (n >= 0) & (n < length[b])                               # unsigned on the device: a negative n is far past len
    n_in = np.where(inside, n, 0)
    back = length[b] - 1 - n_in
    n_up, n_down = n_in, back
    if mutation == "ramp_block_local":
        blk = p - p % KGATHER_RUN
        n_up = p - np.maximum(at, blk)
        n_down = np.minimum(at + length[b], blk + KGATHER_RUN) - 1 - p
    up = np.where(n_up < fade, ramp[np.clip(n_up, 0, len(ramp) - 1)], np.float32(1.0)).astype(np.float32)
    down = np.where(n_down < fade, ramp[np.clip(n_down, 0, len(ramp) - 1)], np.float32(1.0)).astype(np.float32)
    src = np.asarray(wav, dtype=np.float32)[b, np.where(inside, start[b] + n_in, 0)] if wav.shape[1] else np.zeros(cap, np.float32)
    out = np.where(inside, (src * up) * down, np.float32(0.0)).astype(np.float32)
    total = int(off[B]) - (pause if off[B] else 0)
    return out, [int(v) for v in off[:B]] + [total]


STAGE_OF = {"frame_sum_one_run": 0, "accumulate_8_passes": 0, "bounds_first_256": 1, "ref_max_first_256": 1, "first_last_wave0": 1,
            "scan_drops_wave_sums": 2, "scan_per_rounds_down": 2, "total_from_last_owner": 2, "item_of_strict": 3,
            "item_of_first_of_run": 3, "ramp_block_local": 3}


def device_f32(items, wav, F, H, top_db, ref, pad, fade, pause, cap, mutation=None, clean=None):
    """The three launches on a batch: ``dict(mse32, spans, offsets, out)``.  ``mutation``: a key of ``MUTATIONS``.  ``clean``: the
    result without a deviation, whose stages in front of the deviating one are taken over instead of being computed again."""
    assert mutation is None or mutation in MUTATIONS
    stage = STAGE_OF.get(mutation, 0)
    lens = [len(y) for y in items]
    mse = clean["mse32"] if clean and stage > 0 else energies_dev(items, F, H, mutation)
    spans = clean["spans"] if clean and stage > 1 else bounds_dev(mse, lens, H, top_db, ref, pad, mutation)
    off = clean["off"] if clean and stage > 2 else scan_dev([e - s for s, e in spans], pause, mutation)
    out, offsets = gather_dev(wav, spans, off, fade, pause, cap, mutation)
    return dict(mse32=mse, spans=spans, off=off, offsets=offsets, out=out)
