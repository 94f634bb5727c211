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
def block_sums_f32(y, H):
    """``S[j]`` for the blocks that hold a sample: 256 accumulators over i = m, m + 256, ..., quads, then the 64-lane tree."""
    y = np.asarray(y, dtype=np.float32)
    n_blk = -(-len(y) // H)
    rows = -(-H // 256)
    x = np.zeros((n_blk, rows * 256), dtype=np.float32)
    for j in range(n_blk):
        seg = y[j * H:(j + 1) * H]
        x[j, :len(seg)] = seg
    x = x.reshape(n_blk, rows, 256)
    acc = np.zeros((n_blk, 256), dtype=np.float32)
    for r in range(rows):
        acc = acc + x[:, r] * x[:, r]
    v = ((acc[:, 0::4] + acc[:, 1::4]) + acc[:, 2::4]) + acc[:, 3::4]
    o = 32
    while o >= 1:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0]


def mse_f32(y, F, H):
    S, R, T = block_sums_f32(y, H), F // H, frames_of(len(y), H)

    def blk(j):
        return S[j] if 0 <= j < len(S) else np.float32(0.0)

    out = np.zeros(T, dtype=np.float32)
    for t in range(T):
        s = blk(t - R // 2)
        for j in range(t - R // 2 + 1, t + R // 2):
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
