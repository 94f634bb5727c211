"""Every launch of the time stretch on the MI355X -- ``stft_kernel<ts::Spectrum>``, ``ts_step_kernel``, ``ts_scan_kernel`` and
``gl_istft_kernel`` with ``IstftLaunch::sample_counts`` -- each judged on the device's OWN input against the CPU restatement of
the arithmetic csrc/time_stretch.h commits to (oracle/dsp_chain_cases.py; tests/test_oracle_time_stretch_chain.py ties the
restatements to the float64 one, checks the conditions on the bars and shows that the wrong restatements fail).

Exact (``==`` element by element; -0 equals +0, NaN equals nothing): the stored spectrum and the three per-item counts, ``mag``
(every product and sum its own rounding -- no contraction search), the scan ``acc`` from the device's ``inc`` and ``acc[0]``, the
padding bins, and the inverse transform bounded by the items' sample counts.  Held to the bars the oracle module derives, and to
no other tolerance: ``inc`` and ``acc[0]`` (atan2f; units of 2^-32 turn, wrapped difference) and ``out_c`` (sincospif; per
element, relative to the element).  Workspace and output are poisoned with NaN before every call, so what a launch must not
write is still NaN afterwards (read through its bits for ``inc`` and ``acc``) and what it must write is not.  ``mag`` elements
with a subnormal square may be left out only where the device disagrees, at most 0.1 % of an item's, none in a silence case.

RESULTS on an MI355X (ROCm's hipcc, the project's flags), one run; every rerun bit-equal in every buffer.  The bars are the
derived ones and were not adjusted to it:
    stft_kernel<ts::Spectrum>          485 434 elements exact        Spectrum::item (counts)            228 exact
    ts_step_kernel mag                 258 944 exact (the plain form: ``#pragma clang fp contract(off)`` holds; none left out)
    ts_step_kernel inc                  63 745 exact (bar 0: padding, silence, both angles 0), 195 199 within the bar,
                                        worst error / bar 0.905
    ts_scan_kernel acc                 258 944 exact
    ts_scan_kernel acc[0]                2 879 exact (bar 0), 4 933 within the bar, worst error / bar 0.906
    ts_scan_kernel out_c               517 888 within the bar, worst error / bar 0.611
    gl_istft_kernel (sample_counts)    159 322 exact
    ragged item == its batch-of-one call, per buffer: 181 858 elements equal
    mag elements with a float64 re^2 + im^2 < 2^-125 left out because the device disagreed there: 0
All three barred quantities came within a factor 2 of their bars.  The bars are sums of half-ulp rounding terms that a
value can reach, beside the functions' allowances: numpy's fp32 arctan2 reaches 0.90 of the ``inc`` bar on the CPU as well
(tests/test_oracle_time_stretch_chain.py prints it).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.time_stretch import TimeStretch
from oracle import dsp_chain_cases as D

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
NAN_BITS = 0x7FC00000                                            # what the poison reads as in ``inc`` and ``acc``
SESSION = D.Session()
SPEC, STEP, SCAN, ISTFT = "stft_kernel<ts::Spectrum>", "ts_step_kernel", "ts_scan_kernel", "gl_istft_kernel (sample_counts)"
_state = {"left_out": 0}


def model(name) -> TimeStretch:
    if ("ts", name) not in _state:
        cfg = D.TS_CONFIGS[name]
        _state[("ts", name)] = TimeStretch(cfg["n_fft"], cfg["hop_length"], cfg["win_length"], device=DEV)
    return _state[("ts", name)]


def run(name, wav, rate, lengths=None):
    """One poisoned ``forward_device`` -> ``(out [B, n_out], counts [B], buffers)`` as numpy."""
    ts = model(name)
    B, L = wav.shape
    ts._ensure()
    ts._ws(B, L, rate).view(torch.float32).fill_(NAN)
    t = torch.full((B, ts.out_samples(L, rate)), NAN, dtype=torch.float32, device=DEV)   # the block the next torch.empty most likely gets
    torch.cuda.synchronize()
    del t
    out, counts = ts.forward_device(torch.from_numpy(np.array(wav)), rate,
                                    lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy(), {k: v.cpu().numpy() for k, v in ts._read_buffers(B, L, rate).items()}


def same(kind, where, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        bad = D.differing(got, want)
    else:
        assert got.shape == want.shape, (kind, where, got.shape, want.shape)
        bad = int((got != want).sum())
    if bad:
        idx = tuple(np.argwhere(~(got == want))[0])
        raise AssertionError(f"{kind} {where}: {bad} of {got.size} elements differ; first at {idx}: device {got[idx]!r}, restatement {want[idx]!r}")
    SESSION.count(kind, exact=got.size)


def within(kind, where, err, bar):
    """``err <= bar`` element by element; where the bar is 0 the claim is exact and is counted so."""
    over = ~(err <= bar)
    if over.any():
        idx = tuple(np.argwhere(over)[0])
        raise AssertionError(f"{kind} {where}: {int(over.sum())} of {err.size} elements exceed the bar; first at {idx}: error {err[idx]!r}, bar {bar[idx]!r}")
    live = bar > 0
    SESSION.count(kind, exact=int((~live).sum()), frames=int(live.sum()), ratio=float((err[live] / bar[live]).max(initial=0.0)))


def judge(name, clean, wav, rate, lengths, where, silent=False):
    """The four launches of one call on ``wav [B, L]`` (``clean``: the same without the NaN padding), item by item on the
    device's own buffers, then the same call again.  Returns ``(out, buffers)``."""
    cfg, tab = D.TS_CONFIGS[name], D.gl_tables(name)
    d = D.Design(cfg)
    B, L = wav.shape
    T = L // d.hop + 1
    _, T_out, n_out = D.ts_counts(None, T, d.hop, rate)
    out, counts, buf = run(name, wav, rate, lengths)
    assert out.shape == (B, n_out) and buf["c"].shape == (B, T, d.qp) and buf["out_c"].shape == (B, T_out, d.qp), where
    for b in range(B):
        at = f"{where} item {b}"
        Tb, To, n = D.ts_counts(None if lengths is None else lengths[b], T, d.hop, rate)
        assert (buf["frames"][b], buf["frames_out"][b], buf["counts"][b], counts[b]) == (Tb, To, n, n), at
        SESSION.count("Spectrum::item (counts)", exact=4)
        # launch 1: the spectrum
        c, mag, inc, acc, oc = buf["c"][b], buf["mag"][b], buf["inc"][b], buf["acc"][b], buf["out_c"][b]
        assert np.isnan(c[Tb:]).all() and np.isnan(c[:Tb, d.q:]).all(), at
        if Tb:
            same(SPEC, at, c[:Tb, :d.q], D.spectrum_launch(D.window_acc(clean[b, :d.hop * (Tb - 1)], 0, Tb, cfg, tab), cfg))
        # launch 2: the step, on the device's c
        assert np.isnan(mag[To:]).all() and (inc[To:] == NAN_BITS).all() and (acc[To:] == NAN_BITS).all() and np.isnan(oc[To:]).all(), at
        st = D.step_launch(c, Tb, To, rate, cfg)
        got = np.ascontiguousarray(mag[:To])
        diff = ~(got == st["mag"])
        left_out = int((diff & st["tiny"]).sum())
        if (diff & ~st["tiny"]).any():
            same(f"{STEP} mag", at, np.where(st["tiny"], st["mag"], got), st["mag"])
        assert left_out <= (0 if silent else D.DN_TINY_SHARE * got.size) and not np.isnan(got).any(), (at, left_out)
        assert not np.signbit(got[:, d.bins:]).any(), at
        _state["left_out"] += left_out
        SESSION.count(f"{STEP} mag", exact=got.size - left_out)
        within(f"{STEP} inc", at, np.abs(D.ts_unit_diff(inc[:To], st["inc_want"])), st["inc_bar"])
        assert not inc[:To, d.bins:].any(), at
        # launch 3: the scan, on the device's mag, inc and acc[0]
        sc = D.scan_launch(c[0] if Tb else np.zeros(d.q, np.float32), got, inc[:To], To, cfg, acc0=acc[0] if To else np.zeros(d.ks, np.int64))
        same(f"{SCAN} acc", at, acc[:To], sc["acc"])
        if To:
            within(f"{SCAN} acc[0]", at, np.abs(D.ts_unit_diff(acc[0], sc["acc0_want"])), sc["acc0_bar"])
            assert not acc[0, d.bins:].any(), at
        assert not np.isnan(oc[:To]).any(), at
        within(f"{SCAN} out_c", at, np.abs(oc[:To].astype(np.float64) - sc["out_want"]), sc["out_bar"])
        assert not oc[:To, d.q:].any(), at
        # launch 4: the inverse transform bounded by the item's samples, on the device's out_c
        want, written = D.istft_launch(oc, To, T_out, cfg, tab, True, sample_count=n, Ly=n_out)
        assert written.all()
        same(ISTFT, at, out[b], want)
        assert (out[b, n:] == 0).all() and not np.signbit(out[b, n:]).any(), at
        if silent and b == 0:
            assert not got.any() and not oc[:To].any() and not out[b].any(), at
            if not d.taps & (d.taps - 1):
                assert not inc[:To].any() and not acc[:To].any(), at
    again = run(name, wav, rate, lengths)
    assert np.array_equal(again[0], out) and np.array_equal(again[1], counts), where
    assert all(np.array_equal(again[2][k], buf[k], equal_nan=buf[k].dtype == np.float32) for k in buf), where
    return out, buf


# ---- dense -------------------------------------------------------------------------------------------------------------------------
DENSE = D.TS_CASES + (D.TS_HALF,)


@pytest.mark.parametrize("case", DENSE, ids=[D.ts_case_id(c) for c in DENSE])
def test_forward_dense(case):
    name, B, M, rate = case
    wav = D.dn_wave(name, B, M)
    out, _ = judge(name, wav, wav, rate, None, D.ts_case_id(case))
    assert np.isfinite(out).all() and out.any()


def test_small_start_phases():
    """Angles of a few 1e-5 rad in frame 0: the bar of acc[0] is llrintf's own half unit there."""
    name, M, rate = D.TS_SMALL_ANGLES
    wav = D.ts_small_angles(name, M)
    judge(name, wav, wav, rate, None, f"{name} small angles")


# ---- ragged ------------------------------------------------------------------------------------------------------------------------
RAGGED = [(n, M, lengths, rate) for n, M, lengths, rates in D.TS_RAGGED for rate in rates]


@pytest.mark.parametrize("rc", RAGGED, ids=[f"{n}-M{M}-r{rate:.4g}" for n, M, _, rate in RAGGED])
def test_forward_ragged(rc):
    name, M, lengths, rate = rc
    d = D.Design(D.TS_CONFIGS[name])
    clean = D.dn_wave(name, len(lengths), M, seed=30)
    wav = clean.copy()
    for b, m in enumerate(lengths):                              # nothing at or past an item's own samples is read
        wav[b, d.hop * m:] = NAN
    out, buf = judge(name, clean, wav, rate, list(lengths), f"{name} M={M} rate={rate:.4g} ragged")
    for b, m in enumerate(lengths):
        if m < 1:                                                # no frame: nothing written but the counts and a row of +0
            assert all(np.isnan(buf[k][b]).all() for k in ("c", "mag", "out_c")) and (buf["inc"][b] == NAN_BITS).all() and not out[b].any()
            continue
        one, _, alone = run(name, np.ascontiguousarray(clean[b:b + 1, :d.hop * m]), rate)      # the item's batch-of-one call
        Tb, To, n = (int(alone[k][0]) for k in ("frames", "frames_out", "counts"))
        assert (Tb, To, n) == D.ts_counts(m, M + 1, d.hop, rate) and one.shape == (1, n)
        for k, rows in (("c", Tb), ("mag", To), ("inc", To), ("acc", To), ("out_c", To)):
            assert np.array_equal(buf[k][b, :rows], alone[k][0, :rows], equal_nan=True), (name, rate, b, k)
        assert np.array_equal(out[b, :n], one[0])
        SESSION.count("ragged item == its batch-of-one call, per buffer", exact=Tb * d.qp + To * (3 * d.ks + d.qp) + n)


# ---- silence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rate", D.TS_SILENCE, ids=[f"{n}-r{r:.4g}" for n, r in D.TS_SILENCE])
def test_silence(name, rate):
    """atan2f(0, 0) = 0: the bars are 0 wherever both source rows are silent, so the claim is exact there; nothing is NaN."""
    wav = D.ts_silence(name)
    out, buf = judge(name, wav, wav, rate, None, f"{name} rate={rate:.4g} silence", silent=True)
    assert np.isfinite(out).all() and out[1].any() and not buf["acc"][1, 0].any()


# ---- the report --------------------------------------------------------------------------------------------------------------------
def test_report():
    """Runs last: what the session found (RESULTS at the head of this module records what it printed on an MI355X)."""
    for kind, s in sorted(SESSION.stats.items()):
        print(f"{kind}: {s['exact']} elements exact, {s['frames']} within their bar, worst error / bar {s['worst']:.3f}")
    print(f"mag elements with a float64 re^2 + im^2 < 2^-125 left out because the device disagreed there: {_state['left_out']}")
    kinds = {SPEC, f"{STEP} mag", f"{STEP} inc", f"{SCAN} acc", f"{SCAN} acc[0]", f"{SCAN} out_c", ISTFT, "Spectrum::item (counts)"}
    assert kinds <= set(SESSION.stats), kinds - set(SESSION.stats)
    assert all(SESSION.stats[k]["exact"] > 0 for k in kinds - {f"{SCAN} out_c"})
    assert all(SESSION.stats[k]["frames"] > 0 and SESSION.stats[k]["worst"] <= 1.0 for k in (f"{STEP} inc", f"{SCAN} acc[0]", f"{SCAN} out_c"))
