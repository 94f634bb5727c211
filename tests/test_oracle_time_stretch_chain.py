"""The time stretch's part of oracle/dsp_chain_cases.py on the CPU: the per-launch restatements of ``stft_kernel<ts::Spectrum>``,
``ts_step_kernel``, ``ts_scan_kernel`` and ``gl_istft_kernel`` with ``sample_counts`` that tests/test_gpu_time_stretch_chain.py holds
the device to.

* the cases reach what they are there for (T_out 1, below 32, 32, 33, above 64; both ends of the rate; crop and tail live);
* chained from the waveform on the library's tables, ``out`` follows the float64 restatement (tests/time_stretch_restatement.py)
  within ``4 * e32`` and ``mag`` the float64 step on the same spectrum -- e32 as ``time_stretch_cases.e32()`` measures it; the
  fp32 line with numpy's arctan2 lies inside the derived bars of ``inc`` and ``acc[0]``;
* the bars cannot hide a failure: the largest ``inc`` / ``acc[0]`` bar is below 2^19 units, the ``out_c`` bar below
  ``(TS_SINCOSPI_ULP + 1) 2^-23 |mag| + 2^-126``;
* every wrong restatement (the ``ts_`` entries of ``MUTATIONS``) fails against the right one on a committed case -- a barred
  quantity by exceeding its bar.  Dropping ``wrap`` is NOT one of them: ``fixed(x) == fixed(wrap(x))`` modulo 2^32, shown here;
* ``mag`` elements with a subnormal square are at most ``DN_TINY_SHARE`` of every case that is not a silence case;
* ``ts_counts`` is ``out_frames`` / ``out_samples`` of the float64 restatement and the library's ``out_frames_samples`` over a
  sweep.  A half-integer ``L / rate`` cannot occur at the committed rates for ``hop % 4 == 0`` -- 4 L, L / 4, 5 L / 4 are whole
  numbers, 4 L / 5 is a whole number or has a fraction in fifths, and the two irrational rates would have to hit a float64 half
  exactly, which the sweep shows they do not -- but it CAN at an arbitrary rate in [0.25, 4]: ``HALF_CASE`` is the counter-example
  (L = 16, rate = fl(32 / 9): the float64 quotient is exactly 4.5), so half-to-even is the deciding rule there and
  ``ts_n_out_half_up`` is a mutation that case shows;
* the library accepts every config used.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.time_stretch import TimeStretch
from oracle import dsp_chain_cases as D

import time_stretch_cases as C
import time_stretch_restatement as R


def stft_args(name):
    cfg = D.TS_CONFIGS[name]
    return cfg["n_fft"], cfg["hop_length"], cfg["win_length"]


TS_IDS = [D.ts_case_id(c) for c in D.TS_CASES]
HALF_CASE = D.TS_HALF
_state = {}


def rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def forward(key, name, wav, m, rate):
    """One item through the right restatement, computed once."""
    if key not in _state:
        _state[key] = D.ts_forward_np(wav, m, rate, D.TS_CONFIGS[name], D.gl_tables(name))
    return _state[key]


def right(case, b=0):
    name, B, M, rate = case
    return forward(("dense", case, b), name, D.dn_wave(name, B, M)[b], None, rate)


def inputs():
    """Every committed input as ``(key, name, wav [L], m, rate, silence)``, cheapest configs first: the dense cases' first items,
    the half-integer case, the silence cases' items and the ragged cases' items."""
    rows = [(("dense", case, 0), case[0], D.dn_wave(*case[:3])[0], None, case[3], False) for case in D.TS_CASES + (HALF_CASE,)]
    name, M, rate = D.TS_SMALL_ANGLES
    rows.append((("small_angles",), name, D.ts_small_angles(name, M)[0], None, rate, False))
    for name, rate in D.TS_SILENCE:
        rows += [(("silence", name, rate, b), name, y, None, rate, True) for b, y in enumerate(D.ts_silence(name))]
    for name, M, lengths, rates in D.TS_RAGGED:
        wav = D.dn_wave(name, len(lengths), M, seed=30)
        rows += [(("ragged", name, rate, b), name, wav[b], m, rate, False) for rate in rates for b, m in enumerate(lengths)]
    return sorted(rows, key=lambda r: D.TS_CONFIGS[r[1]]["n_fft"] * len(r[2]))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_their_paths():
    d = {name: D.Design(cfg) for name, cfg in D.TS_CONFIGS.items()}
    t_out = {case: D.ts_counts(None, case[2] + 1, d[case[0]].hop, case[3])[1] for case in D.TS_CASES}
    seen = set(t_out.values())
    assert 1 in seen and 32 in seen and 33 in seen and any(1 < t < 32 for t in seen) and any(t > 64 for t in seen)
    assert any(32 < t <= 62 for t in seen)                          # runs of 2 with empty trailing runs
    assert {c[0] for c in D.TS_CASES} == set(D.TS_CONFIGS) > set(D.GL_CONFIGS) and all(c[1] <= 2 and c[2] <= 70 for c in D.TS_CASES)
    assert {c[3] for c in D.TS_CASES} == {1.0, 0.8, 1.25, D.TS_SEMITONE_DOWN, 0.25, 4.0} and D.TS_SEMITONE_DOWN == C.SEMITONE_DOWN
    # the crop and the tail cases are time_stretch_cases's, on its waveforms
    for case in (("default", 2, 32, 0.8), ("default", 2, 39, 1.25)):
        assert case in D.TS_CASES and case in C.CASES and np.array_equal(D.dn_wave(*case[:3]), C.waveform(case))
    hop = d["default"].hop
    assert D.ts_counts(None, 33, hop, 0.8)[2] < hop * (t_out[("default", 2, 32, 0.8)] - 1)
    n, To = D.ts_counts(None, 40, hop, 1.25)[2], t_out[("default", 2, 39, 1.25)]
    assert hop * (To - 1) < n < hop * (To - 1) + d["default"].half + hop
    # a 256-thread block of ts_step_kernel straddles a frame boundary; the last scan block has fewer than 32 live lanes
    assert (d["small"].ks // 4, d["odd_hop"].ks // 4, d["default"].ks // 4) == (9, 13, 129)
    for name, dd in d.items():
        G = dd.ks // 4
        assert 256 % G and 0 < dd.ks % 32 < 32 and max(t for c, t in t_out.items() if c[0] == name) * G > 256, name
    o = d["odd_hop"]
    assert o.n_fft & (o.n_fft - 1) and (o.ks, o.bins) == (52, 49) and o.hop % 8
    # whether the advance is inexact is a matter of n_fft / hop, not of n_fft: odd_hop's is dyadic, three_tap's is not
    inexact = {}
    for name, dd in d.items():
        r = (np.arange(dd.bins) * dd.hop) % dd.n_fft
        truncates = any(int(v) * 2 ** 32 % dd.n_fft for v in r)
        rounds = bool((D.ts_advance(dd)[1].astype(np.float64) * dd.n_fft != r).any())
        assert truncates == rounds == bool(dd.taps & (dd.taps - 1)), name
        inexact[name] = truncates
    assert [n for n, v in inexact.items() if v] == ["three_tap"]
    w = d["wide_hop"]
    assert w.taps == 2 and w.istft_grid_z == 2 and set(((np.arange(w.bins) * w.hop) % w.n_fft).tolist()) == {0, 512}
    for name, M, lengths, rates in D.TS_RAGGED:
        Tb = [D.ts_counts(m, M + 1, d[name].hop, 1.0)[0] for m in lengths]
        assert M in lengths and Tb[1] == 0 and Tb[2] == 2 and {D.K_ROWS, D.K_ROWS + 1} <= set(Tb) and any(2 < t < D.K_ROWS for t in Tb)
        assert min(rates) < 1 < max(rates)
    assert {n for n, _ in D.TS_SILENCE} == set(D.TS_CONFIGS)
    for name in D.TS_CONFIGS:
        quiet, mixed = D.ts_silence(name)
        assert not quiet.any() and not mixed[:d[name].n_fft].any() and mixed.any()


# ---- against the float64 restatement ---------------------------------------------------------------------------------------------
def bars():
    if "bars" not in _state:
        e = C.e32()
        _state["bars"] = {k: 4 * e[k] for k in ("out", "mag")}
    return _state["bars"]


@pytest.mark.parametrize("case", D.TS_CASES, ids=TS_IDS)
def test_chained_forward_follows_the_float64_restatement(case):
    name, B, M, rate = case
    d = D.Design(D.TS_CONFIGS[name])
    for b in range(B):
        got, y = right(case, b), D.dn_wave(name, B, M)[b]
        assert got["counts"] == (M + 1, R.out_frames(M + 1, rate), R.out_samples(d.hop * M, rate))
        e_out = rel(got["out"], R.stretch(y, rate, *stft_args(name)))
        c = got["c"]
        re, im = c[:, 0:2 * d.bins:2], c[:, 1:2 * d.bins:2]
        assert not im[:, 0].any() and not im[:, -1].any() and c.shape[1] == d.q
        e_mag = rel(got["step"]["mag"][:, :d.bins], R.middle(re, im, rate, d.n_fft, d.hop, np.float64)["mag"])
        print(f"{D.ts_case_id(case)} item {b}: out err={e_out:.3e} bar={bars()['out']:.3e}; mag err={e_mag:.3e} bar={bars()['mag']:.3e}")
        assert e_out <= bars()["out"] and e_mag <= bars()["mag"]
        assert not got["step"]["mag"][:, d.bins:].any() and not got["step"]["inc"][:, d.bins:].any()


def test_the_fp32_line_lies_inside_the_derived_bars_and_the_bars_hide_nothing():
    """numpy's fp32 arctan2 stands in for atan2f: the header's line in fp32 stays inside the bars derived for it.  And the
    conditions on the bars: below 2^19 units, below (ulp + 1) 2^-23 |mag| + 2^-126."""
    worst = {"inc": 0.0, "acc0": 0.0, "inc_bar": 0.0, "acc0_bar": 0.0}
    for key, name, wav, m, rate, silent in inputs():
        f = forward(key, name, wav, m, rate)
        st, sc = f["step"], f["scan"]
        for q, err, bar in (("inc", np.abs(D.ts_unit_diff(st["inc"], st["inc_want"])), st["inc_bar"]),
                            ("acc0", np.abs(D.ts_unit_diff(sc["acc0"], sc["acc0_want"])), sc["acc0_bar"])):
            assert (err <= bar).all(), (key, q, float((err - bar).max()))
            if bar.size:
                worst[q + "_bar"] = max(worst[q + "_bar"], float(bar.max()))
                worst[q] = max(worst[q], float((err[bar > 0] / bar[bar > 0]).max(initial=0.0)))
        mag = np.repeat(np.abs(st["mag"].astype(np.float64)), 2, axis=1)
        assert (sc["out_bar"] < (D.TS_SINCOSPI_ULP + 1) * 2.0 ** -23 * mag + 2.0 ** -126 + (mag == 0) * 2.0 ** -140).all(), key
        assert (np.abs(sc["out_c"].astype(np.float64) - sc["out_want"]) <= sc["out_bar"]).all(), key
    print({k: f"{v:.4g}" for k, v in worst.items()})
    assert 0 < worst["inc_bar"] < 2.0 ** 19 and 0 < worst["acc0_bar"] < 2.0 ** 19
    assert all(cfg["n_fft"] <= 4096 for cfg in D.TS_CONFIGS.values())


def test_silence_is_exact_throughout():
    for name, rate in D.TS_SILENCE:
        d = D.Design(D.TS_CONFIGS[name])
        quiet, mixed = (forward(("silence", name, rate, b), name, y, None, rate) for b, y in enumerate(D.ts_silence(name)))
        st, sc = quiet["step"], quiet["scan"]
        assert not quiet["c"].any() and not st["mag"].any() and not st["inc_bar"].any() and not sc["acc0_bar"].any()
        assert np.array_equal(st["inc"].astype(np.float64), np.mod(st["inc_want"], D.TS_UNIT))      # the fp32 line IS the wanted value
        assert not sc["out_want"].any() and sc["out_bar"].max() == D.TS_FLOOR and not quiet["out"].any()
        if not d.taps & (d.taps - 1):
            assert not st["inc"].any() and not sc["acc"].any(), name
        else:
            assert st["inc"][:, :d.bins].any() and sc["acc"].any(), name
        # the mixed item: silent frames in front and in the middle, exact there, and nothing is NaN
        re = mixed["c"][:, 0:2 * d.bins:2]
        dead = ~mixed["c"].any(axis=1)
        assert dead[0] and dead[1:].any() and not dead.all() and np.isfinite(mixed["out"]).all() and mixed["out"].any()
        assert not mixed["scan"]["acc0_bar"].any() and not mixed["scan"]["acc0"].any()
        zero_bar = mixed["step"]["inc_bar"] == 0
        assert zero_bar[:, :d.bins].all(axis=1).any() and np.isfinite(mixed["scan"]["out_want"]).all()
        assert (D.ts_unit_diff(mixed["step"]["inc"], mixed["step"]["inc_want"])[zero_bar] == 0).all()


# ---- what a device test may leave out ---------------------------------------------------------------------------------------------
def test_subnormal_squares_are_rare_outside_the_silence_cases():
    for key, name, wav, m, rate, silent in inputs():
        tiny = forward(key, name, wav, m, rate)["step"]["tiny"][:, :D.Design(D.TS_CONFIGS[name]).bins]
        if not silent and tiny.size:
            share = tiny.sum() / tiny.size                       # a row past the item's last frame is the rule's 0, not a square
            assert share <= D.DN_TINY_SHARE, (key, share)
        elif silent:
            assert tiny.any(), key


# ---- counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.TS_CONFIGS))
def test_counts_are_the_restatement_s_and_the_library_s(name):
    cfg = D.TS_CONFIGS[name]
    hop = cfg["hop_length"]
    assert hop % 4 == 0
    ts = TimeStretch(*stft_args(name))
    rates = sorted({c[3] for c in D.TS_CASES} | {HALF_CASE[3], 1.5})
    for M in list(range(0, 75)) + [499, 1000]:
        L = hop * M
        for rate in rates:
            Tb, To, n = D.ts_counts(None, M + 1, hop, rate)
            assert (To, n) == (R.out_frames(M + 1, rate), R.out_samples(L, rate)), (M, rate)
            if M:
                assert (To, n) == ts.out_frames_samples(L, rate), (M, rate)
            assert D.ts_counts(M, M + 5, hop, rate) == ((M + 1 if M else 0), (To if M else 0), (n if M else 0))
            q = np.float64(L) / np.float64(rate)
            if rate != HALF_CASE[3]:
                assert q - np.floor(q) != 0.5, (M, rate)             # half to even never decides at a committed rate
    assert ts.launch_count(1, hop * 4, 1.25) == 4                     # the library accepts the config


def test_a_half_integer_quotient_exists_at_another_rate_and_is_a_case():
    name, B, M, rate = HALF_CASE
    hop = D.TS_CONFIGS[name]["hop_length"]
    assert np.float64(hop * M) / np.float64(rate) == 4.5 and 0.25 <= rate <= 4.0
    assert D.ts_counts(None, M + 1, hop, rate) == (2, 1, 4) and D.ts_counts(None, M + 1, hop, rate, "ts_n_out_half_up")[2] == 5
    assert TimeStretch(*stft_args(name)).out_frames_samples(hop * M, rate) == (1, 4)
    assert HALF_CASE in [r[0][1] for r in inputs() if r[0][0] == "dense"]


# ---- an equivalent form ----------------------------------------------------------------------------------------------------------------
def test_dropping_wrap_is_the_same_restatement():
    """fixed(x) == fixed(x - rintf(x)) modulo 2^32 for every fp32 x a difference of three turns can be: x - rintf(x) is exact, the
    product by 2^32 is exact, and rint commutes with adding a multiple of 2^32."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-2.0, 2.0, 200000), rng.uniform(-2.0 ** -9, 2.0 ** -9, 50000), rng.uniform(-2.0 ** -30, 2.0 ** -30, 50000),
                        [0.5, -0.5, 1.5, -1.5, 0.0, 1.0, -1.0, 2.0 ** -33, -(2.0 ** -33), 0.75, 1.25]]).astype(np.float32)
    w = x - np.rint(x)
    assert np.array_equal(w.astype(np.float64), x.astype(np.float64) - np.rint(x.astype(np.float64)))        # exact
    assert np.array_equal(D.ts_fixed(x), D.ts_fixed(w))
    case = ("odd_hop", 1, 34, 0.8)
    f = right(case)
    again = D.step_launch(f["c"], *f["counts"][:2], case[3], D.TS_CONFIGS[case[0]], "ts_no_wrap")
    assert np.array_equal(again["inc"], f["step"]["inc"]) and "ts_no_wrap" not in D.MUTATIONS


# ---- wrong restatements ------------------------------------------------------------------------------------------------------------
EXACT_STEP = ("ts_alpha_f32", "ts_lerp_fma_swapped", "ts_mag_fma_re", "ts_mag_fma_im", "ts_row_past_end_kept")
BARRED_INC = ("ts_adv_no_modulo", "ts_adv_fixed_rounded", "ts_row_past_end_kept")
BARRED_START = ("ts_start_phase_0", "ts_fixed_truncated")
BARRED_OUT_C = ("ts_unfixed_u32", "ts_sin_cos_swapped")
ISTFT = ("ts_tail_dropped", "ts_istft_item_rule", "ts_sample_count_ignored")
TS_PAIRS = [("mag", m) for m in EXACT_STEP] + [("inc", m) for m in BARRED_INC] + [("acc0", m) for m in BARRED_START] + \
           [("acc", "ts_scan_inclusive")] + [("out_c", m) for m in BARRED_OUT_C] + [("c", "ts_nyquist_im_kept")] + \
           [("counts", "ts_n_out_truncated"), ("counts", "ts_n_out_half_up")] + [("out", m) for m in ISTFT]


def ts_fails(kind, mut, key, name, wav, m, rate):
    """Whether the wrong restatement, given the launch's right inputs, misses the right one: by a differing element where the
    claim is exact, by exceeding the bar where there is one."""
    cfg, tab = D.TS_CONFIGS[name], D.gl_tables(name)
    d = D.Design(cfg)
    f = forward(key, name, wav, m, rate)
    Tb, To, n = f["counts"]
    T = len(wav) // d.hop + 1
    if kind == "counts":
        return D.ts_counts(m, T, d.hop, rate, mut) != f["counts"]
    if not Tb:
        return False
    if kind == "c":
        return not np.array_equal(D.spectrum_launch(f["acc"], cfg, mut), f["c"])
    st, sc = f["step"], f["scan"]
    if kind in ("mag", "inc"):
        bad = D.step_launch(f["c"], Tb, To, rate, cfg, mut)
        if kind == "mag":
            return not np.array_equal(bad["mag"], st["mag"])
        return bool((np.abs(D.ts_unit_diff(bad["inc"], st["inc_want"])) > st["inc_bar"]).any())
    if kind in ("acc0", "acc", "out_c"):
        bad = D.scan_launch(f["c"][0], st["mag"], st["inc"], To, cfg, acc0=sc["acc0"] if kind != "acc0" else None, mut=mut)
        if kind == "acc0":
            return bool((np.abs(D.ts_unit_diff(bad["acc0"], sc["acc0_want"])) > sc["acc0_bar"]).any())
        if kind == "acc":
            return not np.array_equal(bad["acc"], sc["acc"])
        return bool((np.abs(bad["out_c"].astype(np.float64) - sc["out_want"]) > sc["out_bar"]).any())
    _, T_out, n_out = D.ts_counts(None, T, d.hop, rate)
    bad = D.istft_launch(sc["out_c"], To, T_out, cfg, tab, True, mut, sample_count=n, Ly=n_out)[0]
    return not np.array_equal(bad, f["out"])


@pytest.mark.parametrize("kind,mut", TS_PAIRS, ids=[f"{k}-{m}" for k, m in TS_PAIRS])
def test_mutation_fails(kind, mut):
    """A wrong restatement must miss the right one on at least one committed input (cheapest first; the first that shows it ends
    the search).  tests/test_oracle_dsp_chain.py::test_every_mutation_is_tried_somewhere counts these pairs in."""
    for key, name, wav, m, rate, silent in inputs():
        if ts_fails(kind, mut, key, name, wav, m, rate):
            print(f"{kind} {mut}: visible at {key[:1] + key[1:]}")
            return
    pytest.fail(f"{mut} is invisible in {kind} on every committed input")


def test_where_the_one_unit_mutations_show():
    """A rounded advance_fixed and a truncated ``fixed`` move a value by one unit, far inside the bar of a live bin.  They show
    where the bar is 0 or below one unit: the first in three_tap's digital silence (the claim there is exact; at odd_hop, whose
    advance is dyadic, it is an equivalent form), the second at a start phase whose angle is small enough that the bar is
    llrintf's own half unit."""
    name = "three_tap"
    key = ("silence", name, 0.8, 0)
    assert ts_fails("inc", "ts_adv_fixed_rounded", key, name, D.ts_silence(name)[0], None, 0.8)
    name, M, rate = D.TS_SMALL_ANGLES
    wav = D.ts_small_angles(name, M)[0]
    sc = forward(("small_angles",), name, wav, None, rate)["scan"]
    even = np.arange(2, D.Design(D.TS_CONFIGS[name]).half, 2)
    assert (sc["acc0_bar"][even] < 0.75).all() and (np.abs(sc["acc0_want"][even]) < 2.0 ** 23).all()
    assert ts_fails("acc0", "ts_fixed_truncated", ("small_angles",), name, wav, None, rate)
    for case in (("three_tap", 1, 34, 0.8), ("odd_hop", 1, 34, 0.8)):
        assert not ts_fails("inc", "ts_adv_fixed_rounded", ("dense", case, 0), case[0], D.dn_wave(*case[:3])[0], None, 0.8)
    assert not ts_fails("inc", "ts_adv_fixed_rounded", ("silence", "odd_hop", 0.8, 0), "odd_hop", D.ts_silence("odd_hop")[0], None, 0.8)
