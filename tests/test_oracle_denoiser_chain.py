"""The bias denoiser's part of oracle/dsp_chain_cases.py on the CPU: the per-launch restatements of ``dn_stft_kernel<subtract>``,
``dn_stft_kernel<magnitude>``, ``dn_bias_reduce_kernel`` and ``dn::Window`` that tests/test_gpu_denoiser_chain.py holds the
device to, bit for bit.

* ``window_acc`` at origin 0 is ``update_acc`` bit for bit, and at another origin it is the same rows of the whole utterance;
* the chained forward and the chained bias estimate, on the library's tables, agree with the float64 restatement
  (tests/denoiser_restatement.py) within ``4 * e32`` -- e32 as ``denoiser_cases.e32()`` measures it;
* every wrong restatement (the ``dn_`` entries of ``MUTATIONS``) differs from the right one on at least one case;
* the cases are live: clamped and unclamped elements in every item at ``DN_STRENGTH``, ``mag == 0`` in the silence cases,
  ``scale == 1.0`` and ``scale == 0`` side by side under the forced bias;
* the elements a device test may leave out (float64 re^2 + im^2 below 2^-125) are at most 0.1 % of a case's stored elements;
* ``dn_window`` is ``Denoiser.window_range`` over a sweep; the library accepts every config and the readers' layout is the
  workspace's.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.denoiser import Denoiser
from oracle import dsp_chain_cases as D

import denoiser_cases as C
import denoiser_restatement as R

PLAIN = {"mag": 0}
DN_IDS = [f"{n}-B{B}-M{M}" for n, B, M in D.DN_CASES]
_state = {}


def rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def right(case, b=0, strength=D.DN_STRENGTH):
    """Item b of a dense case through the right restatement, computed once."""
    key = (case, b, strength)
    if key not in _state:
        name, B, M = case
        _state[key] = D.dn_forward_np(D.dn_wave(name, B, M)[b], None, C.bias(case), strength, D.GL_CONFIGS[name], D.gl_tables(name), PLAIN)
    return _state[key]


def silence(name):
    """Both items of a config's silence case through the right restatement."""
    if ("silence", name) not in _state:
        cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
        _state[("silence", name)] = [D.dn_forward_np(y, None, C.config_bias(name), D.DN_STRENGTH, cfg, tab, PLAIN) for y in D.dn_silence(name)]
    return _state[("silence", name)]


# ---- the cases and their inputs ------------------------------------------------------------------------------------------------
def test_cases_reach_their_paths_and_share_their_inputs():
    d = {name: D.Design(cfg) for name, cfg in D.GL_CONFIGS.items()}
    frames = lambda name: {M + 1 for n, _, M in D.DN_CASES if n == name}
    assert 33 in frames("default") and d["default"].update_grid_z == 4 and len(d["default"].slices) == 5
    assert frames("small") == {3, 70} and d["small"].taps == 4
    assert d["two_tap"].taps == 2 and 34 in frames("two_tap")
    o = d["odd_hop"]
    assert o.hop % 8 and o.cp == 16 > o.hop and (o.ks, o.bins) == (52, 49) and frames("odd_hop") == {3, 35}
    w = d["wide_hop"]
    assert w.taps == 2 and w.hop_tiles == 16 and w.istft_grid_z == 2 and frames("wide_hop") == {3, 34}
    assert set(D.GL_CONFIGS) == {n for n, _, _ in D.DN_CASES}
    for name, M, lengths in D.DN_RAGGED:
        Tb = [D.dn_item_frames(m, M + 1) for m in lengths]
        assert M in lengths and Tb[1] == 0 and Tb[2] == 2 and D.K_ROWS in Tb and any(1 < t < D.K_ROWS for t in Tb), (name, Tb)
    for name, M, m0, Mw, final in D.DN_WINDOWS:
        f_lo, f_hi, lo, count = D.dn_window(D.GL_CONFIGS[name], m0, Mw, final)
        assert count > 0 and m0 + Mw <= M and final == (m0 + Mw == M)
    assert {(n, bool(m0), f) for n, _, m0, _, f in D.DN_WINDOWS} >= {(n, True, f) for n in ("default", "odd_hop", "two_tap") for f in (False, True)}
    # the waveforms are denoiser_cases's, sample for sample; the configs of the two modules are the same dicts
    for case in C.CASES:
        assert np.array_equal(D.dn_wave(*case), C.waveform(case)), case
    assert all(C.CONFIGS[n] == cfg for n, cfg in D.GL_CONFIGS.items())
    assert D.DN_STRENGTH == C.STRENGTH


@pytest.mark.parametrize("case", D.DN_CASES, ids=DN_IDS)
def test_window_acc_at_origin_0_is_update_acc(case):
    name, B, M = case
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    for y in D.dn_wave(name, B, M):
        assert np.array_equal(D.window_acc(y, 0, M + 1, cfg, tab), D.update_acc(y, M + 1, cfg, tab))


@pytest.mark.parametrize("w", [w for w in D.DN_WINDOWS if w[0] != "default"], ids=lambda w: "-".join(str(v) for v in w))
def test_window_acc_at_another_origin_is_the_utterance_s_rows(w):
    """A computable frame reads only samples inside the window (or past an end of the utterance, 0 in both), so the window
    form reproduces rows [f_lo, f_hi) of the whole utterance's transform bit for bit -- and an origin off by one hop does not."""
    name, M, m0, Mw, final = w
    cfg, tab, hop = D.GL_CONFIGS[name], D.gl_tables(name), D.GL_CONFIGS[name]["hop_length"]
    y = D.dn_wave(name, 1, M)[0]
    f_lo, f_hi, _, _ = D.dn_window(cfg, m0, Mw, final)
    whole = D.window_acc(y, 0, M + 1, cfg, tab)
    win = y[hop * m0:hop * (m0 + Mw)]
    assert np.array_equal(D.window_acc(win, hop * (f_lo - m0), f_hi - f_lo, cfg, tab), whole[f_lo:f_hi])
    assert not np.array_equal(D.window_acc(win, hop * (f_lo - m0), f_hi - f_lo, cfg, tab, "dn_window_origin_shift"), whole[f_lo:f_hi])


@pytest.mark.parametrize("name", list(D.GL_CONFIGS))
def test_dn_window_is_window_range(name):
    cfg = D.GL_CONFIGS[name]
    dn = Denoiser(*C.stft_args(name))
    hop, seen = cfg["hop_length"], 0
    for m0 in range(0, 13):
        for Mw in range(0, 15):
            for final in (False, True):
                f_lo, f_hi, lo, count = D.dn_window(cfg, m0, Mw, final)
                assert (lo, count) == dn.window_range(hop * m0, hop * Mw, final), (m0, Mw, final)
                assert 0 <= f_hi - f_lo <= Mw + 1
                if count:                                    # what window_slice relies on
                    assert hop * f_lo <= lo and lo + count - hop * f_lo <= hop * (f_hi - f_lo - 1), (m0, Mw, final)
                    seen += 1
    assert seen > 100


# ---- against the float64 restatement ---------------------------------------------------------------------------------------------
def bars():
    if "bars" not in _state:
        e = C.e32()
        _state["bars"] = {k: 4 * e[k] for k in ("out", "bias")}
    return _state["bars"]


@pytest.mark.parametrize("case", D.DN_CASES, ids=DN_IDS)
def test_chained_forward_follows_the_float64_restatement(case):
    name, B, M = case
    for b in range(B):
        got = right(case, b)
        want = R.denoise(D.dn_wave(name, B, M)[b], C.bias(case), D.DN_STRENGTH, *C.stft_args(name))
        err = rel(got["out"], want)
        print(f"{name} M={M} item {b}: out err={err:.3e} bar={bars()['out']:.3e}")
        assert got["frames"] == M + 1 and err <= bars()["out"]


def has_interior(case):
    lo, hi = D.dn_interior(D.GL_CONFIGS[case[0]], case[2] + 1)
    return hi > lo


@pytest.mark.parametrize("case", [c for c in D.DN_CASES if has_interior(c)], ids=[i for c, i in zip(D.DN_CASES, DN_IDS) if has_interior(c)])
def test_chained_bias_estimate_follows_the_float64_restatement(case):
    name, B, M = case
    cfg, y = D.GL_CONFIGS[name], D.dn_wave(name, B, M)[0]
    mag, bias = D.dn_estimate_np(y, cfg, D.gl_tables(name), PLAIN)
    lo, hi = D.dn_interior(cfg, M + 1)
    assert (lo, hi) == R.interior(M + 1, cfg["n_fft"], cfg["hop_length"]) and hi > lo
    err = rel(bias, R.estimate_bias(y, *C.stft_args(name)))
    print(f"{name} M={M}: bias err={err:.3e} bar={bars()['bias']:.3e}")
    assert err <= bars()["bias"]
    # the sum is sequential: numpy's own float64 accumulation in ascending t gives the same bits
    assert np.array_equal(bias, (np.add.accumulate(mag[lo:hi].astype(np.float64), axis=0)[-1] / (hi - lo)).astype(np.float32))


def test_cases_without_an_interior_frame_are_the_ones_left_out():
    """Fewer frames than taps leaves no interior frame -- except at two taps, where frame 1 of 3 is one."""
    assert [c for c in D.DN_CASES if not has_interior(c)] == [("small", 1, 2), ("odd_hop", 1, 2)]
    assert D.dn_interior(D.GL_CONFIGS["wide_hop"], 3) == (1, 2)
    for case in D.DN_CASES:
        dn = Denoiser(*C.stft_args(case[0]))
        if has_interior(case):
            assert dn.estimate_launch_count(D.GL_CONFIGS[case[0]]["hop_length"] * case[2]) == 2
        else:
            with pytest.raises(Exception):
                dn.estimate_launch_count(D.GL_CONFIGS[case[0]]["hop_length"] * case[2])


# ---- live branches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.DN_CASES, ids=DN_IDS)
def test_both_clamp_branches_are_live_in_every_item(case):
    name, B, M = case
    d = D.Design(D.GL_CONFIGS[name])
    for b in range(B):
        acc = right(case, b)["acc"]
        re, im, _ = D.dn_parts(acc, d)
        scale, g, mag = D.subtract_scale(re, im, C.bias(case)[None, :d.half], D.DN_STRENGTH, PLAIN)
        assert (g == 0).any() and (g > 0).any(), (case, b)
        assert ((scale > 0) & (scale < 1)).any()


@pytest.mark.parametrize("rc", D.DN_RAGGED, ids=[f"{n}-M{M}" for n, M, _ in D.DN_RAGGED])
def test_a_ragged_item_is_its_stand_alone_forward_and_both_branches_are_live(rc):
    name, M, lengths = rc
    cfg, tab, bias = D.GL_CONFIGS[name], D.gl_tables(name), C.config_bias(name)
    d = D.Design(cfg)
    wav = D.dn_wave(name, len(lengths), M, seed=30)
    for b, m in enumerate(lengths):
        rag = D.dn_forward_np(wav[b], m, bias, D.DN_STRENGTH, cfg, tab, PLAIN)
        assert rag["frames"] == (m + 1 if m else 0) and (rag["out"][d.hop * m:] == 0).all()
        if m:
            alone = D.dn_forward_np(wav[b][:d.hop * m], None, bias, D.DN_STRENGTH, cfg, tab, PLAIN)
            assert np.array_equal(rag["c"], alone["c"]) and np.array_equal(rag["out"][:d.hop * m], alone["out"])
            g = D.subtract_scale(*D.dn_parts(rag["acc"], d)[:2], bias[None, :d.half], D.DN_STRENGTH, PLAIN)[1]
            assert (g == 0).any() and (g > 0).any(), (name, b)


@pytest.mark.parametrize("name", list(D.GL_CONFIGS))
def test_silence_cases_have_exact_zero_magnitudes(name):
    d = D.Design(D.GL_CONFIGS[name])
    quiet, mixed = silence(name)
    assert (quiet["acc"] == 0).all() and (quiet["c"] == 0).all() and (quiet["out"] == 0).all()
    re, im, nyq = D.dn_parts(mixed["acc"], d)
    mag = np.sqrt(D.sum_sq(re, im, 0))
    dead = (mag == 0).all(axis=1)
    assert dead.any() and (mag > 0).all(axis=1).any() and not dead[0] and not dead[-1]
    assert (mixed["c"][dead] == 0).all() and np.isfinite(mixed["c"]).all() and np.isfinite(mixed["out"]).all()
    assert np.abs(mixed["out"]).max() > 0
    # the guard is what keeps them finite
    bad = D.subtract_launch(mixed["acc"], C.config_bias(name), D.DN_STRENGTH, D.GL_CONFIGS[name], PLAIN, "dn_scale_unguarded")
    assert np.isnan(bad[dead]).any()


@pytest.mark.parametrize("name", list(D.GL_CONFIGS))
def test_forced_bias_gives_scale_one_beside_scale_zero(name):
    case = next(c for c in D.DN_CASES if c[0] == name and c[2] == D.dn_case_m(name))
    d = D.Design(D.GL_CONFIGS[name])
    forced = D.dn_forced_bias(C.bias(case))
    assert forced[0] == 0 and forced[d.half] == 0 and forced[2] == np.float32(1e30) and np.array_equal(forced[1::2], C.bias(case)[1::2])
    acc = right(case)["acc"]
    re, im, nyq = D.dn_parts(acc, d)
    scale, _, mag = D.subtract_scale(re, im, forced[None, :d.half], D.DN_STRENGTH, PLAIN)
    assert (mag > 0).all() and (scale[:, 0::4] == 1.0).all() and (scale[:, 2::4] == 0).all()
    c = D.subtract_launch(acc, forced, D.DN_STRENGTH, D.GL_CONFIGS[name], PLAIN)
    assert np.array_equal(c[:, 0:2 * d.half:8], re[:, 0::4]) and (c[:, 4:2 * d.half:8] == 0).all() and np.array_equal(c[:, 2 * d.half], nyq)


# ---- what a device test may leave out ---------------------------------------------------------------------------------------------
def tiny_share(acc, cfg):
    tiny = D.dn_tiny(acc, cfg)
    return tiny.sum() / tiny.size


def test_subnormal_squares_are_rare_outside_the_silence_cases():
    for case in D.DN_CASES:
        for b in range(case[1]):
            share = tiny_share(right(case, b)["acc"], D.GL_CONFIGS[case[0]])
            assert share <= D.DN_TINY_SHARE, (case, b, share)
    for name, M, lengths in D.DN_RAGGED:
        cfg, wav = D.GL_CONFIGS[name], D.dn_wave(name, len(lengths), M, seed=30)
        for b, m in enumerate(lengths):
            if m:
                assert tiny_share(D.window_acc(wav[b][:cfg["hop_length"] * m], 0, m + 1, cfg, D.gl_tables(name)), cfg) <= D.DN_TINY_SHARE
    for name, M, m0, Mw, final in D.DN_WINDOWS:
        cfg, hop = D.GL_CONFIGS[name], D.GL_CONFIGS[name]["hop_length"]
        f_lo, f_hi, _, _ = D.dn_window(cfg, m0, Mw, final)
        for y in D.dn_wave(name, 2, M, seed=40):
            acc = D.window_acc(y[hop * m0:hop * (m0 + Mw)], hop * (f_lo - m0), f_hi - f_lo, cfg, D.gl_tables(name))
            assert tiny_share(acc, cfg) <= D.DN_TINY_SHARE, (name, m0)
            d = D.Design(cfg)                                 # and a window's items have both branches of the clamp live too
            g = D.subtract_scale(*D.dn_parts(acc, d)[:2], C.config_bias(name)[None, :d.half], D.DN_STRENGTH, PLAIN)[1]
            assert (g == 0).any() and (g > 0).any(), (name, m0)
    # the silence cases are all about them
    assert all(tiny_share(silence(name)[1]["acc"], D.GL_CONFIGS[name]) > D.DN_TINY_SHARE for name in D.GL_CONFIGS)


# ---- the library accepts the configs; the readers' layout -----------------------------------------------------------------------
@pytest.mark.parametrize("case", D.DN_CASES, ids=DN_IDS)
def test_configs_are_accepted_and_the_layout_is_the_workspace(case):
    name, B, M = case
    dn, d = Denoiser(*C.stft_args(name)), D.Design(D.GL_CONFIGS[name])
    L = d.hop * M
    assert dn.launch_count(B, L) == 2
    if has_interior(case):
        assert dn.estimate_launch_count(L) == 2
    layout, floats = dn._workspace_layout(B, L)
    assert max(4 * floats, 256) == dn.workspace_bytes(B, L)
    assert layout["c"] == (0, (B, M + 1, d.qp)) and layout["frames"] == ((B * (M + 1) * d.qp + 63) // 64 * 64, (B,))
    assert 4 * (M + 1) * d.ks <= dn.workspace_bytes(1, L) and d.ks == (dn.n_bins + 3) // 4 * 4       # _read_mag's rows fit


# ---- wrong restatements ------------------------------------------------------------------------------------------------------------
SUBTRACT_MUTS = ("dn_fma_unfused", "dn_divide_last", "dn_im_sign", "dn_nyquist_bias0", "dn_nyquist_im_kept")
ESTIMATE_MUTS = ("dn_bias_sum_f32", "dn_bias_pairwise", "dn_interior_wide", "dn_mean_over_all_frames")
DN_PAIRS = [("subtract", m) for m in SUBTRACT_MUTS] + [("silence", "dn_scale_unguarded")] + [("estimate", m) for m in ESTIMATE_MUTS] + \
           [("ragged", "dn_frames_extra0"), ("window", "dn_window_origin_shift")]
DN_BY_COST = sorted(D.DN_CASES, key=lambda c: D.GL_CONFIGS[c[0]]["n_fft"] * c[2])


def dn_differs(kind, case, mut):
    name, B, M = case
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    if kind == "subtract":
        # at strength 1 the product strength * bias is exact and fused or not is the same number: 0.1 is what tells them apart
        acc = right(case)["acc"]
        return any(not np.array_equal(D.subtract_launch(acc, C.bias(case), s, cfg, PLAIN), D.subtract_launch(acc, C.bias(case), s, cfg, PLAIN, mut))
                   for s in D.DN_STRENGTHS)
    if kind == "silence":
        acc = silence(name)[1]["acc"]
        return D.differing(D.subtract_launch(acc, C.config_bias(name), D.DN_STRENGTH, cfg, PLAIN, mut), silence(name)[1]["c"]) > 0
    y = D.dn_wave(name, B, M)[0]
    if kind == "estimate":
        return has_interior(case) and not np.array_equal(D.dn_estimate_np(y, cfg, tab, PLAIN)[1], D.dn_estimate_np(y, cfg, tab, PLAIN, mut)[1])
    if kind == "ragged":
        m = M // 2
        runs = [D.dn_forward_np(y, m, C.bias(case), D.DN_STRENGTH, cfg, tab, PLAIN, mu) for mu in (None, mut)]
        return runs[0]["frames"] != runs[1]["frames"] and not np.array_equal(runs[0]["out"], runs[1]["out"])
    return not np.array_equal(D.window_acc(y, 0, M + 1, cfg, tab), D.window_acc(y, 0, M + 1, cfg, tab, mut))


@pytest.mark.parametrize("kind,mut", DN_PAIRS, ids=[f"{k}-{m}" for k, m in DN_PAIRS])
def test_mutation_fails(kind, mut):
    """A wrong restatement must differ from the right one on at least one case (cheapest cases first; the first that shows it
    ends the search).  tests/test_oracle_dsp_chain.py::test_every_mutation_is_tried_somewhere counts these pairs in."""
    for case in DN_BY_COST:
        if dn_differs(kind, case, mut):
            print(f"{kind} {mut}: visible at {case}")
            return
    pytest.fail(f"{mut} is invisible in {kind} on every case")


def test_the_contraction_sites_are_distinguishable():
    """The three roundings of re re + im im give different c and different magnitudes on the cases, so a device run can tell
    which one a kernel took -- and whether the two instantiations took the same."""
    case = ("small", 1, 69)
    cfg, acc = D.GL_CONFIGS[case[0]], right(case)["acc"]
    cs = [D.subtract_launch(acc, C.bias(case), D.DN_STRENGTH, cfg, fma) for fma in D.assignments(D.DN_SITES)]
    ms = [D.magnitude_launch(acc, cfg, fma) for fma in D.assignments(D.DN_SITES)]
    assert len(cs) == 3
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(cs[i], cs[j]) and not np.array_equal(ms[i], ms[j])
