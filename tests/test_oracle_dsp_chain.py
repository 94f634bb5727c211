"""oracle/dsp_chain_cases.py on the CPU: the per-launch restatements of the mel front-end and of Griffin-Lim that
tests/test_gpu_dsp_chain.py holds the device to, bit for bit.

* every restatement, fed with its own outputs, agrees with the independent float64 restatements (tests/mel_restatement.py,
  tests/griffin_lim_restatement.py) within ``4 * e32`` -- e32 as ``mel_cases.e32_of`` over ``mel_cases.accuracy_cases()`` and
  ``griffin_lim_cases.e32()`` measure it;
* every wrong restatement (``MUTATIONS``) differs from the right one, on the right one's own tensors, in every launch it touches;
* ``GriffinLim._read_buffers``'s layout is pinned to ``workspace_bytes``, and the library accepts every config;
* the decided-element rule leaves out no frame of any case;
* the cases reach the kernel paths the cases table names.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.griffin_lim import pack_phase
from iris.mel import MelFrontend
from oracle import dsp_chain_cases as D

import griffin_lim_cases as GC
import griffin_lim_restatement as G
import mel_cases as MC
import mel_restatement as M

PLAIN = {"mag": 0, "nnls": 0, "alpha": 0, "den": 0}
GL_IDS = [D.case_id(c) for c in D.GL_CASES]
_state = {}


def rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def right(case, seed=D.GL_SEEDS[0], b=0):
    """The two-pass forward of the right restatement, computed once."""
    key = (case, seed, b)
    if key not in _state:
        name = case[0]
        _state[key] = D.forward_np(D.gl_logmel(case)[b], pack_phase(D.gl_phase(case, seed))[b], D.GL_CONFIGS[name], D.gl_tables(name), 2, PLAIN)
    return _state[key]


# ---- the cases reach what their table says --------------------------------------------------------------------------------------
def test_cases_reach_their_paths():
    d = {name: D.Design(cfg) for name, cfg in D.GL_CONFIGS.items()}
    assert [w for _, w in d["default"].slices] == [256, 256, 256, 256, 8] and d["default"].update_grid_z == 4
    assert d["default"].istft_grid_z == 1 and any(T > D.K_ROWS for n, _, T in D.GL_CASES if n == "default")
    assert d["small"].win < d["small"].n_fft and d["small"].slices == [(0, 72)] and 72 // 8 == 8 + 1
    assert d["small"].taps == 4 and {T for n, _, T in D.GL_CASES if n == "small"} == {3, 70}
    assert d["two_tap"].taps == 2
    o = d["odd_hop"]
    assert o.hop % 8 and o.cp == 16 > o.hop and o.mp == 8 > o.n_mels and (o.ks, o.bins) == (52, 49) and o.win < o.n_fft
    assert o.qp - o.q > 2 and o.ks != o.bins
    w = d["wide_hop"]
    assert w.hop_tiles == 16 and w.istft_grid_z == 2 and w.hop > 256
    assert all(T <= 70 for _, _, T in D.GL_CASES) and all(T <= 70 for _, T, _ in D.GL_RAGGED)
    for name, T, lengths in D.GL_RAGGED:
        assert T in lengths and 0 in lengths and 1 in lengths and any(n % D.K_ROWS == 0 and n for n in lengths)
        assert any(n % D.K_ROWS and 1 < n < T for n in lengths)
    m = {name: D.Design(cfg) for name, cfg in D.MEL_CONFIGS.items()}
    assert m["odd_hop"].cp > m["odd_hop"].hop and m["small"].win < m["small"].n_fft and D.MEL_CONFIGS["small"]["fmin"] == 50.0
    assert {1 + L // m[n].hop for n, _, L in D.MEL_CASES if n == "odd_hop"} == {3, 35}
    for name, L, ns in D.MEL_RAGGED:
        frames = [1 + n // m[name].hop for n in ns]
        assert 1 + L // m[name].hop in frames and 0 in ns and 1 in ns and D.K_ROWS in frames and any(1 < f < D.K_ROWS for f in frames)


# ---- the library accepts the configs; the reader's layout ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.GL_CONFIGS))
def test_configs_are_accepted_and_the_layout_is_the_workspace(name):
    shapes = {(B, T) for n, B, T in D.GL_CASES if n == name} | {(len(L), T) for n, T, L in D.GL_RAGGED if n == name}
    for n_iter in (0, 2):
        gl = D.gl_model(name, n_iter=n_iter)
        for B, T in sorted(shapes):
            assert gl.launch_count(B, T) == 2 * n_iter + 2
            layout, floats = gl._workspace_layout(B, T)
            assert max(4 * floats, 256) == gl.workspace_bytes(B, T), (B, T)
            d = D.Design(D.GL_CONFIGS[name])
            assert [layout[k][1] for k in ("S", "c", "r", "y")] == [(B, T, d.ks), (B, T, d.qp), (B, T, d.qp), (B, d.hop * (T - 1))]
            offs = [layout[k][0] for k in ("S", "c", "r", "y")]
            assert offs == sorted(offs) and all(o % 64 == 0 for o in offs) and offs[0] == 0


@pytest.mark.parametrize("name", list(D.MEL_CONFIGS))
def test_mel_configs_are_accepted(name):
    fe = MelFrontend(**D.MEL_CONFIGS[name])
    for n, B, L in D.MEL_CASES:
        if n == name:
            assert fe.launch_count(B, L) == 1


# ---- against the float64 restatements -----------------------------------------------------------------------------------------
def mel_bar():
    if "mel_bar" not in _state:
        _state["mel_bar"] = 4 * max(MC.e32_of(name, x) for name, x in MC.accuracy_cases())
    return _state["mel_bar"]


@pytest.mark.parametrize("case", D.MEL_CASES, ids=[f"{n}-B{B}-L{L}" for n, B, L in D.MEL_CASES])
def test_mel_chain_follows_the_float64_restatement(case):
    name, B, L = case
    cfg, tab = D.MEL_CONFIGS[name], D.mel_tables(name)
    undecided = 0
    for seed in D.MEL_SEEDS:
        audio = D.mel_audio(name, B, L, seed)
        for form in (audio, D.to_int16(audio)):
            for b in range(B):
                got, frames, ok = D.mel_launch(form[b], L, None, cfg, tab, PLAIN)
                err = rel(got, M.mel_np(D.mel_samples(form[b]), **cfg))
                print(f"{name} L={L} seed={seed} {form.dtype} item {b}: err={err:.3e} bar={mel_bar():.3e}")
                assert frames == 1 + L // cfg["hop_length"] and err <= mel_bar()
                undecided += int((~ok).sum())
    assert undecided == 0


def test_mel_exact_zero_frames_and_the_ragged_form():
    name, L, ns = D.MEL_RAGGED[0]
    cfg, tab = D.MEL_CONFIGS[name], D.mel_tables(name)
    x = D.mel_audio(name, 1, L, 0)[0]
    got, _, ok = D.mel_launch(x, L, None, cfg, tab, PLAIN)
    zf = MC.zero_frames(L, cfg)
    assert zf and (got[:, zf] == D.LOG_CLIP).all() and ok.all()
    for n, cap in zip(ns, (None, None, 0, 9, None)):
        rag, frames, ok = D.mel_launch(x, n, cap, cfg, tab, PLAIN)
        own = min(1 + n // cfg["hop_length"], 10 ** 9 if cap is None else cap)
        assert frames == own and (rag[:, own:] == 0).all() and ok.all()
        if own:
            alone = D.mel_launch(x[:n], n, None, cfg, tab, PLAIN)[0]
            assert np.array_equal(rag[:, :own], alone[:, :own])


@pytest.mark.parametrize("case", D.GL_CASES, ids=GL_IDS)
def test_griffin_lim_chain_follows_the_float64_restatement(case):
    name, B, T = case
    cfg = D.GL_CONFIGS[name]
    e = GC.e32()
    fb64 = M.filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    lm = D.gl_logmel(case)
    for seed in D.GL_SEEDS:
        phi = D.gl_phase(case, seed)
        for b in range(B):
            out = right(case, seed, b)
            S64 = G.invert(lm[b], fb64, D.NNLS_ITERS)
            w64 = G.griffin_lim(S64, phi[b], (0, 1, 2), D.MOMENTUM, cfg["n_fft"], cfg["hop_length"], cfg["win_length"])
            errs = {"S": rel(out["S"], S64), **{n: rel(out["wav"][n], w64[n]) for n in (0, 1, 2)}}
            print(D.case_id(case), seed, b, {k: f"{v:.2e} / {4 * e[k]:.2e}" for k, v in errs.items()})
            for k, v in errs.items():
                assert v <= 4 * e[k], (k, v, 4 * e[k])


def test_every_exp_of_every_case_is_decided():
    for case in D.GL_CASES:
        lm = D.gl_logmel(case).astype(np.float64)
        assert D.decided(np.exp(np.clip(lm, D.LOG_LO, D.LOG_HI))).all(), case
    # the rule itself: a value on a midpoint, and one a double ulp from it, are undecided
    mid = 0.5 * (np.float64(np.float32(1.0)) + np.float64(np.nextafter(np.float32(1.0), np.float32(2.0))))
    assert not D.decided(np.array([mid, np.nextafter(mid, 2.0), np.nextafter(mid, 0.0)])).any()
    assert D.decided(np.array([1.0, mid * (1 + 2.0 ** -39), 0.0, 1e-5])).all()


def test_a_ragged_item_is_its_stand_alone_forward():
    name, T, lengths = D.GL_RAGGED[0]
    case = (name, 1, T)
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    lm, ph = D.gl_logmel(case)[0], pack_phase(D.gl_phase(case, D.GL_SEEDS[0]))[0]
    for n in lengths:
        Tb = D.item_frames(n, T)
        rag = D.forward_np(lm, ph, cfg, tab, 2, PLAIN, length=n)["wav"][2]
        own = cfg["hop_length"] * (Tb - 1) if Tb else 0
        assert (rag[own:] == 0).all()
        if Tb:
            assert np.array_equal(rag[:own], D.forward_np(lm[:, :Tb], ph[:Tb], cfg, tab, 2, PLAIN)["wav"][2])


# ---- wrong restatements ------------------------------------------------------------------------------------------------------------
MEL_MUTS = ("taps_descending", "mel_partial_sums", "ascending", "mel_no_nyquist", "window_uncentred", "frames_shifted", "log_f32")
INVERT_MUTS = ("ascending", "exp_f32", "clip_after_exp", "residual_sign")
ISTFT_MUTS = ("taps_descending", "istft_one_chain", "istft_taps_outside_slices", "ascending", "idft_nyquist_2", "window_uncentred",
              "frames_shifted", "wss_past_end", "trim_short")
UPDATE_MUTS = ("taps_descending", "stft_one_chain", "ascending", "window_uncentred", "frames_shifted", "alpha_momentum",
               "first_uses_rprev", "im_sign")
PAIRS = [("mel", m) for m in MEL_MUTS] + [("invert", m) for m in INVERT_MUTS] + [("istft", m) for m in ISTFT_MUTS] + \
        [("update", m) for m in UPDATE_MUTS]
GL_BY_COST = sorted(D.GL_CASES, key=lambda c: D.GL_CONFIGS[c[0]]["n_fft"] * c[2])


def test_a_doubled_nyquist_weight_is_invisible_in_a_forward_and_why():
    """The filterbank column of bin n_fft / 2 is exactly 0 (the test above), so the row of pinv(fb) is 0, fb^T res is 0 there
    and S[:, n_fft / 2] == 0 in every frame of every case: every c a forward reaches has a zero Nyquist bin, and a wrong weight
    multiplies zeros.  The restatement does read the table entry: fed r (a spectrum whose Nyquist bin is not 0) it differs."""
    for case in D.GL_CASES:
        name, _, T = case
        cfg, tab, out = D.GL_CONFIGS[name], D.gl_tables(name), right(case)
        half = D.Design(cfg).half
        assert (tab["P"][half] == 0).all() and (out["S"][:, half] == 0).all(), case
        assert all((c[:, 2 * half] == 0).all() for c in out["c"]), case
        assert not gl_differs("istft", case, "idft_nyquist_2"), case
        r = out["r"][1]
        assert np.abs(r[:, 2 * half]).max() > 0
        assert not np.array_equal(D.istft_launch(r, T, T, cfg, tab, False)[0], D.istft_launch(r, T, T, cfg, tab, False, "idft_nyquist_2")[0]), case


INVISIBLE = {("mel", "mel_no_nyquist"), ("istft", "idft_nyquist_2")}
PAIRS = [p for p in PAIRS if p not in INVISIBLE]


def test_every_mutation_is_tried_somewhere():
    from test_oracle_denoiser_chain import DN_PAIRS                # the bias denoiser's wrong restatements are tried there
    assert all(m.startswith("dn_") for _, m in DN_PAIRS) and not any(m.startswith("dn_") for _, m in PAIRS)
    from test_oracle_time_stretch_chain import TS_PAIRS           # and the time stretch's there
    assert all(m.startswith("ts_") for _, m in TS_PAIRS) and not any(m.startswith("ts_") for _, m in PAIRS + DN_PAIRS)
    assert {m for _, m in PAIRS} | {m for _, m in INVISIBLE} | {m for _, m in DN_PAIRS} | {m for _, m in TS_PAIRS} == set(D.MUTATIONS)


def test_a_dropped_nyquist_column_is_invisible_in_the_log_mel_and_why():
    """A Slaney triangle ends at fmax <= sample_rate / 2 with weight 0, so the filterbank column of bin n_fft / 2 is exactly
    0 for every valid config: the Nyquist magnitude only ever multiplies zeros and no log-mel can show it.  The column itself
    is judged where it matters: gl_stft_update_kernel stores it (``r[2 half]``), and there ``im_sign`` / ``frames_shifted`` and the
    exact comparison of r see it."""
    for name, cfg in D.MEL_CONFIGS.items():
        d = D.Design(cfg)
        assert (D.mel_tables(name)["fb"][:, d.half] == 0).all(), name
    for case in D.MEL_CASES:
        assert not mel_differs(case, "mel_no_nyquist"), case
    # and the magnitude that is dropped is not itself 0: the restatement does compute it
    case = D.GL_CASES[2]
    assert np.abs(right(case)["r"][0][:, 2 * D.Design(D.GL_CONFIGS[case[0]]).half]).max() > 0


def mel_differs(case, mut):
    name, _, L = case
    x = D.mel_audio(name, 1, L, 0)[0]
    run = lambda m: D.mel_launch(x, L, None, D.MEL_CONFIGS[name], D.mel_tables(name), PLAIN, m)[0]
    return not np.array_equal(run(None), run(mut))


def gl_differs(kind, case, mut):
    name, _, T = case
    cfg, tab, out = D.GL_CONFIGS[name], D.gl_tables(name), right(case)
    if kind == "invert":
        ph = pack_phase(D.gl_phase(case, D.GL_SEEDS[0]))[0]
        return not np.array_equal(out["S"], D.invert_launch(D.gl_logmel(case)[0], ph, T, cfg, tab, D.NNLS_ITERS, PLAIN, mut)[0])
    if kind == "istft":
        # c1: the spectrum of a real pass (c0's random phase would do as well)
        return not np.array_equal(D.istft_launch(out["c"][1], T, T, cfg, tab, False)[0], D.istft_launch(out["c"][1], T, T, cfg, tab, False, mut)[0])
    S = D.pad_cols(out["S"], D.Design(cfg).ks)
    first = mut == "first_uses_rprev"                             # the first pass, handed the r of another pass
    y = out["y"][0 if first else 1]
    want = D.update_launch(D.update_acc(y, T, cfg, tab), S, out["r"][0], cfg, first, PLAIN)
    got = D.update_launch(D.update_acc(y, T, cfg, tab, mut), S, out["r"][0], cfg, first, PLAIN, mut)
    return not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))


@pytest.mark.parametrize("kind,mut", PAIRS, ids=[f"{k}-{m}" for k, m in PAIRS])
def test_mutation_fails(kind, mut):
    """A wrong restatement must differ from the right one on at least one case (cheapest cases first; the first that shows
    it ends the search).  ``window_uncentred`` can only show where win < n_fft, ``istft_taps_outside_slices`` only with more
    than one slice: both have such cases."""
    cases = sorted(D.MEL_CASES, key=lambda c: c[2]) if kind == "mel" else GL_BY_COST
    for case in cases:
        if mel_differs(case, mut) if kind == "mel" else gl_differs(kind, case, mut):
            print(f"{kind} {mut}: visible at {case}")
            return
    pytest.fail(f"{mut} is invisible in {kind} on every case")


# ---- the elementwise fmaf -------------------------------------------------------------------------------------------------------
def test_fmaf32_rounds_once():
    from oracle import chain_oracle as co
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: the product alone rounds the 2^-24 away (a tie, to even), the fused form keeps it
    a = np.float32(1.0 + 2.0 ** -12)
    c = np.float32(2.0 ** -24)
    assert np.float32(a * a) + c == np.float32(1.0 + 2.0 ** -11)
    assert co.fmaf32(a, a, c)[()] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    rng = np.random.default_rng(5)
    x, y, z = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    exact = x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)      # the product is exact in double
    safe = D.decided(exact)                                                             # no double rounding there
    assert safe.sum() > 4000 and np.array_equal(co.fmaf32(x, y, z)[safe], exact.astype(np.float32)[safe])
