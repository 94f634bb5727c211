"""Every launch of the bias denoiser on the MI355X -- ``dn_stft_kernel<subtract>`` (dense, ragged and in its window form),
``gl_istft_kernel`` as ``dn_forward`` launches it (``lengths`` = the frame counts the launch before it wrote, ``zero_tail`` set)
and as a slice of a window, ``dn_stft_kernel<magnitude>`` and ``dn_bias_reduce_kernel`` -- each judged on the device's OWN
input against the CPU restatement of the arithmetic csrc/denoiser.h commits to (oracle/dsp_chain_cases.py;
tests/test_oracle_denoiser_chain.py ties the restatements to the float64 one and shows that the wrong ones fail).

The comparison is ``==`` element by element (-0 equals +0, NaN equals nothing); no tolerance appears in this file.  Workspaces
and outputs are poisoned with NaN before every call, so what a launch must not write is still NaN afterwards and what it must
write is not.  The one contraction site the source leaves open, ``re re + im im``, is searched per instantiation:
``Session.judge`` keeps the assignments that reproduce every element so far and fails when none is left.  The only elements
that may be left out are those whose float64 re^2 + im^2 lies below 2^-125, only where the device disagrees there, at most
0.1 % of a call's stored elements, and never in the silence cases; the last test prints how many were.

RESULTS on an MI355X (ROCm's hipcc, the project's flags), every element bit for bit -- the fused subtraction, the division,
sqrtf and the guarded zeros included -- and every rerun bit-equal:
    dn_stft_kernel<subtract> (dense)        663 096 elements     gl_istft_kernel (dn_forward, dense)     222 032
    dn_stft_kernel<subtract> (ragged)        20 106              gl_istft_kernel (dn_forward, ragged)      8 664
    dn_stft_kernel<subtract> (window)       220 944              gl_istft_kernel (window slice)           54 472
    dn_stft_kernel<magnitude>                44 321              dn_bias_reduce_kernel                     1 750
ONE contraction assignment per instantiation reproduces all of it, and no other does -- the same one in both:
    dn_stft_kernel<subtract>    re re + im im  plain (both products rounded)
    dn_stft_kernel<magnitude>   re re + im im  plain
No element with a subnormal square had to be left out: 0 (the device agrees there too).
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris._native_model import _ptr, _stream
from iris.denoiser import Denoiser
from oracle import dsp_chain_cases as D

import denoiser_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
SESSION = D.Session()
SUB, MAG = "dn_stft_kernel<subtract>", "dn_stft_kernel<magnitude>"
_state = {"left_out": 0}


def model(name) -> Denoiser:
    if ("dn", name) not in _state:
        _state[("dn", name)] = Denoiser(*C.stft_args(name), strength=D.DN_STRENGTH, device=DEV)
    return _state[("dn", name)]


def acc_of(key, wav, y_org, frames, name):
    """``window_acc`` once per input: it does not depend on the strength, the bias or the contraction site."""
    if ("acc",) + key not in _state:
        _state[("acc",) + key] = D.window_acc(wav, y_org, frames, D.GL_CONFIGS[name], D.gl_tables(name))
    return _state[("acc",) + key]


def poison(dn, B, L, out_shape):
    """NaN in the whole workspace and in the block the next ``torch.empty(out_shape)`` most likely gets."""
    dn._ensure()
    dn._ws(B, L).view(torch.float32).fill_(NAN)
    t = torch.full(out_shape, NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    del t


def same(kind, where, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = D.differing(got, want)
    if bad:
        idx = tuple(np.argwhere(~(got == want))[0])
        raise AssertionError(f"{kind} {where}: {bad} of {got.size} elements differ; first at {idx}: device {got[idx]!r}, restatement {want[idx]!r}")
    SESSION.count(kind, exact=got.size)


def judge_subtract(kind, where, name, acc, bias, strength, c_dev, may_leave_out=True):
    """``c_dev [Tb, Qp]`` of one item against ``subtract_launch`` of its own ``acc``; the columns from Q on are still NaN."""
    cfg, d = D.GL_CONFIGS[name], D.Design(D.GL_CONFIGS[name])
    assert np.isnan(c_dev[:, d.q:]).all(), (kind, where)
    got = np.ascontiguousarray(c_dev[:, :d.q])
    tiny = D.dn_tiny(acc, cfg) if may_leave_out else np.zeros(got.shape, bool)
    restate = lambda fma: D.subtract_launch(acc, bias, strength, cfg, fma)
    fma = SESSION.judge(SUB, kind, where, restate, lambda want: D.differing(got, want, ~tiny))
    left_out = D.differing(got, restate(fma), tiny)
    assert left_out <= D.DN_TINY_SHARE * got.size, (kind, where, left_out)
    assert not np.isnan(got).any(), (kind, where)
    _state["left_out"] += left_out
    SESSION.count(kind, exact=got.size - left_out)


def forward(name, wav, bias, strength, lengths=None):
    """One poisoned ``forward_device`` -> ``(out [B, L], c [B, T, Qp], frames [B])`` as numpy."""
    dn = model(name)
    dn.set_bias(bias)
    B, L = wav.shape
    poison(dn, B, L, (B, L))
    out = dn.forward_device(wav, lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV), strength=strength)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dn._read_c(B, L).cpu().numpy(), dn._read_frames(B, L).cpu().numpy()


def judge_forward(name, clean, wav, bias, strength, lengths, key, where, may_leave_out=True):
    """Both launches of ``dn_forward`` on ``wav [B, L]`` (``clean``: the same without the NaN padding), then the same call again."""
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    d = D.Design(cfg)
    B, L = wav.shape
    T = L // d.hop + 1
    out, c, frames = forward(name, wav, bias, strength, lengths)
    form = "dense" if lengths is None else "ragged"
    for b in range(B):
        Tb = D.dn_item_frames(None if lengths is None else lengths[b], T)
        Lb = d.hop * (Tb - 1) if Tb else 0
        assert frames[b] == Tb, (where, b, frames[b], Tb)
        assert np.isnan(c[b, Tb:]).all(), (where, b)                                   # nothing from T_b on is written
        if Tb:
            acc = acc_of(key + (b,), clean[b, :Lb], 0, Tb, name)
            judge_subtract(f"{SUB} ({form})", f"{where} item {b}", name, acc, bias, strength, c[b, :Tb], may_leave_out)
        want, written = D.istft_launch(c[b], Tb, T, cfg, tab, True)                    # on the device's own c
        assert written.all()
        same(f"gl_istft_kernel (dn_forward, {form})", f"{where} item {b}", out[b], want)
        assert (out[b, Lb:] == 0).all() and not np.signbit(out[b, Lb:]).any(), (where, b)
    again = forward(name, wav, bias, strength, lengths)
    assert np.array_equal(again[0], out) and np.array_equal(again[1], c, equal_nan=True) and np.array_equal(again[2], frames), where
    return out, c


# ---- the forward, dense ------------------------------------------------------------------------------------------------------------
BIASES = [(s, False) for s in D.DN_STRENGTHS] + [(D.DN_STRENGTH, True)]


@pytest.mark.parametrize("strength,forced", BIASES, ids=[f"s{s}{'-forced' if f else ''}" for s, f in BIASES])
@pytest.mark.parametrize("case", D.DN_CASES, ids=[f"{n}-B{B}-M{M}" for n, B, M in D.DN_CASES])
def test_forward_dense(case, strength, forced):
    name, B, M = case
    wav = D.dn_wave(name, B, M)
    bias = D.dn_forced_bias(C.bias(case)) if forced else C.bias(case)
    out, c = judge_forward(name, wav, wav, bias, strength, None, ("dense", case), f"{name} M={M} strength={strength} forced={forced}")
    assert np.isfinite(out).all()
    if forced:                                                   # scale == 1: the transform itself; scale == 0: exact zeros
        half = D.Design(D.GL_CONFIGS[name]).half
        assert (c[:, :, 4:2 * half:8] == 0).all() and (c[:, :, 5:2 * half:8] == 0).all()
        plain = forward(name, wav, np.zeros_like(bias), strength)[1]
        assert np.array_equal(c[:, :, 0:2 * half:8], plain[:, :, 0:2 * half:8]) and np.array_equal(c[:, :, 2 * half], plain[:, :, 2 * half])


# ---- the forward, ragged -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", D.DN_RAGGED, ids=[f"{n}-M{M}" for n, M, _ in D.DN_RAGGED])
def test_forward_ragged(rc):
    name, M, lengths = rc
    hop = D.GL_CONFIGS[name]["hop_length"]
    clean = D.dn_wave(name, len(lengths), M, seed=30)
    wav = clean.copy()
    for b, m in enumerate(lengths):                              # nothing at or past an item's own samples is read
        wav[b, hop * m:] = NAN
    out, c = judge_forward(name, clean, wav, C.config_bias(name), D.DN_STRENGTH, list(lengths), ("ragged", rc), f"{name} M={M} ragged")
    for b, m in enumerate(lengths):
        if m < 1:                                                # no frame: c untouched, the row all +0
            assert np.isnan(c[b]).all() and (out[b] == 0).all()


# ---- silence -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.GL_CONFIGS))
def test_silence(name):
    """mag == 0, the guarded division: c is 0 by value there, nothing written is NaN, and no element is left out."""
    wav = D.dn_silence(name)
    M = D.dn_case_m(name)
    out, c = judge_forward(name, wav, wav, C.config_bias(name), D.DN_STRENGTH, None, ("silence", name), f"{name} silence", may_leave_out=False)
    d = D.Design(D.GL_CONFIGS[name])
    assert (c[0, :, :d.q] == 0).all() and (out[0] == 0).all() and np.isfinite(out).all() and np.isfinite(c[:, :, :d.q]).all()
    acc = _state[("acc", "silence", name, 1)]
    re, im, _ = D.dn_parts(acc, d)
    dead = ((re == 0) & (im == 0)).all(axis=1)
    assert dead.any() and not dead.all() and (c[1, :M + 1][dead][:, :d.q] == 0).all()


# ---- windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", D.DN_WINDOWS, ids=lambda w: "-".join(str(v) for v in w))
def test_forward_window(w):
    name, M, m0, Mw, final = w
    cfg, tab, bias = D.GL_CONFIGS[name], D.gl_tables(name), C.config_bias(name)
    d = D.Design(cfg)
    B, GUARD = 2, 64
    f_lo, f_hi, out_lo, count = D.dn_window(cfg, m0, Mw, final)
    frames, y_org, s_org = f_hi - f_lo, d.hop * (f_lo - m0), out_lo - d.hop * f_lo
    win = np.ascontiguousarray(D.dn_wave(name, B, M, seed=40)[:, d.hop * m0:d.hop * (m0 + Mw)])
    dn = model(name)
    dn.set_bias(bias)
    assert dn.window_range(d.hop * m0, d.hop * Mw, final) == (out_lo, count)
    lib, Lw = dn._ensure(), win.shape[1]
    runs = []
    for _ in range(2):
        # out [B, count] with guard floats on both sides: the C entry point, so that the buffer is the test's
        buf = torch.full((B * count + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
        ws = dn._ws(B, Lw)
        ws.view(torch.float32).fill_(NAN)
        wav_dev = torch.from_numpy(win).to(DEV)
        _native.check("iris_denoiser_forward_window", lib.iris_denoiser_forward_window(
            dn._handle, _ptr(wav_dev), B, Lw, ctypes.c_int64(d.hop * m0), int(final), ctypes.c_float(D.DN_STRENGTH), _ptr(buf[GUARD:]),
            _ptr(ws), ctypes.c_uint64(ws.numel()), _stream(DEV)))
        torch.cuda.synchronize()
        runs.append((buf.cpu().numpy(), dn._read_window_c(B, Lw, frames).cpu().numpy(), dn._read_frames(B, Lw).cpu().numpy(),
                     dn._workspace.view(torch.float32).cpu().numpy()))
    buf, c, stored, whole_ws = runs[0]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], runs[1]))
    assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + B * count:]).all()             # the guards on both sides
    assert (stored == frames).all()
    # rows from `frames` on are untouched: behind c [B, frames, Qp] the workspace is NaN up to the frame counts
    off = dn._workspace_layout(B, Lw)[0]["frames"][0]
    assert np.isnan(whole_ws[B * frames * d.qp:off]).all() and np.isnan(whole_ws[off + B:]).all()
    out = buf[GUARD:GUARD + B * count].reshape(B, count)
    where = f"{name} window m0={m0} Mw={Mw} final={final}"
    for b in range(B):
        acc = acc_of(("window", w, b), win[b], y_org, frames, name)
        judge_subtract(f"{SUB} (window)", f"{where} item {b}", name, acc, bias, D.DN_STRENGTH, c[b])
        same("gl_istft_kernel (window slice)", f"{where} item {b}", out[b], D.window_slice(c[b], frames, s_org, count, cfg, tab))
    # and through the Python entry point: the same bits
    assert np.array_equal(dn.forward_window(win, d.hop * m0, final).cpu().numpy(), out)


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------
def has_interior(case):
    lo, hi = D.dn_interior(D.GL_CONFIGS[case[0]], case[2] + 1)
    return hi > lo


EST = [c for c in D.DN_CASES if has_interior(c)]


@pytest.mark.parametrize("case", EST, ids=[f"{n}-M{M}" for n, _, M in EST])
def test_estimate_bias(case):
    name, B, M = case
    cfg = D.GL_CONFIGS[name]
    d = D.Design(cfg)
    wav = D.dn_wave(name, B, M)[:1]
    L, T = wav.shape[1], M + 1
    dn = model(name)
    runs = []
    for _ in range(2):
        poison(dn, 1, L, (dn.n_bins,))
        bias = dn.estimate_bias(wav)
        torch.cuda.synchronize()
        runs.append((bias.cpu().numpy(), dn._read_mag(L).cpu().numpy(), dn._workspace.view(torch.float32).cpu().numpy()))
    bias, mag, whole_ws = runs[0]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], runs[1]))
    where = f"{name} M={M}"
    # every frame of a dense call is written, bins columns of it; the padding up to Ks and the rest of the workspace are not
    assert mag.shape == (T, d.ks) and np.isnan(mag[:, d.bins:]).all() and np.isnan(whole_ws[T * d.ks:]).all(), where
    got = np.ascontiguousarray(mag[:, :d.bins])
    acc = acc_of(("dense", case, 0), wav[0], 0, T, name)
    tiny = D.dn_tiny(acc, cfg)
    tiny = np.concatenate([tiny[:, 0:2 * d.half:2], tiny[:, 2 * d.half:2 * d.half + 1]], axis=1)
    restate = lambda fma: D.magnitude_launch(acc, cfg, fma)
    fma = SESSION.judge(MAG, MAG, where, restate, lambda want: D.differing(got, want, ~tiny))
    left_out = D.differing(got, restate(fma), tiny)
    assert left_out <= D.DN_TINY_SHARE * got.size and not np.isnan(got).any(), (where, left_out)
    _state["left_out"] += left_out
    SESSION.count(MAG, exact=got.size - left_out)
    lo, hi = D.dn_interior(cfg, T)
    same("dn_bias_reduce_kernel", where, bias, D.bias_reduce(got, lo, hi))             # of the device's own magnitudes


# ---- the report --------------------------------------------------------------------------------------------------------------------------
def test_one_contraction_assignment_per_instantiation():
    """Runs last: what the session found (RESULTS at the head of this module records what it printed on an MI355X)."""
    SESSION.report()
    print(f"elements with float64 re^2 + im^2 < 2^-125 left out because the device disagreed there: {_state['left_out']}")
    assert len(SESSION.alive[SUB]) == 1 and len(SESSION.alive[MAG]) == 1, (SESSION.alive[SUB], SESSION.alive[MAG])
    kinds = {f"{SUB} (dense)", f"{SUB} (ragged)", f"{SUB} (window)", "gl_istft_kernel (dn_forward, dense)", "gl_istft_kernel (dn_forward, ragged)",
             "gl_istft_kernel (window slice)", MAG, "dn_bias_reduce_kernel"}
    assert kinds <= set(SESSION.stats), kinds - set(SESSION.stats)
    assert all(SESSION.stats[k]["exact"] > 0 for k in kinds)
