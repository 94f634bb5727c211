"""Every launch of the mel front-end (``mel_kernel``, fp32 / int16 samples, dense / ragged) and of a Griffin-Lim forward
(``gl_invert_kernel``, ``gl_istft_kernel`` in its in-loop and its final form, ``gl_stft_update_kernel`` with ``first`` set and
with momentum) on the MI355X, each judged on the device's OWN input against the CPU restatement of the arithmetic its
header commits to (oracle/dsp_chain_cases.py: the plan, the claims and what survives a forward are written there;
tests/test_oracle_dsp_chain.py ties the restatements to the float64 ones and shows that the wrong ones fail).

The comparison is ``==`` element by element (-0 equals +0, NaN equals nothing).  Workspaces and outputs are poisoned with NaN
before every forward, so what a launch must not write is still NaN afterwards and what it must write is not.

A Griffin-Lim case runs the same inputs at ``n_iter`` = 0, 1 and 2 (and ``small`` at 31 and 32) and takes what one forward
overwrote from the forward before it.  The contraction sites the source leaves open are searched per kernel:
``Session.judge`` keeps the assignments that reproduce every element so far and fails when none is left; the last test prints
what survived, the element counts, the undecided frames and the worst error over bar of anything held to a bar.

RESULTS on an MI355X (ROCm's hipcc, the project's flags), every element bit for bit -- fp32 division and sqrtf included, so
the IEEE-rounding claim stands and no bar replaced it; no frame was undecided, so nothing was held to a bar (worst error over
bar 0.000 everywhere):
    mel_kernel                         12 336 elements     mel_kernel<i16>                    12 336
    mel_kernel_ragged                  28 500              mel_kernel_ragged<i16>             28 500      (0 of 274 / 680 frames undecided)
    gl_invert_kernel                  418 017 (S and c0; 0 of 907 frames undecided)
    gl_istft_kernel (in-loop)         168 752              gl_istft_kernel (final)           265 464
    gl_stft_update_kernel (first)     531 064 (r and c)    gl_stft_update_kernel (momentum)  540 304
ONE contraction assignment per kernel reproduces all of it, and no other does:
    mel_kernel              re re + im im  plain (both products rounded)
    gl_invert_kernel        x - step acc   fused: fmaf(-step, acc, x)
    gl_stft_update_kernel   re - alpha pr  fused: fmaf(-alpha, pr, re);   ar ar + ai ai  plain
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.griffin_lim import pack_phase
from iris.mel import MelFrontend
from oracle import dsp_chain_cases as D

import griffin_lim_cases as GC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
SESSION = D.Session()
_state = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poison_next(shape):
    """Leaves NaN in the block the next ``torch.empty(shape)`` most likely gets, so an element is 0 only if it was stored."""
    t = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    del t


def ulp_ratio(got, want64):
    """|got - want| in fp32 ulps of ``want`` (the bar of an undecided exp / log is 1)."""
    w32 = want64.astype(np.float32)
    return float((np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(w32)).astype(np.float64)).max()) if got.size else 0.0


# ---- mel_kernel ------------------------------------------------------------------------------------------------------------------
def frontend(name) -> MelFrontend:
    if ("fe", name) not in _state:
        _state[("fe", name)] = MelFrontend(**D.MEL_CONFIGS[name])
    return _state[("fe", name)]


def judge_mel(name, audio, n_samples, caps, got, frames, where):
    """``audio [B, L]`` as the device read it; ``n_samples`` / ``caps`` None for the dense form."""
    cfg, tab = D.MEL_CONFIGS[name], D.mel_tables(name)
    B, L = audio.shape
    kind = f"mel_kernel{'_ragged' if n_samples is not None else ''}{'<i16>' if audio.dtype == np.int16 else ''}"
    for b in range(B):
        n_b = L if n_samples is None else n_samples[b]
        cap = None if caps is None else caps[b]
        own = audio[b].copy()
        own[min(max(n_b, 0), L):] = 0                           # the restatement never reads them either; NaN would not index
        restate = lambda fma: D.mel_launch(own, n_b, cap, cfg, tab, fma)

        def compare(r):
            mel, Tb, ok = r
            return int(frames[b] != Tb) + D.differing(got[b][:, ok], mel[:, ok])

        fma = SESSION.judge("mel_kernel", kind, f"{where} item {b}", restate, compare)
        mel, Tb, ok = restate(fma)
        assert (got[b][:, Tb:] == 0).all() and not np.signbit(got[b][:, Tb:]).any()
        ratio = 0.0
        if not ok.all():                                        # undecided logarithms: 1 fp32 ulp
            ratio = ulp_ratio(got[b][:, ~ok], mel[:, ~ok].astype(np.float64))
            assert ratio <= 1.0 and 100 * int((~ok).sum()) <= max(Tb, 1), (where, b, ratio)
        SESSION.count(kind, exact=got[b][:, ok].size, undecided=(~ok).sum(), frames=got.shape[2], ratio=ratio)


MEL_IDS = [f"{n}-B{B}-L{L}" for n, B, L in D.MEL_CASES]


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("seed", D.MEL_SEEDS)
@pytest.mark.parametrize("case", D.MEL_CASES, ids=MEL_IDS)
def test_mel_dense(case, seed, i16):
    name, B, L = case
    audio = D.mel_audio(name, B, L, seed)
    audio = D.to_int16(audio) if i16 else audio
    fe = frontend(name)
    poison_next((B, fe.n_mels, fe.frames_of(L)))
    mel, frames = fe.forward_device(audio)
    judge_mel(name, audio, None, None, mel.cpu().numpy(), frames.cpu().numpy(), f"{name} L={L} seed={seed}")


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("rc", D.MEL_RAGGED, ids=[f"{n}-L{L}" for n, L, _ in D.MEL_RAGGED])
def test_mel_ragged(rc, i16):
    name, L, ns = rc
    B = len(ns)
    clean = D.mel_audio(name, B, L, 3)
    clean = D.to_int16(clean) if i16 else clean
    audio = clean.copy()
    for b, n in enumerate(ns):                                   # nothing at or past n_b is read: NaN (fp32) or full scale (int16)
        audio[b, n:] = -32768 if i16 else np.nan
    caps = [10 ** 6, 10 ** 6, 0, 9, 10 ** 6]
    fe = frontend(name)
    for use_caps in (None, caps):
        poison_next((B, fe.n_mels, fe.frames_of(L)))
        mel, frames = fe.forward_device(audio, lengths=list(ns), max_frames=use_caps)
        judge_mel(name, clean, list(ns), use_caps, mel.cpu().numpy(), frames.cpu().numpy(), f"{name} ragged caps={use_caps is not None}")


# ---- Griffin-Lim ---------------------------------------------------------------------------------------------------------------------
def model(name, n_iter):
    if ("gl", name, n_iter) not in _state:
        _state[("gl", name, n_iter)] = D.gl_model(name, n_iter=n_iter)
    return _state[("gl", name, n_iter)]


def e32():
    if "e32" not in _state:
        _state["e32"] = GC.e32()
    return _state["e32"]


def forward(name, n_iter, lm, phase, lengths=None, **kw):
    """One poisoned forward -> ``(wav, {S, c, r, y})`` as numpy.  ``phase``: the packed device tensor, or "device"."""
    gl = model(name, n_iter)
    B, T = lm.shape[0], lm.shape[2]
    gl._ensure()
    gl._ws(B, T).view(torch.float32).fill_(NAN)
    poison_next((B, gl.samples_of(T)))
    wav = gl.forward_device(lm, phase, lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV), **kw)
    torch.cuda.synchronize()
    return wav.cpu().numpy(), {k: v.cpu().numpy() for k, v in gl._read_buffers(B, T).items()}


def same(kind, where, got, want, mask=None):
    bad = D.differing(got, want, mask)
    if bad:
        idx = np.argwhere(~(got == want) & (True if mask is None else mask))[0]
        raise AssertionError(f"{kind} {where}: {bad} of {got.size} elements differ; first at {tuple(idx)}: device "
                             f"{got[tuple(idx)]!r}, restatement {want[tuple(idx)]!r}")
    SESSION.count(kind, exact=got.size if mask is None else int(mask.sum()))


def judge_invert(name, lm, packed, lengths, run, where):
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    d = D.Design(cfg)
    B, T = lm.shape[0], lm.shape[2]
    for b in range(B):
        Tb = D.item_frames(None if lengths is None else lengths[b], T)
        S_dev, c_dev = run[1]["S"][b], run[1]["c"][b]
        assert np.isnan(S_dev[Tb:]).all() and np.isnan(c_dev[Tb:]).all(), (where, b)         # nothing past T_b is written
        assert np.isnan(S_dev[:Tb, d.bins:]).all() and np.isnan(c_dev[:Tb, d.q:]).all(), (where, b)
        if not Tb:
            continue
        restate = lambda fma: D.invert_launch(lm[b], packed[b], Tb, cfg, tab, D.NNLS_ITERS, fma)
        compare = lambda r: D.differing(S_dev[:Tb, :d.bins][r[2]], r[0][r[2]]) + D.differing(c_dev[:Tb, :d.q][r[2]], r[1][r[2]])
        fma = SESSION.judge("gl_invert_kernel", "gl_invert_kernel", f"{where} item {b}", restate, compare)
        S, c0, ok, m = restate(fma)
        ratio = 0.0
        if not ok.all():                                        # undecided exponentials: S within 4 e32 of the restatement's
            assert 100 * int((~ok).sum()) <= Tb
            ratio = float(np.abs(S_dev[:Tb, :d.bins][~ok] - S[~ok]).max() / max(1.0, np.abs(S).max())) / (4 * e32()["S"])
            assert ratio <= 1.0, (where, b, ratio)
        SESSION.count("gl_invert_kernel", exact=int(ok.sum()) * (d.bins + d.q), undecided=(~ok).sum(), frames=Tb, ratio=ratio)


def judge_istft(name, T, lengths, c_in, out, final, where):
    """``c_in [B, T, Qp]`` -> ``out [B, Ly]``: the in-loop form writes nothing from Ly_b on, the final form of a ragged call zeros."""
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    kind = f"gl_istft_kernel ({'final' if final else 'in-loop'})"
    for b in range(c_in.shape[0]):
        Tb = D.item_frames(None if lengths is None else lengths[b], T)
        y, written = D.istft_launch(c_in[b], Tb, T, cfg, tab, final and lengths is not None)
        assert np.isnan(out[b][~written]).all(), (kind, where, b)
        assert written.all() or not final or lengths is None
        same(kind, f"{where} item {b}", out[b][written], y[written])
        Lyb = cfg["hop_length"] * (Tb - 1) if Tb else 0
        if final and lengths is not None:
            assert (out[b][Lyb:] == 0).all() and not np.signbit(out[b][Lyb:]).any()


def judge_update(name, T, lengths, y_in, S_in, r_prev, r_out, c_out, first, where):
    cfg, tab = D.GL_CONFIGS[name], D.gl_tables(name)
    d = D.Design(cfg)
    kind = f"gl_stft_update_kernel ({'first' if first else 'momentum'})"
    for b in range(y_in.shape[0]):
        Tb = D.item_frames(None if lengths is None else lengths[b], T)
        assert np.isnan(r_out[b][Tb:]).all() and np.isnan(c_out[b][Tb:]).all(), (where, b)
        assert np.isnan(r_out[b][:Tb, d.q:]).all() and np.isnan(c_out[b][:Tb, d.q:]).all(), (where, b)
        if not Tb:
            continue
        acc = D.update_acc(np.nan_to_num(y_in[b], nan=0.0), Tb, cfg, tab)       # y past Ly_b is still NaN and is never read
        restate = lambda fma: D.update_launch(acc, S_in[b], None if first else r_prev[b], cfg, first, fma)
        compare = lambda rc: D.differing(r_out[b][:Tb, :d.q], rc[0]) + D.differing(c_out[b][:Tb, :d.q], rc[1])
        SESSION.judge("gl_stft_update_kernel", kind, f"{where} item {b}", restate, compare)
        SESSION.count(kind, exact=2 * Tb * d.q)


def judge_pass(name, T, lengths, prev, run, first, where):
    """The last pass of ``run`` (a forward of n >= 1 passes), with ``prev`` the forward of one pass fewer on the same inputs."""
    judge_istft(name, T, lengths, prev[1]["c"], run[1]["y"], False, where)
    judge_update(name, T, lengths, run[1]["y"], run[1]["S"], prev[1]["r"], run[1]["r"], run[1]["c"], first, where)
    judge_istft(name, T, lengths, run[1]["c"], run[0], True, where)


def judge_two_passes(name, lm, packed, lengths, where, **kw):
    T = lm.shape[2]
    phase = kw.pop("phase", None)
    runs = [forward(name, n, lm, dev(packed) if phase is None else phase, lengths, **kw) for n in (0, 1, 2)]
    judge_invert(name, lm, packed, lengths, runs[0], where)
    judge_istft(name, T, lengths, runs[0][1]["c"], runs[0][0], True, f"{where} n_iter=0")
    assert np.isnan(runs[0][1]["r"]).all() and np.isnan(runs[0][1]["y"]).all()
    for n in (1, 2):
        ok = ~np.isnan(runs[0][1]["S"])
        assert np.array_equal(runs[n][1]["S"][ok], runs[0][1]["S"][ok]) and np.array_equal(np.isnan(runs[n][1]["S"]), ~ok)
        judge_pass(name, T, lengths, runs[n - 1], runs[n], n == 1, f"{where} n_iter={n}")


@pytest.mark.parametrize("seed", D.GL_SEEDS)
@pytest.mark.parametrize("case", D.GL_CASES, ids=[D.case_id(c) for c in D.GL_CASES])
def test_two_pass_forward(case, seed):
    judge_two_passes(case[0], D.gl_logmel(case), pack_phase(D.gl_phase(case, seed)), None, f"{D.case_id(case)} seed={seed}")


def test_late_loop_state():
    """n_iter = 31 and 32 on ``small``: the update and both inverse transforms on the state the loop reaches after 31 passes."""
    name, B, T = D.GL_LATE
    lm, packed = D.gl_logmel(D.GL_LATE), dev(pack_phase(D.gl_phase(D.GL_LATE, D.GL_SEEDS[0])))
    runs = [forward(name, n, lm, packed) for n in (31, 32)]
    judge_istft(name, T, None, runs[0][1]["c"], runs[0][0], True, "late n_iter=31")
    judge_pass(name, T, None, runs[0], runs[1], False, "late n_iter=32")


@pytest.mark.parametrize("rc", D.GL_RAGGED, ids=[f"{n}-T{T}" for n, T, _ in D.GL_RAGGED])
def test_two_pass_forward_ragged(rc):
    name, T, lengths = rc
    case = (name, len(lengths), T)
    lm, packed = D.gl_logmel(case).copy(), pack_phase(D.gl_phase(case, D.GL_SEEDS[0]))
    for b, n in enumerate(lengths):                              # nothing at t >= T_b is read
        lm[b, :, D.item_frames(n, T):] = NAN
        packed[b, D.item_frames(n, T):] = NAN
    judge_two_passes(name, lm, packed, list(lengths), f"{name} T={T} ragged")


@pytest.mark.parametrize("rc", [(D.GL_CASES[2][0], D.GL_CASES[2][2], None), D.GL_RAGGED[1]], ids=["small-dense", "odd_hop-ragged"])
def test_device_drawn_phase(rc):
    """c0 of a ``phase0="device"`` forward is S times what ``draw_phase`` stores for the same seed and stream, bit for bit."""
    name, T, lengths = rc
    B = 1 if lengths is None else len(lengths)
    lm = D.gl_logmel((name, B, T))
    drawn = model(name, 0).draw_phase(B, T, seed=99, first_item=3).cpu().numpy()
    run = forward(name, 0, lm, "device", None if lengths is None else list(lengths), seed=99, first_item=3)
    judge_invert(name, lm, drawn, None if lengths is None else list(lengths), run, f"{name} T={T} device phase")
    assert not np.array_equal(drawn, model(name, 0).draw_phase(B, T, seed=99, first_item=4).cpu().numpy())


def test_one_contraction_assignment_per_kernel():
    """Runs last: what the session found (RESULTS at the head of this module records what it printed on an MI355X)."""
    SESSION.report()
    for kernel, left in SESSION.alive.items():
        assert left, kernel
    for kind, s in SESSION.stats.items():
        assert 100 * s["undecided"] <= s["frames"] or s["frames"] == 0, kind
    assert {"mel_kernel", "mel_kernel<i16>", "mel_kernel_ragged", "mel_kernel_ragged<i16>", "gl_invert_kernel", "gl_istft_kernel (final)",
            "gl_istft_kernel (in-loop)", "gl_stft_update_kernel (first)", "gl_stft_update_kernel (momentum)"} <= set(SESSION.stats)
