"""The fp32 fmaf chain on the CPU (oracle/chain_oracle.c, oracle/f32_cases.py): what tests/test_gpu_f32_chain.py holds every
fp32 launch to, bit for bit.  No device.

* The chain is the convolution: |chain - conv_fp64| <= (k C_in + 2) 2^-24 absconv elementwise (the standard bound of a
  sequential fp32 sum; absconv = the layer on |x|, |w|, |b|, |res|).
* The C code is the chain: an independent restatement in exact rational arithmetic, rounded once to fp32 per step,
  gives the same bits.
* Order is visible: each wrong restatement changes every launch it touches and no other (shares below).
* The shape list of the GPU test is held to the host-only launch plan.
"""
import collections
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import chain_oracle as co
from oracle import f32_cases as fc

# (kind, C_in, C_out, k, dilation or stride, chunk, L)
LAYER_CASES = ([("conv", 32, 32, k, d, 32, 41) for k in (3, 7, 11) for d in (1, 3, 5)]          # the nine V1 (k, d) pairs
               + [("conv", 128, 128, 11, 5, 64, 23), ("conv", 80, 512, 7, 1, 80, 19)]           # two chunks; conv_pre
               + [("convt", 512, 256, 16, 8, 64, 5), ("convt", 256, 128, 16, 8, 64, 6),         # the four upsamplers
                  ("convt", 128, 64, 4, 2, 64, 9), ("convt", 64, 32, 4, 2, 64, 11)]
               + [("conv", c, c, 5, 2, 32, 29) for c in (6, 12, 24, 40, 80)]                    # ragged channel counts
               + [("convt", 12, 6, 9, 3, 32, 7), ("convt", 48, 24, 8, 4, 64, 5)])               # taps = 3; two taps, 48 channels


def _layer(case, seed):
    kind, ci, cout, k, arg, chunk, L = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, ci, L)).astype(np.float32)
    w = (rng.standard_normal((cout, ci, k) if kind == "conv" else (ci, cout, k)) / np.sqrt(ci * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((2, cout, L)).astype(np.float32) if kind == "conv" and seed % 2 else None
    return x, w, b, res


def _ref64(case, x, w, b, res):
    kind, _, _, k, arg = case[:5]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    if kind == "conv":
        y = F.conv1d(t(x), t(w), t(b), dilation=arg, padding=arg * (k - 1) // 2)
        return (y if res is None else y + t(res)).numpy()
    return F.conv_transpose1d(t(x), t(w), t(b), stride=arg, padding=(k - arg) // 2).numpy()


def _chain(case, x, w, b, res, rows=None, variant=0):
    kind, _, _, k, arg, chunk, L = case
    if kind == "conv":
        return co.chain_conv1d(x, w, b, arg, chunk, rows or [(0, L)], residual=res, variant=variant)
    return co.chain_conv_transpose1d(x, w, b, arg, chunk, rows or [(0, L * arg)], variant=variant)


@pytest.mark.parametrize("n", range(len(LAYER_CASES)))
def test_the_chain_is_the_convolution(n):
    case = LAYER_CASES[n]
    x, w, b, res = _layer(case, 100 + n)
    got = _chain(case, x, w, b, res)
    want = _ref64(case, x, w, b, res)
    absconv = _ref64(case, np.abs(x), np.abs(w), np.abs(b), None if res is None else np.abs(res))
    assert got.shape == want.shape and got.dtype == np.float32
    K = case[3] * case[1] + 2
    assert (np.abs(got.astype(np.float64) - want) <= K * 2.0 ** -24 * absconv).all()
    # row ranges return those rows of the same tensor
    L_out = got.shape[2]
    rows = [(0, 1), (L_out // 2, L_out // 2 + 3), (L_out - 1, L_out)]
    assert np.array_equal(_chain(case, x, w, b, res, rows), co.take_rows(got, rows))


# ---- an independent restatement in exact rational arithmetic --------------------------------------------------------------
def r32(q):
    """Fraction -> the nearest fp32 value (ties to even), as a Fraction: ONE rounding, no detour through fp64."""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                            # 2^e <= a < 2^(e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    r = round(a / ulp) * ulp                              # (round() of a Fraction: ties to even)
    assert r < Fraction(2) ** 128
    return r if q > 0 else -r


def fma_q(a, b, c):
    return r32(Fraction(float(a)) * Fraction(float(b)) + c)


def element_q(case, x, w, b, res, bi, co_, o):
    """One output element of the layer, restated from the chain's definition."""
    kind, ci_n, _, k, arg, chunk, L = case
    order = (0, 4, 1, 5, 2, 6, 3, 7)
    if kind == "conv":
        taps = [(o - arg * (k - 1) // 2 + kap * arg, kap) for kap in range(k)]
        wt = lambda ci, kk: w[co_, ci, kk]
    else:
        u, n_taps = arg, -(-k // arg)
        q = o + (k - u) // 2
        ph, i = q % u, q // u
        taps = [(i - (n_taps - 1) + kap, ph + (n_taps - 1 - kap) * u) for kap in range(n_taps)]
        wt = lambda ci, kk: w[ci, co_, kk]
    acc = Fraction(0)
    for c0 in range(0, ci_n, chunk):
        for row, kk in taps:
            for g in range(c0, min(c0 + chunk, ci_n), 8):
                for e in order:
                    ci = g + e
                    xv = x[bi, ci, row] if (ci < ci_n and 0 <= row < L and kk < k) else 0.0
                    wv = wt(ci, kk) if (ci < ci_n and kk < k) else 0.0
                    acc = fma_q(xv, wv, acc)             # (padding included: fmaf(0, w, acc))
    y = r32(acc + Fraction(float(b[co_])))
    if res is not None:
        y = r32(y + Fraction(float(res[bi, co_, o])))
    return y


def test_r32_rounds_once_to_nearest_even():
    one, eps = Fraction(1), Fraction(2) ** -24
    assert r32(one + eps) == one and r32(one + 3 * eps) == one + 4 * eps and r32(one + eps + eps / 2 ** 40) == one + 2 * eps
    assert r32(Fraction(2) ** -150) == 0 and r32(Fraction(3, 2) * Fraction(2) ** -149) == Fraction(2) ** -148
    for v in (0.1, -3.3e-7, 1e30, 1.17e-38):
        assert r32(Fraction(v)) == Fraction(float(np.float32(v)))


@pytest.mark.parametrize("n", range(len(LAYER_CASES)))
def test_the_c_code_is_the_chain(n):
    """12 elements per case (first and last rows included), 276 in all, bit for bit -- and both forms of the C loop (fmaf as
    glibc's function, fmaf as the FMA instruction where the host has one) give the same tensor."""
    case = LAYER_CASES[n]
    x, w, b, res = _layer(case, 100 + n)
    got = _chain(case, x, w, b, res)
    lib = co.load()
    lib.chain_set_portable(1)
    try:
        assert lib.chain_uses_fma_unit() == 0
        assert np.array_equal(_chain(case, x, w, b, res), got)
    finally:
        lib.chain_set_portable(0)
    rng = np.random.default_rng(n)
    L_out = got.shape[2]
    picks = [(0, 0, 0), (1, got.shape[1] - 1, L_out - 1)] + [(int(rng.integers(2)), int(rng.integers(got.shape[1])),
                                                              int(rng.integers(L_out))) for _ in range(10)]
    for bi, c, o in picks:
        want = element_q(case, x, w, b, res, bi, c, o)
        assert Fraction(float(got[bi, c, o])) == want, (case, bi, c, o)


def test_conv_post_and_helpers_are_their_definitions():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 6, 17)).astype(np.float32)
    w = rng.standard_normal((1, 6, 7)).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32)
    got = co.chain_conv_post_preact(x, w, b, [(0, 17)])
    for bi, o in ((0, 0), (1, 16), (0, 8), (1, 3)):
        acc = Fraction(float(b[0]))                       # bias first, taps ascending, channels ascending
        for kap in range(7):
            for ci in range(6):
                row = o - 3 + kap
                acc = fma_q(x[bi, ci, row] if 0 <= row < 17 else 0.0, w[0, ci, kap], acc)
        assert Fraction(float(got[bi, o])) == acc
    v = np.array([-2.5, -0.0, 0.0, 3.0, -1e-30], dtype=np.float32)
    assert [Fraction(float(t)) for t in co.lrelu32(v)] == [r32(Fraction(float(t)) * Fraction(float(np.float32(0.1)))) if t < 0 else
                                                            Fraction(float(t)) for t in v]
    ys = [rng.standard_normal(50).astype(np.float32) for _ in range(3)]
    m = co.mean32(ys)
    for i in range(50):
        s = r32(r32(Fraction(float(ys[0][i])) + Fraction(float(ys[1][i]))) + Fraction(float(ys[2][i])))
        assert Fraction(float(m[i])) == r32(s / 3)


# ---- wrong restatements are visible ----------------------------------------------------------------------------------------
WALKS = [("v1", 1, 2, 71), ("generic", 3, 37, 72), ("post24", 3, 70, 73)]


@pytest.fixture(scope="module")
def walks():
    out = {}
    for name, B, T, seed in WALKS:
        cfg, _, W = fc.setup(name)
        mel = fc.shape_mel((name, name, B, T, None, seed))
        out[name] = list(fc.walk(cfg, fc.numpy_weights(W), mel, fc.plan_launches(cfg, B, T)))
    return out


@pytest.mark.parametrize("wrong", fc.WRONG)
def test_order_is_visible(walks, wrong):
    """Each wrong restatement differs from the chain in at least one element of every launch it touches and in none of any
    other launch.  Share of differing elements per (case: min ... max over the touched launches):
        ascending (channels 0 ... 7 inside a group)   v1 0.40 ... 0.87, generic 0.17 ... 0.74, post24 0.28 ... 0.81
                                                      (every launch but conv_post, whose own order is ascending)
        tap_major (taps outside chunks)               v1 0.47 ... 0.97 on the 39 launches with C_in > chunk (conv_pre's 80
                                                      channels are ONE chunk: untouched); post24 0.78 on its one such launch
                                                      (ups.0, 96 channels); generic has none (C_in <= 64): bit-identical
        chunk64 (conv_pre as 64 + 16 channels)        v1 0.82 (conv_pre only); generic and post24 have no 80-channel chunk:
                                                      untouched, bit-identical
        bias_first                                    v1 0.63 ... 0.95, generic 0.55 ... 0.86, post24 0.39 ... 0.81
        res_first ((acc + res) + bias)                v1 0.23 ... 0.31, generic 0.21 ... 0.34, post24 0.26 ... 0.32
        mean_mul (* (1 / 3))                          v1 0.52 ... 0.75, post24 0.65 ... 0.78 (of the consumer's outputs)
        mean_assoc ((y0 + (y1 + y2)) / 3)             v1 0.46 ... 0.72, post24 0.58 ... 0.73
    generic has TWO branches: (y0 + y1) * fp32(1 / 2) is exact and the sum of two has one order, so both mean variants are
    bit-identical there (as the bf16 walk found for its two-branch case); a launch that reads a stored mean is untouched.
    (The figures are reprinted by ``pytest -s``.)"""
    for name, recs in walks.items():
        shares = []
        for rec in recs:
            other = rec["restate"](wrong)
            differs = float((other != rec["want"]).mean())
            if wrong in rec["touches"]:
                assert differs > 0, (name, rec["label"], wrong)
                shares.append(differs)
            else:
                assert differs == 0, (name, rec["label"], wrong)
        print(f"{wrong} {name}: touched {len(shares)} of {len(recs)} launches, share "
              + (f"{min(shares):.2f} ... {max(shares):.2f}" if shares else "-"))
        if name == "v1" or (name == "post24" and wrong in ("mean_mul", "mean_assoc")):
            assert shares, (name, wrong)


def test_walk_feeding_itself_is_the_generator(walks):
    """The walk's own waveform against the torch oracle (<= 1e-5: both are fp32 forwards in different orders)."""
    from oracle import hifigan_oracle as orc
    cfg, sd, _ = fc.setup("v1")
    mel = fc.shape_mel(("v1", "v1", 1, 2, None, 71))
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), mel).numpy()[:, 0, :]
    rec = walks["v1"][-1]
    assert rec["kind"] == "wav" and np.abs(np.tanh(rec["want"].astype(np.float64)) - want).max() <= 1e-5
    # conv_pre, per stage the upsampler and 3 pairs x 3 branches x (2 tensors; 1 where the pair is fused: C = 64 / 32), conv_post
    assert len(walks["v1"]) == 1 + 2 * (1 + 18) + 2 * (1 + 9) + 1


# ---- the shapes are held to the plan -----------------------------------------------------------------------------------------
def test_shape_list_visits_every_kernel_instance_of_the_grid():
    cfg = fc.CONFIGS["v1"][0]()
    scan = set()
    for B in fc.SCAN_BATCHES:
        for T in fc.SCAN_FRAMES:
            if B * T > fc.SCAN_MAX_FRAMES:
                break
            scan |= {(r["where"], r["kernel"]) for r in fc.plan_launches(cfg, B, T)}
    seen = set()
    for sid, name, B, T, spec, _ in fc.SHAPES:
        if name == "v1":
            assert B in fc.SCAN_BATCHES and T in fc.SCAN_FRAMES and B * T <= fc.SCAN_MAX_FRAMES, sid
            seen |= fc.visited(cfg, B, T, spec)
    assert seen == scan, (sorted(scan - seen), sorted(seen - scan))


def test_shape_list_yields_every_plan_kind():
    from test_planner_sweep import PLAN_KINDS, plan_kinds
    cfg = fc.CONFIGS["v1"][0]()
    kinds = collections.Counter()
    for sid, name, B, T, spec, _ in fc.SHAPES:
        if name == "v1":
            kinds.update(plan_kinds(cfg, B, T).keys())
    assert set(kinds) == PLAN_KINDS, sorted(PLAN_KINDS - set(kinds))


def test_shapes_outside_v1_reach_the_fallback_kernels():
    g = dict(fc.visited(fc.CONFIGS["generic"][0](), 3, 37))
    p = dict(fc.visited(fc.CONFIGS["post24"][0](), 3, 70))
    assert p["post"] == "conv_post_tanh_kernel<0>" and g["post"] == "conv_post_rows_kernel"
    for where in ("ups.1", "ups.2", "mrf.0", "mrf.1", "mrf.2"):        # the polyphase fallback; grouped Conv1d launches
        assert g[where].startswith("conv_mfma_f32_kernel<"), (where, g[where])
    for where in ("ups.0", "ups.1", "mrf.0", "mrf.1"):
        assert p[where].startswith("conv_mfma_f32_kernel<"), (where, p[where])


_CIC = re.compile(r"^(?:mrf_)?conv_mfma_f32_kernel<\d+, \d+, \d+, (\d+)[,>]")


def test_chunk_values_are_those_of_the_recorded_kernel_names(walks):
    """The chunk a launch is restated with is the CIC of its recorded kernel name; the kernels whose name carries none have
    one instantiation of it (convt_mfma_f32.h: CIC = 64; mrf_small_f32.h: kSmallCic = 64; the pairs: the whole C)."""
    n = 0
    for sid, name, B, T, spec, _ in fc.SHAPES:
        cfg = fc.CONFIGS[name][0]()
        for r in fc.walked(fc.plan_launches(cfg, B, T), spec):
            if r["where"] == "post":
                continue
            c_in = (cfg.in_channels if r["where"] == "pre" else
                    cfg.stage_channels(int(r["where"][4:])) * (2 if r["where"].startswith("ups") else 1))
            m = _CIC.match(r["kernel"])
            want = int(m.group(1)) if m else (64 if r["kernel"].startswith(("convt_", "mrf_small_")) else c_in)
            assert m or r["kernel"].startswith(("convt_mfma_f32_kernel<", "mrf_small_f32_kernel", "mrf_pair_f32")), r
            assert co.chunk_of(r["kernel"], c_in) == want, r
            n += 1
    assert n > 100
    for recs in walks.values():
        for rec in recs:
            m = _CIC.match(rec["kernel"])
            if m:
                assert rec["chunk"] == int(m.group(1)), rec["label"]
    assert {rec["chunk"] for rec in walks["v1"] if rec["where"] == "pre"} == {80}


def test_single_layer_chunk_rule_is_the_recorded_one():
    """``fc.single_layer_chunk`` (the single-layer GPU tests have no recorded kernel name to read) against the CIC in the names
    ``describe_plan`` records for layers of the same channel counts: conv_pre, polyphase upsamplers and MRF steps of the
    three configurations."""
    n = 0
    for name, B, T in (("v1", 1, 300), ("v1", 1, 1), ("generic", 3, 37), ("post24", 3, 70)):
        cfg = fc.CONFIGS[name][0]()
        for r in fc.plan_launches(cfg, B, T):
            m = _CIC.match(r["kernel"])
            if not m:
                continue
            if r["where"] == "pre":
                ci, cout, cf = cfg.in_channels, cfg.upsample_initial_channel, True
            else:
                c = cfg.stage_channels(int(r["where"][4:]))
                ci, cout, cf = (2 * c, c, False) if r["where"].startswith("ups") else (c, c, False)
            assert fc.single_layer_chunk(ci, cout, cf) == int(m.group(1)), (name, r)
            n += 1
    assert n >= 30
