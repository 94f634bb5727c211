"""The text stage's launch-by-launch restatement (oracle/text_chain_cases.py) on the CPU: chained, it IS the text stage; the
fp32 restatement of every launch passes its own claim on every case of tests/test_gpu_text_chain.py; every wrong restatement
fails where it applies; the workspace layout restated in ``iris/encoder.py`` is the ABI's.  No GPU.

Measured here over every case of the GPU test (eleven configurations, both weight seeds, dense B = 1 and 3 with P = 1 .. 97,
the two ragged shapes; EVERY launch of the chained forwards, not only the survivors), printed by ``pytest -s``:
    layernorm    ln32_gemm / ln32_rows against ln_bar: worst err / bar 0.280
    softplus     numpy's expf / log1pf against pred_bar: 0.960 -- the final addition's half ulp at the start of a binade
                 (u = 8.012: 8 u of a bar of 8.015 u); the chosen logits: 0.817
    attention    e32 up to 5.0e-07 with glorot weights, 3.15e-06 on "sharp"
    frames       0 of the 3 054 valid positions of each configuration undecided by float64 alone (the cap is 2 %): with u
                 restated exactly the margin is a few ulp of exp(pred).  Chosen logits: 0 of 853 at max 50, 14 of 853 (1.6 %)
                 at max 1 000 000, where an ulp of raw reaches 0.5 from 4e5 frames on.
"sharp": the float64 scores of blocks1's weights with the query and key kernels times 6.9 have a standard deviation of 7.90
(item 0 of B 3, P 97, seed 21; unscaled 0.17), and exp(m - mn) falls to 3.7e-06 between tiles of head 0.
"slice": the one-chunk chain differs from the sliced chain in 47 % of the pre-norm elements; at k = 1 ("odd", ffn2) in none.
``floor_half_up`` (floor(x + 0.5) in place of rint) differs from rint only where raw is exactly a half-integer, which is by
construction never a DECIDED position: no claim on the frames can see it, here or on the device, and the test says so.
``bias_first`` moves a pre-norm row by an ulp, inside most LayerNorm bars: it must fail on the launches without LayerNorm.
``eps_1e-5`` fails on EVERY LayerNorm launch of every configuration but "shifted", whose rows (mean 64, deviation 0.4) make dm
alone larger than epsilon's 4.5e-6; ``raw_moments`` is visible on "shifted" only.
"""
import ctypes

import numpy as np
import pytest

import encoder_cases
import encoder_restatement as R
from iris import _native
from oracle import chain_oracle as co
from oracle import text_chain_cases as tc

_cache = {}


def _models(name, si):
    if (name, si) not in _cache:
        _cache[(name, si)] = tc.make_models(name, tc.WEIGHT_SEEDS[si])
    return _cache[(name, si)]


def _chained(name, si, B, P, lengths=None):
    """(encoder plan, its tensors) or (None, None), (head plan, its tensors): one case chained on the CPU."""
    enc, head = _models(name, si)
    pe = te = None
    if enc is not None:
        pe = tc.encoder_plan(enc)
        te = tc.chain_forward(pe, {"ids": tc.make_ids(name, B, P, lengths)}, P, lengths)
        enc_in = te["enc_out"]
    else:
        enc_in = tc.make_enc_out(name, B, P)
    if lengths is not None:
        enc_in = tc.nan_past(enc_in, lengths)
    ph = tc.head_plan(head)
    return pe, te, ph, tc.chain_forward(ph, {"enc_in": enc_in}, P, lengths)


def test_the_two_existing_configurations_and_the_recipe_are_kept():
    for name in ("default", "small"):
        assert tc.CONFIGS[name] == encoder_cases.CONFIGS[name], name
    from iris.encoder import DurationPredictor, PhonemeEncoder
    for make in (lambda: PhonemeEncoder(**tc.CONFIGS["small"]["encoder"], seed=1), lambda: DurationPredictor(**tc.CONFIGS["small"]["head"], seed=2)):
        a, b = tc.randomise(make(), 5), R.randomise(make(), 5)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_fmaf32_is_the_c_oracles_fmaf():
    """``fmaf(x1, w1, x0)`` through ``chain_conv1d`` (two channels, the first weight 1) against ``fmaf32``, ties and sums whose
    float64 rounding alone would round twice included."""
    rng = np.random.default_rng(3)
    n = 40000
    x0, x1 = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    w1 = rng.standard_normal(16).astype(np.float32)
    x0[:10000] *= np.float32(2.0 ** -30)                                  # far apart: the sum's error decides the rounding
    x1[10000:12000] = np.float32(1 + 2.0 ** -12); w1[0] = np.float32(1 + 2.0 ** -12); x0[10000:12000] = np.float32(2.0 ** -24)
    w = np.zeros((16, 2, 1), np.float32)
    w[:, 0, 0], w[:, 1, 0] = 1.0, w1
    want = co.chain_conv1d(np.stack([x0, x1])[None], w, np.zeros(16, np.float32), 1, 8, [(0, n)])[0]      # [16, n]
    got = tc.fmaf32(x1[None, :], w1[:, None], x0[None, :])
    assert np.array_equal(got, want)
    twice = (x1[None, :].astype(np.float64) * w1[:, None] + x0[None, :]).astype(np.float32)
    print(f"fmaf32: {int((twice != want).sum())} of {want.size} sums round differently when rounded twice")


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_layout_restatement_is_the_abis(name):
    """``_workspace_layout``: its total is ``workspace_bytes`` and t0 / x0 / d0 sit where ``iris_*_tap`` reports, at several
    shapes (host-only queries: no device)."""
    lib = _native.load()
    enc, head = _models(name, 0)
    for B, P in ((1, 1), (1, 7), (3, 33), (5, 70), (2, 97), (7, 13)):
        for model in (enc, head):
            if model is None:
                continue
            layout, total = model._workspace_layout(B, P)
            assert 4 * total == model.workspace_bytes(B, P), (name, type(model).__name__, B, P)
            if model is head and head.num_layers == 0:
                continue
            off, n = ctypes.c_uint64(), ctypes.c_uint64()
            cfg = model.native_config()
            fn = f"iris_{model._abi_name}_tap"
            _native.check(fn, getattr(lib, fn)(ctypes.byref(cfg), B, P, ctypes.byref(off), ctypes.byref(n)))
            tap = "d0" if model is head else ("t0" if enc.num_blocks else "x0")
            assert off.value == 4 * layout[tap][0] and n.value == layout[tap][1], (name, fn, B, P)
    layout, total = _models("odd", 0)[0]._workspace_layout(3, 7)      # 21 rows: E 88 -> 1848, 3E -> 5544, ffn 260 -> 5460
    assert layout == {"x0": (0, 1848), "x1": (1856, 1848), "t0": (3712, 1848), "qkv": (5568, 5544), "attn": (11136, 1848),
                      "ffn": (12992, 5460)} and total == 18496
    layout, total = _models("odd", 0)[1]._workspace_layout(3, 7)      # hidden 20 -> 420
    assert layout == {"d0": (0, 420), "d1": (448, 420), "d2": (896, 420)} and total == 1344


def test_expected_launches_are_those_the_plan_finds():
    kinds = set()
    for name in tc.CONFIGS:
        enc, head = _models(name, 0)
        if enc is not None:
            got = [l["name"] for l in tc.judged(tc.encoder_plan(enc))]
            assert got == tc.expected_encoder(enc), (name, got)
            kinds |= {tc.kernel_form(l).split(" ")[0] for l in tc.judged(tc.encoder_plan(enc))}
        got = [l["name"] for l in tc.judged(tc.head_plan(head))]
        assert got == tc.expected_head(head), (name, got)
        kinds |= {tc.kernel_form(l).split(" ")[0] for l in tc.judged(tc.head_plan(head))}
    assert kinds == {"txt_embed_kernel", "txt_gemm_kernel", "txt_gemm_kernel<layernorm>", "txt_attention_kernel",
                     "txt_layernorm_kernel", "txt_duration_kernel", "txt_scan_kernel"}, kinds


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("name", [n for n in tc.CONFIGS if n != "slice"])
def test_chained_launches_are_the_text_stage(name):
    """The chained launches against tests/encoder_restatement.py in float64, held to 4 x the restatement's own fp32 error --
    that agreement shows the fused q | k | v matrix, the transpositions and the plan are the reference's operations."""
    enc, head = _models(name, 0)
    B, P, lengths = 3, 33, (1, 33, 20)
    pe, te, ph, th = _chained(name, 0, B, P, lengths)
    ids = te["ids"]
    want, _ = R.encoder_forward(enc.get_config(), enc.weights, np.where(ids == enc.vocab_size - 1, 0, ids), lengths)
    w32, _ = R.encoder_forward(enc.get_config(), enc.weights, np.where(ids == enc.vocab_size - 1, 0, ids), lengths, np.float32)
    e32, err = _rel(w32, want), _rel(te["enc_out"], want)
    enc_in = np.nan_to_num(th["enc_in"], nan=0.0)
    cfg = dict(head.get_config(), num_layers=head.num_layers)
    pw, _ = R.duration_forward(cfg, head.weights, enc_in, lengths)
    p32, _ = R.duration_forward(cfg, head.weights, enc_in, lengths, np.float32)
    e32p, errp = _rel(p32, pw), _rel(th["pred"], pw)
    line = f"text chain {name}: enc_out e32 {e32:.2e} chain {err:.2e}; pred e32 {e32p:.2e} chain {errp:.2e}"
    print(line)
    scale = SHIFT_SCALE if name == "shifted" else 1.0
    assert 0 < e32 < 1e-5 * scale and err <= 4 * e32, line
    assert 0 < e32p < 1e-5 and errp <= 4 * e32p, line


SHIFT_SCALE = 100.0     # "shifted": rows of mean 64 and deviation 0.4 lose two digits in any fp32 LayerNorm


def _all_cases():
    for name in tc.CONFIGS:
        for si in range(len(tc.WEIGHT_SEEDS)):
            for B in tc.DENSE_B:
                for P in tc.DENSE_P:
                    yield name, si, B, P, None
            for B, P, lengths in tc.RAGGED:
                yield name, si, B, P, lengths


def test_fp32_restatements_pass_their_claims_on_every_case_and_float64_decides_the_frames():
    total = tc.Tally()
    per_config = {}
    for name, si, B, P, lengths in _all_cases():
        tally = per_config.setdefault(name, tc.Tally())
        pe, te, ph, th = _chained(name, si, B, P, lengths)
        for plan, t in ((pe, te), (ph, th)):
            if plan is not None:
                names = tc.judge_forward(plan, t, P, lengths, tally, launches=plan)       # EVERY launch, not only survivors
                assert names == [l["name"] for l in plan]
    for name, tally in per_config.items():
        print(f"text chain {name}: {tally.line()}")
        assert all(0 < r < 1 for r in tally.worst.values()), (name, tally.worst)
        assert tally.valid - tally.decided <= 0.02 * tally.valid, (name, tally.decided, tally.valid)
        total.attn += tally.attn
        for k, v in tally.worst.items():
            total.worst[k] = max(total.worst.get(k, 0.0), v)
    print(f"text chain all: {total.worst}, attention e32 up to {total.e32():.2e}")
    assert 0 < total.e32() < 1e-5


def test_sharp_scores_have_a_standard_deviation_of_about_8():
    out = {}
    for name in ("blocks1", "sharp"):
        pe, te, _, _ = _chained(name, 0, 3, 97)
        out[name] = tc.attn_scores_std(te["qkv0"][0], 4)
        alpha_min = None
        if name == "sharp":
            a = te["qkv0"][0].astype(np.float64)
            E = a.shape[1] // 3
            s = (a[:, :64] / 8.0) @ a[:, E:E + 64].T                     # head 0: scores [query, key]
            tile_max = np.stack([s[:, j:j + 32].max(axis=1) for j in range(0, 97, 32)], axis=1)
            run = np.maximum.accumulate(tile_max, axis=1)
            alpha_min = float(np.exp(run[:, :-1] - run[:, 1:]).min())
    print(f"float64 score standard deviation: {out}; smallest exp(m - mn) between tiles of head 0: {alpha_min:.1e}")
    assert 6.0 < out["sharp"] < 10.0 and out["blocks1"] < 1.0 and alpha_min < 1e-4


def test_slice_order_shows_in_the_bits_of_the_slice_head():
    _, _, ph, th = _chained("slice", 0, 3, 33)
    l = ph[0]
    assert l["wb"][0].shape == (256, 520, 3)
    t = {"enc_in": th["enc_in"][0]}
    a, b = tc.gemm_sum(l, t), tc.gemm_sum(l, t, "one_chunk")
    differ = float((a != b).mean())
    print(f"slice: the one-chunk chain differs from the sliced chain in {100 * differ:.1f} % of the pre-norm elements")
    assert differ > 0.1
    _, te, _, _ = _chained("odd", 0, 3, 33)                               # k = 1: the slices cannot be seen
    pe = tc.encoder_plan(_models("odd", 0)[0])
    ffn2 = next(l for l in pe if l["name"] == "block0.ffn2+LN")
    t = {k: te[k][0] for k in ffn2["needs"]}
    assert np.array_equal(tc.gemm_sum(ffn2, t), tc.gemm_sum(ffn2, t, "one_chunk"))


# mutation -> the launches it changes, and where
_TOUCHES = {
    "one_chunk": None,                                   # test_slice_order_shows_in_the_bits_of_the_slice_head
    "floor_half_up": None,                               # invisible: see the docstring and the test below
    "remainder_dropped": lambda l, n: l["kind"] == "gemm" and l["wb"][0].shape[1] > tc.SLICE and l["wb"][0].shape[1] % tc.SLICE,
    # an ulp of a pre-norm row is inside most LayerNorm bars, not all (a channel far above the row's mean |s|): either outcome
    "bias_first": lambda l, n: l["kind"] == "gemm" and (True if l["norm"] is None else None),
    "relu_after_residual": lambda l, n: l["kind"] == "gemm" and l["res"] is not None,
    "no_residual": lambda l, n: l["kind"] == "gemm" and l["res"] is not None,
    "unbiased_variance": lambda l, n: l["norm"] is not None,
    "eps_1e-5": lambda l, n: l["norm"] is not None,
    "raw_moments": lambda l, n: l["kind"] == "ln",      # on "shifted" only (below)
    "scale_before_bias": lambda l, n: l["kind"] == "attn" and n > 1,
    "padded_key": lambda l, n: l["kind"] == "attn" and n % tc.KEY_TILE,
    "tile_key_dropped": lambda l, n: l["kind"] == "attn" and n >= tc.KEY_TILE,
    # a second tile of one key leaves exp(m - mn) at exactly 1 unless that key is a query's largest: either outcome below 64
    "no_rescale": lambda l, n: l["kind"] == "attn" and (n >= 2 * tc.KEY_TILE or (None if n > tc.KEY_TILE else False)),
    "inclusive_offsets": lambda l, n: l["kind"] == "scan",
    "embed_no_position": lambda l, n: l["kind"] == "embed",
    "naive_softplus": None,                              # on the chosen logits (below)
    "no_upper_clip": None,
}


def _fails(l, t, got, e32):
    try:
        kind, r = tc.judge(l, t, got, l["name"])
    except AssertionError:
        return True
    return kind == "attention" and r[0] > 4 * e32


def test_every_wrong_restatement_fails_its_claim_where_it_applies():
    assert set(_TOUCHES) == set(tc.MUTATIONS)
    failed = {m: 0 for m in tc.MUTATIONS}
    cases = [(name, 3, 33, (1, 33, 20)) for name in tc.CONFIGS] + [(name, 1, 65, None) for name in ("small", "odd", "dk128", "dk40", "sharp", "slice")]
    e32 = 0.0
    chained = []
    for name, B, P, lengths in cases:
        pe, te, ph, th = _chained(name, 0, B, P, lengths)
        for plan, t in ((pe, te), (ph, th)):
            if plan is None:
                continue
            tally = tc.Tally()
            tc.judge_forward(plan, t, P, lengths, tally, launches=plan)
            e32 = max(e32, tally.e32())
            chained.append((name, B, P, lengths, plan, t))
    assert e32 > 0
    for name, B, P, lengths, plan, t in chained:
        for l in plan:
            for b in range(B):
                n = P if lengths is None else lengths[b]
                ti = {k: t[k][b, :n] for k in l["needs"]}
                for m, touches in _TOUCHES.items():
                    if touches is None or (m == "raw_moments" and name != "shifted"):
                        continue
                    if m == "eps_1e-5" and name == "shifted":       # a mean of 150 deviations: dm alone is above epsilon's 4.5e-6
                        continue
                    if touches(l, n) is None:
                        continue
                    bad = _fails(l, ti, tc.emulate(l, ti, m), e32)
                    if touches(l, n):
                        assert bad, (name, l["name"], m, b, n)
                        failed[m] += 1
                    else:
                        assert not bad, (name, l["name"], m, b, n)
    # the duration launch on chosen logits
    for max_frames in (50, 1_000_000):
        head = tc.sweep_head(max_frames)
        l = tc.head_plan(head)[0]
        u = tc.sweep_logits(max_frames)
        x = np.zeros((len(u), 4), np.float32)
        x[:, 0] = u
        x[:, 1:] = np.random.default_rng(1).standard_normal((len(u), 3))
        t = {"enc_in": x}
        assert np.array_equal(tc.dot32(x, *l["wb"]), u)
        kind, r = tc.judge(l, t, tc.emulate(l, t), "sweep")
        assert r[0] < 1 and r[2] - r[1] <= 0.02 * r[2], r
        print(f"duration sweep max {max_frames}: softplus err / bar {r[0]:.3f}, {r[2] - r[1]} of {r[2]} undecided")
        for m in ("naive_softplus", "no_upper_clip"):
            assert _fails(l, t, tc.emulate(l, t, m), e32), (m, max_frames)
            failed[m] += 1
        # floor(x + 0.5) differs from rint only on exact ties, and a tie is never decided
        pred, frames = tc.emulate(l, t)
        _, wrong = tc.emulate(l, t, "floor_half_up")
        assert not _fails(l, t, (pred, wrong), e32)
        raw = np.arange(2, 60, dtype=np.float64) + 0.5                    # 0.5 and 1.5 clip to 1 either way
        assert ((tc.frames_of(raw, 10 ** 6) != tc.frames_of(raw, 10 ** 6, "floor_half_up")) == (np.arange(2, 60) % 2 == 0)).all()
        assert not tc.decided(np.log(np.array([2.5, 4.5, 10.5])), max_frames)[1].any()
    for m, n in failed.items():
        if _TOUCHES[m] is None and m in ("one_chunk", "floor_half_up"):      # shown elsewhere / shown invisible above
            continue
        print(f"wrong restatement {m}: fails its claim on {n} launch items")
        assert n, f"{m} fails no claim: the claim is vacuous"
