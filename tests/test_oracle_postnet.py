"""The PostNet's chain restatement (oracle/postnet_cases.py) on the CPU: it is the PostNet, its claims are not vacuous, and
the shapes of tests/test_gpu_postnet_chain.py reach both tile heights.  No GPU.

``e32 = max |fp32 restatement - fp64 restatement| / max(1, max |fp64|)`` (oracle/postnet_oracle.e32: the numpy text of the
reference in fp32 against itself in fp64) and the chain's own distance to fp64, relative in the same way, measured here for
(config, weight seeds, B x T), mel seed 21 (log-mel):
    config   seeds     B x T    e32        chain
    default  (3, 4)    2 x 65   1.69e-07   3.77e-07
    default  (13, 14)  2 x 65   2.35e-07   4.46e-07
    deeper   (3, 4)    2 x 65   2.33e-07   4.66e-07
    deeper   (13, 14)  2 x 65   2.37e-07   3.82e-07
    small    (3, 4)    2 x 65   9.83e-08   8.81e-08
    small    (13, 14)  2 x 65   1.24e-07   1.27e-07
    narrow   (3, 4)    2 x 65   5.28e-08   6.62e-08
    narrow   (13, 14)  2 x 65   5.73e-08   6.92e-08
    narrow2  (3, 4)    2 x 65   1.15e-07   1.24e-07
    narrow2  (13, 14)  2 x 65   5.70e-08   9.06e-08
The chain is held to ``4 * e32``, the bar the encoder, VAE, mel and Griffin-Lim stages use, and ``4 * e32`` to the fixed 2e-5
it replaces in tests/test_postnet.py.
"""
import numpy as np
import pytest

from oracle import f32_cases as fc
from oracle import postnet_cases as pc
from oracle import postnet_oracle as porc

WHOLE = [(name, seeds, 2, 65) for name in pc.CONFIGS for seeds in pc.WEIGHT_SEEDS]
MUTATION_SHAPES = [(1, 1), (1, 4), (3, 33), (2, 65)]


@pytest.mark.parametrize("config,seeds,B,T", WHOLE, ids=[f"{c[0]}-{c[1][0]}-{c[2]}x{c[3]}" for c in WHOLE])
def test_chained_layers_are_the_postnet(config, seeds, B, T):
    pn = pc.make_postnet(config, seeds)
    mel = pc.case_mel(config, B, T, 21)
    want = porc.postnet_forward_raw(pn.weights, mel, pn.num_layers)
    e32 = porc.e32(pn.weights, mel, pn.num_layers)
    outs, out = pc.chain_postnet(pn, mel)
    assert len(outs) == pn.num_layers and out.shape == mel.shape and out.dtype == np.float32
    err = float(np.abs(out - want).max() / max(1.0, np.abs(want).max()))
    print(f"postnet chain {config} seeds {seeds} {B}x{T}: e32 {e32:.2e} chain {err:.2e}")
    assert 0 < e32 and 4 * e32 <= 2e-5, e32
    assert err <= 4 * e32, (err, e32)


def _claims(pn, mel):
    """Every claim of one forward as (kind, layer, check(mutation) -> raises AssertionError when the claim fails); the
    'device' is the restatement itself, mutated."""
    layers = pc.folded_layers(pn)
    outs, _ = pc.chain_postnet(pn, mel)
    T = mel.shape[2]
    rows = [(0, T)]
    claims = []
    for i, wb in enumerate(layers):
        x = mel if i == 0 else outs[i - 1]
        chunk = pc.layer_chunk(wb, i)
        pre = pc.chain_layer(x, wb, chunk, rows)
        if i < len(layers) - 1:
            claims.append(("hidden", i, lambda m, x=x, wb=wb, chunk=chunk, pre=pre, i=i: pc.judge_hidden(
                pc.hidden_layer(x, wb, chunk, rows, m), pre, fc.TOL_TANH, f"layer {i}")))
        else:
            claims.append(("last", i, lambda m, x=x, wb=wb, chunk=chunk, pre=pre, i=i: pc.judge_last(
                pc.chain_layer(x, wb, chunk, rows, m), pre, f"layer {i}")))
    res = outs[-1].transpose(0, 2, 1)
    claims.append(("output", len(layers), lambda m: pc.judge_output(pc.add_residual(mel, res, m), mel, res, None, "output")))
    return claims


def _fails(check, mutation):
    try:
        check(mutation)
    except AssertionError:
        return True
    return False


def test_claims_hold_unmutated_and_every_mutation_fails_its_claim():
    touched = {"drop_first_tap": ("hidden", "last"), "drop_last_tap": ("hidden", "last"), "pad_off_by_one": ("hidden", "last"),
               "tanh_before_bias": ("hidden",), "residual_untransposed": ("output",)}
    assert set(touched) == set(pc.MUTATIONS)
    failed = {(m, kind): [] for m, kinds in touched.items() for kind in kinds}
    for config in pc.CONFIGS:
        pn = pc.make_postnet(config, pc.WEIGHT_SEEDS[0])
        k = pn.kernel_size
        for B, T in MUTATION_SHAPES:
            mel = pc.case_mel(config, B, T, 23)
            for kind, layer, check in _claims(pn, mel):
                check(None)                                                   # the claim holds for the restatement itself
                for m, kinds in touched.items():
                    if kind not in kinds:
                        assert not _fails(check, m), (config, B, T, kind, layer, m)   # ... and for what cannot change it
                        continue
                    if _fails(check, m):
                        failed[(m, kind)].append((config, B, T, layer))
                    elif kind == "output":
                        assert T == 1, (config, B, T, m)                      # [B, 1, C] untransposed IS [B, C, 1]
                    elif m != "tanh_before_bias":
                        assert T <= (k - 1) // 2, (config, B, T, layer, m)    # an edge tap / a shifted row seen by no output row
    for key, cases in failed.items():
        print(f"mutation {key}: fails its claim on {len(cases)} cases")
        assert cases, f"mutation {key} fails no claim: the claim is vacuous"
    # every config catches every mutation it can, not one lucky case
    for key, cases in failed.items():
        assert {c[0] for c in cases} == set(pc.CONFIGS), (key, cases)


def test_shapes_reach_both_tile_heights_at_256_cus():
    seen = {}
    for config, (n_mels, layers, channels, k) in pc.CONFIGS.items():
        shapes = [(B, T) for B in pc.DENSE_B for T in pc.DENSE_T]
        if config == pc.RAGGED_CONFIG:
            shapes += [(B, T) for B, T, _ in pc.RAGGED]
        for B, T in shapes:
            for i in range(layers):
                mt, rows = pc.layer_tile(n_mels if i == layers - 1 else channels, B, T, 256)
                assert rows == 32 * mt * (4 if (n_mels if i == layers - 1 else channels) <= 32 else 1)
                seen.setdefault(mt, set()).add((config, B, T, i))
    assert set(seen) == {1, 2}, sorted(seen)
    # the 64-row tiles: the hidden layers of the (8, 2048) case and nothing else; its last layer (one C_out block) runs 32-row ones
    assert seen[2] == {("default", 8, 2048, 0), ("default", 8, 2048, 1)}, seen[2]
    assert ("default", 8, 2048, 2) in seen[1]
    for B, T, lengths in pc.RAGGED:
        assert len(lengths) == B and all(0 <= n <= T for n in lengths)


def test_chunks_are_those_of_the_kernel():
    """``launch_conv``: 80 channels in one chunk for the channels-first mel in front of more than 64 output channels, 32 where
    both channel counts are at most 32, else 64."""
    got = {name: [pc.layer_chunk(wb, i) for i, wb in enumerate(pc.folded_layers(pc.make_postnet(name, pc.WEIGHT_SEEDS[0])))]
           for name in pc.CONFIGS}
    assert got == {"default": [80, 64, 64], "deeper": [80, 64, 64, 64], "small": [32, 32], "narrow": [32] * 12,
                   "narrow2": [32, 32]}, got


def test_judged_rows_share():
    for B, T, lengths in pc.RAGGED:
        for n in lengths:
            if n:
                rows = fc.judged_rows(1, n, 256 * 256 * 5)
                assert fc.n_rows(rows) >= fc.MIN_SHARE * n
