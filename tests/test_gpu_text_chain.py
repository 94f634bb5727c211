"""Every launch of the phoneme encoder and the duration head against its restatement, on the launch's OWN stored input
(oracle/text_chain_cases.py: the plan, the claims and the derivation of their bars; tests/test_oracle_text_chain.py: the same
claims on the CPU, the wrong restatements, the layout pins).

After a forward the workspace still holds what its later launches did not overwrite (``_read_buffers``); a launch whose inputs
AND output survive is judged.  Read off ``enc_forward`` / ``dur_forward`` (``text_chain_cases.expected_*``), N blocks:
    encoder  N = 0: embed, final_norm.  N = 1: embed, the five launches of block 0, final_norm.  N = 2: the five launches of
             block 1, final_norm.  N >= 3: the last block's attention, ffn1, ffn2 + LN, and final_norm.
             Not judged: with N = 2, embed and block 0 (block 1 reuses x0, qkv, attn, x1 and ffn); with N >= 3 also the last
             block's qkv GEMM and out + LN launch -- that block's input x0 is overwritten by its own ffn2 store.
    head     every conv + LayerNorm layer (num_layers <= 3), the duration launch, the scan.
Every test asserts the list of launches it judged, and that the layout restatement's total is ``workspace_bytes``.

Configurations (``text_chain_cases.CONFIGS``): "default", "small" (the existing two), "blocks1", "blocks2", "odd" (Dk 88, 3E = 264:
nine C_out tiles, ffn 260: slices 256 + 8 and a last tile of 4 channels; head 88 -> 20, k 7, max 50), "dk128" (nd = 4), "dk40",
"bare" (no block; a head without conv layers), "shifted" ("bare" with rows of mean 64), "slice" (a head alone, C_in 520 with
three taps), "sharp" (score standard deviation 7.9).  Two weight seeds; dense B = 1 and 3, P = 1, 7, 31, 32, 33, 64, 65, 97;
ragged (5, 70; 70, 1, 32, 33, 17) and (3, 33; 1, 33, 20) on every configuration, the token row of every padded id NaN and the
head's input NaN past each length.

Measured on the DEVICE (MI355X), worst err / bar per claim over both seeds, both batch sizes and the ragged shapes:
    config      layernorm   softplus   attention err / (4 e32)   4 e32 up to
    default     0.265       0.946      0.411                     1.7e-06
    small       0.245       0.811      0.403                     1.2e-06
    blocks1     0.255       0.887      0.406                     4.4e-07
    blocks2     0.263       0.931      0.337                     2.2e-06
    odd         0.273       0.940      0.392                     6.1e-07
    dk128       0.234       0.889      0.371                     2.0e-06
    dk40        0.243       0.801      0.429                     4.0e-07
    bare        0.228       0.951      -
    shifted     0.238       0.922      -
    slice       0.169       0.856      -
    sharp       0.241       0.907      0.321                     1.3e-05
    chosen logits (max 50 and 1 000 000) 0.817; in_dim 260: 0.718, 516: 0.888
and 2 506 launch items (a launch on one item of a batch) equal to their restatement bit for bit -- embed, every GEMM without
LayerNorm, the scan --, 53.7 million elements judged, every row past a length exactly 0, no frame count different where
float64 decides it (undecided: 0 of every forward's positions; 14 of 853 chosen logits at max 1 000 000, under the 2 % cap).
The duration launch's logit is restated exactly, so its softplus bar holds expf, log1pf and one addition only; 0.95 is the
addition's half ulp at the start of a binade.  No launch differed from its restatement and no kernel changed.  The file ran
in 7 s.
Every test prints its figures (``pytest -s``).
"""
import time

import numpy as np
import pytest
import torch

import encoder_restatement as R
from iris import encoder as E
from oracle import text_chain_cases as tc

pytestmark = pytest.mark.gpu

_cache = {}


def _models(name, si):
    if (name, si) not in _cache:
        _cache[(name, si)] = tc.make_models(name, tc.WEIGHT_SEEDS[si])
    return _cache[(name, si)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buffers(model, B, P):
    bufs, total = model._read_buffers(B, P)
    assert total == model.workspace_bytes(B, P), (type(model).__name__, B, P, total)
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _lens(lengths):
    return None if lengths is None else np.asarray(lengths, dtype=np.int32)


def _run_head(head, enc_in, lengths, tally):
    """One head forward on ``enc_in`` (NaN past each length when ragged), every surviving launch judged."""
    B, P = enc_in.shape[:2]
    if lengths is not None:
        enc_in = tc.nan_past(enc_in, lengths)
    pred, frames, offsets, totals = head.forward_device(_dev(enc_in), _lens(lengths))
    torch.cuda.synchronize()
    plan = tc.head_plan(head)
    t = tc.from_buffers(plan, _buffers(head, B, P), B, P)
    t.update(enc_in=enc_in, pred=pred.cpu().numpy(), frames=frames.cpu().numpy(), offsets=offsets.cpu().numpy(), totals=totals.cpu().numpy())
    assert tc.judge_forward(plan, t, P, lengths, tally) == tc.expected_head(head)
    return t


def _run(name, si, B, P, lengths, tally):
    """The encoder on seeded ids, then the head on the DEVICE's enc_out: both forwards judged launch by launch."""
    enc, head = _models(name, si)
    if enc is None:
        return _run_head(head, tc.make_enc_out(name, B, P), lengths, tally)
    ids = tc.make_ids(name, B, P, lengths)
    enc_out = enc.forward_device(_dev(ids), _lens(lengths))
    torch.cuda.synchronize()
    plan = tc.encoder_plan(enc)
    t = tc.from_buffers(plan, _buffers(enc, B, P), B, P)
    t.update(ids=ids, enc_out=enc_out.cpu().numpy())
    assert tc.judge_forward(plan, t, P, lengths, tally) == tc.expected_encoder(enc)
    return _run_head(head, t["enc_out"], lengths, tally)


def _close(tally, title, t0):
    ratio = tally.check_attention()
    assert tally.valid - tally.decided <= 0.02 * tally.valid, (title, tally.decided, tally.valid)
    assert tally.exact > 0 or tally.worst
    print(f"text chain {title}: {tally.line()} in {time.perf_counter() - t0:.2f} s" + ("" if ratio is None else f" (attention at {ratio:.3f} of its bar)"))


DENSE = [(name, si, B) for name in tc.CONFIGS for si in range(len(tc.WEIGHT_SEEDS)) for B in tc.DENSE_B]


@pytest.mark.parametrize("name,si,B", DENSE, ids=[f"{n}-w{si}-B{B}" for n, si, B in DENSE])
def test_text_every_launch_is_its_restatement_dense(name, si, B):
    tally, t0 = tc.Tally(), time.perf_counter()
    for P in tc.DENSE_P:
        _run(name, si, B, P, None, tally)
    _close(tally, f"{name} w{si} B={B}", t0)


RAGGED = [(name, si) for name in tc.CONFIGS for si in range(len(tc.WEIGHT_SEEDS))]


@pytest.mark.parametrize("name,si", RAGGED, ids=[f"{n}-w{si}" for n, si in RAGGED])
def test_text_every_launch_is_its_restatement_ragged(name, si):
    tally, t0 = tc.Tally(), time.perf_counter()
    for B, P, lengths in tc.RAGGED:
        _run(name, si, B, P, lengths, tally)
    _close(tally, f"ragged {name} w{si}", t0)


def test_bare_encoder_and_head_count_and_run():
    """num_blocks = 0: embed and final_norm, the tap is x0; a head with num_layers = 0 reads in_dim channels directly."""
    enc, head = _models("bare", 0)
    B, P = 2, 9
    assert enc.launch_count(B, P) == 2 and head.launch_count(B, P) == 2
    tally = tc.Tally()
    t = _run("bare", 0, B, P, None, tally)
    assert np.array_equal(enc._read_block0(B, P).cpu().numpy(), tc.chain_forward(tc.encoder_plan(enc)[:1], {"ids": tc.make_ids("bare", B, P)}, P)["emb"])
    ids = tc.make_ids("bare", B, P)
    want, _ = R.encoder_forward(enc.get_config(), enc.weights, ids)
    assert np.abs(t["enc_in"] - want).max() <= 1e-5


@pytest.mark.parametrize("max_frames", [50, 1_000_000])
def test_duration_kernel_on_chosen_logits(max_frames):
    """w = (1, 0, 0, 0), b = 0: u is exactly the test's x[..., 0].  The sweep over [-100, 100], log of values either side of the
    clip edges and of half-integers (outside the decided margin), the expf overflow (88.8, 100) and -100."""
    head = tc.sweep_head(max_frames)
    u = tc.sweep_logits(max_frames)
    x = np.zeros((1, len(u), 4), np.float32)
    x[0, :, 0] = u
    x[0, :, 1:] = np.random.default_rng(1).standard_normal((len(u), 3))
    assert np.array_equal(tc.dot32(x[0], *tc.head_plan(head)[0]["wb"]), u)
    tally, t0 = tc.Tally(), time.perf_counter()
    t = _run_head(head, x, None, tally)
    f = {float(v): int(n) for v, n in zip(u, t["frames"][0])}
    assert f[float(np.float32(88.8))] == f[100.0] == max_frames and f[-100.0] == 1 and f[0.0] == 1
    assert t["frames"].max() == max_frames and tally.valid - tally.decided <= 0.02 * tally.valid
    _close(tally, f"chosen logits, max {max_frames}", t0)


@pytest.mark.parametrize("C", [260, 516])
def test_duration_kernel_strided_channel_loop(C):
    """in_dim above 256: a lane walks more than one quad (260: lane 0 alone; 516: lanes 0 .. 64 of 129 quads)."""
    from iris.encoder import DurationPredictor
    tally, t0 = tc.Tally(), time.perf_counter()
    for si, seed in enumerate(tc.WEIGHT_SEEDS):
        head = DurationPredictor(hidden_dim=4, num_layers=0, in_dim=C, max_frames_per_phoneme=50, seed=1)
        tc.randomise(head, seed)
        x = np.random.default_rng(seed).standard_normal((3, 40, C)).astype(np.float32) * np.float32(1.5)
        _run_head(head, x, None, tally)
        _run_head(head, x, (40, 1, 33), tally)
    _close(tally, f"duration C {C}", t0)


@pytest.mark.parametrize("P", [256, 257, 600, 1000])
def test_scan_device_ragged_with_negative_and_padded_entries(P):
    rng = np.random.default_rng(P)
    B = 3
    lengths = np.array([P, 1, P - 37], np.int32)
    f = rng.integers(-50, 200, (B, P)).astype(np.int32)                  # negatives count as 0; entries past a length are ignored
    f[0, rng.integers(0, P, 20)] = 10_000
    f[2, -1] = 10_000                                                    # past item 2's length
    offsets, totals = E.scan_device(_dev(f), _dev(lengths))
    want_off, want_tot = tc.scan_np(f, lengths)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and np.array_equal(totals.cpu().numpy(), want_tot)
    offsets, totals = E.scan_device(_dev(f))
    want_off, want_tot = tc.scan_np(f)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and np.array_equal(totals.cpu().numpy(), want_tot)
    bad_off, _ = tc.scan_np(f, lengths, "inclusive_offsets")
    assert not np.array_equal(bad_off, tc.scan_np(f, lengths)[0])


def test_length_regulator_long_rows_and_zero_length_runs():
    """P = 300: the binary search over more than 256 offsets, runs of equal offsets at the start, in the middle and at the end
    of an item, and one item whose total is 0."""
    rng = np.random.default_rng(9)
    B, P, Ed = 4, 300, 24
    enc = rng.standard_normal((B, P, Ed)).astype(np.float32)
    d = rng.integers(0, 5, (B, P)).astype(np.int32)
    d[0, :40] = 0; d[0, 120:200] = 0; d[0, -30:] = 0
    d[1, :] = 0
    d[2, 1:-1] = 0; d[2, 0] = 7; d[2, -1] = 3
    d[3, 150] = 400
    T = int(d.sum(axis=1).max())
    want = R.length_regulate(enc, d)
    assert np.array_equal(want, tc.regulate_np(enc, d, T)) and not want[1].any()
    offsets, totals = E.scan_device(_dev(d))
    assert np.array_equal(offsets.cpu().numpy(), tc.scan_np(d)[0])
    got = E.regulate_device(_dev(enc), offsets, totals, T)
    assert np.array_equal(got.cpu().numpy(), want)
    for factor in (1, 4):
        assert np.array_equal(E.length_regulate(enc, d, factor=factor), R.length_regulate(enc, d, factor=factor))
