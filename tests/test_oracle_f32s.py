"""The split-product mode (dtype "f32s") on the CPU: its restatement (oracle/hifigan_oracle.py: ``split_bf16``,
``conv1d_split``, ``generator_forward_f32s``), what the restatement alone proves, and which kernel instances the GPU
tests' shapes reach.  No device is needed.

* the scheme's half of the parity claim: the restated generator stays <= 1e-4 from ``generator_forward_torch`` over a grid
  of weight seeds, gains and post-gains (measured, 2 x 60 frames, fp32 accumulation: 1.6e-7 ... 1.9e-5; worst: seed 3,
  gain 1.25, post-gain 30, log-mel) -- the test prints every figure;
* the discriminating power the GPU layer tests rely on: per layer case, with noise = max|split64 - exact|, summation
  order (fp32 against fp64 accumulation) moves the result by <= 0.1 noise, while a scheme whose ``mid`` is truncated
  instead of rounded, or that loses the ``w_mid`` plane of one tap, is >= 0.8 noise away.  A kernel within
  R = 0.5 noise of split64 (tests/test_gpu_f32s.py) is therefore neither;
* the launch plans: the shapes of the GPU tests reach every instance (three tile configs x two heights x two forms).
"""
import numpy as np
import pytest
import torch

from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
from oracle import f32s_cases as fc
from oracle import hifigan_oracle as orc

TOL_WAV = 1e-4          # north_star


def _trunc_split(v):
    """The WRONG split the GPU tests must tell from the right one: mid truncated to bf16 (low 16 bits masked)."""
    hi, _ = orc.split_bf16(v)
    mid = ((v - hi).contiguous().view(torch.int32) & -65536).view(torch.float32)
    return hi, mid


def test_split_bf16_properties():
    rng = np.random.default_rng(1)
    v = torch.from_numpy((rng.standard_normal(200000) * 10.0 ** rng.uniform(-6, 6, 200000)).astype(np.float32))
    hi, mid = orc.split_bf16(v)
    for t in (hi, mid):
        assert torch.equal(t, t.to(torch.bfloat16).to(torch.float32))                    # both terms are bf16 values
    assert torch.equal(hi, v.to(torch.bfloat16).float()) and torch.equal(mid, (v - hi).to(torch.bfloat16).float())
    assert (((hi.double() + mid.double()) - v.double()).abs() <= 2.0 ** -16 * v.double().abs()).all()
    assert (mid.abs() <= 2.0 ** -8 * v.abs()).all()
    b = v.to(torch.bfloat16).float()
    assert torch.equal(orc.split_bf16(b)[0], b) and not orc.split_bf16(b)[1].any()       # bf16-valued input: mid = 0
    z = orc.split_bf16(torch.zeros(4))
    assert not z[0].any() and not z[1].any()


@pytest.mark.parametrize("C,L,k,d", [(32, 50, 11, 5), (64, 33, 7, 3), (128, 20, 3, 1)])
def test_conv1d_split_is_the_exact_conv_on_bf16_values(C, L, k, d):
    """bf16-valued x and w have mid = 0: two of the three terms vanish and the third is the plain conv, which the numpy
    oracle computes with its own index formulas in fp64."""
    rng = np.random.default_rng(C + L)
    x = fc._bf16_valued(rng.standard_normal((2, C, L)).astype(np.float32))
    w = fc._bf16_valued((rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32))
    b = rng.standard_normal(C).astype(np.float32)
    got = orc.conv1d_split(torch.from_numpy(x), torch.from_numpy(w), b, d).numpy()
    want = orc.conv1d_np(x, w, b, d)
    assert np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()                   # one fp32 rounding of each result
    # and on general inputs the three terms are what the docstring says, against explicit fp64 index arithmetic
    x = rng.standard_normal((1, C, L)).astype(np.float32)
    w = (rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)
    (xh, xm), (wh, wm) = orc.split_bf16(torch.from_numpy(x)), orc.split_bf16(torch.from_numpy(w))
    zero = np.zeros(C, np.float32)
    want = (orc.conv1d_np(xh.numpy(), wm.numpy(), zero, d).astype(np.float64) + orc.conv1d_np(xm.numpy(), wh.numpy(), zero, d)
            + orc.conv1d_np(xh.numpy(), wh.numpy(), zero, d) + b[None, :, None])
    got = orc.conv1d_split(torch.from_numpy(x), torch.from_numpy(w), b, d).numpy()
    assert np.abs(got - want).max() <= 3 * 2.0 ** -22 * np.abs(want).max()


def test_conv_transpose1d_split_is_the_exact_layer_on_bf16_values():
    rng = np.random.default_rng(5)
    x = fc._bf16_valued(rng.standard_normal((2, 64, 37)).astype(np.float32))
    w = fc._bf16_valued((rng.standard_normal((64, 32, 4)) / 8).astype(np.float32))
    b = rng.standard_normal(32).astype(np.float32)
    got = orc.conv_transpose1d_split(torch.from_numpy(x), torch.from_numpy(w), b, 2, 1).numpy()
    want = orc.conv_transpose1d_np(x, w, b, 2, 1)
    assert got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()


# the weight grid of the mode's accuracy claim: seeds x gains x post-gains, both mel kinds, plus the suite's own set
GRID = [(1, 1.0, 1.0), (2, 1.18, 20.0), (3, 1.25, 30.0), (4, 1.3, 10.0), (5, 1.1, 50.0), (2025, 1.18, 20.0)]


@pytest.mark.parametrize("wseed,gain,post", GRID)
def test_restated_generator_keeps_the_parity_bar(wseed, gain, post):
    """The scheme's half of "<= 1e-4 from the reference": ``generator_forward_f32s`` (fp32 accumulation) against
    ``generator_forward_torch``.  If a case someone adds exceeds the bar, that is a finding about the scheme."""
    cfg = GeneratorConfig()
    folded = orc.to_torch_folded(seeded_state_dict(cfg, seed=wseed, gain=gain, post_gain=post))
    for mseed, log_mel in ((11, False), (12, True)):
        mel = seeded_mel(mseed, 2, 60, log_mel=log_mel)
        t32, ts = {}, {}
        ref = orc.generator_forward_torch(folded, mel, taps=t32)
        got = orc.generator_forward_f32s(folded, mel, taps=ts)
        assert sorted(t32) == sorted(ts) and all(t32[k].shape == ts[k].shape for k in t32)
        assert torch.equal(t32["ups.0"], ts["ups.0"])                    # conv_pre and the first upsampler are plain fp32
        err = float((got - ref).abs().max())
        print(f"f32s restatement vs fp32 oracle: weights seed {wseed} gain {gain} post {post} log_mel {log_mel}: "
              f"max|wav| {float(ref.abs().max()):.3f} err {err:.3e}")
        assert got.shape == ref.shape and torch.isfinite(got).all()
        assert 0.0 < err <= TOL_WAV, err


def test_restated_generator_other_config():
    cfg = fc.non_v1_config()
    ocfg = orc.OracleConfig(cfg.in_channels, cfg.upsample_rates, cfg.upsample_kernel_sizes, cfg.upsample_initial_channel,
                            cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)
    folded = orc.to_torch_folded(seeded_state_dict(cfg, seed=8, gain=1.1, post_gain=10.0))
    mel = seeded_mel(3, 2, 30, n_mels=cfg.in_channels)
    ref = orc.generator_forward_torch(folded, mel, ocfg)
    got = orc.generator_forward_f32s(folded, mel, ocfg)
    assert got.shape == ref.shape == (2, 1, cfg.hop_length * 30)
    assert 0.0 < float((got - ref).abs().max()) <= TOL_WAV


CONV_CASES = fc.conv_cases()


def test_layer_cases_cover_v1_pairs_at_both_heights():
    for MT in (1, 2):
        assert {(c[4], c[5]) for c in CONV_CASES if c[7] == MT and c[8] == "normal"} >= set(fc.V1_KD), MT
    assert {(c[3], c[7]) for c in CONV_CASES} >= {(C, MT) for C in (32, 64, 128, 256) for MT in (1, 2)}
    assert {c[6] for c in CONV_CASES} == {True, False}
    assert {(c[4], c[7]) for c in fc.convt_cases()} == {(Co, MT) for Co in (256, 128, 64, 32) for MT in (1, 2)}


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_references_can_tell_a_wrong_kernel_from_summation_order(case):
    """What the GPU layer test's ratio R = 0.5 stands on, from the references alone (see the module docstring)."""
    _, B, L, C, k, d, use_res, _, kind = case
    x, w, b, _ = fc.conv_inputs(case)
    xa = torch.from_numpy(orc.lrelu_np(x, 0.1))
    wt = torch.from_numpy(w)
    s64 = orc.conv1d_split(xa, wt, b, d)
    exact = torch.nn.functional.conv1d(xa.double(), wt.double(), torch.from_numpy(b).double(), dilation=d,
                                       padding=d * (k - 1) // 2).float()
    noise = float((s64 - exact).abs().max())
    if kind == "bf16_xw":
        assert noise == 0.0                                            # nothing to tell apart: the scheme adds nothing
        return
    s32 = orc.conv1d_split(xa, wt, b, d, acc=np.float32)
    order = float((s32 - s64).abs().max())
    trunc = float((orc.conv1d_split(xa, wt, b, d, x_planes=_trunc_split(xa)) - s64).abs().max())
    wh, wm = orc.split_bf16(wt)
    wm1 = wm.clone()
    wm1[:, :, k // 2] = 0
    tap = float((orc.conv1d_split(xa, wt, b, d, w_planes=(wh, wm1)) - s64).abs().max())
    print(f"{case[0]}: noise {noise:.3e} ({noise / float(exact.abs().max()):.2e} of max|exact|)  order/noise {order / noise:.3f}  "
          f"trunc/noise {trunc / noise:.2f}  tap/noise {tap / noise:.1f}")
    assert noise > 0.0
    assert order <= 0.1 * noise
    assert tap >= 0.8 * noise
    if kind != "bf16_x":                                               # (x_mid = 0: nothing to truncate)
        assert trunc >= 0.8 * noise


# ---- which kernel instances the GPU tests reach ------------------------------------------------------------------------
def _check_mirror(cfg, B, T):
    """The plan of one forward, after checking fc.expected_mt (which the single-layer cases are drawn by) against it."""
    inst = fc.plan_instances(cfg, B, T)
    nk, nd = cfg.num_kernels, len(cfg.resblock_dilation_sizes[0])
    L = T
    for i in range(cfg.num_upsamples):
        L *= cfg.upsample_rates[i]
        C = cfg.stage_channels(i)
        for step in range(2 * nd):
            zs = step == 2 * nd - 1                                    # the stage's last step always folds the mean
            want = fc.instance(C, fc.expected_mt(C, L, B, nk, zs), zs)
            assert inst[i * 2 * nd + step] == (i, step, want), (B, T, i, step)
    return inst


def test_gpu_shapes_reach_every_kernel_instance():
    """Host-only, from ``iris_hifigan_describe_plan``: if the 2.5-blocks-per-CU rule or the tiles move, this fails here and
    the shapes of oracle/f32s_cases.py are re-drawn -- not silently on the GPU box."""
    cfg = GeneratorConfig()
    every = {fc.instance(C, MT, zs) for C in (32, 64, 128) for MT in (1, 2) for zs in (False, True)}
    assert len(every) == 12
    # the per-step forward_until checks: the stages (and steps) they look at reach all twelve
    seen = set()
    for B, T, stages, first_pair in fc.UNTIL_SHAPES:
        seen |= {ins for stage, step, ins in _check_mirror(cfg, B, T) if stage in stages and step >= 2 * first_pair}
    assert seen == every, sorted(every - seen)
    inst = {(B, T): fc.plan_instances(cfg, B, T) for B, T, _, _ in fc.UNTIL_SHAPES}
    assert all(ins[2] == 1 for _, _, ins in inst[(1, 4)])
    assert {(s, st): ins[2] for s, st, ins in inst[(1, 641)]}[(1, 0)] == 2 and 64 * 641 % fc.t_blk(128, 2) != 0
    # the single-layer cases (nz = 1, never summing) reach the six non-summing ones, ConvTranspose1d included
    assert {fc.instance(c[3], c[7], False) for c in fc.conv_cases()} == {i for i in every if not i[5]}
    assert {fc.instance(c[4], c[7], False) for c in fc.convt_cases()} == {i for i in every if not i[5]}
    # batch independence: at one stage at least the item alone and the batch run different heights, in both forms
    for B, T in fc.INDEPENDENCE_SHAPES:
        alone, batch = _check_mirror(cfg, 1, T), _check_mirror(cfg, B, T)
        differ = {ins[5] for (_, _, a), (_, _, ins) in zip(alone, batch) if a[2] != ins[2]}
        assert differ, (B, T)
    assert {ins[5] for B, T in fc.INDEPENDENCE_SHAPES
            for (_, _, a), (_, _, ins) in zip(fc.plan_instances(cfg, 1, T), fc.plan_instances(cfg, B, T)) if a[2] != ins[2]} == {False, True}
    # the sweep: the plan changes between its shapes
    plans = {tuple(ins for _, _, ins in _check_mirror(cfg, B, T)) for B, T in fc.SWEEP_SHAPES}
    assert len(plans) >= 5, len(plans)
    for B, T in fc.LONG_WIDE_SHAPES + fc.GRAPH_SHAPES:
        _check_mirror(cfg, B, T)
    # two passes of 65 and 5 items of 1000 frames
    from iris import _native
    assert _native.describe_plan(cfg, 70, 1000, _native.DTYPE_F32_SPLIT)["passes"] == 2
    assert {ins[2] for _, _, ins in fc.plan_instances(cfg, 1, 1000)} == {1, 2}       # (the item alone: both heights)
    # the other config: two branches per step, channels 128 / 64 / 32
    cfg2 = fc.non_v1_config()
    assert [cfg2.stage_channels(i) for i in range(3)] == [128, 64, 32] and cfg2.num_kernels == 2
    assert {ins[2] for B, T in fc.NON_V1_SHAPES for _, _, ins in _check_mirror(cfg2, B, T)} == {1, 2}
