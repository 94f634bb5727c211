"""The per-launch criterion of the bf16 forward (oracle/bf16_cases.py) on the CPU: the constant it stands on, what it tells
apart, and which kernel forms the GPU test's shapes reach.  No device is needed.

* ``C_ABS``.  Every launch of every shape of ``bf16_cases.SHAPES`` is restated with ATen's fp32 accumulation and with fp64
  on the same operands; the largest |conv_fp32 - conv_fp64| / absconv is printed per launch.  Measured here (8 host
  threads): 2.0e-8 ... 1.4e-7 on the Conv1d launches, 1.2e-7 ... 2.83e-7 on the ConvTranspose1d launches (the maximum:
  v1-3x57, ups.1); C_ABS = 1.15e-6 is 4 x 2.85e-7.  The test holds the constant to 4 x the measured maximum within [0.8, 2] -- the fp32
  summation order of ATen moves with the host's thread count and ISA, the constant must not.
* The share of elements that round exactly like fp64: the fp32-accumulating restatement stays >= SHARE_MIN_REF = 0.9995 on
  every tensor (measured: 0.99965 ... 1.0), so the GPU test's SHARE_MIN = 0.999 cannot fail for a reason other than the
  kernel; it passes the whole criterion, the waveform bar included (measured: 2e-7 ... 1.1e-6 of 2.2e-5).
* Mutations of the restatement, each with fp32 accumulation, each FAILS at the launches it touches and nowhere else: the
  mel or the activations truncated to bf16; LeakyReLU per branch before the mean; a branch tensor's last row read as
  zero; the divisor of three branches used for two; the y_j left unrounded before the fp32 mean conv_post takes.
* The launch plans (``iris_hifigan_describe_plan``): the shapes reach both NIN = 3 block shapes of convt_mfma_bf16_kernel
  and its C_in = 128 one, the NIN = 1 form behind the summing pair, the polyphase fallback with two and with three
  branch tensors, the grouped three-branch conv launch, the summing pair in both output types and all three conv_post
  kernels.
"""
import functools

import numpy as np
import pytest

from oracle import bf16_cases as bc

IDS = [s[0] for s in bc.SHAPES]


@functools.lru_cache(maxsize=None)
def _setup(name, post_gain=None):
    if post_gain is None:
        return bc.setup(name)
    from iris._weights import folded_layers, seeded_state_dict
    import torch
    make, kw = bc.CONFIGS[name]
    cfg = make()
    sd = seeded_state_dict(cfg, **dict(kw, post_gain=post_gain))
    return cfg, sd, {s.name: (torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(np.ascontiguousarray(b)))
                     for s, w, b in folded_layers(cfg, sd)}


def _figures(rec):
    """A record of the walk reduced to its figures (the tensors of the large shapes are not kept)."""
    if rec["kind"] == "wav":
        small = rec["pre_tanh"].abs() <= 1.0
        err = (rec["got"].double() - rec["want64"]).abs()
        return {"label": rec["label"], "kind": "wav", "err": float(err.max()), "err_small": float(err[small].max()) if small.any() else 0.0,
                "share_small": float(small.double().mean())}
    f = bc.judge(rec["got"].numpy(), rec["want64"].numpy(), rec["absconv"].numpy())
    f.update(label=rec["label"], kind="bf16",
             acc=float(((rec["y32"].double() - rec["want64"]).abs() / rec["absconv"].clamp_min(2.0 ** -126)).max()))
    return f


@functools.lru_cache(maxsize=None)
def _walk(shape_id, mutation=None, post_gain=None):
    shape = bc.SHAPES[IDS.index(shape_id)]
    cfg, _, W = _setup(shape[1], post_gain)
    return [_figures(r) for r in bc.walk(cfg, W, bc.shape_mel(shape), None, shape[4], mutation)]


def _passes(f):
    if f["kind"] == "wav":
        return f["err"] <= bc.TOL_WAV
    return f["ok_abs"] and f["share"] >= bc.SHARE_MIN


def test_number_format_helpers():
    import torch
    rng = np.random.default_rng(2)
    v = (rng.standard_normal(100000) * 10.0 ** rng.uniform(-8, 8, 100000)).astype(np.float32)
    t = torch.from_numpy(v)
    assert np.array_equal(bc.r16_f64(v.astype(np.float64)), bc.r16(t).numpy().astype(np.float64))     # one rounding either way from fp32
    assert (bc.t16(t).abs() <= t.abs()).all() and ((bc.t16(t) - t).abs() <= t.abs() * 2.0 ** -7).all()
    assert 0.3 < float((bc.t16(t) != bc.r16(t)).double().mean()) < 0.7
    tie = np.float64(1.0 + 2.0 ** -8)                     # halfway between two bf16 values: to even
    assert bc.r16_f64(np.array([tie, tie + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8]))[:].tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6]
    y = [torch.from_numpy(rng.standard_normal(1000).astype(np.float32)) for _ in range(3)]
    assert torch.equal(bc.mrf_mean(y), ((y[0] + y[1]) + y[2]) * torch.tensor(1.0 / 3.0, dtype=torch.float32))
    assert torch.equal(bc.mrf_mean(y[:2]), (y[0] + y[1]) * 0.5)


@pytest.mark.parametrize("shape_id", IDS)
def test_fp32_restatement_passes_the_criterion(shape_id):
    """The honest restatement, launch by launch on its own inputs: the share floor, the whole criterion, and the figure
    C_ABS is taken from."""
    figs = _walk(shape_id)
    shape = bc.SHAPES[IDS.index(shape_id)]
    assert (figs[-1]["kind"] == "wav") == (shape[4] is None)
    for f in figs:
        if f["kind"] == "wav":
            print(f"{shape_id} {f['label']}: max err {f['err']:.2e}")
            assert f["err"] <= bc.TOL_WAV
            continue
        print(f"{shape_id} {f['label']}: fp32 accumulation {f['acc']:.2e} of absconv, err/ulp {f['err_ulp']:.2f}, "
              f"share {f['share']:.5f}, (err - ulp)/absconv {f['excess']:.2e}")
        assert f["share"] >= bc.SHARE_MIN_REF, f
        assert f["ok_abs"] and f["acc"] <= bc.C_ABS / 2, f


def test_c_abs_is_four_times_the_measured_accumulation_error():
    worst = max((f["acc"], s, f["label"]) for s in IDS for f in _walk(s) if f["kind"] == "bf16")
    print(f"max |conv_fp32 - conv_fp64| / absconv = {worst[0]:.3e} ({worst[1]}, {worst[2]}); 4 x = {4 * worst[0]:.3e}; C_ABS = {bc.C_ABS:.3e}")
    assert 0.8 * 4 * worst[0] <= bc.C_ABS <= 2 * 4 * worst[0], worst


def _failing(figs):
    return [f["label"] for f in figs if not _passes(f)]


def test_mutation_truncated_mel_fails():
    assert _failing(_walk("v1-2x12", "trunc_mel")) == ["conv_pre"]
    assert _failing(_walk("generic-3x37", "trunc_mel")) == ["conv_pre"]


@pytest.mark.parametrize("shape_id", ["v1-2x12", "generic-3x37"])
def test_mutation_truncated_activations_fails(shape_id):
    figs = _walk(shape_id, "trunc_act")
    touched = [f["label"] for f in figs if f["label"].startswith("ups.") or (f["label"].startswith("stage") and int(f["label"].split()[3]) % 2 == 0)]
    assert touched and _failing(figs) == touched      # (only the negative half of a LeakyReLU's input needs a rounding at all)


@pytest.mark.parametrize("shape_id,mutation", [("v1-2x12", "lrelu_per_branch"), ("generic-3x37", "lrelu_per_branch"),
                                               ("post24-3x70", "lrelu_per_branch"), ("v1-2x12", "drop_last_row"),
                                               ("generic-3x37", "drop_last_row"), ("post24-3x70", "drop_last_row"),
                                               ("generic-3x37", "inv_n_of_three")])
def test_mutation_of_the_mean_fails_at_every_later_upsampler(shape_id, mutation):
    figs = _walk(shape_id, mutation)
    cfg = _setup(bc.SHAPES[IDS.index(shape_id)][1])[0]
    assert _failing(figs) == [f"ups.{i}" for i in range(1, cfg.num_upsamples)]
    if mutation == "drop_last_row":
        # a few rows of one tensor: the share need not notice (it does not on a long tensor), the bound must
        assert not any(f["ok_abs"] for f in figs if f["label"] in _failing(figs))


def test_mutation_unrounded_branch_tensors_fail_the_waveform_bar():
    """Judged where tanh does not hide it: weights with a conv_post gain of 1, pre-tanh values mostly inside +-1."""
    honest = _walk("v1-2x12", None, 1.0)[-1]
    wrong = _walk("v1-2x12", "unrounded_y", 1.0)[-1]
    print(f"|pre-tanh| <= 1 on {honest['share_small']:.3f} of the samples; honest err {honest['err']:.2e}, unrounded y_j {wrong['err_small']:.2e}")
    assert honest["kind"] == wrong["kind"] == "wav" and honest["share_small"] > 0.5
    assert honest["err"] <= bc.TOL_WAV < wrong["err_small"]
    assert _failing(_walk("v1-2x12", "unrounded_y", 1.0)) == ["conv_post + tanh"]
    assert _failing(_walk("generic-3x37", "unrounded_y")) == ["conv_post + tanh"]


# ---- which forms the GPU test's shapes reach -------------------------------------------------------------------------------
def test_gpu_shapes_reach_every_forward_only_form():
    """Host-only, from ``iris_hifigan_describe_plan``: if a planner rule moves, this fails here and the shapes are re-drawn."""
    forms = {s[0]: bc.plan_forms(_setup(s[1])[0], s[2], s[3]) for s in bc.SHAPES}
    small, mid, big, gen, p24 = (forms[i] for i in IDS)
    # convt_mfma_bf16_kernel, three branch tensors: ups.1 narrow below 2 blocks per CU, 64 x 256 from there on; ups.2 (CIC = 64)
    for f in (small, mid):
        assert f["ups"][1] == ("gemm", (2, 1, 1, 4, 128), 3)
    assert big["ups"][1] == ("gemm", (2, 2, 1, 4, 128), 3)
    B, T = bc.SHAPES[2][2:4]
    assert -(-(8 * T + 1) // 64) * (8 * 4 // 8) * B == 2 * bc.CU            # exactly at the threshold
    for f in (small, mid):
        assert f["ups"][2] == ("gemm", (2, 1, 1, 4, 64), 3)
        # one tensor: pre (LeakyReLU while staging), and the summing pair's output (IN_ACT_NONE)
        assert f["ups"][0] == ("gemm", (2, 1, 1, 4, 128), 1) and f["ups"][3] == ("gemm", (2, 1, 2, 2, 64), 1)
        assert f["mrf"][2][-1] == "mrf_pair_bf16_sum_kernel"                # bf16 out, feeds ups.3
        assert f["mrf"][3][-1] == "mrf_pair_bf16_sum_kernel" and f["post"] == "rows_f32"      # fp32 out, feeds conv_post
        assert f["mrf"][1] == ["mrf_pair_bf16_kernel"] * 3                  # C = 128: fused pairs, no summing form
        # stage 0 (C = 256): six launches of the grouped conv kernel, three branches in one grid
        assert len(f["mrf"][0]) == 6 and all(n.startswith("conv_mfma_bf16_kernel<") for n in f["mrf"][0]) and f["grouped"][0] == 3
    # the polyphase fallback: two branch tensors (k = 2u and k = 3u), three branch tensors
    assert gen["ups"] == [("gemm", (2, 1, 1, 4, 64), 1), ("polyphase", 2), ("polyphase", 2)]
    assert p24["ups"] == [("polyphase", 1), ("polyphase", 3)]
    assert gen["grouped"][1:] == [2, 2] and p24["grouped"] == [3, 3]
    # conv_post: every kernel a config with channel counts that are multiples of 8 can reach
    assert {small["post"], gen["post"], p24["post"]} == {"rows_f32", "rows_bf16", "tanh_bf16"}
