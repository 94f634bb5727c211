"""The split-product mode (dtype "f32s"): fp32 storage and accumulation, ResBlock conv products formed from two bf16
terms per operand (hi*hi + hi*mid + mid*hi on the bf16 MFMA).  It is held to the SAME bar as the fp32 path --
north_star's 1e-4 max-abs against the reference fp32 generator (goldens and oracle) -- and observed at <= 1.2e-5.

Two kinds of checks.  Against the EXACT layer / the fp32 generator (TOL_LAYER = 6e-5, TOL_WAV = 1e-4, 3e-5): they bound
what the mode costs, and have to leave room for the scheme's own noise -- a kernel that truncates ``mid`` passes them.
Against the RESTATEMENT of the kernel's arithmetic (oracle.conv1d_split with fp64 accumulation, "split64"):

    max|got - split64| <= R * max|split64 - exact|,   R = 0.5

The right-hand side is the scheme's own distance to the exact layer, computed per case from the references alone.
tests/test_oracle_f32s.py pins on the CPU that summation order (fp32 against fp64 accumulation) stays <= 0.1 of it
(0.02 ... 0.07) while a truncated ``mid`` is 0.96 ... 2.0 and a lost ``w_mid`` tap >= 100 away, so R = 0.5 separates them.
Observed on the MI355X (printed per case by every test):
  * single Conv1d layers (both tile heights of every tile config, all V1 (k, d), inputs of other kinds): 0.026 ... 0.29,
    and 0.44 for bf16-valued x at C = 256, k = 11 -- there x_mid = 0, so the noise is that of the weights' split alone
    (1.0e-5 against 1.5e-5) while the fp32 accumulation chain (3 k C / 16 = 528 MFMAs) is unchanged;
  * ConvTranspose1d layers: 0.05 ... 0.18;
  * every MRF step of whole forwards on the GPU's own inputs: 0.04 ... 0.44.  The top values are steps whose noise is
    3e-7 ... 7e-7 on outputs of magnitude 2 ... 4: one fp32 ulp of such an output is 2.4e-7, so there the ratio measures the
    rounding of the result itself, not the accumulation (no step is off by more than one ulp of its largest output).
With both operands bf16-valued the scheme IS the exact conv: then the fp32 layer bar of tests/test_gpu_parity.py applies
(observed 1e-7 ... 4e-7 of max|exact|).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import f32s_cases as fc
from oracle import hifigan_oracle as orc

pytestmark = pytest.mark.gpu

TOL_WAV = 1e-4          # north_star
TOL_LAYER = 6e-5        # relative to max|reference output| of one conv (two-term split: ~2^-16 per product)
TOL_LAYER_F32 = 2e-5    # tests/test_gpu_parity.py's bar for a plain fp32 layer: holds where the scheme adds nothing
R = 0.5                 # max|got - split64| <= R * max|split64 - exact|: see the module docstring


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


@pytest.mark.parametrize("B,L,C,k,d,use_res", [
    (1, 64, 32, 3, 1, False), (2, 517, 32, 11, 5, True), (1, 200, 64, 7, 3, True), (2, 131, 64, 3, 1, False),
    (1, 130, 128, 7, 5, True), (1, 70, 256, 11, 3, True), (1, 264, 256, 3, 1, False), (1, 1, 32, 11, 5, True)])
def test_f32s_conv1d_matches_oracle(B, L, C, k, d, use_res):
    from iris import _native
    lib = _native.load()
    rng = np.random.default_rng(B * 1000 + L + C + k + d)
    x = rng.standard_normal((B, C, L)).astype(np.float32)
    w = (rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    res = rng.standard_normal((B, C, L)).astype(np.float32) if use_res else None
    want = orc.conv1d_np(orc.lrelu_np(x, 0.1), w, b, d)
    if use_res:
        want = want + res
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    rd = torch.from_numpy(np.ascontiguousarray(res.transpose(0, 2, 1))).cuda() if use_res else None
    yd = torch.full((B, L, C), float("nan"), device="cuda")
    _native.check("op_conv1d_f32s", lib.iris_hifigan_op_conv1d_f32s(
        xd.data_ptr(), _fp(w), _fp(b), rd.data_ptr() if use_res else None, yd.data_ptr(), B, L, C, k, d, 0.1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= TOL_LAYER * np.abs(want).max()


@pytest.mark.parametrize("B,L,Ci,Co,k,u", [(1, 40, 512, 256, 16, 8), (2, 130, 256, 128, 16, 8), (1, 300, 128, 64, 4, 2),
                                            (2, 517, 64, 32, 4, 2), (1, 1, 64, 32, 4, 2), (1, 700, 64, 32, 4, 2)])
def test_f32s_conv_transpose1d_matches_oracle(B, L, Ci, Co, k, u):
    from iris import _native
    lib = _native.load()
    rng = np.random.default_rng(L + Ci + k)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, k)) / np.sqrt(Ci * k / u)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    want = orc.conv_transpose1d_np(orc.lrelu_np(x, 0.1), w, b, u, (k - u) // 2)
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    yd = torch.full((B, L * u, Co), float("nan"), device="cuda")
    _native.check("op_conv_transpose1d_f32s", lib.iris_hifigan_op_conv_transpose1d_f32s(
        xd.data_ptr(), _fp(w), _fp(b), yd.data_ptr(), B, L, Ci, Co, k, u, 0.1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.abs(got - want).max() <= TOL_LAYER * np.abs(want).max()


@pytest.mark.parametrize("case", ["v1_default_T4_taps", "v1_default_B2_T16", "v1_amplified_T24"])
def test_f32s_generator_matches_reference_goldens(case, golden, case_setup, dev):
    """Against the waveform the REFERENCE produced for the same weights and mel."""
    from iris._engine import GeneratorEngine
    cfg, sd = case_setup(case)
    g = golden(case)
    eng = GeneratorEngine(cfg, sd, dev)
    got = eng.forward(torch.from_numpy(g["mel"]).to(dev), dtype="f32s").cpu().numpy()
    assert np.abs(got - g["wav"][:, 0, :]).max() <= TOL_WAV
    eng.close()


@pytest.mark.parametrize("B,T,seed,log_mel", [(1, 100, 1001, False), (3, 57, 5, True), (1, 1, 9, False), (2, 300, 4, True),
                                               (1, 1000, 1002, False)])
def test_f32s_generator_matches_oracle(B, T, seed, log_mel, dev):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel = seeded_mel(seed, B, T, log_mel=log_mel)
    eng = GeneratorEngine(cfg, sd, dev)
    md = torch.from_numpy(mel).to(dev)
    got = eng.forward(md, dtype="f32s")
    assert torch.equal(eng.forward(md, dtype="f32s"), got)                      # deterministic
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), mel).numpy()[:, 0, :]
    err = np.abs(got.cpu().numpy() - want).max()
    assert err <= TOL_WAV, err
    assert err <= 3e-5          # observed <= 1e-5: an order of magnitude inside the budget
    eng.close()


def test_f32s_batch_independence_and_unsupported_config(dev, case_setup):
    from iris import _native
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=3, gain=1.1, post_gain=10.0), dev)
    mel = torch.from_numpy(seeded_mel(77, 4, 40)).to(dev)
    full = eng.forward(mel, dtype="f32s").clone()
    for b in range(4):
        assert torch.equal(eng.forward(mel[b:b + 1].contiguous(), dtype="f32s")[0], full[b])
    assert eng.workspace_bytes(2, 50, "f32s") == eng.workspace_bytes(2, 50, "f32")
    eng.close()
    cfg2, sd2 = case_setup("small_cfg_B3_T19")      # ResBlock channels 24 / 12 / 6: no split-product mode
    eng2 = GeneratorEngine(cfg2, sd2, dev)
    with pytest.raises(_native.NativeCallError) as exc:
        eng2.forward(torch.zeros((1, cfg2.in_channels, 5), device=dev), dtype="f32s")
    assert "multiples of 32" in str(exc.value)
    eng2.close()
    # a single layer with a channel count the tiles do not divide is refused as well (96 = 1.5 x 64)
    lib = _native.load()
    x = torch.zeros((1, 8, 96), device=dev)
    w = np.zeros((96, 96, 3), np.float32)
    rc = lib.iris_hifigan_op_conv1d_f32s(x.data_ptr(), _fp(w), _fp(np.zeros(96, np.float32)), None, x.data_ptr(), 1, 8, 96, 3, 1, 0.1, None)
    assert rc == 4      # IRIS_HIFIGAN_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# the kernel against the restatement of its own arithmetic (oracle.conv1d_split), not against the exact conv
# ------------------------------------------------------------------------------------------------
def _exact_conv(xa, w, b, d):
    k = w.shape[-1]
    return torch.nn.functional.conv1d(torch.as_tensor(xa).double(), torch.as_tensor(w).double(), torch.as_tensor(b).double(),
                                      dilation=d, padding=d * (k - 1) // 2).float().numpy()


def _ratio_assert(label, got, split64, exact, noise):
    """got within R of the scheme's own distance to the exact layer (``noise``, from the references alone); where the
    scheme IS the exact layer (noise = 0: bf16-valued operands) the plain fp32 layer bar applies."""
    err = float(np.abs(got - split64).max())
    if noise == 0.0:
        print(f"f32s ratio {label}: noise 0, max|got - exact| / max|exact| = {err / float(np.abs(exact).max()):.2e}")
        assert err <= TOL_LAYER_F32 * np.abs(exact).max(), (label, err)
        return 0.0
    print(f"f32s ratio {label}: max|got - split64| {err:.3e} / noise {noise:.3e} = {err / noise:.3f}")
    assert err <= R * noise, (label, err, noise, err / noise)
    return err / noise


CONV_CASES = fc.conv_cases()
CONVT_CASES = fc.convt_cases()


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_f32s_conv1d_matches_restatement(case):
    """Each case names the template instance it is meant to reach: C picks the tile config (32: <4, 1, MT, 1, 32>, 64:
    <2, 2, MT, 1, 64>, 128 / 256: <2, 2, MT, 2, 64>, 256 with two C_out blocks), MT the height (oracle/f32s_cases.py derives B
    and L from the tile constants and the 2.5-blocks-per-CU rule; tests/test_oracle_f32s.py holds them to the plan)."""
    from iris import _native
    lib = _native.load()
    cid, B, L, C, k, d, use_res, MT, kind = case
    x, w, b, res = fc.conv_inputs(case)
    xa = orc.lrelu_np(x, 0.1)
    split64 = orc.conv1d_split(torch.from_numpy(xa), torch.from_numpy(w), b, d).numpy()
    exact = _exact_conv(xa, w, b, d)
    noise = float(np.abs(split64 - exact).max())
    if use_res:
        split64, exact = split64 + res, exact + res
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    rd = torch.from_numpy(np.ascontiguousarray(res.transpose(0, 2, 1))).cuda() if use_res else None
    yd = torch.full((B, L, C), float("nan"), device="cuda")
    _native.check("op_conv1d_f32s", lib.iris_hifigan_op_conv1d_f32s(
        xd.data_ptr(), _fp(w), _fp(b), rd.data_ptr() if use_res else None, yd.data_ptr(), B, L, C, k, d, 0.1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert np.isfinite(got).all()
    assert np.abs(got - exact).max() <= TOL_LAYER * np.abs(exact).max()
    assert (noise == 0.0) == (kind == "bf16_xw")
    _ratio_assert(cid, got, split64, exact, noise)


@pytest.mark.parametrize("case", CONVT_CASES, ids=[c[0] for c in CONVT_CASES])
def test_f32s_conv_transpose1d_matches_restatement(case):
    """The four V1 upsamplers as u phase problems (z_is_phase) of L_in + 1 row indices: filling the tiles exactly, spilling
    one index into a further tile, ragged; half and full height; B > 1."""
    from iris import _native
    lib = _native.load()
    cid, B, L, Ci, Co, k, u, MT = case
    x, w, b = fc.convt_inputs(case)
    xa = torch.from_numpy(orc.lrelu_np(x, 0.1))
    split64 = orc.conv_transpose1d_split(xa, torch.from_numpy(w), b, u, (k - u) // 2).numpy()
    exact = torch.nn.functional.conv_transpose1d(xa.double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                                 stride=u, padding=(k - u) // 2).float().numpy()
    noise = float(np.abs(split64 - exact).max())
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    yd = torch.full((B, L * u, Co), float("nan"), device="cuda")
    _native.check("op_conv_transpose1d_f32s", lib.iris_hifigan_op_conv_transpose1d_f32s(
        xd.data_ptr(), _fp(w), _fp(b), yd.data_ptr(), B, L, Ci, Co, k, u, 0.1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert got.shape == exact.shape and np.isfinite(got).all()
    assert np.abs(got - exact).max() <= TOL_LAYER * np.abs(exact).max()
    assert noise > 0.0
    _ratio_assert(cid, got, split64, exact, noise)


@pytest.mark.parametrize("C,B,k,d", [(32, 8, 3, 1), (64, 8, 7, 3), (256, 4, 11, 1)])
def test_f32s_full_height_ragged_tile_writes_only_its_own_rows(C, B, k, d):
    """A full-height tile is two 32-row halves per wave.  With L = n * T_BLK + 32 the last tile's first half is inside the
    item and its second half is beyond L: those rows must be dropped -- not stored 32 rows further, which would be the next
    batch item's first rows or, for the last item, memory behind the tensor.  The output is allocated with 64 guard rows
    behind it that must keep their fill; the rows of every item are held to the restatement as usual."""
    from iris import _native
    lib = _native.load()
    n = -(-5 * fc.CU // (2 * B * (C // (fc.tile(C)[1] * fc.tile(C)[2] * 32))))
    L = n * fc.t_blk(C, 2) + 32
    assert fc.expected_mt(C, L, B, 1) == 2
    case = (f"C{C}-guard-L{L}", B, L, C, k, d, True, 2, "normal")
    x, w, b, res = fc.conv_inputs(case)
    xa = orc.lrelu_np(x, 0.1)
    split64 = orc.conv1d_split(torch.from_numpy(xa), torch.from_numpy(w), b, d).numpy()
    exact = _exact_conv(xa, w, b, d)
    noise = float(np.abs(split64 - exact).max())
    xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    rd = torch.from_numpy(np.ascontiguousarray(res.transpose(0, 2, 1))).cuda()
    fill = 12345.0
    yd = torch.full((B * L + 64, C), fill, device="cuda")
    for _ in range(2):
        _native.check("op_conv1d_f32s", lib.iris_hifigan_op_conv1d_f32s(
            xd.data_ptr(), _fp(w), _fp(b), rd.data_ptr(), yd.data_ptr(), B, L, C, k, d, 0.1, None))
        out = yd.cpu().numpy()
        assert (out[B * L:] == fill).all(), "rows behind the last item were written"
        got = out[:B * L].reshape(B, L, C).transpose(0, 2, 1)
        assert np.isfinite(got).all()
        _ratio_assert(case[0], got, split64 + res, exact + res, noise)


# ------------------------------------------------------------------------------------------------
# the forms only the forward launches: three branches interleaved along blockIdx.x, full-height tiles, the summing form
# ------------------------------------------------------------------------------------------------
def _windows(L, rows=256):
    """Row ranges a step is restated on: everything for a short tensor, else its first and last two tiles' worth (the
    ragged end included) and a stretch in the middle that is aligned to nothing."""
    if L <= 6 * rows:
        return [(0, L)]
    mid = (L // 2) | 77
    return [(0, 2 * rows + 9), (mid - rows, mid + rows), (L - 2 * rows - 9, L)]


def _restate_rows(xin, w, b, d, wins):
    """(split64, exact) of LeakyReLU + conv on the row ranges ``wins`` of xin [B, C, L], concatenated along the rows: each
    range is computed from its own rows plus the conv's halo (rows a cut pads with zeros lie outside the range)."""
    k, L = w.shape[-1], xin.shape[2]
    halo = d * (k - 1) // 2
    s_parts, e_parts = [], []
    for a, e in wins:
        lo, hi = max(0, a - halo), min(L, e + halo)
        xa = orc.lrelu_np(np.ascontiguousarray(xin[:, :, lo:hi]), 0.1)
        s = orc.conv1d_split(torch.from_numpy(xa), torch.as_tensor(w), b, d).numpy()
        x = _exact_conv(xa, w, b, d)
        s_parts.append(s[:, :, a - lo: e - lo])
        e_parts.append(x[:, :, a - lo: e - lo])
    return np.concatenate(s_parts, axis=2), np.concatenate(e_parts, axis=2)


def _rows(t, wins):
    return np.concatenate([t[:, :, a:e] for a, e in wins], axis=2)


@pytest.mark.parametrize("B,T,stages,first_pair", fc.UNTIL_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in fc.UNTIL_SHAPES])
def test_f32s_every_step_matches_restatement_on_its_own_inputs(B, T, stages, first_pair, dev):
    """The f32s twin of test_generator_intermediates_match_oracle_every_step: xt after every dilated conv, y after every
    conv + residual, and the mean the stage's last step folds, against ``conv1d_split`` applied to the GPU's OWN previous
    tensors -- nothing propagates, so the layer tests' ratio R holds per step.  A branch computed with another branch's
    weights, a lost tile, a mean in another order or by a multiplication fail here; the waveform tests cannot see most of
    them inside 1e-4.  Which instances each shape reaches: oracle/f32s_cases.py, asserted by tests/test_oracle_f32s.py."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    folded = orc.fold_state_dict(sd)
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)
    mel = torch.from_numpy(seeded_mel(31, B, T)).to(dev)
    nd, nk = len(cfg.resblock_dilation_sizes[0]), cfg.num_kernels
    plan = {(s, st): ins for s, st, ins in fc.plan_instances(cfg, B, T)}
    worst = {}
    for stage in stages:
        if first_pair == 0:
            x = eng.forward_until(mel, stage, 0, dtype="f32s")["up"]
            cur = [x] * nk
        else:
            cur = eng.forward_until(mel, stage, 2 * first_pair - 1, dtype="f32s")["y"]
        wins = _windows(cur[0].shape[2])
        for m in range(first_pair, nd):
            taps = eng.forward_until(mel, stage, 2 * m, dtype="f32s")
            assert not taps["mean_in_y0"]
            xt = taps["xt"]
            for j, dil in enumerate(cfg.resblock_dilation_sizes):
                pfx = f"resblocks.{stage * nk + j}.convs1.{m}"
                s64, exact = _restate_rows(cur[j], folded[pfx + ".weight"], folded[pfx + ".bias"], dil[m], wins)
                got = _rows(xt[j], wins)
                assert np.isfinite(xt[j]).all()
                r = _ratio_assert(f"{B}x{T} stage {stage} step {2 * m} branch {j} {plan[(stage, 2 * m)]}", got, s64, exact,
                                  float(np.abs(s64 - exact).max()))
                worst[plan[(stage, 2 * m)]] = max(worst.get(plan[(stage, 2 * m)], 0.0), r)
            taps = eng.forward_until(mel, stage, 2 * m + 1, dtype="f32s")
            ins = plan[(stage, 2 * m + 1)]
            want, want_exact = [], []
            for j in range(nk):
                pfx = f"resblocks.{stage * nk + j}.convs2.{m}"
                s64, exact = _restate_rows(xt[j], folded[pfx + ".weight"], folded[pfx + ".bias"], 1, wins)
                res = _rows(cur[j], wins)
                want.append(s64 + res)
                want_exact.append(exact + res)
            if m == nd - 1:
                # the stage's last step: forward_f32 always folds the mean for f32s (ZS), in place over branch 0's residual
                assert taps["mean_in_y0"] and ins[5]
                assert nk == 3
                mean = ((want[0] + want[1]) + want[2]) / np.float32(3)
                mean_exact = ((want_exact[0] + want_exact[1]) + want_exact[2]) / np.float32(3)
                assert mean.dtype == np.float32
                assert np.isfinite(taps["y"][0]).all()
                r = _ratio_assert(f"{B}x{T} stage {stage} step {2 * m + 1} mean {ins}", _rows(taps["y"][0], wins), mean, mean_exact,
                                  float(np.abs(mean - mean_exact).max()))
                worst[ins] = max(worst.get(ins, 0.0), r)
            else:
                assert not taps["mean_in_y0"] and not ins[5]
                for j in range(nk):
                    assert np.isfinite(taps["y"][j]).all()
                    r = _ratio_assert(f"{B}x{T} stage {stage} step {2 * m + 1} branch {j} {ins}", _rows(taps["y"][j], wins),
                                      want[j], want_exact[j], float(np.abs(want[j] - want_exact[j]).max()))
                    worst[ins] = max(worst.get(ins, 0.0), r)
                cur = taps["y"]
    for ins, r in sorted(worst.items()):
        print(f"f32s worst ratio {B}x{T} <WT, WC, MT, NT, CIC, ZS> = {ins}: {r:.3f}")
    eng.close()


def test_f32s_stage_ends_against_the_restated_generator(dev):
    """ups.i / mrf.i of a whole forward against ``generator_forward_f32s``.  RECORDED, not held to a ratio: once errors
    propagate through the stack, summation order alone (the restatement with fp32 against fp64 accumulation) moves the
    waveform by 0.4 ... 0.6 of the scheme's whole distance to the fp32 oracle, so a ratio has no discriminating power end to
    end -- which is why the per-step test above, on the GPU's own inputs, carries the assertion.  Here only the waveform bar."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    folded = orc.to_torch_folded(sd)
    mel = seeded_mel(1001, 2, 60, log_mel=True)
    rest, ref = {}, {}
    wav_rest = orc.generator_forward_f32s(folded, mel, taps=rest).numpy()[:, 0, :]
    wav_ref = orc.generator_forward_torch(folded, mel, taps=ref).numpy()[:, 0, :]
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)
    md = torch.from_numpy(mel).to(dev)
    last = 2 * len(cfg.resblock_dilation_sizes[0]) - 1
    for i in range(cfg.num_upsamples):
        taps = eng.forward_until(md, i, last, dtype="f32s")
        assert taps["mean_in_y0"]
        for name, got in ((f"ups.{i}", taps["up"]), (f"mrf.{i}", taps["y"][0])):
            want, w32 = rest[name].numpy(), ref[name].numpy()
            scale = float(np.abs(want).max())
            print(f"f32s taps {name}: max|got - rest| / max|rest| = {np.abs(got - want).max() / scale:.2e}, "
                  f"max|rest - fp32 oracle| / max|rest| = {np.abs(want - w32).max() / scale:.2e}")
            assert np.isfinite(got).all()
            assert np.abs(got - want).max() <= TOL_WAV * max(1.0, scale), name
    got = eng.forward(md, dtype="f32s").cpu().numpy()
    print(f"f32s wav: max|got - rest| = {np.abs(got - wav_rest).max():.2e}, max|rest - fp32 oracle| = {np.abs(wav_rest - wav_ref).max():.2e}, "
          f"max|got - fp32 oracle| = {np.abs(got - wav_ref).max():.2e}")
    assert np.abs(got - wav_ref).max() <= TOL_WAV and np.abs(got - wav_rest).max() <= TOL_WAV
    eng.close()


# ------------------------------------------------------------------------------------------------
# the fp32 path's shape matrix, for f32s
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine2025(dev):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)         # the amplified set: tanh reaches +-0.99
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)                   # eager launches: the planner's own choices
    yield eng, orc.to_torch_folded(sd)
    eng.close()


@pytest.mark.parametrize("B,T", fc.INDEPENDENCE_SHAPES)
def test_f32s_batch_independent_across_the_tile_height_switch(B, T, dev):
    """An item alone runs half-height tiles where the same item in the batch runs full-height ones, in both forms
    (tests/test_oracle_f32s.py asserts that from the plan): other template instances, the same bits.  Repeated runs too:
    the summing form writes the mean in place."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    alone_plan, batch_plan = fc.plan_instances(cfg, 1, T), fc.plan_instances(cfg, B, T)
    assert any(a[2][2] != b[2][2] for a, b in zip(alone_plan, batch_plan))
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=3, gain=1.1, post_gain=10.0), dev, graph_max_frames=0)
    mel = torch.from_numpy(seeded_mel(77, B, T)).to(dev)
    full = eng.forward(mel, dtype="f32s").clone()
    for _ in range(2):
        assert torch.equal(eng.forward(mel, dtype="f32s"), full)
    for b in sorted({0, B // 2, B - 1}):
        alone = eng.forward(mel[b:b + 1].contiguous(), dtype="f32s")
        assert torch.equal(alone[0], full[b]), b
    assert torch.equal(eng.forward(mel, dtype="f32s"), full)
    eng.close()


def test_f32s_planner_sweep_matches_oracle(engine2025, dev):
    """A subset of the fp32 planner sweep between whose shapes the f32s plan changes.  The bar is north_star's; the error of
    every shape is printed (the scheme alone reaches 2e-5 on the CPU grid of tests/test_oracle_f32s.py)."""
    from iris._weights import seeded_mel
    eng, folded = engine2025
    for n, (B, T) in enumerate(fc.SWEEP_SHAPES):
        mel = seeded_mel(7000 + n, B, T, log_mel=bool(n & 1))
        got = eng.forward(torch.from_numpy(mel).to(dev), dtype="f32s").cpu().numpy()
        idx = sorted({0, B - 1})
        want = orc.generator_forward_torch(folded, mel[idx]).numpy()[:, 0, :]
        assert got.shape == (B, 256 * T) and np.isfinite(got).all()
        err = float(np.abs(got[idx] - want).max())
        print(f"f32s sweep {B}x{T}: max-abs err vs the fp32 oracle {err:.3e}")
        assert 0.0 < err <= TOL_WAV, (B, T, err)


@pytest.mark.parametrize("B,T", fc.LONG_WIDE_SHAPES)
def test_f32s_long_and_wide_shapes(B, T, engine2025, dev):
    from iris._weights import seeded_mel
    eng, folded = engine2025
    mel = seeded_mel(B + T, B, T, log_mel=True)
    got = eng.forward(torch.from_numpy(mel).to(dev), dtype="f32s").cpu().numpy()
    idx = sorted({0, B // 2, B - 1})
    want = orc.generator_forward_torch(folded, mel[idx]).numpy()[:, 0, :]
    assert got.shape == (B, 256 * T)
    err = float(np.abs(got[idx] - want).max())
    print(f"f32s {B}x{T}: max-abs err vs the fp32 oracle {err:.3e}")
    assert err <= TOL_WAV
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0


def test_f32s_large_batch_runs_as_passes_sharing_one_workspace(dev):
    """70 x 1000 frames: a pass of 65 items and one of 5 over one workspace; items of the first pass, across the pass
    boundary and of the last pass equal the item alone bit for bit (which runs other tile heights)."""
    from iris import _native
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=77, gain=1.1, post_gain=8.0), dev, graph_max_frames=0)
    B, T = 70, 1000
    plan = _native.describe_plan(cfg, B, T, _native.DTYPE_F32_SPLIT)
    assert plan["passes"] == 2
    assert eng.workspace_bytes(B, T, "f32s") == eng.workspace_bytes(65, T, "f32s") == plan["workspace_bytes"] < 16e9
    mel = torch.from_numpy(seeded_mel(4242, B, T)).to(dev)
    wav = eng.forward(mel, dtype="f32s")
    torch.cuda.synchronize()
    assert torch.isfinite(wav).all()
    for i in (0, 64, 65, 69):
        alone = eng.forward(mel[i:i + 1].contiguous(), dtype="f32s")
        assert torch.equal(wav[i:i + 1], alone), i
    eng.close()


def test_f32s_hipgraph_replay_matches_eager(engine2025, dev):
    from iris._weights import seeded_mel
    eng, _ = engine2025
    for (B, T) in fc.GRAPH_SHAPES:
        for seed in (1, 2):
            mel = torch.from_numpy(seeded_mel(seed, B, T, log_mel=True)).to(dev)
            eager = eng.forward(mel, dtype="f32s").clone()
            for _ in range(2):
                replay = eng.forward_graph(mel, dtype="f32s").clone()
                assert torch.equal(eager, replay), (B, T, seed)


@pytest.mark.parametrize("B,T", fc.NON_V1_SHAPES)
def test_f32s_other_config_two_branches(B, T, dev):
    """ResBlock channels 128 / 64 / 32 and two MRF kernels (nz = 2: the branch of a block and the mean's divisor are not
    V1's constants), kernel sizes 5 and 9, dilations (1, 2, 4) and (1, 3, 5): against the fp32 oracle (north_star's bar) and
    against the restated generator."""
    from conftest import oracle_config
    from iris._engine import GeneratorEngine
    from iris._weights import seeded_mel, seeded_state_dict
    cfg = fc.non_v1_config()
    sd = seeded_state_dict(cfg, seed=8, gain=1.1, post_gain=10.0)
    folded = orc.to_torch_folded(sd)
    mel = seeded_mel(3, B, T, n_mels=cfg.in_channels)
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)
    got = eng.forward(torch.from_numpy(mel).to(dev), dtype="f32s").cpu().numpy()
    ref = orc.generator_forward_torch(folded, mel, oracle_config(cfg)).numpy()[:, 0, :]
    rest = orc.generator_forward_f32s(folded, mel, oracle_config(cfg)).numpy()[:, 0, :]
    e_ref, e_rest = float(np.abs(got - ref).max()), float(np.abs(got - rest).max())
    print(f"f32s other config {B}x{T}: max|wav| {np.abs(ref).max():.3f}, err vs the fp32 oracle {e_ref:.3e}, vs the restatement {e_rest:.3e}, "
          f"restatement vs the fp32 oracle {np.abs(rest - ref).max():.3e}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert 0.0 < e_ref <= TOL_WAV and e_rest <= TOL_WAV
    # the last step of every stage left the mean of TWO branches in y[0]
    last = 2 * len(cfg.resblock_dilation_sizes[0]) - 1
    md = torch.from_numpy(mel).to(dev)
    taps = {}
    orc.generator_forward_f32s(folded, mel, oracle_config(cfg), taps=taps)
    for i in range(cfg.num_upsamples):
        t = eng.forward_until(md, i, last, dtype="f32s")
        want = taps[f"mrf.{i}"].numpy()
        assert t["mean_in_y0"]
        assert np.abs(t["y"][0] - want).max() <= TOL_WAV * max(1.0, float(np.abs(want).max())), i
    eng.close()
