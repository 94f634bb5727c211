"""Parity of the HIP path (through the C-ABI) against the oracle and the reference's goldens.

Needs a real MI355X: every test is marked ``gpu``.  Tolerance: BASELINE.json's north_star states
<= 1e-4 max-abs against the reference fp32 generator for the waveform; single layers are held to a
relative 2e-5 of the layer's output scale (fp32 fmaf chains vs ATen/fp64: pure rounding noise).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import oracle_config
from oracle import hifigan_oracle as orc

pytestmark = pytest.mark.gpu

TOL_WAV = 1e-4      # north_star
TOL_LAYER = 2e-5    # relative to max|reference output| of the layer


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from iris import _native
    return _native.load()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _cl(x_cf):  # [B,C,L] numpy -> channels-last device tensor [B,L,C]
    return torch.from_numpy(np.ascontiguousarray(x_cf.transpose(0, 2, 1))).cuda()


def _check(fn, status):
    from iris import _native
    _native.check(fn, status)


# ------------------------------------------------------------------------------------------------
# single layers
# ------------------------------------------------------------------------------------------------
CONV_CASES = [
    # (B, L, C_in, C_out, k, d, act, residual)      -- the V1 shapes of every tile config ...
    (1, 300, 32, 32, 3, 1, 1, True), (2, 517, 32, 32, 11, 5, 1, False), (1, 260, 32, 32, 7, 3, 1, True),
    (1, 200, 64, 64, 11, 5, 1, True), (2, 131, 64, 64, 3, 3, 1, False),
    (1, 130, 128, 128, 7, 5, 1, True), (1, 70, 256, 256, 11, 3, 1, True), (1, 64, 256, 256, 3, 1, 1, False),
    (2, 33, 80, 512, 7, 1, 0, False),          # conv_pre shape
    # ... and ragged ones: channels not multiples of 8/4, generic tap count, tiny length
    (1, 5, 32, 32, 11, 5, 1, True), (3, 41, 24, 24, 5, 2, 1, True), (1, 77, 6, 6, 5, 6, 1, True),
    (1, 50, 12, 40, 9, 1, 0, False), (1, 1, 32, 32, 3, 1, 1, False),
]


@pytest.mark.parametrize("B,L,Ci,Co,k,d,act,use_res", CONV_CASES)
def test_conv1d_matches_oracle(lib, B, L, Ci, Co, k, d, act, use_res):
    rng = np.random.default_rng(B * 1000 + L + Ci + k + d)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, k)) / np.sqrt(Ci * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    res = rng.standard_normal((B, Co, L)).astype(np.float32) if use_res else None
    xin = orc.lrelu_np(x, 0.1) if act else x
    want = orc.conv1d_np(xin, w, b, d)
    if use_res:
        want = want + res
    xd = _cl(x)
    rd = _cl(res) if use_res else None
    yd = torch.full((B, L, Co), float("nan"), device="cuda")
    _check("op_conv1d", lib.iris_hifigan_op_conv1d(
        xd.data_ptr(), _fp(w), _fp(b), rd.data_ptr() if use_res else None, yd.data_ptr(),
        B, L, Ci, Co, k, d, act, 0.1, 0, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max())


def test_conv1d_channels_first_input(lib):
    """conv_pre reads the mel in the reference's own layout [B, 80, T] (hifigan_pretrained.py:228)."""
    rng = np.random.default_rng(11)
    B, L, Ci, Co, k = 2, 45, 80, 512, 7
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, k)) / np.sqrt(Ci * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    want = orc.conv1d_np(x, w, b, 1)
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((B, L, Co), float("nan"), device="cuda")
    _check("op_conv1d", lib.iris_hifigan_op_conv1d(xd.data_ptr(), _fp(w), _fp(b), None, yd.data_ptr(),
                                                   B, L, Ci, Co, k, 1, 0, 0.1, 1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert np.abs(got - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max())


CONVT_CASES = [
    # (B, L, C_in, C_out, k, u) -- the four V1 upsamplers, then ragged ones
    (1, 37, 512, 256, 16, 8), (2, 65, 256, 128, 16, 8), (1, 130, 128, 64, 4, 2), (1, 300, 64, 32, 4, 2),
    (1, 19, 48, 24, 8, 4), (2, 20, 12, 6, 9, 3), (1, 1, 64, 32, 4, 2), (1, 7, 24, 12, 4, 2), (1, 9, 16, 8, 2, 2),
]


@pytest.mark.parametrize("B,L,Ci,Co,k,u", CONVT_CASES)
def test_conv_transpose1d_matches_oracle(lib, B, L, Ci, Co, k, u):
    rng = np.random.default_rng(L * 7 + Ci + k)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, k)) / np.sqrt(Ci * k / u)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    want = orc.conv_transpose1d_np(orc.lrelu_np(x, 0.1), w, b, u, (k - u) // 2)
    xd = _cl(x)
    yd = torch.full((B, L * u, Co), float("nan"), device="cuda")
    _check("op_conv_transpose1d", lib.iris_hifigan_op_conv_transpose1d(
        xd.data_ptr(), _fp(w), _fp(b), yd.data_ptr(), B, L, Ci, Co, k, u, 1, 0.1, None))
    got = yd.cpu().numpy().transpose(0, 2, 1)
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max())


CONV_POST_CASES = [(1, 700, 32, 7, True), (2, 300, 32, 7, False), (1, 100, 6, 7, True), (1, 3, 32, 7, True)]      # (B, L, C, k, three)


@pytest.mark.parametrize("B,L,C,k,three", CONV_POST_CASES)
def test_conv_post_matches_oracle(lib, B, L, C, k, three):
    rng = np.random.default_rng(L + C)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) * 2 for _ in range(3 if three else 1)]
    w = (rng.standard_normal((1, C, k)) * 0.3).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32)
    x = xs[0]
    if three:
        x = ((xs[0] + xs[1]) + xs[2]) / np.float32(3)
    want = np.tanh(orc.conv1d_np(orc.lrelu_np(x, 0.1), w, b, 1))[:, 0, :]
    xd = [_cl(v) for v in xs]
    yd = torch.full((B, L), float("nan"), device="cuda")
    _check("op_conv_post", lib.iris_hifigan_op_conv_post(
        xd[0].data_ptr(), xd[1].data_ptr() if three else None, xd[2].data_ptr() if three else None,
        _fp(w), _fp(b), yd.data_ptr(), B, L, C, k, 0.1, None))
    got = yd.cpu().numpy()
    assert np.abs(got - want).max() <= 2e-6 + TOL_LAYER


# ------------------------------------------------------------------------------------------------
# the hot kernel on its own: one grouped MRF step (mrf_conv_mfma_f32_kernel) in each of its launch modes
# ------------------------------------------------------------------------------------------------
MRF_STEP_CASES = [
    # (B, L, C, dils, residual)   every tile configuration of the kernel (C <= 32 / <= 64 / > 64), ragged lengths
    (1, 700, 32, (5, 5, 5), False), (2, 333, 32, (1, 1, 1), True), (1, 520, 64, (3, 3, 3), True),
    (1, 200, 128, (5, 5, 5), True), (2, 70, 256, (1, 1, 1), True), (1, 97, 256, (3, 3, 3), False),
]


def _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean):
    """Runs iris_hifigan_op_mrf_step; returns the three branch outputs [B,C,L] or the mean."""
    ks = (3, 7, 11)
    xd = [_cl(x) for x in xs]
    rd = [_cl(r) for r in rs] if rs is not None else None
    yd = [torch.full((B, L, C), float("nan"), device="cuda") for _ in range(3)]
    md = torch.full((B, L, C), float("nan"), device="cuda") if mean else None
    vp3, fp3 = ctypes.c_void_p * 3, ctypes.POINTER(ctypes.c_float) * 3
    status = lib.iris_hifigan_op_mrf_step(
        vp3(*[t.data_ptr() for t in xd]), fp3(*[_fp(w) for w in ws]), fp3(*[_fp(b) for b in bs]),
        vp3(*[t.data_ptr() for t in rd]) if rd is not None else None, vp3(*[t.data_ptr() for t in yd]),
        md.data_ptr() if mean else None, B, L, C, (ctypes.c_int32 * 3)(*ks), (ctypes.c_int32 * 3)(*dils),
        0.1, plan, None)
    return status, ([t.cpu().numpy().transpose(0, 2, 1) for t in yd] if not mean else md.cpu().numpy().transpose(0, 2, 1))


@pytest.mark.parametrize("plan", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("B,L,C,dils,use_res", MRF_STEP_CASES)
def test_mrf_step_matches_oracle(lib, B, L, C, dils, use_res, plan):
    """One conv step of the three ResBlock branches (k = 3/7/11; hifigan_pretrained.py:64-71) through the persistent
    MRF kernel, in the library's own plan (0), with full-height tiles (1), half-height tiles (2), one branch per
    block (3), through the small-problem kernel (4: 16 x 16 jobs on v_mfma_f32_16x16x4_f32) and with snake-ordered
    (tile, branch) jobs (5, 6: C >= 128), against the numpy oracle's conv1d_np.  All plans run the same fmaf
    chains: they must agree bit for bit."""
    if plan >= 5 and C < 128:
        pytest.skip("the job mode needs two C_in chunks")
    rng = np.random.default_rng(C * 7 + L + plan)
    ks = (3, 7, 11)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    ws = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    bs = [rng.standard_normal(C).astype(np.float32) for _ in ks]
    rs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks] if use_res else None
    status, got = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean=False)
    _check("op_mrf_step", status)
    for j in range(3):
        want = orc.conv1d_np(orc.lrelu_np(xs[j], 0.1), ws[j], bs[j], dils[j])
        if use_res:
            want = want + rs[j]
        assert np.isfinite(got[j]).all()
        assert np.abs(got[j] - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max()), (j, plan)
    if plan != 0:
        _, auto = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, 0, mean=False)
        for j in range(3):
            assert np.array_equal(auto[j], got[j]), (j, plan)


@pytest.mark.parametrize("B,L,C,dils", [(1, 6100, 256, (1, 1, 1)), (2, 7001, 128, (5, 5, 5)), (3, 1999, 256, (3, 3, 3))])
def test_mrf_job_mode_agrees_bitwise_when_blocks_draw_many_jobs(lib, B, L, C, dils):
    """Shapes with more (tile, branch) jobs than the chip has block slots, so that blocks do take follow-up jobs of other
    branches and tiles in later rounds of the snake order: plans 5 and 6 against plan 1 (checked against the oracle above), bit for bit."""
    rng = np.random.default_rng(L + C)
    ks = (3, 7, 11)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    ws = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    bs = [rng.standard_normal(C).astype(np.float32) for _ in ks]
    rs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    status, want = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, 1, mean=False)
    _check("op_mrf_step", status)
    for plan in (5, 6, 0):
        status, got = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean=False)
        _check("op_mrf_step", status)
        for j in range(3):
            assert np.array_equal(want[j], got[j]), (j, plan)


MRF_SUM_CASES = [(1, 700, 32), (1, 300, 64), (2, 130, 128), (1, 90, 256)]      # (B, L, C)


@pytest.mark.parametrize("plan", [0, 1, 2])
@pytest.mark.parametrize("B,L,C", MRF_SUM_CASES)
def test_mrf_summing_step_matches_oracle(lib, B, L, C, plan):
    """The last step of a stage stores only ((y0 + y1) + y2) / 3 (hifigan_pretrained.py:131-137, the reference's
    order and a true division)."""
    rng = np.random.default_rng(C + L + plan)
    ks, dils = (3, 7, 11), (1, 1, 1)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    ws = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    bs = [rng.standard_normal(C).astype(np.float32) for _ in ks]
    rs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    status, got = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean=True)
    _check("op_mrf_step", status)
    ys = [(orc.conv1d_np(orc.lrelu_np(xs[j], 0.1), ws[j], bs[j], 1) + rs[j]).astype(np.float32) for j in range(3)]
    want = ((ys[0] + ys[1]) + ys[2]) / np.float32(3)
    assert np.abs(got - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max())
    # and it is bit for bit what the separate branch outputs give when summed in the reference's order
    _, sep = _mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean=False)
    assert np.array_equal(got, ((sep[0] + sep[1]) + sep[2]) / np.float32(3))


MRF_PAIR_CASES = [(1, 700, 32, (1, 1, 1)), (2, 333, 32, (5, 5, 5)), (1, 520, 64, (3, 3, 3)), (3, 190, 64, (5, 5, 5)),      # (B, L, C, dils)
                  (1, 5, 32, (3, 3, 3)), (2, 11000, 64, (3, 3, 3)),    # (128-row tiles at C = 64)
                  (5, 30000, 32, (3, 3, 3))]   # 3,810 jobs: persistent blocks walk several jobs each
MRF_PAIR_SMALL = 400_000     # B L C up to which the pair is also held to the CPU oracles (they are slow)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,L,C,dils", MRF_PAIR_CASES)
def test_mrf_fused_pair_matches_oracle_and_separate_steps(lib, B, L, C, dils, mode):
    """The fused fp32 conv pair (csrc/mrf_pair_f32.h, mode 0; its persistent, prefetching form csrc/mrf_pair_f32_pf.h, modes 1 / 2 = jobs drawn from a
    counter / fixed stride:
    conv1 -> xt in LDS -> conv2 + residual, C = 32 / 64) against the numpy oracle's ResBlock arithmetic
    (hifigan_pretrained.py:64-71), and bit for bit against the two separate launches of the persistent kernel it replaces --
    several tiles per branch, ragged lengths, a length shorter than the kernel, more jobs than block slots."""
    rng = np.random.default_rng(C * 11 + L)
    ks = (3, 7, 11)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in ks]
    w1 = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    b1 = [rng.standard_normal(C).astype(np.float32) for _ in ks]
    w2 = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in ks]
    b2 = [rng.standard_normal(C).astype(np.float32) for _ in ks]
    xd = [_cl(x) for x in xs]
    yd = [torch.full((B, L, C), float("nan"), device="cuda") for _ in range(3)]
    vp3, fp3 = ctypes.c_void_p * 3, ctypes.POINTER(ctypes.c_float) * 3

    def pair(y_tensors, mean_tensor, m):
        return lib.iris_hifigan_op_mrf_pair(
            vp3(*[t.data_ptr() for t in xd]), fp3(*[_fp(w) for w in w1]), fp3(*[_fp(b) for b in b1]),
            fp3(*[_fp(w) for w in w2]), fp3(*[_fp(b) for b in b2]),
            vp3(*[t.data_ptr() for t in y_tensors]) if y_tensors is not None else None,
            ctypes.c_void_p(mean_tensor.data_ptr()) if mean_tensor is not None else None,
            B, L, C, (ctypes.c_int32 * 3)(*ks), (ctypes.c_int32 * 3)(*dils), 0.1, m, None)

    _, xt = _mrf_step(lib, xs, w1, b1, None, B, L, C, dils, 0, mean=False)
    _, sep = _mrf_step(lib, xt, w2, b2, xs, B, L, C, (1, 1, 1), 0, mean=False)
    small = B * L * C <= MRF_PAIR_SMALL                  # (the numpy oracle is slow: large cases are checked bit for bit only)
    rc = pair(yd, None, mode)
    if mode >= 1:
        # IRIS_HIFIGAN_UNSUPPORTED: the library carries the persistent kernel in its summing form only (the plain persistent
        # pairs measured slower) -- the summing form is checked below
        assert rc == 4, rc
    else:
        _check("op_mrf_pair", rc)
    got = [t.cpu().numpy().transpose(0, 2, 1) for t in yd]
    for j in range(3 if mode == 0 else 0):
        assert np.isfinite(got[j]).all()
        if small:
            want_xt = orc.conv1d_np(orc.lrelu_np(xs[j], 0.1), w1[j], b1[j], dils[j]).astype(np.float32)
            want = orc.conv1d_np(orc.lrelu_np(want_xt, 0.1), w2[j], b2[j], 1) + xs[j]
            assert np.abs(got[j] - want).max() <= 2 * TOL_LAYER * max(1.0, np.abs(want).max()), j
        assert np.array_equal(got[j], sep[j]), j
    # aliased buffers are refused (a block's window overlaps the rows its neighbours write)
    assert pair(xd, None, mode) != 0
    if mode >= 1:
        if small:                                       # (the oracle itself, not only the separate launches)
            want = [orc.conv1d_np(orc.lrelu_np(orc.conv1d_np(orc.lrelu_np(xs[j], 0.1), w1[j], b1[j], dils[j]).astype(np.float32), 0.1),
                                  w2[j], b2[j], 1) + xs[j] for j in range(3)]
            want_mean = ((want[0] + want[1]) + want[2]) / 3.0
        # the same launch as the LAST pair of a stage: only ((y_0 + y_1) + y_2) / 3 is stored (hifigan_pretrained.py:131-137),
        # bit for bit the reference-order sum of the separate branch outputs
        mean = torch.full((B, L, C), float("nan"), device="cuda")
        _check("op_mrf_pair (summing)", pair(None, mean, mode))
        got_mean = mean.cpu().numpy().transpose(0, 2, 1)
        assert np.array_equal(got_mean, ((sep[0] + sep[1]) + sep[2]) / np.float32(3))
        if small:
            assert np.abs(got_mean - want_mean).max() <= 2 * TOL_LAYER * max(1.0, np.abs(want_mean).max())
        assert pair(None, xd[1], mode) != 0             # the mean may not overwrite an input either
    else:
        assert pair(None, torch.empty((B, L, C), device="cuda"), 0) == 4      # IRIS_HIFIGAN_UNSUPPORTED: mode 0 cannot sum


def test_mrf_step_rejects_what_the_kernel_cannot_take(lib):
    x = [np.zeros((1, 30, 40), np.float32)] * 3
    w = [np.zeros((30, 30, k), np.float32) for k in (3, 7, 11)]
    b = [np.zeros(30, np.float32)] * 3
    status, _ = _mrf_step(lib, x, w, b, None, 1, 40, 30, (1, 1, 1), 0, mean=False)        # C % 4 != 0
    assert status == 4                                                                     # IRIS_HIFIGAN_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# intermediates of a whole forward against the reference's own per-layer taps
# ------------------------------------------------------------------------------------------------
def test_generator_intermediates_match_reference_taps(golden, case_setup, dev):
    """conv_pre, every ConvTranspose1d output and every MRF output of a forward, read out of the workspace
    (iris_hifigan_forward_until), against the activations hooked out of the REFERENCE for the same weights and mel
    (tests/golden/v1_default_T4_taps.npz): a wrong layer shows up where it happens, not only as a waveform error."""
    from iris._engine import GeneratorEngine
    cfg, sd = case_setup("v1_default_T4_taps")
    g = golden("v1_default_T4_taps")
    eng = GeneratorEngine(cfg, sd, dev)
    mel = torch.from_numpy(g["mel"]).to(dev)
    last = 2 * len(cfg.resblock_dilation_sizes[0]) - 1
    for i in range(cfg.num_upsamples):
        taps = eng.forward_until(mel, i, last)
        if i == 0:
            assert np.abs(taps["pre"] - g["conv_pre"]).max() <= TOL_LAYER * np.abs(g["conv_pre"]).max()
        assert np.abs(taps["up"] - g[f"ups_{i}"]).max() <= TOL_LAYER * max(1.0, np.abs(g[f"ups_{i}"]).max()), i
        y = taps["y"]
        mrf = y[0] if taps["mean_in_y0"] else ((y[0] + y[1]) + y[2]) / np.float32(3)
        assert np.abs(mrf - g[f"mrf_{i}"]).max() <= TOL_LAYER * max(1.0, np.abs(g[f"mrf_{i}"]).max()), i
    eng.close()


@pytest.mark.parametrize("T", [4, 300])
def test_generator_intermediates_match_oracle_every_step(T, dev):
    """Every MRF step of every stage (xt after the dilated conv, y after conv + residual) against the numpy oracle's
    ResBlock arithmetic applied to the GPU's own stage input -- at T = 4 (one branch per block) and T = 300 (persistent
    tiles, mean folded by the last step)."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    folded = orc.fold_state_dict(sd)
    eng = GeneratorEngine(cfg, sd, dev)
    mel = torch.from_numpy(seeded_mel(31, 1, T)).to(dev)
    nd = len(cfg.resblock_dilation_sizes[0])
    stage = 3 if T == 4 else 1            # (one stage is enough at T = 300: the oracle's fp64 loops are slow)
    x = eng.forward_until(mel, stage, 0)["up"]
    cur = [x, x, x]
    for m in range(nd):
        taps = eng.forward_until(mel, stage, 2 * m)
        for j, d in enumerate(cfg.resblock_dilation_sizes):
            pfx = f"resblocks.{stage * cfg.num_kernels + j}"
            want = orc.conv1d_np(orc.lrelu_np(cur[j], 0.1), folded[f"{pfx}.convs1.{m}.weight"], folded[f"{pfx}.convs1.{m}.bias"], d[m])
            assert np.abs(taps["xt"][j] - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max()), (m, j)
        xt = taps["xt"]
        taps = eng.forward_until(mel, stage, 2 * m + 1)
        nxt = []
        for j in range(cfg.num_kernels):
            pfx = f"resblocks.{stage * cfg.num_kernels + j}"
            want = orc.conv1d_np(orc.lrelu_np(xt[j], 0.1), folded[f"{pfx}.convs2.{m}.weight"], folded[f"{pfx}.convs2.{m}.bias"], 1) + cur[j]
            nxt.append(want.astype(np.float32))
        if taps["mean_in_y0"]:
            assert m == nd - 1
            want = ((nxt[0] + nxt[1]) + nxt[2]) / np.float32(3)
            assert np.abs(taps["y"][0] - want).max() <= TOL_LAYER * max(1.0, np.abs(want).max())
        else:
            for j in range(cfg.num_kernels):
                assert np.abs(taps["y"][j] - nxt[j]).max() <= TOL_LAYER * max(1.0, np.abs(nxt[j]).max()), (m, j)
            cur = taps["y"]
    eng.close()


# ------------------------------------------------------------------------------------------------
# whole generator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["v1_default_T4_taps", "v1_default_B2_T16", "v1_amplified_T24", "small_cfg_B3_T19"])
def test_generator_matches_reference_goldens(case, golden, case_setup, dev):
    """HIP output vs the waveform the REFERENCE produced for the same weights and mel."""
    from iris._engine import GeneratorEngine
    cfg, sd = case_setup(case)
    g = golden(case)
    eng = GeneratorEngine(cfg, sd, dev)
    got = eng.forward(torch.from_numpy(g["mel"]).to(dev)).cpu().numpy()
    want = g["wav"][:, 0, :]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= TOL_WAV
    eng.close()


@pytest.mark.parametrize("B,T,seed,log_mel", [(1, 100, 1001, False), (3, 57, 5, True), (1, 1, 9, False), (5, 2, 10, False)])
def test_generator_matches_oracle(B, T, seed, log_mel, dev):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel = seeded_mel(seed, B, T, log_mel=log_mel)
    eng = GeneratorEngine(cfg, sd, dev)
    got = eng.forward(torch.from_numpy(mel).to(dev)).cpu().numpy()
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), mel).numpy()[:, 0, :]
    assert got.shape == (B, 256 * T)
    assert np.abs(got - want).max() <= TOL_WAV
    eng.close()


def test_generator_empty_inputs(dev):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg), dev)
    assert eng.forward(torch.empty((0, 80, 10), device=dev)).shape == (0, 2560)
    assert eng.forward(torch.empty((2, 80, 0), device=dev)).shape == (2, 0)
    with pytest.raises(ValueError):
        eng.forward(torch.empty((2, 81, 4), device=dev))
    eng.close()


@pytest.mark.parametrize("B,T", [(4, 40), (12, 40), (2, 282)])
def test_generator_is_deterministic_and_batch_independent(B, T, dev):
    """Batch items are independent: item b of a batch equals the same mel run alone -- bit for bit, also
    when the batch and the single item take different kernels (12 x 40 frames: the stage-0 MRF steps of the batch run on
    the persistent kernel, those of a 40-frame item alone on the 16 x 16-job kernel; 2 x 282: different launch plans)."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=3, gain=1.1, post_gain=10.0), dev)
    mel = torch.from_numpy(seeded_mel(77, B, T)).to(dev)
    full = eng.forward(mel).clone()
    again = eng.forward(mel).clone()
    assert torch.equal(full, again)
    for b in sorted({0, B // 2, B - 1}):
        alone = eng.forward(mel[b:b + 1].contiguous())
        assert torch.equal(alone[0], full[b])
    eng.close()


def test_profile_records_cover_algorithmic_work(dev):
    from iris._engine import GeneratorEngine, algorithmic_work
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg), dev)
    eng.set_profiling(True)
    B, T = 2, 50
    eng.forward(torch.from_numpy(seeded_mel(1, B, T)).to(dev))
    torch.cuda.synchronize()
    recs = eng.read_profile()
    # 1 + 4 * (1 + 6) + 1 layers; the C = 64 / 32 stages run their three conv pairs fused (one launch per pair) at this size
    assert len(recs) == 30 - 2 * 3
    work = algorithmic_work(cfg)
    assert work["flop_per_frame"] == 614_105_088 and work["elements_per_frame"] == 1_305_936
    assert sum(r["flops"] for r in recs) == pytest.approx(work["flop_per_frame"] * B * T, rel=1e-12)
    act_bytes = sum(r["bytes"] for r in recs) - 4.0 * work["weight_values"]
    assert act_bytes == pytest.approx(4.0 * work["elements_per_frame"] * B * T, rel=1e-12)
    assert all(r["ms"] > 0 for r in recs) and all(r["launches"] == 1 for r in recs)
    # grouped records (what bench.py times with): the six MRF launches of a stage share one record -- same work, 11 records
    eng.set_profiling(2)
    eng.forward(torch.from_numpy(seeded_mel(1, B, T)).to(dev))
    eng.forward(torch.from_numpy(seeded_mel(1, B, T)).to(dev))
    torch.cuda.synchronize()
    grouped = eng.read_profile()
    assert len(grouped) == 2 * (1 + 4 * 2 + 1)
    assert [g["kind"] for g in grouped[:4]] == ["conv_pre", "upsample", "mrf_resblock_conv", "upsample"]
    assert sum(g["launches"] for g in grouped) == 2 * 24
    assert [g["launches"] for g in grouped[:10] if g["kind"] == "mrf_resblock_conv"] == [6, 6, 3, 3]
    assert sum(g["flops"] for g in grouped) == pytest.approx(2 * sum(r["flops"] for r in recs), rel=1e-12)
    assert sum(g["bytes"] for g in grouped) == pytest.approx(2 * sum(r["bytes"] for r in recs), rel=1e-12)
    assert all(g["ms"] > 0 for g in grouped)
    eng.set_profiling(False)
    eng.close()


# ------------------------------------------------------------------------------------------------
# BASELINE.json configurations at full size, and the drop-in wrappers
# ------------------------------------------------------------------------------------------------
def test_config2_full_size_matches_oracle(dev):
    """configs[1]: batch 1, 80 x 1000 frames, fp32 -- the bench workload, against the torch oracle."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel = seeded_mel(1002, 1, 1000)
    eng = GeneratorEngine(cfg, sd, dev)
    got = eng.forward(torch.from_numpy(mel).to(dev)).cpu().numpy()
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), mel).numpy()[:, 0, :]
    assert got.shape == (1, 256000)
    assert np.abs(got - want).max() <= TOL_WAV
    assert np.abs(got).max() <= 1.0 and np.abs(got).max() > 0.9      # tanh range is exercised
    eng.close()


def test_config3_batch32_properties(dev):
    """configs[2] shape (batch 32 x 500 frames; fp32 here): too big for the CPU oracle in a test, so
    it is checked through size-independent properties -- every item equals the same mel run alone
    (bit-exact), two items match the oracle, output is finite and inside tanh's range."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel_np = seeded_mel(1003, 32, 500, log_mel=True)
    eng = GeneratorEngine(cfg, sd, dev)
    mel = torch.from_numpy(mel_np).to(dev)
    full = eng.forward(mel).clone()
    assert full.shape == (32, 128000) and torch.isfinite(full).all() and full.abs().max() <= 1.0
    for _ in range(3):      # every CU holds two blocks here: repeated runs must agree bit for bit
        assert torch.equal(eng.forward(mel), full)
    for b in (0, 13, 31):
        alone = eng.forward(mel[b:b + 1].contiguous())
        assert torch.equal(alone[0], full[b])
    folded = orc.to_torch_folded(sd)
    for b in (5, 30):
        want = orc.generator_forward_torch(folded, mel_np[b:b + 1]).numpy()[0, 0]
        assert np.abs(full[b].cpu().numpy() - want).max() <= TOL_WAV
    eng.close()


@pytest.mark.parametrize("B,T", [(32, 1000), (256, 100)])
def test_config4_per_rank_and_short_shapes(B, T, dev):
    """configs[3] (global batch 256 over 8 GPUs): the per-rank workload at N = 8 (32 x 1000 frames) and the
    whole global batch at the grid's shortest length (256 x 100) on one GPU -- finite, inside tanh's range, items
    0 / mid / last against the oracle, and every checked item bit-identical to the same mel vocoded alone."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel_np = seeded_mel(1004, B, T, log_mel=True)
    eng = GeneratorEngine(cfg, sd, dev)
    mel = torch.from_numpy(mel_np).to(dev)
    full = eng.forward(mel).clone()
    assert full.shape == (B, 256 * T) and torch.isfinite(full).all() and full.abs().max() <= 1.0
    assert torch.equal(eng.forward(mel), full)
    folded = orc.to_torch_folded(sd)
    for b in (0, B // 2, B - 1):
        alone = eng.forward(mel[b:b + 1].contiguous())
        assert torch.equal(alone[0], full[b]), b
        want = orc.generator_forward_torch(folded, mel_np[b:b + 1]).numpy()[0, 0]
        assert np.abs(full[b].cpu().numpy() - want).max() <= TOL_WAV, b
    eng.close()


def test_engine_on_a_device_that_is_not_current(dev):
    """The native calls select the engine's device themselves: with two or more GPUs the engine runs on cuda:1 while
    cuda:0 is current; on a one-GPU box the same code path runs with the guard as a no-op."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    target = torch.device("cuda", 1 if torch.cuda.device_count() > 1 else 0)
    torch.cuda.set_device(0)
    eng = GeneratorEngine(cfg, sd, target)
    mel_np = seeded_mel(8, 1, 30)
    got = eng.forward(torch.from_numpy(mel_np).to(target))
    assert torch.cuda.current_device() == 0 and got.device == target
    want = orc.generator_forward_torch(orc.to_torch_folded(sd), mel_np).numpy()[:, 0, :]
    assert np.abs(got.cpu().numpy() - want).max() <= TOL_WAV
    eng.close()


def test_dropin_pretrained_module_on_gpu(tmp_path, manifest, golden, case_setup):
    """iris.hifigan_pretrained: checkpoint containers, squeeze rules and dtypes as recorded from the
    reference (tests/golden/manifest.json), numerics vs the reference's golden waveform."""
    from iris import hifigan_pretrained as hp
    cfg, sd = case_setup("v1_default_B2_T16")
    g = golden("v1_default_B2_T16")
    flat = tmp_path / "generator.ckpt"
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, flat)
    gen = hp.HiFiGANGenerator(flat)
    assert gen.device.type == "cuda" and gen.checkpoint_path == flat and hasattr(gen, "model")
    out = gen(g["mel"])
    assert out.dtype == np.float32 and np.abs(out - g["wav"][:, 0, :]).max() <= TOL_WAV
    sem = manifest["wrapper_semantics"]
    for shape_s, per_entry in sem.items():
        if not shape_s.startswith("["):
            continue
        shape = tuple(int(v) for v in shape_s.strip("[]").split(","))
        x = np.random.default_rng(0).standard_normal(shape)            # float64, like the recording
        a = gen(x)
        b = hp.infer_hifigan(x, sample_rate=22050, hop_length=256, checkpoint_path=flat)
        assert list(a.shape) == per_entry["generator_call"]["shape"] and str(a.dtype) == per_entry["generator_call"]["dtype"]
        assert list(b.shape) == per_entry["infer_hifigan"]["shape"] and str(b.dtype) == per_entry["infer_hifigan"]["dtype"]
    # singleton: same path -> same instance; force_reload -> new one
    first = hp.get_pretrained_hifigan(flat)
    assert hp.get_pretrained_hifigan(flat) is first and hp.get_pretrained_hifigan(flat, force_reload=True) is not first
    for key in ("generator", "model", "state_dict"):
        nested = tmp_path / f"nested_{key}.ckpt"
        torch.save({key: {k: torch.from_numpy(v) for k, v in sd.items()}}, nested)
        assert np.array_equal(hp.HiFiGANGenerator(nested)(g["mel"]), out)
    # HiFiGANModel.forward keeps the reference's tensor contract
    m = hp.HiFiGANModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    y = m(torch.from_numpy(g["mel"]).cuda())
    assert y.shape == (2, 1, 4096) and y.is_cuda and np.abs(y.cpu().numpy() - g["wav"]).max() <= TOL_WAV


def test_dropin_keras_twin_on_gpu(golden, case_setup):
    """iris.vocoder: Keras-layout parameters (no weight-norm, [k,C_in,C_out] / [k,C_out,C_in] kernels)
    loaded from the PyTorch twin's folded weights reproduce the reference's golden waveform; wrapper
    shape rules of HiFiGANVocoder.infer (vocoder.py:191-207)."""
    from iris import vocoder
    from iris._weights import folded_layers, reference_to_keras_layout
    cfg, sd = case_setup("v1_default_B2_T16")
    g = golden("v1_default_B2_T16")
    voc = vocoder.create_vocoder()
    weights = {}
    for spec, w, b in folded_layers(cfg, sd):
        weights[f"{spec.name}.kernel"] = reference_to_keras_layout(spec, w)
        weights[f"{spec.name}.bias"] = b
    voc.model.set_weights_dict(weights)
    out = voc.infer(g["mel"].astype(np.float64))                      # float64 in, like demo_vocoder.py:101
    assert out.shape == (2, 4096) and out.dtype == np.float32
    assert np.abs(out - g["wav"][:, 0, :]).max() <= TOL_WAV
    assert voc(g["mel"][0]).shape == (4096,)                          # [80,T] -> [256T]
    assert voc.infer(g["mel"][:1]).shape == (1, 4096)                 # batch-1 3-D input stays 2-D
    y = voc.model(np.transpose(g["mel"], (0, 2, 1)), training=False)  # channels-last model call
    assert y.shape == (2, 4096, 1)


def test_hipgraph_replay_matches_eager(dev):
    """forward_graph (hipGraph replay of the 30 launches) is bit-identical to the eager forward, for
    several shapes, repeated replays with new inputs, and across a workspace re-allocation."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0), dev, graph_max_frames=0)   # forward = eager
    # (1,300) grows the workspace; (1,64) is re-captured; (3,700) is large enough for the per-forward memset of the
    # MRF kernel's tile counters, which must be part of the captured graph
    for (B, T) in ((1, 64), (2, 33), (1, 300), (1, 64), (3, 700)):
        for seed in (1, 2):
            mel = torch.from_numpy(seeded_mel(seed, B, T, log_mel=True)).to(dev)
            eager = eng.forward(mel).clone()
            replay = eng.forward_graph(mel).clone()
            assert torch.equal(eager, replay), (B, T, seed)
    assert eng.forward_graph(torch.empty((0, 80, 5), device=dev)).shape == (0, 1280)
    eng.close()


@pytest.mark.parametrize("B,T", [(1, 3000), (300, 3), (7, 129)])
def test_generator_long_and_wide_shapes(B, T, dev):
    """A 35-second utterance (L = 768k rows at the last stage, thousands of tiles per launch), a batch
    of 300 three-frame items (batch index folded into the tile index) and an odd in-between shape."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    sd = seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0)
    mel = seeded_mel(B + T, B, T, log_mel=True)
    eng = GeneratorEngine(cfg, sd, dev)
    got = eng.forward(torch.from_numpy(mel).to(dev)).cpu().numpy()
    folded = orc.to_torch_folded(sd)
    idx = sorted({0, B // 2, B - 1})
    want = orc.generator_forward_torch(folded, mel[idx]).numpy()[:, 0, :]
    assert got.shape == (B, 256 * T)
    assert np.abs(got[idx] - want).max() <= TOL_WAV
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
    eng.close()


def test_bench_collective_path_runs_on_rccl(tmp_path):
    """bench.py's N > 1 path (RCCL process group bound to the device, barrier, all-gather of the waveforms,
    max-reduce of the time) exercised with a single rank on the one GPU of this box; the multi-rank control flow
    itself is covered by the world_size-2 gloo tests on CPU."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    repo = Path(__file__).resolve().parents[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    out = subprocess.run([sys.executable, str(repo / "bench.py"), "--gpus", "1", "--force-dist", "--steps", "2", "--warmup", "1",
                          "--frames", "64", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["roofline"]["frac"] > 0


def test_bench_dump_outputs_match_the_oracle(tmp_path):
    """bench.py --dump-outputs writes the waveform of its last timed step: the headline path's output for bench.py's own
    seeded weights (seed 2024) and mel (seed 1002)."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    repo = Path(__file__).resolve().parents[1]
    out = subprocess.run([sys.executable, str(repo / "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "2",
                          "--frames", "64", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["steps"] == 2
    got = np.load(tmp_path / "waveform.npy")
    want = orc.generator_forward_torch(orc.to_torch_folded(seeded_state_dict(GeneratorConfig(), seed=2024)),
                                       seeded_mel(1002, 2, 64)).numpy()[:, 0, :]
    assert got.dtype == np.float32 and got.shape == want.shape == (2, 64 * 256)
    assert np.abs(got - want).max() <= TOL_WAV


def test_integration_md_ctypes_stub_runs(dev):
    """The ctypes stub printed in INTEGRATION.md section 2 (what a reference maintainer would paste) is executed as
    written -- only the library name is made absolute -- against a model with the reference's attribute layout."""
    import re
    from pathlib import Path
    from iris import _native
    from iris.hifigan_pretrained import HiFiGANModel
    from iris._weights import seeded_mel
    text = (Path(__file__).resolve().parents[1] / "INTEGRATION.md").read_text()
    code = re.search(r"```python\n# src/iris/_hifigan_mi355x\.py.*?\n(.*?)```", text, re.S).group(1)
    code = code.replace('ctypes.CDLL("libiris_hifigan.so")', f'ctypes.CDLL("{_native.library_path()}")')
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    torch.manual_seed(0)
    model = HiFiGANModel().to(dev)
    gen = ns["MI355XGenerator"](model)
    mel = torch.from_numpy(seeded_mel(3, 2, 40)).to(dev)
    got = gen(mel)
    want = model(mel)
    assert got.shape == want.shape == (2, 1, 40 * 256)
    # (the stub folds weight-norm with torch, the module with numpy: last-bit differences in the weights)
    assert (got - want).abs().max().item() <= 1e-5


def test_large_batch_runs_as_passes_sharing_one_workspace(dev):
    """A batch of more than 65,536 mel frames runs as consecutive passes over sub-batches that share ONE workspace
    (iris_hifigan_workspace_bytes is bounded: 15 GB instead of 229 KB x every frame).  Batch items are independent, so
    every item must equal -- bit for bit -- the same item vocoded alone; checked on items of the first pass, across the
    pass boundary and in the last (partial) pass."""
    from iris import _native
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=77, gain=1.1, post_gain=8.0), dev)
    B, T = 70, 1000                                    # 70,000 frames: a pass of 65 items and one of 5
    plan = _native.describe_plan(cfg, B, T, _native.DTYPE_F32)
    assert plan["passes"] == 2
    assert eng.workspace_bytes(B, T) == eng.workspace_bytes(65, T) == plan["workspace_bytes"] < 16e9
    mel = torch.from_numpy(seeded_mel(4242, B, T)).to(dev)
    wav = eng.forward(mel)
    torch.cuda.synchronize()
    assert torch.isfinite(wav).all()
    for i in (0, 64, 65, 69):
        alone = eng.forward(mel[i:i + 1].contiguous())
        assert torch.equal(wav[i:i + 1], alone), i
    eng.close()


def test_prepare_and_profiling_survive_graph_capture(dev):
    """ABI v3: the packings beyond fp32 are built on first use (iris_hifigan_prepare, or the first forward of the dtype), and
    capturing a forward into a hipGraph while profiling is on PAUSES the records instead of resetting them."""
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=5, gain=1.1, post_gain=6.0), dev)
    mel = torch.from_numpy(seeded_mel(8, 1, 40)).to(dev)
    eng.prepare("bf16")                                   # explicit: nothing left to build inside the capture below
    eng.prepare("bf16")                                   # idempotent
    eng.set_profiling(1)
    want = eng.forward(mel).clone()
    torch.cuda.synchronize()
    n_one = len(eng.read_profile())
    assert n_one >= 20
    got = eng.forward_graph(mel)                          # first use of this shape: warm-up + capture, profiling paused
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert len(eng.read_profile()) == n_one               # the records of the eager forward are still there, none were added
    eng.forward(mel)
    torch.cuda.synchronize()
    assert len(eng.read_profile()) == 2 * n_one           # ... and profiling is on again
    b16 = eng.forward_graph(mel, dtype="bf16")            # captured without a lazy build inside the capture
    torch.cuda.synchronize()
    assert torch.isfinite(b16).all() and (b16 - want).abs().max() <= 6e-2
    eng.close()
