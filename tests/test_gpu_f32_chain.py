"""Every fp32 launch against its fmaf chain, BIT FOR BIT, from a CPU oracle (oracle/chain_oracle.c).

DESIGN.md section 3 defines the chain every fp32 output element is; the suite otherwise holds fp32 kernel against kernel
(bitwise) or against ATen / fp64 with 20 ... 100 x the rounding noise of slack.  Here:

* single layers, at the cases of tests/test_gpu_parity.py (imported, not copied): Conv1d (the channels-first one included),
  ConvTranspose1d, the MRF step in every plan 0 ... 6, the summing step, the fused pair and its summing form at the shapes
  that module flags ``small``: ``np.array_equal(got, chain)``; conv_post: |got - tanh_fp64(chain pre-activation)| <= 2e-6;
* whole forwards (``forward_until``, eager launches): every launch listed in oracle/f32_cases.SHAPES restated from the GPU's
  OWN input tensors (nothing propagates), equality again; the waveform at 2e-6 behind the chain's pre-activation.

Large launches are restated on row windows (f32_cases.judged_rows: first and last 256 rows, two stretches of 611 rows
aligned to no tile, every 37th row; all channels, all batch items); a test fails if a launch was judged on under 3 % of
its rows.  tests/test_oracle_chain.py holds the oracle to exact arithmetic and the shape list to the launch plan.
Time.  A case is bound by the CPU restatement, not by the device (a few ``forward_until`` calls and copies): with random
tensors in place of the device's, the 25 forward cases restate 305 tensors / 137.6 M elements in 59 s on 8 cores (the C
loop runs about 10 G fmaf/s there); slowest v1-3x150 (two whole stages, 22 tensors) 7.7 s, then v1-4x500 6.0 s, v1-4x560
5.8 s, v1-1x480 5.7 s, v1-3x1249 5.0 s; no case reaches the 10 s at which its walked stages would be shrunk.  Every case
prints its tensors, judged elements and wall time (``pytest -s``).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import test_gpu_parity as tp
from oracle import chain_oracle as co
from oracle import f32_cases as fc

pytestmark = pytest.mark.gpu
lib = tp.lib
dev = tp.dev
KS = (3, 7, 11)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ from the chain; first at {i}: "
                             f"got {got[i]!r} chain {want[i]!r}; rows {sorted(set(bad[:, -1].tolist()))[:12]}")


@pytest.mark.parametrize("B,L,Ci,Co,k,d,act,use_res", tp.CONV_CASES)
def test_conv1d_is_the_chain(lib, B, L, Ci, Co, k, d, act, use_res):
    rng = np.random.default_rng(B * 1000 + L + Ci + k + d)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, k)) / np.sqrt(Ci * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    res = rng.standard_normal((B, Co, L)).astype(np.float32) if use_res else None
    xd, rd = tp._cl(x), (tp._cl(res) if use_res else None)
    yd = torch.full((B, L, Co), float("nan"), device="cuda")
    tp._check("op_conv1d", lib.iris_hifigan_op_conv1d(xd.data_ptr(), tp._fp(w), tp._fp(b), rd.data_ptr() if use_res else None,
                                                     yd.data_ptr(), B, L, Ci, Co, k, d, act, 0.1, 0, None))
    want = co.chain_conv1d(co.lrelu32(x) if act else x, w, b, d, fc.single_layer_chunk(Ci, Co), [(0, L)], residual=res)
    _same(yd.cpu().numpy().transpose(0, 2, 1), want, "conv1d")


def test_conv1d_channels_first_is_the_chain(lib):
    rng = np.random.default_rng(11)
    B, L, Ci, Co, k = 2, 45, 80, 512, 7
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, k)) / np.sqrt(Ci * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((B, L, Co), float("nan"), device="cuda")
    tp._check("op_conv1d", lib.iris_hifigan_op_conv1d(xd.data_ptr(), tp._fp(w), tp._fp(b), None, yd.data_ptr(),
                                                     B, L, Ci, Co, k, 1, 0, 0.1, 1, None))
    _same(yd.cpu().numpy().transpose(0, 2, 1), co.chain_conv1d(x, w, b, 1, fc.single_layer_chunk(Ci, Co, True), [(0, L)]), "conv_pre")


@pytest.mark.parametrize("B,L,Ci,Co,k,u", tp.CONVT_CASES)
def test_conv_transpose1d_is_the_chain(lib, B, L, Ci, Co, k, u):
    rng = np.random.default_rng(L * 7 + Ci + k)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, k)) / np.sqrt(Ci * k / u)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    xd = tp._cl(x)
    yd = torch.full((B, L * u, Co), float("nan"), device="cuda")
    tp._check("op_conv_transpose1d", lib.iris_hifigan_op_conv_transpose1d(
        xd.data_ptr(), tp._fp(w), tp._fp(b), yd.data_ptr(), B, L, Ci, Co, k, u, 1, 0.1, None))
    # (the GEMM kernel and the polyphase one at C_in > 32 stage 64 channels; below that one chunk holds them all)
    want = co.chain_conv_transpose1d(co.lrelu32(x), w, b, u, fc.single_layer_chunk(Ci, Co), [(0, L * u)])
    _same(yd.cpu().numpy().transpose(0, 2, 1), want, "conv_transpose1d")


@pytest.mark.parametrize("B,L,C,k,three", tp.CONV_POST_CASES)
def test_conv_post_is_tanh_of_the_chain(lib, B, L, C, k, three):
    rng = np.random.default_rng(L + C)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) * 2 for _ in range(3 if three else 1)]
    w = (rng.standard_normal((1, C, k)) * 0.3).astype(np.float32)
    b = rng.standard_normal(1).astype(np.float32)
    xd = [tp._cl(v) for v in xs]
    yd = torch.full((B, L), float("nan"), device="cuda")
    tp._check("op_conv_post", lib.iris_hifigan_op_conv_post(
        xd[0].data_ptr(), xd[1].data_ptr() if three else None, xd[2].data_ptr() if three else None,
        tp._fp(w), tp._fp(b), yd.data_ptr(), B, L, C, k, 0.1, None))
    pre = co.chain_conv_post_preact(co.lrelu32(co.mean32(xs) if three else xs[0]), w, b, [(0, L)])
    got = yd.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - np.tanh(pre.astype(np.float64))).max() <= fc.TOL_TANH


def _mrf_inputs(seed, B, L, C, use_res=True):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in KS]
    ws = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in KS]
    bs = [rng.standard_normal(C).astype(np.float32) for _ in KS]
    rs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in KS] if use_res else None
    return xs, ws, bs, rs


@pytest.mark.parametrize("B,L,C,dils,use_res", tp.MRF_STEP_CASES)
def test_mrf_step_is_the_chain_in_every_plan(lib, B, L, C, dils, use_res):
    xs, ws, bs, rs = _mrf_inputs(C * 7 + L, B, L, C, use_res)
    chunk = fc.single_layer_chunk(C, C)
    want = [co.chain_conv1d(co.lrelu32(xs[j]), ws[j], bs[j], dils[j], chunk, [(0, L)], residual=rs[j] if use_res else None)
            for j in range(3)]
    for plan in range(7):
        if plan >= 5 and C < 128:
            continue                                    # (the job mode needs two C_in chunks)
        status, got = tp._mrf_step(lib, xs, ws, bs, rs, B, L, C, dils, plan, mean=False)
        tp._check("op_mrf_step", status)
        for j in range(3):
            _same(got[j], want[j], f"plan {plan} branch {j}")


@pytest.mark.parametrize("B,L,C", tp.MRF_SUM_CASES)
def test_mrf_summing_step_is_the_chain(lib, B, L, C):
    xs, ws, bs, rs = _mrf_inputs(C + L, B, L, C)
    chunk = fc.single_layer_chunk(C, C)
    ys = [co.chain_conv1d(co.lrelu32(xs[j]), ws[j], bs[j], 1, chunk, [(0, L)], residual=rs[j]) for j in range(3)]
    for plan in (0, 1, 2):
        status, got = tp._mrf_step(lib, xs, ws, bs, rs, B, L, C, (1, 1, 1), plan, mean=True)
        tp._check("op_mrf_step", status)
        _same(got, co.mean32(ys), f"summing step, plan {plan}")


@pytest.mark.parametrize("B,L,C,dils", [c for c in tp.MRF_PAIR_CASES if c[0] * c[1] * c[2] <= tp.MRF_PAIR_SMALL])
def test_mrf_fused_pair_is_the_chain(lib, B, L, C, dils):
    """The shapes of test_mrf_fused_pair_matches_oracle_and_separate_steps that it flags ``small`` (B L C <= 400,000)."""
    rng = np.random.default_rng(C * 11 + L)
    xs = [rng.standard_normal((B, C, L)).astype(np.float32) for _ in KS]
    w1 = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in KS]
    b1 = [rng.standard_normal(C).astype(np.float32) for _ in KS]
    w2 = [(rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for k in KS]
    b2 = [rng.standard_normal(C).astype(np.float32) for _ in KS]
    want = [fc.pair(xs[j], (w1[j], b1[j]), (w2[j], b2[j]), dils[j], C, [(0, L)]) for j in range(3)]
    xd = [tp._cl(x) for x in xs]
    vp3, fp3 = ctypes.c_void_p * 3, ctypes.POINTER(ctypes.c_float) * 3

    def run(y_tensors, mean_tensor, mode):
        return lib.iris_hifigan_op_mrf_pair(
            vp3(*[t.data_ptr() for t in xd]), fp3(*[tp._fp(w) for w in w1]), fp3(*[tp._fp(b) for b in b1]),
            fp3(*[tp._fp(w) for w in w2]), fp3(*[tp._fp(b) for b in b2]),
            vp3(*[t.data_ptr() for t in y_tensors]) if y_tensors is not None else None,
            ctypes.c_void_p(mean_tensor.data_ptr()) if mean_tensor is not None else None,
            B, L, C, (ctypes.c_int32 * 3)(*KS), (ctypes.c_int32 * 3)(*dils), 0.1, mode, None)
    yd = [torch.full((B, L, C), float("nan"), device="cuda") for _ in range(3)]
    tp._check("op_mrf_pair", run(yd, None, 0))
    for j in range(3):
        _same(yd[j].cpu().numpy().transpose(0, 2, 1), want[j], f"pair branch {j}")
    for mode in (1, 2):                                  # the summing form: jobs drawn from a counter / fixed stride
        mean = torch.full((B, L, C), float("nan"), device="cuda")
        tp._check("op_mrf_pair (summing)", run(None, mean, mode))
        _same(mean.cpu().numpy().transpose(0, 2, 1), co.mean32(want), f"summing pair, mode {mode}")


# ---- whole forwards, every listed launch ------------------------------------------------------------------------------------
class _DeviceTensors:
    """The tensors of one device forward, as ``fc.walk`` asks for them.  Every call stops at an ODD step, so that a stage runs
    the forward's own launches (a stop behind a conv1 would un-fuse its pairs): ("xt", i, m) and ("y", i, m) both come from
    ``forward_until(i, 2 m + 1)``, whose xt buffers still hold conv1's output when the pair ran as two launches."""

    def __init__(self, eng, mel, nd):
        self.eng, self.mel, self.nd, self.cache = eng, mel, nd, {}

    def until(self, i, m):
        if (i, m) not in self.cache:
            if len(self.cache) >= 2:
                self.cache.pop(next(iter(self.cache)))
            self.cache[(i, m)] = self.eng.forward_until(self.mel, i, 2 * m + 1, dtype="f32")
        return self.cache[(i, m)]

    def get(self, key):
        if key[0] == "pre":
            return self.until(0, 0)["pre"]
        if key[0] == "up":
            return self.until(key[1], 0)["up"]
        if key[0] == "wav":
            return self.eng.forward(self.mel, dtype="f32").cpu().numpy()
        t = self.until(key[1], key[2])
        if key[0] == "xt":
            return t["xt"]
        assert not t["mean_in_y0"] or key[2] == self.nd - 1
        return [t["y"][0]] if t["mean_in_y0"] else t["y"]


@pytest.mark.parametrize("shape", fc.SHAPES, ids=[s[0] for s in fc.SHAPES])
def test_f32_every_launch_is_its_chain_on_its_own_inputs(shape, dev):
    from iris._engine import GeneratorEngine
    sid, name, B, T, spec, _ = shape
    cfg, sd, W = fc.setup(name)
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)
    mel = fc.shape_mel(shape)
    launches = fc.plan_launches(cfg, B, T, torch.cuda.get_device_properties(dev).multi_processor_count)
    t0 = time.perf_counter()
    prov = _DeviceTensors(eng, torch.from_numpy(mel).to(dev), len(cfg.resblock_dilation_sizes[0]))
    bad, n, elements = [], 0, 0
    for rec in fc.walk(cfg, fc.numpy_weights(W), mel, launches, prov, spec):
        n += 1
        got, want = rec["got"], rec["want"]
        assert got.shape == want.shape and np.isfinite(got).all(), rec["label"]
        judged = fc.n_rows(rec["rows"])
        assert judged >= fc.MIN_SHARE * rec["total_rows"], (rec["label"], judged, rec["total_rows"])
        elements += got.size
        if rec["kind"] == "wav":
            err = float(np.abs(got - np.tanh(want.astype(np.float64))).max())
            print(f"f32 chain {sid} {rec['label']}: max err {err:.2e} on {judged} of {rec['total_rows']} rows")
            if not err <= fc.TOL_TANH:
                bad.append((rec["label"], err))
            continue
        diff = got != want
        print(f"f32 chain {sid} {rec['label']} [{rec['kernel']}, chunk {rec['chunk']}]: {int(diff.sum())} of {got.size} differ, "
              f"{judged} of {rec['total_rows']} rows")
        if diff.any():
            i = tuple(np.argwhere(diff)[0])
            bad.append((rec["label"], rec["kernel"], int(diff.sum()), got.size, f"first at {i}: got {got[i]!r} chain {want[i]!r}",
                        f"max |diff| {float(np.abs(got - want).max()):.3e}"))
    print(f"f32 chain {sid}: {n} tensors, {elements} elements judged in {time.perf_counter() - t0:.1f} s")
    eng.close()
    assert n > 0
    assert not bad, bad
