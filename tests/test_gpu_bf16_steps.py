"""Every launch of a bf16 forward against the restatement of that one launch on the GPU's OWN input tensors.

tests/test_gpu_bf16.py reaches the bf16 kernels through the ``iris_hifigan_op_*_bf16`` entry points: one problem, one input
tensor.  ``bf16_forward`` launches forms those cannot reach: conv_pre staging the fp32 channels-first mel, ConvTranspose1d
forming the mean of two or three branch tensors while it stages them (both block shapes of the GEMM kernel and the
polyphase fallback), ConvTranspose1d with no activation behind the summing pair, the grouped conv launch of all branches,
the summing pair inside a forward, and the three conv_post kernels.  Here ``forward_until`` returns the tensors of a
forward and oracle/bf16_cases.py restates each launch on them, so nothing propagates and the single-layer bar holds per
launch:

    |got - want64| <= ulp_bf16(want64) * 1.001 + C_ABS * absconv      and      share(got == r16(want64)) >= 0.999

(want64: the layer in fp64 on the operands as the kernel forms them; absconv: the same on their magnitudes.)  C_ABS and
the share floor come from tests/test_oracle_bf16.py, which derives them from the references alone, shows that a truncated
mel or activation, LeakyReLU per branch, a dropped input row, a wrong divisor and unrounded branch tensors each fail, and
holds the shapes below to the kernel forms they are meant to reach.  The upsampler of stage i is restated on the branch
tensors of ``forward_until(i - 1, last)``, where stage i - 1 ran as plain pairs, while in the ``(i, 0)`` call it ran in
its forward form: the one check holds the summing pair and the three-tensor staging to the per-branch tensors.  The
fp32 waveform is held to the conv_post bar of tests/test_gpu_parity.py (2e-6 + 2e-5).

Every test prints, per launch, the worst err/ulp, the exact share and max (err - ulp)/absconv, and per shape the worst of
each kind of launch and the time taken.  Figures of the fp32-accumulating CPU restatement on the same shapes, for
comparison (tests/test_oracle_bf16.py): err/ulp 0.5 ... 113 (the large values on cancelled outputs), share 0.99965 ... 1.0,
(err - ulp)/absconv <= 6.6e-8, waveform 2e-7 ... 1.1e-6.  The ranges observed on the MI355X are not recorded here yet: copy them from the
`bf16 steps <shape> worst ...` lines of the first run.
"""
import time

import numpy as np
import pytest
import torch

from oracle import bf16_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


class _DeviceTensors:
    """The tensors of one device forward, as ``bc.walk`` asks for them: one ``forward_until`` per MRF step."""

    def __init__(self, eng, mel):
        self.eng, self.mel, self.key, self.taps = eng, mel, None, None

    def until(self, stage, step):
        if self.key != (stage, step):
            t = self.eng.forward_until(self.mel, stage, step, dtype="bf16")
            assert not t["mean_in_y0"]
            self.key, self.taps = (stage, step), t
        return self.taps

    def pre(self):
        return torch.from_numpy(self.until(0, 0)["pre"])

    def up(self, i):
        return torch.from_numpy(self.until(i, 0)["up"])

    def xt(self, i, m):
        return [torch.from_numpy(t) for t in self.until(i, 2 * m)["xt"]]

    def y(self, i, m):
        return [torch.from_numpy(t) for t in self.until(i, 2 * m + 1)["y"]]

    def wav(self):
        return self.eng.forward(self.mel, dtype="bf16").cpu()


@pytest.mark.parametrize("shape", bc.SHAPES, ids=[s[0] for s in bc.SHAPES])
def test_bf16_every_launch_matches_restatement_on_its_own_inputs(shape, dev):
    from iris._engine import GeneratorEngine
    sid, name, B, T, stages, _ = shape
    cfg, sd, W = bc.setup(name)
    eng = GeneratorEngine(cfg, sd, dev, graph_max_frames=0)
    mel = bc.shape_mel(shape)
    t0 = time.perf_counter()
    bad, worst = [], {}
    n = 0
    for rec in bc.walk(cfg, W, mel, _DeviceTensors(eng, torch.from_numpy(mel).to(dev)), stages):
        n += 1
        if rec["kind"] == "wav":
            got = rec["got"]
            assert got.shape == (B, T * cfg.hop_length) and torch.isfinite(got).all()
            err = float((got.double() - rec["want64"]).abs().max())
            print(f"bf16 steps {sid} {rec['label']}: max err {err:.2e} (max |pre-tanh| {float(rec['pre_tanh'].abs().max()):.2f})")
            if not err <= bc.TOL_WAV:
                bad.append((rec["label"], err))
            continue
        got, want = rec["got"].numpy(), rec["want64"].numpy()
        assert got.shape == want.shape, rec["label"]
        f = bc.judge(got, want, rec["absconv"].numpy())
        print(f"bf16 steps {sid} {rec['label']}: err/ulp {f['err_ulp']:.2f}, share {f['share']:.5f}, "
              f"(err - ulp)/absconv {f['excess']:.2e}")
        kind = rec["label"].split()[0] if not rec["label"].startswith("stage") else "mrf"
        w = worst.setdefault(kind, [0.0, 1.0, -1.0])
        w[0], w[1], w[2] = max(w[0], f["err_ulp"]), min(w[1], f["share"]), max(w[2], f["excess"])
        if not (f["ok_abs"] and f["share"] >= bc.SHARE_MIN):
            d = np.abs(got - want) - bc.ulp_bf16(want) * 1.001 - bc.C_ABS * rec["absconv"].numpy()
            b, c, r = np.unravel_index(int(np.argmax(d)), d.shape)
            bad.append((rec["label"], f, f"worst at item {b} channel {c} restated row {r}: got {got[b, c, r]!r} want {want[b, c, r]!r}"))
    nd = len(cfg.resblock_dilation_sizes[0])
    n_stages = cfg.num_upsamples if stages is None else max(stages) + 1
    assert n == 1 + n_stages * (1 + 2 * nd * cfg.num_kernels) + (stages is None)
    for kind, w in sorted(worst.items()):
        print(f"bf16 steps {sid} worst {kind}: err/ulp {w[0]:.2f}, share {w[1]:.5f}, (err - ulp)/absconv {w[2]:.2e}")
    print(f"bf16 steps {sid}: {n} launches checked in {time.perf_counter() - t0:.1f} s")
    eng.close()
    assert not bad, bad
