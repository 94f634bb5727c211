"""The bf16-storage forward (dtype "bf16"), launch by launch.  TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

``bf16_forward`` (csrc/iris_hifigan_bf16.hip) launches forms that no ``iris_hifigan_op_*_bf16`` entry point reaches: the
fp32 channels-first mel staged by conv_pre, ConvTranspose1d forming the MRF mean of two or three branch tensors while it
stages its input, the grouped Conv1d launch of all branches, the summing pair and the three conv_post kernels.  ``walk``
restates every launch of one forward on the operands AS THE KERNEL FORMS THEM -- input activated in fp32, then rounded to
bf16; weights rounded to bf16; bias, residual and the MRF mean ((y0 + y1) + y2) * fp32(1/n) in fp32
(``hifigan_oracle.generator_forward_bf16`` documents the rounding points) -- from the tensors a provider hands it: the
GPU's own tensors (tests/test_gpu_bf16_steps.py; nothing propagates from launch to launch), or, with no provider, the
tensors of the walk itself with fp32 accumulation (tests/test_oracle_bf16.py: what the references alone can tell apart).

The criterion for one bf16 tensor (``judge``), with want64 the layer in fp64 and absconv the same layer on |x|, |w|, |b|
(+ |res|):

    |got - want64| <= ulp_bf16(want64) * 1.001 + C_ABS * absconv      and      share(got == r16(want64)) >= SHARE_MIN

``C_ABS * absconv`` is the room for fp32 accumulation in another order than fp64's: forward tensors contain cancelled
outputs, on which the accumulation error is many ulp OF THE OUTPUT but a fixed small multiple of 2^-24 of absconv.
C_ABS is 4 x the largest |conv_fp32 - conv_fp64| / absconv that ATen's fp32 convs show over the shapes below;
tests/test_oracle_bf16.py measures it, holds this constant to the measurement and records the figures.  The fp32
waveform is held to the bar of tests/test_gpu_parity.py::test_conv_post_matches_oracle (TOL_WAV).
"""
import re

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.1
C_ABS = 1.15e-6             # 4 x 2.85e-7: tests/test_oracle_bf16.py measures 2.83e-7 (v1-3x57, ups.1) and holds this to it
SHARE_MIN = 0.999           # the kernel: elements that are exactly r16(want64), per tensor
SHARE_MIN_REF = 0.9995      # the fp32-accumulating restatement must stay above this, so that SHARE_MIN can only fail for the kernel
TOL_WAV = 2e-6 + 2e-5       # test_conv_post_matches_oracle's bar, absolute on the tanh output
CU = 256                    # MI355X; describe_plan's default as well


# ---- configurations and shapes -------------------------------------------------------------------------------------------
def v1_config():
    from iris._weights import GeneratorConfig
    return GeneratorConfig()


def generic_config():
    """tests/test_gpu_bf16.py::test_bf16_generic_config_and_unsupported_config's generator: two MRF kernels, rates 4/2/3,
    channels 64 -> 32/16/8.  ups.1 and ups.2 take the polyphase fallback with n_mrf = 2; conv_post reads two bf16 tensors."""
    from iris._weights import GeneratorConfig
    return GeneratorConfig(in_channels=16, upsample_rates=(4, 2, 3), upsample_kernel_sizes=(8, 4, 9),
                           upsample_initial_channel=64, resblock_kernel_sizes=(3, 5),
                           resblock_dilation_sizes=((1, 2), (2, 6)))


def post24_config():
    """Channels 96 -> 48/24, three MRF kernels: C = 24 is a multiple of 8 that conv_post_rows_kernel does not take, so
    conv_post runs on conv_post_tanh_bf16_kernel; C_in = 48 keeps ups.1 off the GEMM kernel: the polyphase fallback
    with n_mrf = 3."""
    from iris._weights import GeneratorConfig
    return GeneratorConfig(in_channels=24, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4),
                           upsample_initial_channel=96, resblock_kernel_sizes=(3, 5, 7),
                           resblock_dilation_sizes=((1, 3), (1, 3), (1, 3)))


CONFIGS = {"v1": (v1_config, dict(seed=2025, gain=1.18, post_gain=20.0)),
           "generic": (generic_config, dict(seed=7, gain=1.3, post_gain=6.0)),
           "post24": (post24_config, dict(seed=11, gain=1.2, post_gain=4.0))}

# (id, config, B, T, stages or None = all and the waveform, mel seed).  v1-2x12: every tensor ragged against every tile.
# v1-8x127: ceil((1016 + 1) / 64) * 4 * 8 = 512 = 2 * 256 blocks: the 64 x 256 NIN = 3 form of ups.1; stages 0-1 only.
SHAPES = [("v1-2x12", "v1", 2, 12, None, 31), ("v1-3x57", "v1", 3, 57, None, 32), ("v1-8x127", "v1", 8, 127, (0, 1), 33),
          ("generic-3x37", "generic", 3, 37, None, 34), ("post24-3x70", "post24", 3, 70, None, 35)]


def setup(name):
    """(cfg, state dict, {layer: (weight fp32, bias fp32) torch}) -- the folded fp32 weights are the ones the engine
    uploads (iris._weights.folded_layers), so that rounding them to bf16 here gives the kernel's operand bit for bit."""
    from iris._weights import folded_layers, seeded_state_dict
    make, kw = CONFIGS[name]
    cfg = make()
    sd = seeded_state_dict(cfg, **kw)
    W = {s.name: (torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(np.ascontiguousarray(b)))
         for s, w, b in folded_layers(cfg, sd)}
    return cfg, sd, W


def shape_mel(shape):
    from iris._weights import seeded_mel
    _, name, B, T, _, seed = shape
    return seeded_mel(seed, B, T, n_mels=CONFIGS[name][0]().in_channels, log_mel=bool(seed & 1))


# ---- number formats ------------------------------------------------------------------------------------------------------
def r16(t):
    """fp32 tensor -> nearest-even bf16 value, as fp32 (v_cvt_pk_bf16_f32)."""
    return t.to(torch.bfloat16).to(torch.float32)


def t16(t):
    """The WRONG rounding: truncation to bf16 (low 16 bits masked)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def r16_f64(a):
    """fp64 numpy -> nearest-even bf16 value in ONE rounding (not through fp32), as fp64."""
    m, e = np.frexp(a)
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)


def ulp_bf16(ref):
    """One bf16 ulp at the magnitude of ref, as tests/test_gpu_bf16.py defines it (8 significand bits)."""
    return np.maximum(np.abs(ref), 2.0 ** -126) * 2.0 ** -7


def lrelu32(t, slope=SLOPE):
    return torch.where(t > 0, t, t * torch.tensor(slope, dtype=torch.float32))


def mrf_mean(ys, n=None):
    """((y0 + y1) + y2) * fp32(1/n) in fp32, as every consumer of a stage's branch tensors forms it."""
    s = ys[0]
    for y in ys[1:]:
        s = s + y
    return s * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n or len(ys)), dtype=torch.float32))


def judge(got, want64, absconv, c=C_ABS):
    """The per-tensor figures and the two conditions.  got: bf16 values; want64, absconv: fp64."""
    got, want64, absconv = (np.asarray(a, dtype=np.float64) for a in (got, want64, absconv))
    err = np.abs(got - want64)
    ulp = ulp_bf16(want64)
    return {"err_ulp": float((err / ulp).max()), "share": float((got == r16_f64(want64)).mean()),
            "excess": float(((err - ulp) / np.maximum(absconv, 2.0 ** -126)).max()),
            "ok_abs": bool(np.isfinite(got).all() and (err <= ulp * 1.001 + c * absconv).all())}


# ---- one layer on row windows --------------------------------------------------------------------------------------------
def windows(B, L, C):
    """Row ranges a launch is restated on: the whole tensor unless the fp64 convs would take seconds (V1's 8 x 127 shape
    at C = 128); then its first and last two tiles' worth, the ragged end included, and a stretch aligned to nothing."""
    if L <= 1536 or B * L * C * C <= 3e8:
        return [(0, L)]
    mid = (L // 2) | 77
    return [(0, 521), (mid - 256, mid + 256), (L - 521, L)]


def rows(t, wins):
    return t if len(wins) == 1 and wins[0] == (0, t.shape[2]) else torch.cat([t[:, :, a:e] for a, e in wins], dim=2)


def conv_rows(x16, w16, b, d, res, wins, dt):
    """Conv1d ('same' zero padding, dilation d) + bias (+ residual) on the output rows ``wins``, in dtype ``dt``: each
    range from its own rows plus the halo (rows a cut pads with zeros lie outside the range)."""
    k, L = w16.shape[-1], x16.shape[2]
    h = d * (k - 1) // 2
    parts = []
    for a, e in wins:
        lo, hi = max(0, a - h), min(L, e + h)
        y = F.conv1d(x16[:, :, lo:hi].to(dt), w16.to(dt), b.to(dt), dilation=d, padding=h)[:, :, a - lo: e - lo]
        parts.append(y if res is None else y + res[:, :, a:e].to(dt))
    return torch.cat(parts, dim=2)


def convt_rows(x16, w16, b, u, wins_in, dt):
    """ConvTranspose1d(k, stride u, padding (k - u) / 2) + bias on the output rows [a * u, e * u) of the INPUT row ranges
    ``wins_in``."""
    k, L = w16.shape[-1], x16.shape[2]
    h = -(-k // u)
    parts = []
    for a, e in wins_in:
        lo, hi = max(0, a - h), min(L, e + h)
        y = F.conv_transpose1d(x16[:, :, lo:hi].to(dt), w16.to(dt), b.to(dt), stride=u, padding=(k - u) // 2)
        parts.append(y[:, :, (a - lo) * u: (e - lo) * u])
    return torch.cat(parts, dim=2)


def _apply(kind, x16, w16, b, arg, res, wins, dt):
    if kind == "conv":
        return conv_rows(x16, w16, b, arg, res, wins, dt)
    return convt_rows(x16, w16, b, arg, wins, dt)


# ---- the walk ------------------------------------------------------------------------------------------------------------
MUTATIONS = ("trunc_mel", "trunc_act", "lrelu_per_branch", "drop_last_row", "unrounded_y", "inv_n_of_three")


def walk(cfg, W, mel, prov=None, stages=None, mutation=None):
    """Yields one record per launch of a bf16 forward of ``mel`` (fp32 numpy [B, C, T]):
    {label, kind: "bf16" | "wav", got, want64, absconv, y32} -- torch tensors on the restated rows; want64 is the layer
    in fp64 on the operands, absconv the same on their magnitudes, y32 the same with ATen's fp32 accumulation.

    prov: the tensors of a device forward -- ``pre()``, ``up(i)``, ``xt(i, m)``, ``y(i, m)`` (lists over the branches),
    ``wav()``, fp32 torch [B, C, L] -- every launch is then restated on THEIR values.  None: the walk feeds itself with
    got = r16(y32), the restatement with fp32 accumulation.
    stages: the stages to walk (a prefix); the waveform is checked only when None.
    mutation (prov None only): a WRONG restatement, one of MUTATIONS, that ``got`` then follows; want64 never does."""
    assert mutation is None or (prov is None and mutation in MUTATIONS)
    mel = torch.as_tensor(mel).float()
    B = mel.shape[0]
    nk, nd = cfg.num_kernels, len(cfg.resblock_dilation_sizes[0])

    def rec(label, kind, x16, w, b, arg, res, wins_in, wins_out, got_full, x16_got=None):
        w16 = r16(w)
        want = _apply(kind, x16, w16, b, arg, res, wins_in, torch.float64)
        absc = _apply(kind, x16.abs(), w16.abs(), b.abs(), arg, None if res is None else res.abs(), wins_in, torch.float64)
        y32 = _apply(kind, x16, w16, b, arg, res, wins_in, torch.float32)
        if got_full is None:                       # the walk feeds itself: full length, fp32 accumulation, maybe mutated
            whole = [(0, x16.shape[2])]
            if x16_got is None and wins_in == whole:
                got_full = r16(y32)
            else:
                got_full = r16(_apply(kind, x16 if x16_got is None else x16_got, w16, b, arg, res, whole, torch.float32))
        return {"label": label, "kind": "bf16", "got": rows(got_full, wins_out), "want64": want, "absconv": absc,
                "y32": y32}, got_full

    # conv_pre: the fp32 channels-first mel, rounded while it is staged
    w, b = W["conv_pre"]
    L = mel.shape[2]
    r, pre = rec("conv_pre", "conv", r16(mel), w, b, 1, None, [(0, L)], [(0, L)], prov.pre() if prov else None,
                 t16(mel) if mutation == "trunc_mel" else None)
    yield r
    ys, last_y32 = None, None
    for i in range(cfg.num_upsamples if stages is None else max(stages) + 1):
        u, C = cfg.upsample_rates[i], cfg.stage_channels(i)
        # LeakyReLU + ConvTranspose1d on pre, or on the fp32 mean of the previous stage's branch tensors
        src = pre if i == 0 else mrf_mean(ys)
        x16_got = None
        if mutation == "trunc_act":
            x16_got = t16(lrelu32(src))
        elif i > 0 and mutation == "lrelu_per_branch":
            x16_got = r16(mrf_mean([lrelu32(y) for y in ys]))
        elif i > 0 and mutation == "drop_last_row":
            cut = [y.clone() for y in ys]
            cut[-1][:, :, -1] = 0
            x16_got = r16(lrelu32(mrf_mean(cut)))
        elif i > 0 and mutation == "inv_n_of_three":
            x16_got = r16(lrelu32(mrf_mean(ys, 3)))
        w, b = W[f"ups.{i}"]
        r, up = rec(f"ups.{i}", "convt", r16(lrelu32(src)), w, b, u, None, [(0, L)], [(0, L * u)],
                    prov.up(i) if prov else None, x16_got)
        yield r
        L *= u
        wins = windows(B, L, C)
        cur, last_y32 = [up] * nk, []
        for m in range(nd):
            xts, nxt = [], []
            got_xt = prov.xt(i, m) if prov else [None] * nk
            for j in range(nk):                   # conv1 of every branch: ONE grouped launch
                w, b = W[f"resblocks.{i * nk + j}.convs1.{m}"]
                r, xt = rec(f"stage {i} step {2 * m} branch {j}", "conv", r16(lrelu32(cur[j])), w, b,
                            cfg.resblock_dilation_sizes[j][m], None, wins, wins, got_xt[j],
                            t16(lrelu32(cur[j])) if mutation == "trunc_act" else None)
                xts.append(xt)
                yield r
            got_y = prov.y(i, m) if prov else [None] * nk
            for j in range(nk):                   # conv2 + residual on THAT xt (C <= 128: the fused pair, xt on chip)
                w, b = W[f"resblocks.{i * nk + j}.convs2.{m}"]
                x16 = r16(lrelu32(xts[j]))
                r, y = rec(f"stage {i} step {2 * m + 1} branch {j}", "conv", x16, w, b, 1, cur[j], wins, wins, got_y[j])
                if mutation == "unrounded_y" and m == nd - 1:
                    last_y32.append(_apply("conv", x16, r16(w), b, 1, cur[j], [(0, L)], torch.float32))
                nxt.append(y)
                yield r
            cur = nxt
        ys = cur
    if stages is not None:
        return
    # LeakyReLU (fp32, unrounded) + conv_post (fp32 weights) + tanh on the fp32 mean of the last stage's branch tensors
    w, b = W["conv_post"]
    k = w.shape[-1]
    x = lrelu32(mrf_mean(ys))
    pre_tanh = F.conv1d(x.double(), w.double(), b.double(), padding=(k - 1) // 2)[:, 0, :]
    if prov:
        got = prov.wav()
    else:
        xg = lrelu32(mrf_mean(last_y32)) if mutation == "unrounded_y" else x
        got = torch.tanh(F.conv1d(xg, w, b, padding=(k - 1) // 2))[:, 0, :]
    yield {"label": "conv_post + tanh", "kind": "wav", "got": got, "want64": torch.tanh(pre_tanh), "pre_tanh": pre_tanh}


# ---- the launch plan: which kernel runs which launch -----------------------------------------------------------------------
_CONVT = re.compile(r"convt_mfma_bf16_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>")


def plan_forms(cfg, B, T):
    """The forms of one bf16 forward, from the host-only launch plan (``iris_hifigan_describe_plan``): a dict with
    ``ups`` [per stage: ("gemm", (MT, NT, WR, WC, CIC), NIN) or ("polyphase", n_inputs)], ``mrf`` [per stage: the kernel
    names of its launches, in order], ``post`` ("rows_f32" | "rows_bf16" | "tanh_bf16") and ``grouped`` [per stage: the
    branches that share one conv_mfma_bf16_kernel launch, from its grid].  The launch order is bf16_forward's: conv_pre,
    then per stage the upsampler and the MRF launches, then conv_post."""
    from iris import _native
    plan = _native.describe_plan(cfg, B, T, _native.DTYPE_BF16, CU)
    assert plan["passes"] == 1
    L = plan["launches"]
    assert L[0]["kernel"].startswith("conv_mfma_bf16_kernel<"), L[0]
    nk = cfg.num_kernels
    out = {"ups": [], "mrf": [], "grouped": [], "pre": L[0]["kernel"]}
    n = 1
    for i in range(cfg.num_upsamples):
        m = _CONVT.match(L[n]["kernel"])
        if m:
            g = tuple(int(v) for v in m.groups())
            out["ups"].append(("gemm", g[:5], g[5]))
        else:
            assert L[n]["kernel"].startswith("conv_mfma_bf16_kernel<"), L[n]
            out["ups"].append(("polyphase", 1 if i == 0 else nk))
        n += 1
        names, grouped = [], 0
        while _steps(names) < 2 * len(cfg.resblock_dilation_sizes[0]):
            names.append(L[n]["kernel"])
            if names[-1].startswith("conv_mfma_bf16_kernel<"):
                gy = L[n]["grid"][1]
                grouped = max(grouped, nk if gy in (nk, B * nk) else 1)     # z_in_y: the branch is (part of) blockIdx.y
            else:
                assert names[-1] in ("mrf_pair_bf16_kernel", "mrf_pair_bf16_sum_kernel"), names
            n += 1
        out["mrf"].append(names)
        out["grouped"].append(grouped)
    assert n == len(L) - 1, (n, [r["kernel"] for r in L])
    post = L[-1]["kernel"]
    if post == "conv_post_rows_kernel":           # one fp32 input behind the summing pair, else the bf16 branch tensors
        out["post"] = "rows_f32" if out["mrf"][-1][-1] == "mrf_pair_bf16_sum_kernel" else "rows_bf16"
    else:
        assert post == "conv_post_tanh_bf16_kernel", post
        out["post"] = "tanh_bf16"
    return out


def _steps(names):
    """MRF steps a list of launches covers: a pair kernel is two steps, a grouped conv launch one."""
    return sum(2 if n.startswith("mrf_pair_bf16") else 1 for n in names)
