"""Shapes and inputs of the split-product (dtype "f32s") tests.  TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

The kernel (csrc/conv_mfma_f32s.h) has three tile configs by channel count and, for each, two tile heights and two
forms (one branch per block / all branches summed in a block, ``ZS``).  Which instance a launch gets depends on the
grid: the tile is halved (``MT = 1``) while the full-height grid has fewer than 2.5 blocks per CU.  ``tile()`` and
``expected_mt()`` mirror ``s3::pick_tile`` and that rule; the CPU tests (tests/test_oracle_f32s.py) check the mirror
against ``iris_hifigan_describe_plan`` for whole forwards, and everything below derives its lengths from it, so that a
change of the rule fails on the host and the shapes are re-drawn.

Shared by tests/test_oracle_f32s.py (CPU: what the references alone can tell apart) and tests/test_gpu_f32s.py (the
kernel against the restatement, on exactly these cases).
"""
import re

import numpy as np

CU = 256                         # MI355X; describe_plan's default as well
V1_KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]            # every (kernel size, dilation) of the V1 ResBlocks

_KERNEL = re.compile(r"conv_mfma_f32s_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false)>")


def tile(C):
    """s3::pick_tile: (WT, WC, NT, CIC); rows of a tile = WT * MT * 32, output channels of a block = WC * NT * 32."""
    if C <= 32:
        return 4, 1, 1, 32
    if C <= 64:
        return 2, 2, 1, 64
    return 2, 2, 2, 64


def t_blk(C, MT):
    return tile(C)[0] * MT * 32


def expected_mt(C, n_rows, B, nz, zs=False, cu=CU):
    """Tile height s3::launch picks: 2 from 2.5 full-height blocks per CU on, else 1.  n_rows: output rows per problem
    (a ConvTranspose1d: L_in + taps - 1 per phase, nz = u phases)."""
    WT, WC, NT, _ = tile(C)
    blocks2 = -(-n_rows // (WT * 2 * 32)) * (1 if zs else nz) * (C // (WC * NT * 32)) * B
    return 2 if 2 * blocks2 >= 5 * cu else 1


def instance(C, MT, zs):
    WT, WC, NT, CIC = tile(C)
    return (WT, WC, MT, NT, CIC, zs)


def plan_instances(cfg, B, T):
    """[(stage, step, (WT, WC, MT, NT, CIC, ZS))] of one f32s forward, from the host-only launch plan: every MRF step of
    every stage is one launch of this kernel, in order."""
    from iris import _native
    plan = _native.describe_plan(cfg, B, T, _native.DTYPE_F32_SPLIT, CU)
    assert plan["passes"] == 1
    found = [m for m in (_KERNEL.match(rec["kernel"]) for rec in plan["launches"]) if m]
    steps = 2 * len(cfg.resblock_dilation_sizes[0])
    assert len(found) == cfg.num_upsamples * steps, [rec["kernel"] for rec in plan["launches"]]
    out = []
    for n, m in enumerate(found):
        WT, WC, MT, NT, CIC, _ = (int(g) for g in m.groups()[:6])
        out.append((n // steps, n % steps, (WT, WC, MT, NT, CIC, m.group(7) == "true")))
    return out


# ---- single layers (iris_hifigan_op_conv1d_f32s: one problem, nz = 1) ----------------------------------------------------
def _mt2_shape(C):
    """(B, n): the smallest power-of-two batch and tile count n with B * n tiles of full height reaching MT = 2."""
    n_co = C // (tile(C)[1] * tile(C)[2] * 32)
    B = 8 // n_co
    n = -(-5 * CU // (2 * B * n_co))
    return B, n


def conv_cases():
    """(id, B, L, C, k, d, use_res, MT, kind): around the tile edges n * T_BLK - 1, n * T_BLK, n * T_BLK + 1 of both tile
    heights of every tile config, (k, d) and the residual rotated through V1's nine pairs so that each pair meets both
    heights; L = 1 and L shorter than the halo; and inputs that are not iid N(0, 1) (``kind``)."""
    cases, i = [], 0
    for C in (32, 64, 128, 256):
        for MT in (1, 2):
            B, n = (1, 2) if MT == 1 else _mt2_shape(C)
            for dl in (-1, 0, 1):
                L = n * t_blk(C, MT) + dl
                k, d = V1_KD[(i * 4 + MT) % 9]
                cases.append((f"C{C}-MT{MT}-L{L}", B, L, C, k, d, bool((i + MT) & 1), MT, "normal"))
                i += 1
    for C, L, (k, d) in ((32, 1, (11, 5)), (64, 1, (3, 1)), (256, 1, (7, 3)), (32, 5, (11, 5)), (128, 9, (7, 5)), (256, 24, (11, 5))):
        cases.append((f"C{C}-short-L{L}", 2, L, C, k, d, True, 1, "normal"))
    for kind in ("scales", "negative_item", "zeros", "bf16_x", "bf16_xw"):
        cases.append((f"C64-{kind}", 2, 300, 64, 7, 3, True, 1, kind))
        cases.append((f"C256-{kind}", 2, 200, 256, 11, 5, kind != "scales", 1, kind))
    for c in cases:
        assert expected_mt(c[3], c[2], c[1], 1) == c[7], c
    return cases


def _bf16_valued(a):
    import torch
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def conv_inputs(case):
    """x [B, C, L] (before LeakyReLU), w [C, C, k], bias [C], residual [B, C, L] or None -- fp32 numpy, seeded by the case."""
    cid, B, L, C, k, d, use_res, _, kind = case
    rng = np.random.default_rng(sum(cid.encode()) * 7919 + B * 1000 + L + C + k + d)
    x = rng.standard_normal((B, C, L)).astype(np.float32)
    w = (rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    res = rng.standard_normal((B, C, L)).astype(np.float32) if use_res else None
    if kind == "scales":                       # per-channel scales over 1e-3 ... 1e3 (the split is relative: nothing may assume |x| ~ 1)
        x *= (10.0 ** rng.uniform(-3, 3, C)).astype(np.float32)[None, :, None]
    elif kind == "negative_item":              # the slope multiply precedes the split
        x[B - 1] = -np.abs(x[B - 1]) - np.float32(0.01)
    elif kind == "zeros":                      # exact zeros: whole rows, whole channels, and a scatter
        x[:, :, L // 3: L // 2] = 0
        x[:, ::5, :] = 0
        x[rng.random(x.shape) < 0.3] = 0
    elif kind == "bf16_x":                     # LeakyReLU(x) has bf16 values (x >= 0): x_mid = 0
        x = _bf16_valued(np.abs(x))
    elif kind == "bf16_xw":                    # both operands bf16-valued: the scheme is the exact conv
        x = _bf16_valued(np.abs(x))
        w = _bf16_valued(w)
    return x, w, b, res


# ---- ConvTranspose1d (iris_hifigan_op_conv_transpose1d_f32s: u phase problems of L_in + taps - 1 rows) --------------------
V1_UPS = [(512, 256, 16, 8), (256, 128, 16, 8), (128, 64, 4, 2), (64, 32, 4, 2)]


def convt_cases():
    """(id, B, L_in, C_in, C_out, k, u, MT): the four V1 upsamplers, B > 1, at L_in = n * T_BLK - 1 (the n_idx = L_in + 1 row
    indices fill n tiles exactly), n * T_BLK (one row index spills into a further tile) and a ragged length, half-height
    tiles; and at L_in = n * T_BLK with enough tiles for the full height."""
    cases = []
    for Ci, Co, k, u in V1_UPS:
        T1, T2 = t_blk(Co, 1), t_blk(Co, 2)
        n_co = Co // (tile(Co)[1] * tile(Co)[2] * 32)
        for L in (2 * T1 - 1, 2 * T1, 2 * T1 + 37):
            cases.append((f"{Ci}to{Co}-MT1-L{L}", 2, L, Ci, Co, k, u, 1))
        B = 2 if u * n_co >= 16 else 4
        n = -(-5 * CU // (2 * B * u * n_co))
        cases.append((f"{Ci}to{Co}-MT2-L{n * T2}", B, n * T2, Ci, Co, k, u, 2))
    for c in cases:
        assert expected_mt(c[4], c[2] + c[5] // c[6] - 1, c[1], c[6]) == c[7], c
    return cases


def convt_inputs(case):
    cid, B, L, Ci, Co, k, u, _ = case
    rng = np.random.default_rng(sum(cid.encode()) * 104729 + L + Ci + k)
    x = rng.standard_normal((B, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Ci, Co, k)) / np.sqrt(Ci * k / u)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    return x, w, b


# ---- whole forwards ------------------------------------------------------------------------------------------------------
# forward_until, every step (tests C): (B, T, stages, first pair).  (1, 4): every launch at half height.  (1, 641): the
# C = 128 stage at full height with a ragged last tile (41,024 = 320.5 x 128 rows) but its summing step at half height,
# the C = 64 and C = 32 stages at full height in both forms.  (3, 1707): the C = 256 and C = 128 stages at full height in
# both forms, ragged (13,656 = 106.7 x 128; 109,248 = 853.5 x 128) -- 5,121 frames, so only the last conv pair of each.
UNTIL_SHAPES = [(1, 4, (0, 1, 2, 3), 0), (1, 641, (1, 2, 3), 0), (3, 1707, (0, 1), 2)]
# batch independence across the height switch (tests D): an item alone runs at half height where the batch runs at full
INDEPENDENCE_SHAPES = [(4, 160), (12, 40)]
# a subset of tests/test_planner_sweep.py's SWEEP_SHAPES between which the f32s plan changes, and the long / wide shapes
SWEEP_SHAPES = [(1, 130), (1, 282), (1, 501), (1, 850), (2, 450), (3, 333), (5, 200), (5, 800)]
LONG_WIDE_SHAPES = [(1, 3000), (300, 3), (7, 129)]
GRAPH_SHAPES = [(1, 64), (3, 700)]
NON_V1_SHAPES = [(2, 37), (4, 700)]          # non_v1_config(): every launch at half height / the C = 64 and C = 32 stages at full


def non_v1_config():
    """ResBlock channels 128 / 64 / 32 and TWO MRF kernels: nz = 2, so the branch interleave of blockIdx.x and the divisor
    of the mean are not V1's constants."""
    from iris._weights import GeneratorConfig
    return GeneratorConfig(in_channels=40, upsample_rates=(4, 4, 2), upsample_kernel_sizes=(8, 8, 4),
                           upsample_initial_channel=256, resblock_kernel_sizes=(5, 9),
                           resblock_dilation_sizes=((1, 2, 4), (1, 3, 5)))
