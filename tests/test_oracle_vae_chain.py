"""The VAE's launch-by-launch restatement (oracle/vae_chain_cases.py) on the CPU: chained, it IS the VAE; its claims are not
vacuous; the launches it expects to judge are those its plan finds.  No GPU.

``e32 = max |fp32 restatement - fp64 restatement| / max(1, max |fp64|)`` of tests/vae_restatement.py /
vae_posterior_restatement.py, and the chained launches' own distance to fp64, relative in the same way, the larger of the
outputs of each call; B = 2, 9 latent rows, weight seed 11, measured here:
    config    generate (mel, residual)   encode (mean, logvar)    decode_posterior (recon, residual)
              e32        chain           e32        chain         e32        chain
    default   1.08e-06   1.80e-06        8.63e-07   1.51e-06      1.13e-06   2.22e-06
    small     4.60e-07   5.93e-07        3.41e-07   7.36e-07      1.12e-06   1.96e-06
    blocks1   7.83e-07   1.56e-06        5.91e-07   1.19e-06      9.95e-07   1.43e-06
    blocks2   8.50e-07   1.45e-06        8.29e-07   1.46e-06      9.15e-07   1.62e-06
    blocks3   9.73e-07   1.49e-06        8.43e-07   1.37e-06      1.12e-06   2.27e-06
    blocks4   1.08e-06   1.80e-06        6.51e-07   1.32e-06      1.39e-06   2.28e-06
    wide      9.51e-07   8.43e-07        6.03e-07   6.04e-07      8.56e-07   1.39e-06
    odd       2.70e-07   7.27e-07        2.86e-07   2.53e-07      5.85e-07   9.38e-07
    bare      5.93e-07   9.45e-07        -          -             -          -
The chain is held to ``4 * e32``, the repository's rule.  That agreement is what shows that the odd-row restatement of the
stride-2 conv and the repeat restatement of the up conv are the reference's operations.

The flow's e32 (``flow_np`` fp32 against fp64 on the film rows the chained conditioning GEMM gives; weight seed 11, B = 3,
the largest over the latent rows 1 .. 65 of tests/test_gpu_vae_chain.py), reverse / forward:
    default 1.99e-07 / 1.95e-07 (blocks1 .. blocks4 hold the same couplings: the same figures)   small 1.87e-07 / 2.13e-07
    wide 1.51e-07 / 1.66e-07   odd 1.49e-07 / 1.49e-07   bare 1.98e-07 / 1.98e-07 (latent_dec_proj alone)
The fp32 GELU restatement's largest err / bar_g: 0.079 on the cases' pre-activations, 0.074 on a grid over [-20, 20].
"""
import numpy as np
import pytest

import vae_posterior_cases
import vae_posterior_restatement as vpr
import vae_restatement as vr
from oracle import vae_chain_cases as vc

SEED = vc.WEIGHT_SEEDS[0]
_cache = {}


def _pair(name):
    if name not in _cache:
        _cache[name] = vc.make_pair(name, SEED)
    return _cache[name]


def _cfg(enc, vae):
    cfg = vae.get_config()
    if enc is not None:
        cfg["num_wavenet_blocks"] = enc.num_wavenet_blocks
    return cfg


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))


def test_the_two_existing_configurations_are_kept():
    for name in ("default", "small"):
        want = dict(vc._DEFAULT)
        want.update(vae_posterior_cases.CONFIGS[name])
        assert vc.CONFIGS[name] == want, name


def _chained(name, B, Tq):
    """Every tensor of the three chained forwards of one case: (generate, encode or None, decode_posterior or None)."""
    enc, vae = _pair(name)
    T = Tq << vae.down_stages
    cond, z, mel = vc.make_inputs(name, B, T)
    gen = vc.chain_forward(vc.decoder_plan(vae), vae, {"cond": cond, "z": z})
    if enc is None:
        return T, cond, z, mel, gen, None, None
    e = vc.chain_forward(vc.encoder_plan(enc), enc, {"mel_in": mel, "cond": cond})
    L = enc.latent_dim
    post = vc.chain_forward(vc.decoder_plan(vae, posterior=True), vae, {"cond": cond, "z": e["heads"][..., :L]})
    return T, cond, z, mel, gen, e, post


@pytest.mark.parametrize("name", list(vc.CONFIGS))
def test_chained_launches_are_the_vae(name):
    enc, vae = _pair(name)
    B, Tq = 2, 9
    T, cond, z, mel, gen, e, post = _chained(name, B, Tq)
    cfg = _cfg(enc, vae)
    want = vr.generate_np(vae.weights, cfg, cond, z)
    w32 = vr.generate_np(vae.weights, cfg, cond, z, dtype=np.float32)
    e32 = max(_rel(a, b) for a, b in zip(w32, want))
    err = max(_rel(gen["mel"], want[0]), _rel(gen["residual"], want[1]))
    line = f"vae chain {name}: generate e32 {e32:.2e} chain {err:.2e}"
    assert 0 < e32 < 1e-5 and err <= 4 * e32, line
    if enc is not None:
        L = enc.latent_dim
        recon, (mean, logvar), residual = vpr.reconstruct_np(enc.weights, vae.weights, cfg, mel, cond)
        r32, (m32, l32), s32 = vpr.reconstruct_np(enc.weights, vae.weights, cfg, mel, cond, dtype=np.float32)
        e32e = max(_rel(m32, mean), _rel(l32, logvar))
        erre = max(_rel(e["heads"][..., :L], mean), _rel(e["heads"][..., L:], logvar))
        e32p = max(_rel(r32, recon), _rel(s32, residual))
        errp = max(_rel(post["mel"], recon), _rel(post["residual"], residual))
        line += f"; encode e32 {e32e:.2e} chain {erre:.2e}; decode_posterior e32 {e32p:.2e} chain {errp:.2e}"
        assert 0 < e32e < 1e-5 and erre <= 4 * e32e, line
        assert 0 < e32p < 1e-5 and errp <= 4 * e32p, line
    print(line)


def test_fp32_gelu_stays_inside_bar_g():
    worst = 0.0
    for name in vc.CONFIGS:
        enc, vae = _pair(name)
        _, _, _, _, gen, e, _ = _chained(name, 2, 9)
        for plan, model, t in ((vc.decoder_plan(vae), vae, gen),) + (((vc.encoder_plan(enc), enc, e),) if enc is not None else ()):
            for l in plan:
                if l["kind"] in ("stride2", "up", "fused"):
                    pre = vc.preact(l, t[l["x"]])
                    r = float((np.abs(vc.gelu32(pre) - vc.gelu64(pre)) / vc.bar_g(pre)).max())
                    assert r < 1, (name, l["name"], r)
                    worst = max(worst, r)
    grid = np.linspace(-20, 20, 400001).astype(np.float32)
    grid = grid[grid != 0]
    rg = float((np.abs(vc.gelu32(grid) - vc.gelu64(grid)) / vc.bar_g(grid)).max())
    print(f"fp32 gelu: largest err / bar_g {worst:.3f} on the cases' pre-activations, {rg:.3f} on the grid")
    assert 0 < worst < 1 and 0 < rg < 1


def _fails(plan, model, tensors, T, l, got):
    try:
        vc.judge_forward(plan, model, dict(tensors, **{l["y"]: got}), T, launches=[l])
    except AssertionError:
        return True
    return False


# mutation -> the launches it changes
_TOUCHES = {
    "stride2_even": lambda l: l["kind"] == "stride2",
    "repeat_shift": lambda l: l["kind"] == "up",
    "no_dilation": lambda l: l["kind"] == "fused" and l["dil"] > 1,
    "film_swapped": lambda l: l["kind"] == "fused",
    "gelu_before_bias": lambda l: l["kind"] in ("stride2", "up", "fused"),
    "res_from_h": lambda l: l["kind"] == "fused",
    "out_untransposed": lambda l: l["name"] == "out_proj",
    "heads_swapped": lambda l: l["name"] == "latent heads",
    "cond_at_half": lambda l: l["name"] == "conditioning GEMM",
}


def test_claims_hold_unmutated_and_every_wrong_restatement_fails_its_claim():
    assert set(_TOUCHES) == set(vc.MUTATIONS)
    failed = {m: [] for m in vc.MUTATIONS}
    for name in ("small", "odd", "blocks4"):
        enc, vae = _pair(name)
        T, _, _, _, gen, e, post = _chained(name, 2, 9)
        for plan, model, t in ((vc.decoder_plan(vae), vae, gen), (vc.encoder_plan(enc), enc, e),
                               (vc.decoder_plan(vae, posterior=True), vae, post)):
            names, worst, flows, _ = vc.judge_forward(plan, model, t, T, launches=plan)       # EVERY launch, not only survivors
            assert names == [l["name"] for l in plan]
            assert all(r < 1 for r in worst.values()), worst
            assert all(err <= 4 * e32 for err, e32, _ in flows), flows
            for l in plan:
                for m, touches in _TOUCHES.items():
                    if l["kind"] == "flow":
                        continue
                    bad = _fails(plan, model, t, T, l, vc.emulate(l, model, t, m))
                    if not touches(l):
                        assert not bad, (name, l["name"], m)
                    elif bad:
                        failed[m].append((name, l["name"]))
                    else:
                        # the one case a wrong restatement may pass: half == hp, where the couplings' columns do not move
                        assert m == "cond_at_half" and (model.latent_dim // 2) % 4 == 0, (name, l["name"], m)
    for m, cases in failed.items():
        print(f"wrong restatement {m}: fails its claim on {len(cases)} launches")
        assert cases, f"{m} fails no claim: the claim is vacuous"
    assert {c[0] for c in failed["cond_at_half"]} == {"small", "odd"}, failed["cond_at_half"]
    assert {n for _, n in failed["no_dilation"]} >= {"dec_block_1", "dec_block_2", "dec_block_3", "enc_block_1"}, failed["no_dilation"]


def test_expected_launches_are_those_the_plan_finds():
    """``expected_*`` is read off the forwards, ``judged`` computed from the slots: two statements of one thing.  Together
    the configurations reach every instantiation ``launch_gemm`` and ``launch_flow`` name, and the FUSED form at every
    dilation."""
    forms, dils = set(), set()
    for name in vc.CONFIGS:
        enc, vae = vc.make_pair(name, SEED) if name not in _cache else _cache[name]
        plans = [vc.decoder_plan(vae), vc.decoder_plan(vae, posterior=True)] + ([vc.encoder_plan(enc)] if enc is not None else [])
        wants = [vc.expected_decoder(vae)] * 2 + ([vc.expected_encoder(enc)] if enc is not None else [])
        for plan, want in zip(plans, wants):
            got = vc.judged(plan)
            assert [l["name"] for l in got] == want, (name, [l["name"] for l in got], want)
            for l in got:
                forms.add(vc.kernel_form(l, False).split(" ")[0])
                if l["kind"] == "fused":
                    dils.add(l["dil"])
                if l["kind"] in ("stride2", "up"):
                    forms.add(l["kind"])
                if l["y_layout"] == "cf":
                    forms.add("channels-first")
    assert forms == {"vae_gemm_kernel", "vae_gemm_kernel<fused>", "vae_gemm_kernel<mel_in>", "vae_gemm_kernel<split_out>",
                     "vae_flow_kernel", "vae_flow_kernel<forward>", "stride2", "up", "channels-first"}, forms
    assert dils == {1, 2, 4, 8}, dils
    for name, B, T, lengths in vc.RAGGED:
        S = vc.CONFIGS[name]["down_stages"]
        assert len(lengths) == B and all(0 <= n <= T and n % (1 << S) == 0 for n in lengths) and T % (1 << S) == 0


def test_layout_restatement_needs_no_device():
    """64-float rounding, struct order; the ABI totals and tap offsets are compared in tests/test_gpu_vae_chain.py (creating
    a handle uploads the weights)."""
    enc, vae = _pair("odd")
    layout, total = vae._workspace_layout(3, 8)       # C 20, S 3: 24 frames, 3 latent rows; film_cols 40 + 4 * 4
    assert layout == {"p": (0, 480), "q": (512, 480), "latcond": (1024, 60), "film": (1088, 168), "d0": (1280, 60),
                      "da": (1344, 60), "db": (1408, 60)} and total == 1472
    layout, total = enc._workspace_layout(3, 8)       # N 1: film 24 x 40
    assert layout == {"film": (0, 960), "h0": (960, 480), "ha": (1472, 480), "hb": (1984, 480), "d0": (2496, 240),
                      "d1": (2752, 120)} and total == 2880


def test_flow_e32_of_the_gpu_cases():
    """Re-measures the flow table of the docstring: the decoder chained up to the flow on the dense inputs of the GPU test."""
    out = []
    for name in vc.CONFIGS:
        _, vae = _pair(name)
        worst = [0.0, 0.0]
        for Tq in vc.DENSE_TQ:
            T = Tq << vae.down_stages
            cond, z, _ = vc.make_inputs(name, 3, T)
            plan = vc.decoder_plan(vae)
            upto = [l["kind"] for l in plan].index("flow")
            t = vc.chain_forward(plan[:upto], vae, {"cond": cond, "z": z})
            for fwd in (0, 1):
                want = vc.flow_np(vae, z, t.get("film"), bool(fwd), np.float64)
                worst[fwd] = max(worst[fwd], _rel(vc.flow_np(vae, z, t.get("film"), bool(fwd), np.float32), want))
        out.append(f"{name} {worst[0]:.2e} / {worst[1]:.2e}")
        assert 0 < worst[0] < 1e-6 and 0 < worst[1] < 1e-6, out[-1]
    print("flow e32 (reverse / forward): " + "   ".join(out))
