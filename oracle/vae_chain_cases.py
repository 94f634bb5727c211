"""The VAE decoder and posterior encoder (csrc/vae_decoder.h; ``vae_forward`` in csrc/iris_vae_decoder.hip, ``enc_forward`` in
csrc/iris_vae_encoder.hip), launch by launch, each on its OWN input tensor.  TEST INFRASTRUCTURE ONLY, like the rest of
``oracle/``.

``vae_gemm_kernel`` stages all of C_in at once and ``mma_loop`` (csrc/gemm_tile_f32.h) walks taps ascending, groups of 8
channels ascending and the channels 0, 4, 1, 5, 2, 6, 3, 7 of a group: ``chain_oracle.chain_conv1d`` with ONE chunk,
``chunk = (C_in + 7) & ~7``.  ``w`` is the Keras kernel transposed to ``[C_out, C_in, k]`` as ``blob()`` does; the fused
conditioning / FiLM / heads matrices are assembled here as ``iris_vae_*_create`` assembles them.

    stride 1   ``chain_conv1d`` as it is (dilation ``1 << (i % 4)`` in the WaveNet blocks);
    stride 2   y[i] = sum_kap x[2 i - 1 + kap] W[kap] (pad 1 | 2, even length) is the k = 5 'same' conv at the ODD rows 2 i + 1;
    up         the chain over ``np.repeat(x, 2, axis=time)``;
    FUSED      the chain gives ``pre`` exactly; h and y follow from it in float64.

``plan`` lists a forward's launches with the workspace buffer each writes; ``judged`` keeps those whose inputs AND output no
later launch overwrites.  ``emulate`` is the fp32 restatement of what a launch stores (``MUTATIONS``: wrong ones);
``judge`` holds a stored tensor to the launch's claim and raises, naming the launch, the instantiation, the channel counts,
k / dil / stride, the first differing element and the rows that differ.

Claims (eps = 2^-24, ``gelu64`` = the kernel's formula in float64 with its two fp32 constants):

* exact (no GELU): ``np.array_equal(got, chain)`` -- the channels-first transposition, the mean | logvar split and the exact
  zeros of the padded conditioning columns included.
* GELU (down, up):  |got - gelu64(pre)| <= bar_g(pre) = 0.5 |pre| (TOL_TANH + 8 eps) + 2 eps |gelu64(pre)|.
  The kernel stores fl(fl(0.5 x) fl(1 + t^)), t^ = tanhf(u^), u^ = fl(c0 fl(x + fl(c1 fl(fl(x x) x)))).  0.5 x is exact.
  u^ carries at most five roundings (fewer where the compiler contracts a multiply-add), each relative to a partial result no
  larger than |u| (all terms have x's sign): |u^ - u| <= 5 eps |u| to first order, and tanh moves by at most
  |u| (1 - tanh^2 u) per unit of relative change, < 0.45 for every u: 2.25 eps.  tanhf itself: TOL_TANH (the project's bar,
  ``f32_cases.TOL_TANH``).  fl(1 + t^) adds eps (1 + t^) <= 2 eps.  So |fl(1 + t^) - (1 + tanh u)| <= TOL_TANH + 4.25 eps; the
  bar allows 8 eps.  Times 0.5 |x|; the last product rounds once more, eps |result| -- 2 eps |gelu64| with room for the
  result not being gelu64 itself.
* FUSED: h64 = gamma gelu64(pre) + beta with gamma, beta the DEVICE's own film rows, y64 = res + b2 + sum w2 h64, and per element
  sum_ci |w2[co, ci]| (|gamma_ci| bar_g(pre_ci) + 2 eps (|gamma_ci g_ci| + |beta_ci|)) + (C + 2) eps (sum |w2 h64| + |b2| + |res|):
  the product and the sum of the FiLM round once each (or once, fused), the second chain has C fmaf roundings and the
  epilogue two additions.
* flow: ``flow_np`` restates ``vae_flow_kernel`` on the device's own z and film (x1 never changes: the couplings add and do
  not compound); |got - fp64| / max(1, max |fp64|) <= 4 e32, e32 the same distance of the fp32 run of ``flow_np`` on the same
  inputs, taken over all forwards of one test.
"""
import numpy as np

from oracle import chain_oracle as co
from oracle import f32_cases as fc

EPS = 2.0 ** -24
TOL_TANH = fc.TOL_TANH
C0, C1 = np.float32(0.7978845608028654), np.float32(0.044715)

# ---- cases -----------------------------------------------------------------------------------------------------------------
# Both halves share a configuration (``enc_n_mels``: the encoder's n_mels where it must differ).  "default" and "small" are
# tests/vae_posterior_cases.CONFIGS.  "blocksN": default widths with N decoder and N encoder blocks -- the judged last block
# runs dilation 1, 2, 4, 8 for N = 1 .. 4.  "wide": 8 waves, S = 0 (down_cond_proj judged).  "odd": C = 20 pads Cp to 24 in the
# staging and in the FUSED tile, n_mels = 6 takes the bounded scalar channels-first store, S = 3; the encoder needs
# n_mels % 4 == 0 and gets 8.  "bare": no block, no coupling -- decoder only.
_DEFAULT = dict(n_mels=80, cond_dim=256, model_channels=192, latent_dim=16, num_wavenet_blocks=8, decoder_blocks=4,
                wavenet_kernel_size=5, down_stages=2, flow_layers=4, flow_hidden=64)
CONFIGS = {
    "default": dict(_DEFAULT),
    "small": dict(n_mels=20, cond_dim=24, model_channels=48, latent_dim=4, num_wavenet_blocks=5, decoder_blocks=5,
                  wavenet_kernel_size=3, down_stages=1, flow_layers=3, flow_hidden=12),
    "blocks1": dict(_DEFAULT, num_wavenet_blocks=1, decoder_blocks=1),
    "blocks2": dict(_DEFAULT, num_wavenet_blocks=2, decoder_blocks=2),
    "blocks3": dict(_DEFAULT, num_wavenet_blocks=3, decoder_blocks=3),
    "blocks4": dict(_DEFAULT, num_wavenet_blocks=4, decoder_blocks=4),
    "wide": dict(_DEFAULT, model_channels=256, latent_dim=8, num_wavenet_blocks=2, decoder_blocks=2, wavenet_kernel_size=3,
                 down_stages=0),
    "odd": dict(n_mels=6, enc_n_mels=8, cond_dim=12, model_channels=20, latent_dim=4, num_wavenet_blocks=1, decoder_blocks=1,
                wavenet_kernel_size=7, down_stages=3, flow_layers=4, flow_hidden=12),
    "bare": dict(_DEFAULT, decoder_blocks=0, flow_layers=0),
}
DECODER_ONLY = ("bare",)
WEIGHT_SEEDS = (11, 12)
DENSE_B = (1, 3)
DENSE_TQ = (1, 2, 9, 16, 17, 32, 33, 65)      # latent rows; T = Tq * 2^S.  The flow tile is 16 rows, the GEMM tile 32
# (config, B, T, lengths): latent rows 66, 0, 1, 31, 32, 33 at S = 2; 35, 0, 1, 16 at S = 1
RAGGED = [("default", 6, 264, [264, 0, 4, 124, 128, 132]), ("small", 4, 70, [70, 0, 2, 32])]
DEC_KEYS = ("n_mels", "cond_dim", "model_channels", "latent_dim", "num_wavenet_blocks", "decoder_blocks", "wavenet_kernel_size",
            "down_stages", "flow_layers", "flow_hidden")
ENC_KEYS = ("n_mels", "cond_dim", "model_channels", "latent_dim", "num_wavenet_blocks", "wavenet_kernel_size", "down_stages")


def randomise(model, seed):
    """EVERY parameter random (the recipe of tests/vae_restatement.randomise): kernels glorot-sized, FiLM biases so that
    gamma is near 1, other biases +-0.1 -- zero-initialised net_post and latent_logvar_proj included."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, cur in model.weights.items():
        if key.endswith(".kernel"):
            lim = np.sqrt(6.0 / (int(np.prod(cur.shape[:-1])) + cur.shape[-1]))
            out[key] = rng.uniform(-lim, lim, cur.shape).astype(np.float32)
        else:
            b = rng.uniform(-0.1, 0.1, cur.shape)
            if ".film.proj." in key:
                b[: cur.shape[0] // 2] += 1.0
            out[key] = b.astype(np.float32)
    model.set_weights_dict(out)
    return out


def make_pair(name, seed):
    """(VAEPosteriorEncoder or None, TextConditionedVAE) of config ``name``, sharing one ``downsample.blocks.*`` set."""
    from iris.vae import TextConditionedVAE, VAEPosteriorEncoder
    cfg = CONFIGS[name]
    vae = TextConditionedVAE(**{k: cfg[k] for k in DEC_KEYS}, seed=1)
    randomise(vae, seed)
    if name in DECODER_ONLY:
        return None, vae
    kw = {k: cfg[k] for k in ENC_KEYS}
    kw["n_mels"] = cfg.get("enc_n_mels", cfg["n_mels"])
    enc = VAEPosteriorEncoder(**kw, seed=2)
    w = randomise(enc, seed + 100)
    w.update({k: v for k, v in vae.weights.items() if k.startswith("downsample.blocks.")})
    enc.set_weights_dict(w)
    return enc, vae


def make_inputs(name, B, T, seed=0):
    """cond [B, T, cond_dim], z [B, T / 2^S, latent], mel [B, enc n_mels, T]: standard normals."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(90000 + 1000 * B + T + seed)
    cond = rng.standard_normal((B, T, cfg["cond_dim"])).astype(np.float32)
    z = rng.standard_normal((B, T >> cfg["down_stages"], cfg["latent_dim"])).astype(np.float32)
    mel = rng.standard_normal((B, cfg.get("enc_n_mels", cfg["n_mels"]), T)).astype(np.float32)
    return cond, z, mel


def nan_past(a, lengths, axis, shift=0):
    """A copy of ``a`` that is NaN at and past each item's length (``lengths[b] >> shift`` rows along ``axis``)."""
    a = a.copy()
    for b, n in enumerate(lengths):
        idx = [slice(None)] * a.ndim
        idx[0], idx[axis] = b, slice(int(n) >> shift, None)
        a[tuple(idx)] = np.nan
    return a


# ---- GELU ------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.float64(C0) * (x + np.float64(C1) * (x * x * x))))


def gelu32(x):
    """``gelu_tanh`` of csrc/vae_decoder.h in fp32, every operation rounded, tanh the correctly rounded one."""
    x = np.asarray(x, dtype=np.float32)
    u = C0 * (x + C1 * (x * x * x))
    t = np.tanh(u.astype(np.float64)).astype(np.float32)
    return (np.float32(0.5) * x) * (np.float32(1.0) + t)


def bar_g(pre):
    p = np.abs(np.asarray(pre, dtype=np.float64))
    return 0.5 * p * (TOL_TANH + 8 * EPS) + 2 * EPS * np.abs(gelu64(pre))


# ---- weights as the device holds them --------------------------------------------------------------------------------------------
def gemm_w(weights, prefix):
    """(w [C_out, C_in, k], b): Conv1D [k, in, out] or Dense [in, out] transposed as ``blob()`` does."""
    k = weights[f"{prefix}.kernel"]
    k = k[None] if k.ndim == 2 else k
    return np.ascontiguousarray(k.transpose(2, 1, 0)), weights[f"{prefix}.bias"]


def cond_gemm_w(vae, mutation=None):
    """The decoder's conditioning GEMM as ``iris_vae_decoder_create`` assembles it: block i's film.proj at column 2C i,
    coupling j's cond_proj at ce_off + hp j (hp = half padded to 4), padding columns exactly 0.  ``cond_at_half``: the
    couplings packed ``half`` apart."""
    C, half = vae.model_channels, vae.latent_dim // 2
    hp = (half + 3) & ~3
    ce_off = vae.decoder_blocks * 2 * C
    cols = ce_off + vae.flow_layers * hp
    w, b = np.zeros((cols, C, 1), np.float32), np.zeros(cols, np.float32)
    for i in range(vae.decoder_blocks):
        w[i * 2 * C:(i + 1) * 2 * C], b[i * 2 * C:(i + 1) * 2 * C] = gemm_w(vae.weights, f"dec_block_{i}.film.proj")
    step = half if mutation == "cond_at_half" else hp
    for j in range(vae.flow_layers):
        o = ce_off + j * step
        w[o:o + half], b[o:o + half] = gemm_w(vae.weights, f"vpflow.ap_{j}.cond_proj")
    return w, b


def film_gemm_w(enc):
    C = enc.model_channels
    w, b = np.zeros((enc.num_wavenet_blocks * 2 * C, enc.cond_dim, 1), np.float32), np.zeros(enc.num_wavenet_blocks * 2 * C, np.float32)
    for i in range(enc.num_wavenet_blocks):
        w[i * 2 * C:(i + 1) * 2 * C], b[i * 2 * C:(i + 1) * 2 * C] = gemm_w(enc.weights, f"enc_block_{i}.film.proj")
    return w, b


def heads_w(enc):
    wm, bm = gemm_w(enc.weights, "latent_mean_proj")
    wl, bl = gemm_w(enc.weights, "latent_logvar_proj")
    return np.concatenate([wm, wl]), np.concatenate([bm, bl])


# ---- the launches of a forward ---------------------------------------------------------------------------------------------------
# A launch: name, kind ("plain", "stride2", "up", "fused", "flow"), form (what launch_gemm / launch_flow call the
# instantiation), x / y (logical tensors), slot (the workspace buffer y is written to; None: a caller's tensor), sh_in /
# sh_out (halvings of the rows of x / y below the frame rate), wb, and per kind: dil, film / index (fused), layouts.
def _launch(name, kind, x, y, slot, sh_in, sh_out, wb=None, form="", **kw):
    d = dict(name=name, kind=kind, form=form, x=x, y=y, slot=slot, sh_in=sh_in, sh_out=sh_out, wb=wb, dil=1, x_layout="cl",
             y_layout="cl", needs=(x,))
    d.update(kw)
    return d


def decoder_plan(vae, posterior=False, residual=True):
    """``vae_forward``.  Logical tensors: cond, z (inputs); dc, down{s}, film, d0, dec{i}, up{s}; mel, residual (outputs)."""
    w, S, N = vae.weights, vae.down_stages, vae.decoder_blocks
    pq = ("p", "q")
    plan = [_launch("down_cond_proj", "plain", "cond", "dc", "latcond" if S == 0 else "p", 0, 0, gemm_w(w, "down_cond_proj"))]
    cur = "dc"
    for s in range(S):
        plan.append(_launch(f"downsample.blocks.{s}", "stride2", cur, f"down{s}", "latcond" if s == S - 1 else pq[(s + 1) & 1],
                            s, s + 1, gemm_w(w, f"downsample.blocks.{s}")))
        cur = f"down{s}"
    lat = cur
    has_film = N > 0 or vae.flow_layers > 0
    if has_film:
        plan.append(_launch("conditioning GEMM", "plain", lat, "film", "film", S, S, cond_gemm_w(vae)))
    plan.append(_launch("flow", "flow", "z", "d0", "d0", S, S, None, "forward" if posterior else "", forward=posterior,
                        needs=("z", "film") if vae.flow_layers > 0 else ("z",)))
    cur = "d0"
    for i in range(N):
        plan.append(_launch(f"dec_block_{i}", "fused", cur, f"dec{i}", "db" if i & 1 else "da", S, S,
                            gemm_w(w, f"dec_block_{i}.conv"), "fused", dil=1 << (i % 4), index=i,
                            wb2=gemm_w(w, f"dec_block_{i}.res_proj"), needs=(cur, "film")))
        cur = f"dec{i}"
    for s in range(S):
        plan.append(_launch(f"upsample.refine.{s}", "up", cur, f"up{s}", pq[s & 1], S - s, S - s - 1, gemm_w(w, f"upsample.refine.{s}")))
        cur = f"up{s}"
    plan.append(_launch("out_proj", "plain", cur, "mel", None, 0, 0, gemm_w(w, "out_proj"), y_layout="cf", zero_tail=True))
    if residual:
        plan.append(_launch("residual_proj", "plain", cur, "residual", None, 0, 0, gemm_w(w, "residual_proj"), zero_tail=True))
    return plan


def encoder_plan(enc):
    """``enc_forward``.  Logical tensors: mel_in, cond (inputs); h0, film, blk{i}, down{s}; heads = mean | logvar (outputs)."""
    w, S, N = enc.weights, enc.down_stages, enc.num_wavenet_blocks
    plan = [_launch("in_proj", "plain", "mel_in", "h0", "h0", 0, 0, gemm_w(w, "in_proj"), "mel_in", x_layout="cf")]
    if N > 0:
        plan.append(_launch("FiLM GEMM", "plain", "cond", "film", "film", 0, 0, film_gemm_w(enc)))
    cur = "h0"
    for i in range(N):
        plan.append(_launch(f"enc_block_{i}", "fused", cur, f"blk{i}", "hb" if i & 1 else "ha", 0, 0,
                            gemm_w(w, f"enc_block_{i}.conv"), "fused", dil=1 << (i % 4), index=i,
                            wb2=gemm_w(w, f"enc_block_{i}.res_proj"), needs=(cur, "film")))
        cur = f"blk{i}"
    for s in range(S):
        plan.append(_launch(f"downsample.blocks.{s}", "stride2", cur, f"down{s}", f"d{s & 1}", s, s + 1,
                            gemm_w(w, f"downsample.blocks.{s}")))
        cur = f"down{s}"
    plan.append(_launch("latent heads", "plain", cur, "heads", None, S, S, heads_w(enc), "split_out", zero_tail=True))
    return plan


def survivors(plan):
    """{logical tensor: slot} of the workspace tensors no later launch of the plan overwrites."""
    last = {}
    for i, l in enumerate(plan):
        if l["slot"] is not None:
            last[l["slot"]] = i
    return {l["y"]: l["slot"] for i, l in enumerate(plan) if l["slot"] is not None and last[l["slot"]] == i}


def judged(plan):
    """The launches whose inputs and output all survive the forward (a caller's tensor always does)."""
    alive = survivors(plan)
    made = {l["y"] for l in plan}
    ok = lambda t: t not in made or t in alive or t in ("mel", "residual", "heads")
    return [l for l in plan if ok(l["y"]) and all(ok(t) for t in l["needs"])]


def kernel_form(l, ragged):
    """What ``launch_gemm`` / ``launch_flow`` name the instantiation, and the launch's sizes."""
    if l["kind"] == "flow":
        return f"vae_flow_kernel{'_ragged' if ragged else ''}{'<forward>' if l['forward'] else ''}"
    name = f"vae_gemm_kernel{'_ragged' if ragged else ''}{'<' + l['form'] + '>' if l['form'] else ''}"
    co_, ci, k = l["wb"][0].shape
    stride = 2 if l["kind"] == "stride2" else 1
    extra = {"stride2": " + GELU", "up": " over the x2 repeat + GELU", "fused": " + GELU + FiLM + 1x1 + residual"}.get(l["kind"], "")
    if l["y_layout"] == "cf":
        extra += ", channels-first store"
    return f"{name} {ci} -> {co_}, k {k} dil {l['dil']} stride {stride}{extra}"


# ---- restatements ------------------------------------------------------------------------------------------------------------
MUTATIONS = ("stride2_even", "repeat_shift", "no_dilation", "film_swapped", "gelu_before_bias", "res_from_h",
             "out_untransposed", "heads_swapped", "cond_at_half")


def _chain(x, w, b, dil, rows=None, residual=None):
    """x [B, L, C_in] channels-last -> (acc + bias) (+ residual) [B, rows, C_out], one chunk."""
    L = x.shape[1]
    rows = [(0, L)] if rows is None else rows
    xc = np.asarray(x, dtype=np.float32).transpose(0, 2, 1)
    res = None if residual is None else np.asarray(residual, dtype=np.float32).transpose(0, 2, 1)
    out = co.chain_conv1d(xc, w, b, dil, (x.shape[2] + 7) & ~7, rows, residual=res)
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def preact(l, x, mutation=None, bias=True):
    """The chain pre-activation of a GEMM launch on x [B, L_in, C_in] (channels-last) -> [B, L_out, C_out]."""
    w, b = l["wb"]
    if not bias:
        b = np.zeros_like(b)
    if l["kind"] == "stride2":
        L = x.shape[1]
        assert L % 2 == 0 and w.shape[2] == 5, (L, w.shape)
        first = 0 if mutation == "stride2_even" else 1
        return _chain(x, w, b, 1, [(r, r + 1) for r in range(first, L, 2)])
    if l["kind"] == "up":
        if mutation == "repeat_shift":
            L = x.shape[1]
            x = x[:, np.minimum((np.arange(2 * L) + 1) >> 1, L - 1)]
        else:
            x = np.repeat(x, 2, axis=1)
        return _chain(x, w, b, 1)
    return _chain(x, w, b, 1 if mutation == "no_dilation" else l["dil"])


def film_rows(l, film, C):
    """(gamma, beta) [B, L, C] of the fused launch l from the conditioning / FiLM GEMM's output [B, L, cols]."""
    o = l["index"] * 2 * C
    return film[..., o:o + C], film[..., o + C:o + 2 * C]


def flow_np(vae, z, film, forward, dtype):
    """``vae_flow_kernel`` in numpy: z [B, Tq, latent], film [B, Tq, cols] (or None without couplings) -> d0 [B, Tq, C].
    x1 = z[..., :half] in every coupling; reverse runs the couplings last first with x2 - t, forward in order with x2 + t."""
    w = {k: np.asarray(v).astype(dtype) for k, v in vae.weights.items()}
    half, C = vae.latent_dim // 2, vae.model_channels
    hp = (half + 3) & ~3
    ce_off = vae.decoder_blocks * 2 * C
    z = np.asarray(z).astype(dtype)
    x1, x2 = z[..., :half], z[..., half:].copy()
    act = gelu32 if dtype == np.float32 else gelu64
    order = range(vae.flow_layers)
    for j in (order if forward else reversed(order)):
        p = f"vpflow.ap_{j}"
        ce = act(np.asarray(film[..., ce_off + j * hp: ce_off + j * hp + half]).astype(dtype))
        hin = np.pad(x1 + ce, ((0, 0), (1, 1), (0, 0)))
        Tq = z.shape[1]
        pre = np.zeros(z.shape[:2] + (vae.flow_hidden,), dtype) + w[f"{p}.net_pre.bias"]
        for kap in range(3):
            pre = pre + hin[:, kap:kap + Tq] @ w[f"{p}.net_pre.kernel"][kap]
        t = act(pre) @ w[f"{p}.net_post.kernel"][0] + w[f"{p}.net_post.bias"]
        gb = ce @ w[f"{p}.film.proj.kernel"] + w[f"{p}.film.proj.bias"]
        t = gb[..., :half] * t + gb[..., half:]
        x2 = x2 + t if forward else x2 - t
    out = np.concatenate([x1, x2], axis=-1) @ w["latent_dec_proj.kernel"] + w["latent_dec_proj.bias"]
    assert out.dtype == dtype
    return out


def emulate(l, model, t, mutation=None):
    """What launch l stores, restated in fp32 from the tensors ``t`` (logical name -> array, channels-last unless the
    launch's layout says otherwise).  ``mutation``: a WRONG restatement."""
    if l["kind"] == "flow":
        return flow_np(model, t["z"], t.get("film"), l["forward"], np.float32)
    x = t[l["x"]]
    if l["x_layout"] == "cf":
        x = x.transpose(0, 2, 1)
    if l["kind"] == "plain":
        if l["name"] == "conditioning GEMM" and mutation == "cond_at_half":
            l = dict(l, wb=cond_gemm_w(model, mutation))
        y = preact(l, x, mutation)
        if l["form"] == "split_out" and mutation == "heads_swapped":
            n = y.shape[2] // 2
            y = np.concatenate([y[..., n:], y[..., :n]], axis=-1)
        if l["y_layout"] == "cf":
            y = y.reshape(y.shape[0], y.shape[2], y.shape[1]) if mutation == "out_untransposed" else y.transpose(0, 2, 1)
        return np.ascontiguousarray(y)
    if mutation == "gelu_before_bias":
        g = (gelu32(preact(l, x, mutation, bias=False)) + l["wb"][1]).astype(np.float32)
    else:
        g = gelu32(preact(l, x, mutation))
    if l["kind"] != "fused":
        return g
    gamma, beta = film_rows(l, t["film"], x.shape[2])
    if mutation == "film_swapped":
        gamma, beta = beta, gamma
    h = (gamma * g + beta).astype(np.float32)
    w2, b2 = l["wb2"]
    return _chain(h, w2, b2, 1, residual=h if mutation == "res_from_h" else x)


# ---- claims ------------------------------------------------------------------------------------------------------------------
def _where(bad, what, got, want):
    idx = np.argwhere(bad)
    i = tuple(idx[0])
    return (f"{what}: {len(idx)} of {got.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}; "
            f"rows {sorted(set(idx[:, 1].tolist()))[:12]}")


def _finite(got, what, want):
    if not np.isfinite(got).all():
        raise AssertionError(_where(~np.isfinite(got), what + " is not finite", got, want))


def _ratio(err, bar, what, got, want, kind):
    """max err / bar; raises where err > bar."""
    if not (err <= bar).all():
        worst = float((err / np.maximum(bar, 1e-300)).max())
        raise AssertionError(_where(err > bar, f"{what}: {kind} err / bar up to {worst:.3g}", got, want))
    nz = bar > 0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


def judge(l, model, t, got, what):
    """``got`` [B, L_out, C_out] (channels-last, already cut to the rows judged) against launch l's claim on the inputs
    ``t``.  Returns (claim kind, worst err / bar or, for the flow, (err, e32))."""
    if l["kind"] == "flow":
        want = flow_np(model, t["z"], t.get("film"), l["forward"], np.float64)
        _finite(got, what, want)
        scale = max(1.0, float(np.abs(want).max()))
        e32 = float(np.abs(flow_np(model, t["z"], t.get("film"), l["forward"], np.float32) - want).max()) / scale
        return "flow", (float(np.abs(got - want).max()) / scale, e32)
    x = t[l["x"]]
    if l["x_layout"] == "cf":
        x = x.transpose(0, 2, 1)
    pre = preact(l, x)
    assert got.shape == pre.shape, (what, got.shape, pre.shape)
    _finite(got, what, pre)
    if l["kind"] == "plain":
        if not np.array_equal(got, pre):
            raise AssertionError(_where(got != pre, what + " differs from the chain", got, pre))
        return "exact", 0.0
    g = gelu64(pre)
    if l["kind"] != "fused":
        return "gelu", _ratio(np.abs(got - g), bar_g(pre), what, got, g, "GELU")
    C = x.shape[2]
    gamma, beta = (a.astype(np.float64) for a in film_rows(l, t["film"], C))
    w2, b2 = l["wb2"][0][:, :, 0].astype(np.float64), l["wb2"][1].astype(np.float64)
    res = x.astype(np.float64)
    h = gamma * g + beta
    want = res + b2 + h @ w2.T
    a2 = np.abs(w2).T
    bar = (np.abs(gamma) * bar_g(pre) + 2 * EPS * (np.abs(gamma * g) + np.abs(beta))) @ a2 + \
        (C + 2) * EPS * (np.abs(h) @ a2 + np.abs(b2) + np.abs(res))
    return "fused", _ratio(np.abs(got - want), bar, what, got, want, "FUSED")


def judge_tail(name, tail, what):
    """Rows of an output at and past an item's length: exactly 0 (and so not NaN)."""
    if tail.size and not (tail == 0).all():
        raise AssertionError(_where(~(tail == 0), f"{what}: {name} past the item's length is not 0", tail, np.zeros_like(tail)))


def rows_of(n_frames, sh):
    return int(n_frames) >> sh


def judge_forward(plan, model, tensors, T, lengths=None, only=None, launches=None):
    """Every judged launch of one forward on the tensors it left (``tensors``: logical name -> array, the caller's inputs
    and outputs and the surviving workspace tensors; channels-last except mel / mel_in [B, C, T]).  Ragged (``lengths``):
    item by item on the item's own rows, the chain being that of the item ALONE, and the output tails exactly 0.
    ``only``: names to keep; ``launches``: judge these instead of the survivors (a CPU-chained forward keeps every tensor).
    -> ([names judged], {claim kind: worst err / bar}, [(err, e32) of each flow judged], elements judged)."""
    names, worst, flows, elements = [], {}, [], 0
    B = next(iter(tensors.values())).shape[0]
    for l in (judged(plan) if launches is None else launches):
        if only is not None and l["name"] not in only:
            continue
        names.append(l["name"])
        items = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(n)) for b, n in enumerate(lengths)]
        for sl, n in items:
            r_in, r_out = rows_of(n, l["sh_in"]), rows_of(n, l["sh_out"])
            y = tensors[l["y"]][sl]
            y = y.transpose(0, 2, 1) if l["y_layout"] == "cf" else y
            what = (f"{l['name']} [{kernel_form(l, lengths is not None)}] B {B} T {T}"
                    f"{'' if lengths is None else f' item {sl.start} of {n} frames'}")
            if lengths is not None and l.get("zero_tail"):
                judge_tail(l["y"], y[:, r_out:], what)
            if r_out == 0:
                continue
            t = {}
            for key in l["needs"]:
                a = tensors[key][sl]
                if key == "mel_in":
                    t[key] = a[:, :, :r_in]
                else:
                    t[key] = a[:, :r_in] if key == l["x"] or key == "z" else a[:, :r_out]
            kind, r = judge(l, model, t, np.ascontiguousarray(y[:, :r_out]), what)
            if kind == "flow":
                flows.append(r + (what,))
            else:
                worst[kind] = max(worst.get(kind, 0.0), r)
            elements += y[:, :r_out].size
    return names, worst, flows, elements


def chain_forward(plan, model, inputs, mutation=None):
    """The whole forward with the launches chained on the CPU (``emulate``): every logical tensor, inputs included."""
    t = dict(inputs)
    for l in plan:
        t[l["y"]] = emulate(l, model, t, mutation)
    return t


# ---- a device forward's tensors ----------------------------------------------------------------------------------------------
def logical_shapes(plan, B, T, model):
    """{logical workspace tensor: (rows per item, channels)}"""
    return {l["y"]: (T >> l["sh_out"], model.model_channels if l["kind"] == "flow" else l["wb"][0].shape[0])
            for l in plan if l["slot"] is not None}


def from_buffers(plan, model, bufs, B, T):
    """The surviving logical tensors [B, rows, C] cut from ``_read_buffers``' flat buffers."""
    shapes = logical_shapes(plan, B, T, model)
    out = {}
    for name, slot in survivors(plan).items():
        rows, C = shapes[name]
        out[name] = np.asarray(bufs[slot][:B * rows * C]).reshape(B, rows, C)
    return out


def expected_decoder(vae):
    """The decoder launches whose input and output both survive, READ OFF ``vae_forward`` (not computed from the plan):
    d0 -> da -> db -> da ...; up stage s writes p, q, p ...; down_cond_proj and the decoder's own down stages go through p
    and q, which the up stages overwrite."""
    N, S = vae.decoder_blocks, vae.down_stages
    names = []
    if S == 0:
        names.append("down_cond_proj")
    if N > 0 or vae.flow_layers > 0:
        names.append("conditioning GEMM")
    names.append("flow")
    if 1 <= N <= 2:
        names.append("dec_block_0")
    if N >= 2:
        names.append(f"dec_block_{N - 1}")
    if S <= 2:
        names += [f"upsample.refine.{s}" for s in range(S)]
    else:
        names.append(f"upsample.refine.{S - 1}")     # S = 3: stage 2 overwrites stage 0's output, stage 1's input
    return names + ["out_proj", "residual_proj"]


def expected_encoder(enc):
    """As ``expected_decoder``, off ``enc_forward``: h0 -> ha -> hb -> ha ...; down stage s writes d0, d1, d0 ..."""
    N, S = enc.num_wavenet_blocks, enc.down_stages
    names = ["in_proj"]
    if N > 0:
        names.append("FiLM GEMM")
    if 1 <= N <= 2:
        names.append("enc_block_0")
    if N >= 2:
        names.append(f"enc_block_{N - 1}")
    if S <= 2:
        names += [f"downsample.blocks.{s}" for s in range(S)]
    else:
        names.append(f"downsample.blocks.{S - 1}")
    return names + ["latent heads"]
