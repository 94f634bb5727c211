"""The text stage (csrc/text_encoder.h; ``enc_forward`` and ``dur_forward`` in csrc/iris_text_encoder.hip), launch by launch,
each on its OWN stored input.  TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

``plan`` lists a forward's launches with the workspace buffer each writes; ``judged`` keeps those whose inputs AND output no
later launch overwrites (read off the forwards in ``expected_encoder`` / ``expected_head``):
    encoder  N = 0: embed, final_norm.  N = 1: embed and the five launches of block 0, final_norm.  N = 2: the five launches of
             block 1 and final_norm (block 1's ffn2 stores into x0, the embedding's buffer, and qkv / attn / x1 / ffn hold
             block 1's tensors: nothing of block 0 but its output t0 is left).  N >= 3: the last block reads x0 and its own
             ffn2 stores into x0, so its qkv GEMM (input gone) and its out + LN launch (residual gone) are NOT judged; its
             attention, ffn1, ffn2 + LN and final_norm are.
    head     every conv + LN layer (num_layers <= 3: d0, d2, d1), the duration launch and the scan.
A ragged forward is judged item by item on the item's own prefix -- the chain is that of the item ALONE -- and every row past
a length must be exactly 0.

Claims (u = 2^-24; ``w`` as ``blob()`` / ``*_create`` hold it: ``[C_out, C_in, k]``, query | key | value one ``[3E, E]`` matrix):

* embed: ``tok[id] + pos[p]`` in fp32, exactly.
* GEMM without LayerNorm (qkv; ffn1 with ReLU): ``np.array_equal`` with ``chain_oracle.chain_conv1d``,
  ``chunk = min((C_in + 7) & ~7, 256)`` -- the accumulator carries across the slices --, bias last, then ``max(., 0)``.
* GEMM with LayerNorm (out + res, ffn2 + res, the head's conv + ReLU): the pre-norm row ``s = res + act(chain + bias)`` is known
  EXACTLY in fp32; the claim is ``|got - LN64(s)| <= ln_bar`` with the device's gamma, beta and ``eps = 1e-6f``.
  ``txt_layernorm_kernel``: the same claim on its stored input.
  Derivation of ``ln_bar`` (n = C, S1 = sum |s_i|, mu, d_i = s_i - mu, V = sum d_i^2 / n, r = 1 / sqrt(V + eps),
  y_i = d_i r gamma_i + beta_i, all first order in u):
    1. the row sum passes through at most D additions on its deepest path, each rounding relative to a partial sum no larger
       than S1: |tot^ - tot| <= D u S1.  GEMM kernel: 16 (sequential register sum) + 1 (the two half-wave partials) + nw (the LDS
       loop over the waves), nw = ceil(C / 32).  txt_layernorm_kernel: 2 (pairs within a quad) + ceil(C / 256) (the strided lane
       loop) + 6 (the xor butterfly).
    2. a true division (one rounding, relative to |mu| <= S1 / n): |mean^ - mu| <= (D + 1) u S1 / n =: dm.
    3. d^_i = fl(s_i - mean^): |d^_i - d_i| <= dm + u |d_i|.
    4. sum d^_i^2: the common shift dm enters only through 2 dm sum d_i = 0, second order; the roundings of step 3 move it by
       at most 2 u sum d_i^2; the fmaf chain and the same reduction round D2 = D times (GEMM kernel: 16 fmaf) relative to a sum
       of non-negative terms; the division by n and the addition of eps round once each: V + eps is off by at most
       (D + 4) u relative.  sqrtf halves that and, like the division 1 / ., is allowed 2 u (one ulp):
       |r^ / r - 1| <= rho := ((D + 4) / 2 + 4) u.
    5. fl(d^_i r^) rounds once (u), the final fmaf once, relative to |y_i|:
       ln_bar_i = |gamma_i| r (dm + |d_i| (rho + 2 u)) + u |y_i|.
  It holds no measured constant.  ``ln32_gemm`` / ``ln32_rows`` restate the two kernels' orders in fp32 (the fmaf of the
  squared deviations through float64: a double rounding is possible, so they are held to the bar, not to the bits).
* attention: per head, float64 softmax attention on the device's own qkv buffer, ``scale`` (the fp32 value) applied to the whole
  of q, only the item's own keys: |got - want| <= 4 e32 max(1, max |want|).  e32 is the same distance of ``attn32``, the fp32
  restatement in the kernel's order on the same qkv (32-key tiles, running maximum and sum, rescale by exp(m - mn), the
  16-register sum of a tile's weights and its partner, division at the end; the products themselves by fp32 matmul), the
  largest over all forwards of one test.  The factor 4 is the project's margin for another summation order, expf and the
  division.
* duration: ``u = x . w + b`` is restated EXACTLY (``dot32``: the per-lane fmaf chains over the quads lane, lane + 64, ..., the xor
  butterfly, one addition; ``fmaf32`` is a correctly rounded fp32 fma through float64 rounded to odd).  pred against
  ``softplus64(u)``: bar_p = 4 u t / (1 + t) + 4 u log1p(t) + u softplus64 + 2^-126, t = exp(-|u|): expf and log1pf are
  allowed two ulp each (twice the one ulp HIP documents for them; t's relative error reaches log1p through t / (1 + t)), the
  final addition rounds once, and 2^-126 covers a result below the normal range.
  frames: with raw = exp(softplus64) - 1 and margin = exp(softplus64) (bar_p + 5 u) (expf two ulp, the subtraction one
  rounding), a position is DECIDED where ``clip(rint(.), 1, max)`` is the same at raw - margin and raw + margin (the rule of
  tests/encoder_cases.decided -- further than the margin from every half-integer and clip edge -- stated on the interval, so
  that values beyond the upper clip, where float64 has no half-integers, are decided too); there ``frames`` must equal it.
* scan: exclusive prefix sum of ``max(frames, 0)`` over the item's own positions, the total from there on; exact.
* gather (``regulate_np``): exact.
"""
import numpy as np

from oracle import chain_oracle as co

U = 2.0 ** -24
LN_EPS = np.float32(1e-6)
SLICE, KEY_TILE = 256, 32

# ---- cases -----------------------------------------------------------------------------------------------------------------
# "default" and "small" are tests/encoder_cases.CONFIGS.  "blocksN": default widths with N blocks.  "odd": Dk = 88 (nd = 3 with
# a partial tile), 3E = 264 (9 C_out tiles: a second blockIdx.y with one active wave), ffn C_in = 260 (slices 256 + 8) and a last
# C_out tile of 4 channels, a head with C_in = 20 (Cp = 24, a one-wave LayerNorm), k = 7 and max_frames 50.  "dk128": nd = 4.
# "dk40": Dk = 40, a key_dim above 32 that is no multiple of 32.  "bare": no block, a head without conv layers.  "shifted":
# "bare" with 64 added to the position table, rows whose mean is ~150 standard deviations (mean first, deviations second).
# "slice": a head alone on random enc_out, C_in = 520 = 256 + 256 + 8 with three taps.  "sharp": the "blocks1" weights with
# the query and key kernels times SHARP_GAIN: the float64 scores have a standard deviation of about 8.
_ENC = dict(vocab_size=80)
CONFIGS = {
    "default": dict(encoder=dict(_ENC), head=dict(hidden_dim=256)),
    "small": dict(encoder=dict(vocab_size=11, embed_dim=48, num_heads=3, ffn_dim=80, num_blocks=3, max_length=150),
                  head=dict(hidden_dim=40, num_layers=3, kernel_size=5, in_dim=48)),
    "blocks1": dict(encoder=dict(_ENC, num_blocks=1), head=dict(hidden_dim=256)),
    "blocks2": dict(encoder=dict(_ENC, num_blocks=2), head=dict(hidden_dim=256)),
    "odd": dict(encoder=dict(vocab_size=13, embed_dim=88, num_heads=1, ffn_dim=260, num_blocks=1, max_length=120),
                head=dict(hidden_dim=20, kernel_size=7, num_layers=2, in_dim=88, max_frames_per_phoneme=50)),
    "dk128": dict(encoder=dict(vocab_size=17, embed_dim=128, num_heads=1, ffn_dim=64, num_blocks=2, max_length=120),
                  head=dict(hidden_dim=64, num_layers=1, in_dim=128)),
    "dk40": dict(encoder=dict(vocab_size=17, embed_dim=120, num_heads=3, ffn_dim=96, num_blocks=1, max_length=120),
                 head=dict(hidden_dim=40, num_layers=1, in_dim=120)),
    "bare": dict(encoder=dict(_ENC, num_blocks=0), head=dict(hidden_dim=256, num_layers=0)),
    "shifted": dict(encoder=dict(_ENC, num_blocks=0), head=dict(hidden_dim=256, num_layers=0)),
    "slice": dict(head=dict(hidden_dim=256, num_layers=1, kernel_size=3, in_dim=520)),
    "sharp": dict(encoder=dict(_ENC, num_blocks=1), head=dict(hidden_dim=256)),
}
SHARP_GAIN = 6.9
SHIFT = 64.0
WEIGHT_SEEDS = (21, 22)
DENSE_B = (1, 3)
DENSE_P = (1, 7, 31, 32, 33, 64, 65, 97)
# (B, P, lengths): whole tiles past an item's end (lengths 1, 17, 32, 33 under P = 70); an offset that is no multiple of the tile
RAGGED = [(5, 70, (70, 1, 32, 33, 17)), (3, 33, (1, 33, 20))]


def randomise(model, seed, duration_bias=1.0):
    """EVERY parameter random (the recipe of tests/encoder_restatement.randomise): kernels glorot-sized, embeddings +-0.5,
    gamma 1 +- 0.2, biases and beta +-0.1, ``duration_output.bias`` around ``duration_bias``."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, cur in model.weights.items():
        if key.endswith(".embeddings"):
            a = rng.uniform(-0.5, 0.5, cur.shape)
        elif key.endswith(".kernel"):
            if ".attention.output." in key:
                fan = int(np.prod(cur.shape[:2])) + cur.shape[2]
            elif ".attention." in key:
                fan = cur.shape[0] + int(np.prod(cur.shape[1:]))
            else:
                fan = int(np.prod(cur.shape[:-1])) + cur.shape[-1]
            lim = np.sqrt(6.0 / fan)
            a = rng.uniform(-lim, lim, cur.shape)
        elif key.endswith(".gamma"):
            a = 1.0 + rng.uniform(-0.2, 0.2, cur.shape)
        else:
            a = rng.uniform(-0.1, 0.1, cur.shape) + (duration_bias if key == "duration_output.bias" else 0.0)
        out[key] = a.astype(np.float32)
    model.set_weights_dict(out)
    return out


def make_models(name, seed):
    """(PhonemeEncoder or None, DurationPredictor) of config ``name``.  Token row ``vocab - 1`` is NaN: ``make_ids`` uses that id
    only past an item's length, so any read of a padded position shows."""
    from iris.encoder import DurationPredictor, PhonemeEncoder
    cfg = CONFIGS[name]
    enc = None
    if "encoder" in cfg:
        enc = PhonemeEncoder(**cfg["encoder"], seed=1)
        w = randomise(enc, seed)
        if name == "sharp":
            for i in range(enc.num_blocks):
                for part in ("query", "key"):
                    w[f"transformer_block_{i}.attention.{part}.kernel"] *= np.float32(SHARP_GAIN)
        if name == "shifted":
            w["positional_embedding.position_embedding.embeddings"] += np.float32(SHIFT)
        w["phoneme_embedding.embeddings"][-1] = np.nan
        enc.set_weights_dict(w)
    head = DurationPredictor(**cfg["head"], seed=2)
    randomise(head, seed + 100)
    return enc, head


def make_ids(name, B, P, lengths=None, seed=0):
    vocab = CONFIGS[name]["encoder"]["vocab_size"]
    ids = np.random.default_rng(7000 * B + P + seed).integers(0, vocab - 1, (B, P)).astype(np.int32)
    if lengths is not None:
        ids[np.arange(P)[None, :] >= np.asarray(lengths)[:, None]] = vocab - 1
    return ids


def make_enc_out(name, B, P, seed=0):
    """Random encoder output for a head that runs alone."""
    C = CONFIGS[name]["head"]["in_dim"]
    return np.random.default_rng(8000 * B + P + seed).standard_normal((B, P, C)).astype(np.float32)


def nan_past(a, lengths):
    """A copy of ``a [B, P, ...]`` that is NaN at and past each item's length."""
    a = a.copy()
    for b, n in enumerate(lengths):
        a[b, int(n):] = np.nan
    return a


# ---- the direct duration test ----
def sweep_head(max_frames):
    from iris.encoder import DurationPredictor
    """A head without conv layers whose logit is its input's channel 0: in_dim 4, w = (1, 0, 0, 0), b = 0."""
    head = DurationPredictor(hidden_dim=4, num_layers=0, in_dim=4, max_frames_per_phoneme=max_frames, seed=1)
    w = dict(head.weights)
    w["duration_output.kernel"] = np.array([1, 0, 0, 0], np.float32).reshape(1, 4, 1)
    w["duration_output.bias"] = np.zeros(1, np.float32)
    head.set_weights_dict(w)
    return head


def sweep_logits(max_frames):
    """The chosen logits of the direct duration test: a sweep over [-100, 100], log of values either side of the clip edges
    and of half-integers, the expf overflow and the deep negative end."""
    edges = [0.5, 1.5, 2.5, 3.5, 10.5, 49.5, 50.5, max_frames - 0.5, max_frames + 0.5, 1.0, float(max_frames)]
    near = [np.log(h * (1 + s * d)) for h in edges for d in (1e-3, 1e-5) for s in (-1, 1)]
    u = np.concatenate([np.linspace(-100, 100, 801), np.array(near), np.array([88.8, 100.0, -100.0, 88.72, 88.73, -87.4, -103.0, 0.0])])
    return u.astype(np.float32)


# ---- weights as the device holds them --------------------------------------------------------------------------------------------
def _dense(kernel_in_out, bias):
    return np.ascontiguousarray(kernel_in_out.T)[:, :, None], np.asarray(bias).ravel()


def block_w(w, p, E):
    """{launch: (w [C_out, C_in, 1], b)} of one Transformer block as ``PhonemeEncoder.blob`` lays it out."""
    qkv = np.concatenate([w[f"{p}.attention.{part}.kernel"].reshape(E, E).T for part in ("query", "key", "value")], axis=0)
    bqkv = np.concatenate([w[f"{p}.attention.{part}.bias"].ravel() for part in ("query", "key", "value")])
    return {"qkv": (np.ascontiguousarray(qkv)[:, :, None], bqkv),
            "out": _dense(w[f"{p}.attention.output.kernel"].reshape(E, E), w[f"{p}.attention.output.bias"]),
            "ffn1": _dense(w[f"{p}.ffn.0.kernel"], w[f"{p}.ffn.0.bias"]),
            "ffn2": _dense(w[f"{p}.ffn.2.kernel"], w[f"{p}.ffn.2.bias"])}


# ---- the launches of a forward ---------------------------------------------------------------------------------------------------
# A launch: name, kind ("embed", "gemm", "attn", "ln", "duration", "scan"), x / y (logical tensors), slot (the workspace buffer
# y is written to; None: a caller's tensor), needs (every tensor it reads), and per kind: wb, relu, res, norm = (gamma, beta).
CALLER = ("ids", "enc_out", "enc_in", "pred", "frames", "offsets", "totals")


def _launch(name, kind, x, y, slot, **kw):
    d = dict(name=name, kind=kind, x=x, y=y, slot=slot, wb=None, relu=False, res=None, norm=None, needs=(x,))
    d.update(kw)
    if d["res"] is not None:
        d["needs"] = (x, d["res"])
    return d


def encoder_plan(enc):
    """``enc_forward``.  Logical tensors: ids (input); emb, qkv{i}, attn{i}, mid{i}, h{i}, blk{i}; enc_out (output)."""
    w, E = enc.weights, enc.embed_dim
    norm = lambda p: (w[f"{p}.gamma"], w[f"{p}.beta"])
    plan = [_launch("embed", "embed", "ids", "emb", "x0", tok=w["phoneme_embedding.embeddings"],
                    pos=w["positional_embedding.position_embedding.embeddings"])]
    cur = "emb"
    for i in range(enc.num_blocks):
        p = f"transformer_block_{i}"
        bw = block_w(w, p, E)
        plan += [_launch(f"block{i}.qkv", "gemm", cur, f"qkv{i}", "qkv", wb=bw["qkv"]),
                 _launch(f"block{i}.attention", "attn", f"qkv{i}", f"attn{i}", "attn", H=enc.num_heads, bq=bw["qkv"][1][:E]),
                 _launch(f"block{i}.out+LN", "gemm", f"attn{i}", f"mid{i}", "x1", wb=bw["out"], res=cur, norm=norm(f"{p}.attention_norm")),
                 _launch(f"block{i}.ffn1", "gemm", f"mid{i}", f"h{i}", "ffn", wb=bw["ffn1"], relu=True),
                 _launch(f"block{i}.ffn2+LN", "gemm", f"h{i}", f"blk{i}", "t0" if i == 0 else "x0", wb=bw["ffn2"], res=f"mid{i}",
                         norm=norm(f"{p}.ffn_norm"))]
        cur = f"blk{i}"
    plan.append(_launch("final_norm", "ln", cur, "enc_out", None, norm=norm("encoder_output_norm")))
    return plan


def head_plan(head):
    """``dur_forward``.  Logical tensors: enc_in (input); dur{i}; pred | frames, offsets | totals (outputs)."""
    w = head.weights
    plan, cur = [], "enc_in"
    for i in range(head.num_layers):
        wb = (np.ascontiguousarray(w[f"duration_conv_{i}.kernel"].transpose(2, 1, 0)), w[f"duration_conv_{i}.bias"])
        plan.append(_launch(f"duration_conv_{i}+LN", "gemm", cur, f"dur{i}", "d0" if i == 0 else f"d{1 + (i & 1)}", wb=wb, relu=True,
                            norm=(w[f"duration_norm_{i}.gamma"], w[f"duration_norm_{i}.beta"])))
        cur = f"dur{i}"
    plan.append(_launch("duration", "duration", cur, "pred", None, wb=(w["duration_output.kernel"].ravel(), w["duration_output.bias"][0]),
                        max_frames=head.max_frames_per_phoneme))
    plan.append(_launch("scan", "scan", "frames", "offsets", None))
    return plan


def survivors(plan):
    """{logical tensor: slot} of the workspace tensors no later launch of the plan overwrites."""
    last = {l["slot"]: i for i, l in enumerate(plan) if l["slot"] is not None}
    return {l["y"]: l["slot"] for i, l in enumerate(plan) if l["slot"] is not None and last[l["slot"]] == i}


def judged(plan):
    """The launches whose inputs and output all survive the forward (a caller's tensor always does)."""
    alive = survivors(plan)
    ok = lambda t: t in CALLER or t in alive
    return [l for l in plan if ok(l["y"]) and all(ok(t) for t in l["needs"])]


def expected_encoder(enc):
    """The encoder launches whose inputs and output survive, READ OFF ``enc_forward`` (not computed from the plan)."""
    N = enc.num_blocks
    five = lambda i: [f"block{i}.{s}" for s in ("qkv", "attention", "out+LN", "ffn1", "ffn2+LN")]
    if N == 0:
        return ["embed", "final_norm"]
    if N == 1:
        return ["embed"] + five(0) + ["final_norm"]
    if N == 2:
        return five(1) + ["final_norm"]
    return [f"block{N - 1}.{s}" for s in ("attention", "ffn1", "ffn2+LN")] + ["final_norm"]


def expected_head(head):
    assert head.num_layers <= 3
    return [f"duration_conv_{i}+LN" for i in range(head.num_layers)] + ["duration", "scan"]


def kernel_form(l):
    """What the launch is called (``launch_kernel_named``) and its sizes."""
    if l["kind"] == "gemm":
        co_, ci, k = l["wb"][0].shape
        extra = (" + ReLU" if l["relu"] else "") + (" + residual" if l["res"] else "") + (" + LayerNorm" if l["norm"] else "")
        return f"txt_gemm_kernel{'<layernorm>' if l['norm'] else ''} {ci} -> {co_}, k {k}{extra}"
    if l["kind"] == "attn":
        return f"txt_attention_kernel H {l['H']}"
    if l["kind"] == "ln":
        return f"txt_layernorm_kernel C {len(l['norm'][0])}"
    if l["kind"] == "duration":
        return f"txt_duration_kernel C {len(l['wb'][0])} max {l['max_frames']}"
    return f"txt_{l['kind']}_kernel"


# ---- restatements ------------------------------------------------------------------------------------------------------------
MUTATIONS = ("one_chunk", "remainder_dropped", "bias_first", "relu_after_residual", "no_residual", "unbiased_variance",
             "eps_1e-5", "raw_moments", "scale_before_bias", "padded_key", "tile_key_dropped", "no_rescale", "naive_softplus",
             "floor_half_up", "no_upper_clip", "inclusive_offsets", "embed_no_position")


def fmaf32(a, b, c):
    """fl32(a b + c), correctly rounded: the product is exact in float64, the sum is rounded to odd (TwoSum gives its error)
    and 53 >= 2 * 24 + 2 bits make the second rounding harmless."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        need = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(need, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def gemm_act(l, x, mutation=None):
    """act(chain + bias) of a GEMM launch on ONE item's rows ``x [n, C_in]`` -> ``[n, C_out]``, fp32."""
    w, b = l["wb"]
    ci = w.shape[1]
    chunk, variant = min((ci + 7) & ~7, SLICE), 0
    if mutation == "one_chunk":
        chunk = (ci + 7) & ~7
    if mutation == "remainder_dropped" and ci > SLICE and ci % SLICE:
        x, w = x[:, :ci // SLICE * SLICE], w[:, :ci // SLICE * SLICE]
    if mutation == "bias_first":
        variant = co.BIAS_FIRST
    xc = np.ascontiguousarray(np.asarray(x, np.float32).T)[None]
    y = np.ascontiguousarray(co.chain_conv1d(xc, w, b, 1, chunk, [(0, x.shape[0])], variant=variant)[0].T)
    return np.maximum(y, np.float32(0)) if l["relu"] else y


def gemm_sum(l, t, mutation=None):
    """The row a GEMM launch normalises (or stores): ``res + act(chain + bias)`` in fp32."""
    v = gemm_act(l, t[l["x"]], mutation)
    if l["res"] is not None and mutation != "no_residual":
        v = (t[l["res"]].astype(np.float32) + v).astype(np.float32)
        if mutation == "relu_after_residual":
            v = np.maximum(v, np.float32(0))
    return v


def ln64(s, gamma, beta, eps=LN_EPS, unbiased=False):
    s = np.asarray(s, np.float64)
    mean = s.mean(axis=-1, keepdims=True)
    d = s - mean
    var = (d * d).sum(axis=-1, keepdims=True) / (s.shape[-1] - (1 if unbiased else 0))
    return d / np.sqrt(var + np.float64(eps)) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def ln_depth(C, kind):
    """D of the derivation: additions on the deepest path of the row sum."""
    return 16 + 1 + (C + 31) // 32 if kind == "gemm" else 2 + (C + 255) // 256 + 6


def ln_bar(s, gamma, beta, kind):
    s = np.asarray(s, np.float64)
    n = s.shape[-1]
    D = ln_depth(n, kind)
    mean = s.mean(axis=-1, keepdims=True)
    d = s - mean
    r = 1.0 / np.sqrt((d * d).sum(axis=-1, keepdims=True) / n + np.float64(LN_EPS))
    g = np.abs(np.asarray(gamma, np.float64))
    dm = (D + 1) * U * np.abs(s).sum(axis=-1, keepdims=True) / n
    rho = ((D + 4) / 2 + 4) * U
    return g * r * (dm + np.abs(d) * (rho + 2 * U)) + U * np.abs(d * r * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64))


def _butterfly(v):
    """``wave_sum``: v [rows, 64] -> [rows], every lane ends with the same bits."""
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ s]).astype(np.float32)
    return v[:, 0]


def _ln32_finish(s, mean, tot2, gamma, beta, eps):
    n = np.float32(s.shape[-1])
    rstd = (np.float32(1) / np.sqrt((tot2 / n + np.float32(eps)).astype(np.float32))).astype(np.float32)
    d = (s - mean[:, None]).astype(np.float32)
    return fmaf32((d * rstd[:, None]).astype(np.float32), np.asarray(gamma, np.float32), np.asarray(beta, np.float32))


def ln32_gemm(s, gamma, beta, eps=LN_EPS):
    """The LayerNorm epilogue of ``txt_gemm_kernel`` in its order: wave ct holds channels 32 ct .. 32 ct + 31, a lane the
    registers 4 g + e = channel 8 g + 4 hi + e; channels past C are zeros."""
    s = np.asarray(s, np.float32)
    rows, C = s.shape
    nw = (C + 31) // 32
    n = np.float32(C)

    def reduce(regs):                                   # regs [rows, nw, g, hi, e] -> [rows]
        part = np.zeros((rows, nw, 2), np.float32)
        for g in range(4):
            for e in range(4):
                part = regs(part, g, e)
        tot = np.zeros(rows, np.float32)
        for w in range(nw):
            tot = (tot + (part[:, w, 0] + part[:, w, 1]).astype(np.float32)).astype(np.float32)
        return tot
    pad = np.zeros((rows, nw * 32), np.float32)
    pad[:, :C] = s
    a = pad.reshape(rows, nw, 4, 2, 4)
    tot = reduce(lambda part, g, e: (part + a[:, :, g, :, e]).astype(np.float32))
    mean = (tot / n).astype(np.float32)
    inside = (np.arange(nw * 32) < C).reshape(nw, 4, 2, 4)
    d = np.where(inside, (a - mean[:, None, None, None, None]).astype(np.float32), np.float32(0))
    tot2 = reduce(lambda part, g, e: fmaf32(d[:, :, g, :, e], d[:, :, g, :, e], part))
    return _ln32_finish(s, mean, tot2, gamma, beta, eps)


def ln32_rows(s, gamma, beta, eps=LN_EPS):
    """``txt_layernorm_kernel`` in its order: a lane sums the quads lane, lane + 64, ... as (v0 + v1) + (v2 + v3), then the xor
    butterfly; the squared deviations by fmaf in channel order."""
    s = np.asarray(s, np.float32)
    rows, C = s.shape
    J = (C + 255) // 256
    pad = np.zeros((rows, J * 256), np.float32)
    pad[:, :C] = s
    a = pad.reshape(rows, J, 64, 4)
    inside = (np.arange(J * 256) < C).reshape(J, 64, 4)
    acc = np.zeros((rows, 64), np.float32)
    for j in range(J):
        quad = ((a[:, j, :, 0] + a[:, j, :, 1]).astype(np.float32) + (a[:, j, :, 2] + a[:, j, :, 3]).astype(np.float32)).astype(np.float32)
        acc = np.where(inside[j, :, 0], (acc + quad).astype(np.float32), acc)
    mean = (_butterfly(acc) / np.float32(C)).astype(np.float32)
    qq = np.zeros((rows, 64), np.float32)
    for j in range(J):
        for e in range(4):
            d = (a[:, j, :, e] - mean[:, None]).astype(np.float32)
            qq = np.where(inside[j, :, e], fmaf32(d, d, qq), qq)
    return _ln32_finish(s, mean, _butterfly(qq), gamma, beta, eps)


def ln32_mutated(s, gamma, beta, mutation):
    """The wrong LayerNorms, in fp32 where the precision is the point (``raw_moments``), else through float64."""
    if mutation == "raw_moments":
        s = np.asarray(s, np.float32)
        n = np.float32(s.shape[-1])
        mean = (s.sum(axis=-1, dtype=np.float32) / n).astype(np.float32)
        var = ((s * s).sum(axis=-1, dtype=np.float32) / n - mean * mean).astype(np.float32)
        rstd = (np.float32(1) / np.sqrt(np.maximum(var, np.float32(0)) + LN_EPS)).astype(np.float32)
        return ((s - mean[:, None]) * rstd[:, None] * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)).astype(np.float32)
    if mutation == "unbiased_variance":
        return ln64(s, gamma, beta, unbiased=True).astype(np.float32)
    assert mutation == "eps_1e-5", mutation
    return ln64(s, gamma, beta, eps=np.float32(1e-5)).astype(np.float32)


_LN_MUT = ("unbiased_variance", "eps_1e-5", "raw_moments")


def _heads(a, H):
    n, E = a.shape
    return a.reshape(n, H, E // H).transpose(1, 0, 2)


def attn64(qkv, H):
    """float64 softmax attention of one item on its stored ``qkv [n, 3E]`` -> ``[n, E]``."""
    n, E = qkv.shape[0], qkv.shape[1] // 3
    scale = np.float64(np.float32(1.0 / np.sqrt(float(E // H))))
    a = np.asarray(qkv, np.float64)
    q, k, v = _heads(a[:, :E] * scale, H), _heads(a[:, E:2 * E], H), _heads(a[:, 2 * E:], H)
    s = q @ k.transpose(0, 2, 1)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    o = (p / p.sum(axis=-1, keepdims=True)) @ v
    return np.ascontiguousarray(o.transpose(1, 0, 2)).reshape(n, E)


def attn_scores_std(qkv, H):
    n, E = qkv.shape[0], qkv.shape[1] // 3
    a = np.asarray(qkv, np.float64)
    q, k = _heads(a[:, :E] / np.sqrt(float(E // H)), H), _heads(a[:, E:2 * E], H)
    return float((q @ k.transpose(0, 2, 1)).std())


def attn32(qkv, H, mutation=None, bq=None):
    """``txt_attention_kernel`` in fp32 and in its order (see the module docstring) on one item's ``qkv [n, 3E]``."""
    f32 = np.float32
    qkv = np.asarray(qkv, f32)
    n, E = qkv.shape[0], qkv.shape[1] // 3
    Dk = E // H
    scale = f32(1.0 / np.sqrt(float(Dk)))
    qs = qkv[:, :E]
    if mutation == "scale_before_bias":
        qs = ((qs - bq) * scale + bq).astype(f32)
    else:
        qs = (qs * scale).astype(f32)
    q, k, v = _heads(qs, H), _heads(qkv[:, E:2 * E], H), _heads(qkv[:, 2 * E:], H)
    m, l, o = np.full((H, n), -np.inf, f32), np.zeros((H, n), f32), np.zeros((H, n, Dk), f32)
    with np.errstate(invalid="ignore"):
        for j0 in range(0, n, KEY_TILE):
            kt, vt = k[:, j0:j0 + KEY_TILE], v[:, j0:j0 + KEY_TILE]
            if mutation == "tile_key_dropped" and kt.shape[1] == KEY_TILE:
                kt, vt = kt[:, :-1], vt[:, :-1]
            if mutation == "padded_key" and kt.shape[1] < KEY_TILE:
                kt = np.concatenate([kt, np.zeros((H, 1, Dk), f32)], axis=1)
                vt = np.concatenate([vt, np.zeros((H, 1, Dk), f32)], axis=1)
            s = (q @ kt.transpose(0, 2, 1)).astype(f32)
            mn = np.maximum(m, s.max(axis=-1))
            alpha = np.exp(m - mn).astype(f32)
            p = np.exp(s - mn[..., None]).astype(f32)
            pp = np.zeros((H, n, KEY_TILE), f32)
            pp[..., :p.shape[-1]] = p
            pp = pp.reshape(H, n, 4, 2, 4)
            part = np.zeros((H, n, 2), f32)
            for g in range(4):
                for e in range(4):
                    part = (part + pp[:, :, g, :, e]).astype(f32)
            l = fmaf32(l, alpha, (part[..., 0] + part[..., 1]).astype(f32))
            if mutation != "no_rescale":
                o = (o * alpha[..., None]).astype(f32)
            o = (o + (p @ vt).astype(f32)).astype(f32)
            m = mn
    out = (o / l[..., None]).astype(f32)
    return np.ascontiguousarray(out.transpose(1, 0, 2)).reshape(n, E)


def dot32(x, w, b):
    """``u`` of ``txt_duration_kernel``, exactly: x [n, C], w [C], b scalar."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    n, C = x.shape
    J = (C + 255) // 256
    xp, wp = np.zeros((n, J * 256), np.float32), np.zeros(J * 256, np.float32)
    xp[:, :C], wp[:C] = x, w
    xp, wp = xp.reshape(n, J, 64, 4), wp.reshape(J, 64, 4)
    s = np.zeros((n, 64), np.float32)
    for j in range(J):
        for e in range(4):
            s = fmaf32(xp[:, j, :, e], wp[j, :, e], s)
    return (_butterfly(s) + np.float32(b)).astype(np.float32)


def softplus64(u):
    return np.logaddexp(np.asarray(u, np.float64), 0.0)


def pred_bar(u):
    u = np.asarray(u, np.float64)
    t = np.exp(-np.abs(u))
    return 4 * U * t / (1 + t) + 4 * U * np.log1p(t) + U * softplus64(u) + 2.0 ** -126


def softplus32(u, mutation=None):
    u = np.asarray(u, np.float32)
    with np.errstate(over="ignore"):
        if mutation == "naive_softplus":
            return np.log((np.float32(1) + np.exp(u)).astype(np.float32)).astype(np.float32)
        return (np.maximum(u, np.float32(0)) + np.log1p(np.exp(-np.abs(u)).astype(np.float32)).astype(np.float32)).astype(np.float32)


def frames_of(raw, max_frames, mutation=None):
    """``clip(rint(raw), 1, max)`` in float64 (np.rint: half to even)."""
    r = np.floor(raw + 0.5) if mutation == "floor_half_up" else np.rint(raw)
    return np.clip(r, 1.0, np.inf if mutation == "no_upper_clip" else float(max_frames))


def frames32(pred, max_frames, mutation=None):
    """The kernel's frames from ITS pred, in fp32."""
    with np.errstate(over="ignore"):
        raw = (np.exp(np.asarray(pred, np.float32)) - np.float32(1)).astype(np.float32)
    f = np.minimum(frames_of(raw.astype(np.float64), max_frames, mutation), 2.0 ** 31 - 1)
    return f.astype(np.int64)


def decided(u, max_frames):
    """(frames float64 decides, decided mask) for the logits ``u`` (see the module docstring)."""
    sp = softplus64(u)
    with np.errstate(over="ignore"):
        e = np.exp(sp)
        raw, margin = e - 1.0, e * (pred_bar(u) + 5 * U)
        lo, hi = frames_of(raw - margin, max_frames), frames_of(raw + margin, max_frames)
    return frames_of(raw, max_frames).astype(np.int64), lo == hi


def scan_np(frames, lengths=None, mutation=None):
    """``txt_scan_kernel``: (offsets [B, P + 1], totals [B]) int64."""
    f = np.maximum(np.asarray(frames, np.int64), 0)
    B, P = f.shape
    if lengths is not None:
        f = np.where(np.arange(P)[None, :] < np.asarray(lengths)[:, None], f, 0)
    c = np.cumsum(f, axis=1)
    if mutation == "inclusive_offsets":
        return np.concatenate([c, c[:, -1:]], axis=1), c[:, -1]
    return np.concatenate([np.zeros((B, 1), np.int64), c], axis=1), c[:, -1]


def regulate_np(enc, frames, T_pad):
    """``txt_gather_kernel`` after the scan: np.repeat per item, zeros from the item's total on."""
    out = np.zeros((enc.shape[0], T_pad, enc.shape[2]), enc.dtype)
    for b in range(enc.shape[0]):
        r = np.repeat(enc[b], np.maximum(frames[b], 0), axis=0)
        out[b, :len(r)] = r
    return out


def emulate(l, t, mutation=None):
    """What launch l stores for ONE item, restated in fp32 from the item's own rows ``t`` (logical name -> [n, ...]).  The
    duration launch gives (pred, frames), the scan (offsets, total).  ``mutation``: a WRONG restatement."""
    kind = l["kind"]
    if kind == "embed":
        ids = t["ids"]
        pos = l["pos"][:len(ids)]
        return l["tok"][ids].copy() if mutation == "embed_no_position" else (l["tok"][ids] + pos).astype(np.float32)
    if kind == "gemm":
        s = gemm_sum(l, t, mutation)
        if l["norm"] is None:
            return s
        return ln32_mutated(s, *l["norm"], mutation) if mutation in _LN_MUT else ln32_gemm(s, *l["norm"])
    if kind == "ln":
        s = t[l["x"]]
        return ln32_mutated(s, *l["norm"], mutation) if mutation in _LN_MUT else ln32_rows(s, *l["norm"])
    if kind == "attn":
        return attn32(t[l["x"]], l["H"], mutation, l["bq"])
    if kind == "duration":
        pred = softplus32(dot32(t[l["x"]], *l["wb"]), mutation)
        return pred, frames32(pred, l["max_frames"], mutation)
    assert kind == "scan", kind
    off, tot = scan_np(t["frames"][None], None, mutation)
    return off[0], tot[0]


# ---- claims ------------------------------------------------------------------------------------------------------------------
def _where(bad, what, got, want):
    idx = np.argwhere(bad)
    i = tuple(idx[0])
    return (f"{what}: {len(idx)} of {got.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}; "
            f"rows {sorted(set(idx[:, 0].tolist()))[:12]}")


def _exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        raise AssertionError(_where(~(got == want), what + " differs from its restatement", got, want))


def _ratio(err, bar, what, got, want, kind):
    if not (err <= bar).all():
        worst = float(np.nanmax(err / np.maximum(bar, 1e-300))) if np.isfinite(err).any() else float("nan")
        raise AssertionError(_where(~(err <= bar), f"{what}: {kind} err / bar up to {worst:.3g}", got, want))
    nz = bar > 0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


def judge(l, t, got, what):
    """``got``: what the launch stored for ONE item's own rows (for the duration launch (pred, frames), for the scan (offsets,
    total)), against launch l's claim on the item's inputs ``t``.  -> (claim kind, figure): "exact" 0.0; "layernorm" and
    "softplus" the worst err / bar; "attention" (err, e32); the duration launch adds (decided, valid) positions."""
    kind = l["kind"]
    if kind in ("embed", "scan") or (kind == "gemm" and l["norm"] is None):
        want = emulate(l, t)
        if kind == "scan":
            _exact(np.asarray(got[0], np.int64), want[0], what + " (offsets)")
            _exact(np.asarray(got[1], np.int64), np.asarray(want[1]), what + " (total)")
        else:
            _exact(got, want, what)
        return "exact", 0.0
    if kind in ("gemm", "ln"):
        s = gemm_sum(l, t) if kind == "gemm" else t[l["x"]]
        want = ln64(s, *l["norm"])
        assert got.shape == want.shape, (what, got.shape, want.shape)
        return "layernorm", _ratio(np.abs(got - want), ln_bar(s, *l["norm"], kind), what, got, want, "LayerNorm")
    if kind == "attn":
        H = l["H"]
        want = attn64(t[l["x"]], H)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if not np.isfinite(got).all():
            raise AssertionError(_where(~np.isfinite(got), what + " is not finite", got, want))
        n, E = want.shape
        per_head = lambda a: np.abs(a).reshape(n, H, E // H).max(axis=(0, 2))
        scale = np.maximum(1.0, per_head(want))
        return "attention", (float((per_head(got - want) / scale).max()), float((per_head(attn32(t[l["x"]], H) - want) / scale).max()))
    assert kind == "duration", kind
    pred, frames = got
    u = dot32(t[l["x"]], *l["wb"])
    want = softplus64(u)
    r = _ratio(np.abs(pred - want), pred_bar(u), what, pred, want, "softplus")
    f64, dec = decided(u, l["max_frames"])
    frames = np.asarray(frames, np.int64)
    if not np.array_equal(frames[dec], f64[dec]):
        raise AssertionError(_where(dec & (frames != f64), what + ": frames differ where float64 decides them", frames, f64))
    lo = 1
    if not ((frames >= lo) & (frames <= l["max_frames"])).all():
        raise AssertionError(_where((frames < lo) | (frames > l["max_frames"]), what + ": frames outside [1, max]", frames, f64))
    return "softplus", (r, int(dec.sum()), int(dec.size))


def _tail_zero(name, tail, what):
    if tail.size and not (tail == 0).all():
        raise AssertionError(_where(~(tail == 0), f"{what}: {name} past the item's length is not 0", tail, np.zeros_like(tail)))


class Tally:
    """What a test judged: names, worst err / bar per claim kind, every attention's (err, e32, what), exact launches and
    elements compared, decided / valid positions."""

    def __init__(self):
        self.worst, self.attn, self.exact, self.elements, self.decided, self.valid = {}, [], 0, 0, 0, 0

    def e32(self):
        return max((a[1] for a in self.attn), default=0.0)

    def check_attention(self):
        """The attention claim, with e32 the largest over everything tallied."""
        if not self.attn:
            return None
        err, _, what = max(self.attn, key=lambda a: a[0])
        e32 = self.e32()
        assert e32 > 0 and err <= 4 * e32, f"{what}: |got - fp64| / max(1, max |fp64|) = {err:.3e} > 4 e32 = {4 * e32:.3e}"
        return err / (4 * e32)

    def line(self):
        out = ", ".join(f"{k} err / bar {v:.3f}" for k, v in sorted(self.worst.items()))
        if self.attn:
            err = max(a[0] for a in self.attn)
            out += f", attention err {err:.2e} / (4 e32 = {4 * self.e32():.2e}) = {err / max(4 * self.e32(), 1e-300):.3f}"
        return out + f"; {self.exact} launch items exact, {self.elements} elements judged, {self.valid - self.decided} of {self.valid} frames undecided"


def judge_forward(plan, tensors, P, lengths=None, tally=None, launches=None):
    """Every judged launch of one forward on the tensors it left (``tensors``: logical name -> [B, P, ...], totals [B]).
    Ragged: item by item on the item's own prefix, every output row past it exactly 0.  ``launches``: judge these instead of
    the survivors (a CPU-chained forward keeps every tensor).  -> [names judged]; figures go to ``tally``."""
    tally = Tally() if tally is None else tally
    B = next(iter(tensors.values())).shape[0]
    names = []
    for l in (judged(plan) if launches is None else launches):
        names.append(l["name"])
        outs = {"duration": ("pred", "frames"), "scan": ("offsets",)}.get(l["kind"], (l["y"],))
        for b in range(B):
            n = P if lengths is None else int(lengths[b])
            what = f"{l['name']} [{kernel_form(l)}] B {B} P {P} item {b} of {n} positions"
            if l["kind"] == "scan":
                _tail_zero("frames", tensors["frames"][b, n:], what)
                got = (tensors["offsets"][b, :n + 1], tensors["totals"][b])
                if not (np.asarray(tensors["offsets"][b, n:]) == tensors["totals"][b]).all():
                    raise AssertionError(f"{what}: offsets from the item's length on are not its total")
            else:
                for o in outs:
                    _tail_zero(o, tensors[o][b, n:], what)
                got = tuple(np.ascontiguousarray(tensors[o][b, :n]) for o in outs)
                got = got[0] if len(got) == 1 else got
            t = {key: tensors[key][b, :n] for key in l["needs"]}
            kind, r = judge(l, t, got, what)
            if kind == "attention":
                tally.attn.append(r + (what,))
            elif kind == "softplus":
                tally.worst[kind] = max(tally.worst.get(kind, 0.0), r[0])
                tally.decided += r[1]
                tally.valid += r[2]
            elif kind == "exact":
                tally.exact += 1
            else:
                tally.worst[kind] = max(tally.worst.get(kind, 0.0), r)
            tally.elements += n * (tensors[outs[0]].shape[2] if tensors[outs[0]].ndim == 3 else 1)
    return names


def chain_forward(plan, inputs, P, lengths=None, mutation=None):
    """The whole forward with the launches chained on the CPU (``emulate``), item by item, zeros past each length: every
    logical tensor, inputs included."""
    t = dict(inputs)
    B = next(iter(t.values())).shape[0]
    for l in plan:
        per_item = []
        for b in range(B):
            n = P if lengths is None else int(lengths[b])
            per_item.append((n, emulate(l, {key: t[key][b, :n] for key in l["needs"]}, mutation)))
        if l["kind"] == "duration":
            t["pred"], t["frames"] = np.zeros((B, P), np.float32), np.zeros((B, P), np.int32)
            for b, (n, (pred, frames)) in enumerate(per_item):
                t["pred"][b, :n], t["frames"][b, :n] = pred, frames
        elif l["kind"] == "scan":
            t["offsets"], t["totals"] = np.zeros((B, P + 1), np.int64), np.zeros(B, np.int64)
            for b, (n, (off, tot)) in enumerate(per_item):
                t["offsets"][b, :n + 1], t["offsets"][b, n + 1:], t["totals"][b] = off, tot, tot
        else:
            out = np.zeros((B, P) + per_item[0][1].shape[1:], np.float32)
            for b, (n, y) in enumerate(per_item):
                out[b, :n] = y
            t[l["y"]] = out
    return t


# ---- a device forward's tensors ----------------------------------------------------------------------------------------------
def from_buffers(plan, bufs, B, P):
    """The surviving logical tensors [B, P, C] cut from ``_read_buffers``' flat buffers."""
    out = {}
    width = {l["y"]: (l["wb"][0].shape[0] if l["kind"] == "gemm" else None) for l in plan}
    for name, slot in survivors(plan).items():
        C = width[name]
        if C is None:                                   # emb, attn: the embedding width
            C = len(plan[-1]["norm"][0])
        out[name] = np.asarray(bufs[slot][:B * P * C]).reshape(B, P, C)
    return out
