"""The PostNet (csrc/postnet.h, ``postnet_forward`` in csrc/iris_hifigan.hip), launch by launch, against the fmaf chain.
TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

A PostNet layer is one launch of the generic fp32 conv kernel (csrc/conv_mfma_f32.h) over the BatchNorm-folded weights
(``iris.postnet.fold_batchnorm``): layer 0 stages the channels-first mel, layers 0 .. L-2 end in the tanh epilogue
(``out_act = 1``), the last one stores the residual channels-last and ``postnet_residual_kernel`` adds it to the mel.
So a launch is judged on its OWN input tensor (nothing propagates from layer to layer):

* hidden layer:  |got - tanh_fp64(chain pre-activation)| <= tol, every element finite   (``judge_hidden``);
* last layer:    got == chain, bit for bit                                               (``judge_last``);
* output:        out[b, c, t] == float32(mel[b, c, t] + res[b, t, c]) bit for bit, 0 past an item's length  (``judge_output``).

``chain_layer`` is the restatement: ``chain_oracle.chain_conv1d`` with the chunk ``f32_cases.single_layer_chunk`` reads from
``pick_tile`` / ``launch_conv`` (80 for the channels-first 80 -> more than 64 channels launch, 32 where both channel counts
are at most 32, else 64).  ``MUTATIONS`` are wrong restatements; tests/test_oracle_postnet.py shows that each fails its claim.
``layer_tile`` restates how ``launch_conv`` picks the tile height, so that the shape list can be held to what it is meant to
reach (32-row tiles, MT = 1, and 64-row tiles, MT = 2).
"""
import numpy as np

from oracle import chain_oracle as co
from oracle import f32_cases as fc

# ---- cases -----------------------------------------------------------------------------------------------------------------
# name: (n_mels, layers, channels, k).  "narrow": more taps than some items have frames, 12 layers; its 14 channels are no
# multiple of 4, so its hidden layers take the kernel's scalar staging and its scalar (bounded) epilogue WITH the tanh, and
# its last layer (6 channels) the scalar epilogue without.  Only the layers L-3 .. L-1 of a deep net survive in the workspace,
# so "narrow2" (the same widths read the other way: 2 layers of 12 channels) judges the channels-first k = 7 launch as well.
CONFIGS = {
    "default": (80, 3, 256, 5),
    "deeper": (80, 4, 256, 5),
    "small": (20, 2, 24, 3),
    "narrow": (6, 12, 14, 7),
    "narrow2": (6, 2, 12, 7),
}
WEIGHT_SEEDS = ((3, 4), (13, 14))            # (PostNet(seed=...), randomise(seed)): two sets of parameters
DENSE_T = (1, 2, 4, 31, 32, 33, 63, 64, 65, 97)
DENSE_B = (1, 3)                             # T odd at B = 3: items start off a 16-byte boundary in the channels-first mel
# (B, T, lengths); the last is the (8, 2048) case of tests/test_postnet_ragged.py: the one shape whose hidden layers run
# 64-row tiles (MT = 2) at 256 CUs, lengths one below, at and one above both tile edges
RAGGED = [
    (6, 70, [31, 32, 33, 63, 64, 65]),
    (4, 70, [70, 0, 1, 69]),
    (8, 2048, [2048, 63, 64, 65, 127, 129, 33, 1]),
]
RAGGED_CONFIG = "default"
CU = 256                                     # MI355X


def randomise(pn, seed):
    """Every parameter random, as ``_randomise`` of tests/test_postnet.py: non-trivial BatchNorm statistics and biases."""
    rng = np.random.default_rng(seed)
    w = dict(pn.weights)
    for key, val in w.items():
        if key.endswith(".bias") or key.endswith(".beta") or key.endswith(".moving_mean"):
            w[key] = rng.normal(0, 0.3, val.shape).astype(np.float32)
        elif key.endswith(".gamma"):
            w[key] = rng.uniform(0.5, 1.5, val.shape).astype(np.float32)
        elif key.endswith(".moving_variance"):
            w[key] = rng.uniform(0.2, 2.0, val.shape).astype(np.float32)
    pn.set_weights_dict(w)


def make_postnet(config, seeds):
    from iris.postnet import PostNet
    n_mels, layers, channels, k = CONFIGS[config]
    pn = PostNet(n_mels, num_layers=layers, channels=channels, kernel_size=k, seed=seeds[0])
    randomise(pn, seeds[1])
    return pn


def case_mel(config, B, T, seed):
    """[B, n_mels, T] fp32: a log-mel (magnitudes up to about 11) for odd seeds, a standard normal otherwise."""
    from iris._weights import seeded_mel
    return seeded_mel(seed, B, T, n_mels=CONFIGS[config][0], log_mel=bool(seed & 1))


def folded_layers(pn):
    """[(w [C_out, C_in, k], b [C_out])] per layer: the values the device is handed (``PostNet.folded_blob``)."""
    from iris.postnet import fold_batchnorm
    names = ("kernel", "bias", "gamma", "beta", "moving_mean", "moving_variance")
    return [fold_batchnorm(*(pn.weights[f"{pn._prefix(i)}.{n}"] for n in names)) for i in range(pn.num_layers)]


def layer_chunk(wb, i):
    """The CIC of layer i's launch; only layer 0 stages a channels-first input."""
    return fc.single_layer_chunk(wb[0].shape[1], wb[0].shape[0], channels_first=(i == 0))


# ---- the tile of a launch ----------------------------------------------------------------------------------------------------
def layer_tile(c_out, B, T, cu=CU):
    """(MT, rows per tile) of a PostNet layer's launch: ``pick_tile`` gives WT x WC waves by C_out (4 x 1 up to 32 channels,
    2 x 2 up to 64, else 1 x 4), and ``launch_conv`` halves the tile (MT = 1) while the grid of WT * 2 * 32-row tiles has fewer
    than two blocks per CU (one problem per launch; not a ConvTranspose phase)."""
    wt, wc = (4, 1) if c_out <= 32 else ((2, 2) if c_out <= 64 else (1, 4))
    t_blk2 = wt * 2 * 32
    blocks2 = -(-T // t_blk2) * -(-c_out // (wc * 32)) * B
    mt = 1 if blocks2 < 2 * cu else 2
    return mt, wt * mt * 32


def kernel_form(pn, i, B, T, cu=CU, ragged=False):
    """What a failure names: the instantiation and the paths layer i's launch takes."""
    c_in = pn.n_mels if i == 0 else pn.channels
    c_out = pn.n_mels if i == pn.num_layers - 1 else pn.channels
    wt, wc = (4, 1) if c_out <= 32 else ((2, 2) if c_out <= 64 else (1, 4))
    mt, rows = layer_tile(c_out, B, T, cu)
    chunk = fc.single_layer_chunk(c_in, c_out, channels_first=(i == 0))
    return (f"conv_mfma_f32_kernel{'_ragged' if ragged else ''}<{wt}, {wc}, {mt}, {chunk}> {c_in} -> {c_out}, k {pn.kernel_size}, "
            f"{rows}-row tiles, {'channels-first' if i == 0 else 'channels-last'} staging, "
            f"{'16-byte' if c_out % 4 == 0 else 'scalar'} epilogue{'' if i == pn.num_layers - 1 else ' + tanh'}")


# ---- restatement -----------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_first_tap", "drop_last_tap", "pad_off_by_one", "tanh_before_bias", "residual_untransposed")


def layer_rows(B, L, wb):
    """The row windows a launch of L rows is judged on (``f32_cases.judged_rows``: all of them up to 2048 rows)."""
    return fc.judged_rows(B, L, wb[0].size)


def chain_layer(x, wb, chunk, rows, mutation=None):
    """The chain pre-activation (acc + bias) of one PostNet layer on the rows ``rows``: x [B, C_in, L] fp32 (the launch's own
    input) -> [B, C_out, rows].  ``mutation``: a WRONG restatement (the taps and the padding ones)."""
    w, b = wb
    x = np.ascontiguousarray(x, dtype=np.float32)
    if mutation in ("drop_first_tap", "drop_last_tap"):
        w = w.copy()
        w[:, :, 0 if mutation == "drop_first_tap" else -1] = 0
    elif mutation == "pad_off_by_one":                      # output row t reads the rows of t - 1
        shifted = np.zeros_like(x)
        shifted[:, :, 1:] = x[:, :, :-1]
        x = shifted
    return co.chain_conv1d(x, w, b, 1, chunk, rows)


def tanh32(pre):
    """fp32 tanh of an fp32 pre-activation: the correctly rounded one (the CPU's stand-in for ``tanhf``)."""
    return np.tanh(np.asarray(pre, dtype=np.float32).astype(np.float64)).astype(np.float32)


def hidden_layer(x, wb, chunk, rows, mutation=None):
    """What a hidden layer stores, restated in fp32.  ``tanh_before_bias``: tanh(acc) + bias."""
    if mutation == "tanh_before_bias":
        acc = co.chain_conv1d(np.ascontiguousarray(x, dtype=np.float32), wb[0], np.zeros_like(wb[1]), 1, chunk, rows)
        return (tanh32(acc) + wb[1][None, :, None]).astype(np.float32)
    return tanh32(chain_layer(x, wb, chunk, rows, mutation))


def add_residual(mel, res_btc, mutation=None):
    """out[b, c, t] = float32(mel[b, c, t] + res[b, t, c]): one fp32 add.  ``residual_untransposed``: res read as if it were
    channels-first already."""
    res = np.asarray(res_btc, dtype=np.float32)
    r = res.reshape(mel.shape) if mutation == "residual_untransposed" else res.transpose(0, 2, 1)
    return (np.asarray(mel, dtype=np.float32) + r).astype(np.float32)


def chain_postnet(pn, mel, mutation=None):
    """A whole PostNet with the layers chained on the CPU: ([layer outputs [B, C, T] fp32 ...], out [B, n_mels, T])."""
    layers = folded_layers(pn)
    x = np.ascontiguousarray(mel, dtype=np.float32)
    T = x.shape[2]
    outs = []
    for i, wb in enumerate(layers):
        chunk = layer_chunk(wb, i)
        if i < len(layers) - 1:
            x = hidden_layer(x, wb, chunk, [(0, T)], mutation)
        else:
            x = chain_layer(x, wb, chunk, [(0, T)], mutation)
        outs.append(x)
    return outs, add_residual(mel, x.transpose(0, 2, 1), mutation)


# ---- claims ----------------------------------------------------------------------------------------------------------------
def _where(bad, what, got, want):
    idx = np.argwhere(bad)
    i = tuple(idx[0])
    return (f"{what}: {len(idx)} of {got.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}; "
            f"rows {sorted(set(idx[:, -1].tolist()))[:12]}")


def judge_hidden(got, pre, tol, what):
    """got [B, C, rows] against tanh_fp64 of the chain's pre-activation.  Returns the worst error; raises with the layer, the
    kernel form (in ``what``), the first differing element and the rows that differ."""
    assert got.shape == pre.shape, (what, got.shape, pre.shape)
    if not np.isfinite(got).all():
        raise AssertionError(_where(~np.isfinite(got), what + " is not finite", got, pre))
    want = np.tanh(pre.astype(np.float64))
    err = np.abs(got - want)
    worst = float(err.max()) if err.size else 0.0
    if not worst <= tol:
        raise AssertionError(_where(err > tol, f"{what}: max |got - tanh(chain)| {worst:.3e} > {tol:.3e}", got, want))
    return worst


def judge_last(got, chain, what):
    assert got.shape == chain.shape, (what, got.shape, chain.shape)
    if not np.isfinite(got).all():
        raise AssertionError(_where(~np.isfinite(got), what + " is not finite", got, chain))
    if not np.array_equal(got, chain):
        raise AssertionError(_where(got != chain, what + " differs from the chain", got, chain))


def judge_output(out, mel, res_btc, lengths, what):
    """out, mel [B, C, T]; res [B, T, C] (the device's own).  Frames at or past lengths[b] (None: T) must be exactly 0 and
    are read from neither mel nor res."""
    B, C, T = out.shape
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        want = add_residual(mel[b:b + 1, :, :n], res_btc[b:b + 1, :n])
        got = out[b:b + 1, :, :n]
        if not np.array_equal(got, want):       # (NaN != NaN: a non-finite output fails here too)
            raise AssertionError(_where(~(got == want), f"{what} item {b}: out != float32(mel + res^T)", got, want))
        if out[b, :, n:].any() or np.isnan(out[b, :, n:]).any():
            tail = out[b:b + 1, :, n:]
            raise AssertionError(_where(~(tail == 0), f"{what} item {b}: output past its length {n} is not 0", tail, np.zeros_like(tail)))
