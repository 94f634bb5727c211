"""The fp32 forward (dtype "f32"), launch by launch, against the fmaf chain.  TEST INFRASTRUCTURE ONLY, like the rest of
``oracle/``.

Every output element of the fp32 path is one fixed fmaf chain (``oracle/chain_oracle.c`` states it), so
a launch is judged by EQUALITY with the chain on the launch's own input tensors.  ``walk`` restates every launch of one
forward from the tensors a provider hands it -- the GPU's own (tests/test_gpu_f32_chain.py: nothing propagates from launch
to launch) or, with no provider, the tensors of the walk itself (tests/test_oracle_chain.py) -- with the chunk (CIC) of
each launch read from its kernel name in the host-only launch plan (``iris_hifigan_describe_plan``), which also says which
conv pairs run fused (their xt never reaches the workspace: both convs are restated from the pair's input), which launch
forms the MRF mean and whether an upsampler reads that mean or averages the three branch tensors while it stages them.

``SHAPES`` lists, per shape, the launches walked; tests/test_oracle_chain.py holds the list to the plan: the (stage, kernel
instance) pairs it visits are those a scan of the grid stated below finds.
"""
import re

import numpy as np

from oracle import chain_oracle as co
from oracle.bf16_cases import CONFIGS, CU, setup  # noqa: F401  (the configurations and seeded weights are shared)

TOL_TANH = 2e-6      # |tanhf - tanh_fp64|: the tanh term of tests/test_gpu_parity.py::test_conv_post_matches_oracle's bar

# ---- shapes --------------------------------------------------------------------------------------------------------------
# (id, config, B, T, walked, mel seed).  walked: "pre", "ups.i", "mrf.i" (every launch of stage i's MRF), "mrf.i.pM" (conv pair
# M of it only: a stage costs the CPU seconds per launch, and every pair of a stage runs the same kernel instances except the
# last, which holds the summing forms), "post" (the waveform); None = everything.  V1 at 256 CUs; what each shape is for:
#   2x57, 3x150    stages 2, 3: MRF tiles <2,2,1,..> / <4,1,1,..> resp. full height (MT = 2), plain and summing, behind fused
#                  pairs of 64 resp. 128 rows; convt<2,1,2,2,2,1>
#   1x46, 1x57     stage 1: fixed ranges (mode 1) / snake jobs at half height
#   1x190          stage 0: fixed ranges; stage 1: snake jobs at full height
#   4x57, 1x717    stage 0: snake jobs at half / full height
#   3x337, 2x921   stage 0: serial and summing at half / full height; convt<2,2,1,4,2,1> at ups.1
#   1x480          stage 1: serial and summing at full height; convt<1,1,1,4,2,1> at ups.2
#   1x950, 3x1249  stage 1 / 0: 128-row tiles (MT = 4)
#   2x560, 4x560   stage 3 / 2: mrf_pair_f32_pf_kernel<sum>;  4x500  stage 2: serial and summing tiles drawn from a counter
#   24x64, 32x1    ups.0: convt<2,2,..,1> and <2,1,..,1>;  32x8, 32x16  ups.1: <2,1,..,3> and <2,2,..,3> (three inputs averaged
#                  while staging);  4x127, 4x130  ups.2: <2,1,..,1> and <2,1,..,3>
#   1x1, 5x2       every tensor shorter than every tile: mrf_small_f32_kernel, the pairs, every <1,1,..> upsampler
#   generic, post24: the polyphase fallback with two / three averaged inputs, generic grouped Conv1d launches with two
#   branches, conv_post_tanh_kernel, a mean divisor that is not 3
_S23 = ("ups.2", "mrf.2", "ups.3", "mrf.3")
SHAPES = [
    ("v1-2x57", "v1", 2, 57, _S23, 41), ("v1-3x150", "v1", 3, 150, _S23, 42),
    ("v1-1x46", "v1", 1, 46, ("mrf.1.p0",), 43), ("v1-1x57", "v1", 1, 57, ("pre", "mrf.1.p0"), 44),
    ("v1-1x190", "v1", 1, 190, ("pre", "ups.0", "mrf.0.p0", "ups.1", "mrf.1.p0"), 45),
    ("v1-4x57", "v1", 4, 57, ("mrf.0.p0",), 46), ("v1-1x717", "v1", 1, 717, ("mrf.0.p0",), 47),
    ("v1-3x337", "v1", 3, 337, ("mrf.0.p2",), 48), ("v1-2x921", "v1", 2, 921, ("mrf.0.p2", "ups.1"), 49),
    ("v1-1x480", "v1", 1, 480, ("ups.1", "mrf.1", "ups.2"), 50),
    ("v1-1x950", "v1", 1, 950, ("mrf.1.p0",), 51), ("v1-3x1249", "v1", 3, 1249, ("mrf.0.p0",), 52),
    ("v1-2x560", "v1", 2, 560, ("ups.3", "mrf.3.p2"), 53), ("v1-4x560", "v1", 4, 560, ("ups.2", "mrf.2.p2"), 54),
    ("v1-4x500", "v1", 4, 500, ("mrf.2.p2",), 65),
    ("v1-24x64", "v1", 24, 64, ("ups.0",), 55), ("v1-32x1", "v1", 32, 1, ("pre", "ups.0"), 56),
    ("v1-32x8", "v1", 32, 8, ("ups.1",), 57), ("v1-32x16", "v1", 32, 16, ("ups.1",), 58),
    ("v1-4x127", "v1", 4, 127, ("ups.2",), 59), ("v1-4x130", "v1", 4, 130, ("ups.2",), 60),
    ("v1-1x1", "v1", 1, 1, None, 61), ("v1-5x2", "v1", 5, 2, None, 62),
    ("generic-3x37", "generic", 3, 37, None, 63), ("post24-3x70", "post24", 3, 70, None, 64),
]

# The grid the V1 shapes are held to (tests/test_oracle_chain.py): every (stage, kernel instance) pair that a forward of
# B x T frames launches anywhere on it is visited by SHAPES, and SHAPES visits nothing else.
SCAN_BATCHES = range(1, 33)
SCAN_FRAMES = range(1, 1708)
SCAN_MAX_FRAMES = 6000        # per shape: B * T


def single_layer_chunk(c_in, c_out, channels_first=False):
    """The CIC of a single-layer call (``iris_hifigan_op_*``), whose entry points record no kernel name: the rule of
    ``pick_tile`` / ``launch_conv`` (csrc/conv_mfma_f32.h), which the MRF kernels share.  It matters only where C_in exceeds
    it.  tests/test_oracle_chain.py holds it, on the host, to the kernel names ``describe_plan`` records for layers of the
    same channel counts, so that a planner change fails there and not as a bit mismatch on the GPU."""
    if c_in == 80 and channels_first and c_out > 64:
        return 80
    return 32 if (c_in <= 32 and c_out <= 32) else 64


def shape_mel(shape):
    from iris._weights import seeded_mel
    _, name, B, T, _, seed = shape
    return seeded_mel(seed, B, T, n_mels=CONFIGS[name][0]().in_channels, log_mel=bool(seed & 1))


def numpy_weights(W):
    """{layer: (w, b)} of ``setup`` as fp32 numpy."""
    return {k: (np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.numpy(), dtype=np.float32))
            for k, (w, b) in W.items()}


# ---- the launch plan -------------------------------------------------------------------------------------------------------
_MRF = re.compile(r"mrf_conv_mfma_f32_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\w+), (\d+)")


def plan_launches(cfg, B, T, cu=CU):
    """The launches of one fp32 forward, from the host-only plan: a list of dicts {where: "pre" | "ups.i" | "mrf.i" |
    "post", kernel, and for MRF launches: pair (index m), form: "step1" | "step2" | "step2_sum" | "pair" | "pair_sum"}, in
    launch order (forward_f32: conv_pre, per stage the upsampler and the MRF launches, conv_post)."""
    from iris import _native
    plan = _native.describe_plan(cfg, B, T, _native.DTYPE_F32, cu)
    assert plan["passes"] == 1, plan["passes"]
    names = [r["kernel"] for r in plan["launches"]]
    assert names[0].startswith("conv_mfma_f32_kernel<"), names[0]
    out = [{"where": "pre", "kernel": names[0]}]
    nd = len(cfg.resblock_dilation_sizes[0])
    n = 1
    for i in range(cfg.num_upsamples):
        assert names[n].startswith(("convt_mfma_f32_kernel<", "conv_mfma_f32_kernel<")), names[n]
        out.append({"where": f"ups.{i}", "kernel": names[n]})
        n += 1
        step = 0
        while step < 2 * nd:
            k = names[n]
            rec = {"where": f"mrf.{i}", "kernel": k, "pair": step // 2}
            if k.startswith("mrf_pair_f32_pf_kernel"):
                assert step % 2 == 0 and k.endswith("<sum>") and step == 2 * nd - 2, (k, step)
                rec["form"], step = "pair_sum", step + 2
            elif k.startswith("mrf_pair_f32_kernel"):
                assert step % 2 == 0, (k, step)
                rec["form"], step = "pair", step + 2
            else:
                m = _MRF.match(k)
                assert m or k.startswith(("mrf_small_f32_kernel", "conv_mfma_f32_kernel<")), k
                summing = bool(m) and m.group(9) == "true"
                assert not summing or step == 2 * nd - 1, (k, step)
                rec["form"] = "step1" if step % 2 == 0 else ("step2_sum" if summing else "step2")
                step += 1
            out.append(rec)
            n += 1
    assert n == len(names) - 1 and names[n].startswith("conv_post_"), (n, names)
    out.append({"where": "post", "kernel": names[n]})
    return out


def walked(launches, spec):
    """The launches of ``plan_launches`` that a shape with ``spec`` walks."""
    if spec is None:
        return list(launches)
    return [r for r in launches if r["where"] in spec or ("pair" in r and f"{r['where']}.p{r['pair']}" in spec)]


def visited(cfg, B, T, spec=None):
    """{(where, kernel)} of the launches a shape walks."""
    return {(r["where"], r["kernel"]) for r in walked(plan_launches(cfg, B, T), spec)}


# ---- row windows -------------------------------------------------------------------------------------------------------------
FULL_FMA = 3e9       # a launch is restated on all rows while that costs at most this many fmaf calls (about 2 s of CPU)
MIN_SHARE = 0.03     # ... and never on fewer than this share of its rows


def ranges_of(mask):
    """Boolean row mask -> [(a, e), ...]"""
    d = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def judged_rows(B, L, fma_per_row):
    """The output rows of a launch that are restated (all channels, all batch items): all of them when that is cheap;
    otherwise the first and the last 256, two stretches of 611 rows at offsets aligned to no tile (the fused pairs advance
    by 128 - (k - 1) rows: their seams are at no multiple of a tile height) and every 37th row."""
    if L <= 2048 or float(B) * L * fma_per_row <= FULL_FMA:
        return [(0, L)]
    mask = np.zeros(L, dtype=bool)
    mask[:256] = True
    mask[L - 256:] = True
    for a in ((L // 3) // 64 * 64 + 45, (2 * L // 3) // 64 * 64 + 19):
        mask[a:a + 611] = True
    mask[::37] = True
    return ranges_of(mask)


def n_rows(rows):
    return sum(e - a for a, e in rows)


# ---- restatements ----------------------------------------------------------------------------------------------------------------
WRONG = ("ascending", "tap_major", "chunk64", "bias_first", "res_first", "mean_mul", "mean_assoc")
_VARIANT = {"ascending": co.ASCENDING, "tap_major": co.TAP_MAJOR, "bias_first": co.BIAS_FIRST, "res_first": co.RES_FIRST}


def mean_of(ys, wrong=None):
    """The MRF mean ((y0 + y1) + y2) / n; wrong: ``mean_mul`` = * (1 / n), ``mean_assoc`` = (y0 + (y1 + y2)) / n."""
    n = np.float32(len(ys))
    if wrong == "mean_mul":
        s = ys[0]
        for y in ys[1:]:
            s = s + y
        return (s * (np.float32(1.0) / n)).astype(np.float32)
    if wrong == "mean_assoc":
        s = ys[-1]
        for y in ys[-2::-1]:
            s = y + s
        return (s / n).astype(np.float32)
    return co.mean32(ys)


def conv(x_act, wb, d, chunk, rows, res=None, wrong=None):
    return co.chain_conv1d(x_act, wb[0], wb[1], d, chunk, rows, residual=res, variant=_VARIANT.get(wrong, 0))


def pair(x, wb1, wb2, d, chunk, rows, wrong=None):
    """One fused conv pair on the output rows ``rows``: xt = conv1(lrelu(x)) on the rows conv2 reads (zero outside the
    tensor), y = conv2(lrelu(xt)) + x."""
    B, C, L = x.shape
    h2 = (wb2[0].shape[2] - 1) // 2
    mask = np.zeros(L, dtype=bool)
    for a, e in rows:
        mask[max(0, a - h2):min(L, e + h2)] = True
    need = ranges_of(mask)
    xt = np.zeros((B, C, L), dtype=np.float32)
    xt[:, :, co.row_index(need, L)] = conv(co.lrelu32(x), wb1, d, chunk, need, None, wrong)
    return conv(co.lrelu32(xt), wb2, 1, chunk, rows, x, wrong)


class SelfTensors:
    """The provider of a walk that feeds itself: every tensor is the chain's own, on all rows."""

    def __init__(self):
        self.t = {}

    def get(self, key):
        return self.t[key]


def walk(cfg, W, mel, launches, prov=None, spec=None):
    """Yields one record per walked launch of an fp32 forward of ``mel`` (fp32 numpy [B, C, T]) -- a grouped launch yields
    one per branch tensor it writes:
    {label, where, kernel, form, chunk, kind, rows, total_rows, got, want, restate, touches}.  ``want`` is the chain on the
    restated rows, ``got`` the launch's own output on them, ``restate(wrong)`` the restatement again in one of ``WRONG``
    and ``touches`` the wrong restatements that can change this launch (the others must leave it bit for bit).
    kind "wav" (conv_post): want is the chain's pre-activation (fp32), got the waveform.

    W: ``numpy_weights(setup(name)[2])``; launches: ``plan_launches(cfg, B, T)``.
    prov: the tensors of a device forward -- ``get(key)`` with key ("pre",), ("up", i), ("wav",) -> array, ("xt", i, m),
    ("y", i, m) -> list over the branches; ("y", i, m) of a launch that forms the MRF mean is [mean].  None: the walk
    feeds itself and restates all rows of every launch."""
    own = prov is None
    if own:
        prov = SelfTensors()
    mel = np.ascontiguousarray(mel, dtype=np.float32)
    B, T = mel.shape[0], mel.shape[2]
    nk, nd = cfg.num_kernels, len(cfg.resblock_dilation_sizes[0])
    keep = {id(r) for r in walked(launches, spec)}
    by_where = {}
    for r in launches:
        by_where.setdefault(r["where"], []).append(r)

    def rows_for(L, fma_per_row):
        return [(0, L)] if own else judged_rows(B, L, fma_per_row)

    def record(r, label, chunk, rows, total, restate, touches, got_full, kind="f32"):
        want = restate(None)
        return {"label": label, "where": r["where"], "kernel": r["kernel"], "form": r.get("form"), "chunk": chunk, "kind": kind,
                "rows": rows, "total_rows": total, "got": want if got_full is None else co.take_rows(got_full, rows),
                "want": want, "restate": restate, "touches": touches}

    # conv_pre: the channels-first mel, no activation
    r = by_where["pre"][0]
    if id(r) in keep or own:
        wb = W["conv_pre"]
        chunk = co.chunk_of(r["kernel"], mel.shape[1])
        rows = rows_for(T, wb[0].size)
        touches = {"ascending", "bias_first"} | ({"tap_major"} if mel.shape[1] > chunk else set()) | \
                  ({"chunk64"} if chunk == 80 else set())

        def restate(wrong, wb=wb, chunk=chunk, rows=rows):
            return conv(mel, wb, 1, 64 if wrong == "chunk64" and chunk == 80 else chunk, rows, None, wrong)
        rec = record(r, "conv_pre", chunk, rows, T, restate, touches, None if own else prov.get(("pre",)))
        if own:
            prov.t[("pre",)] = rec["want"]
        if id(r) in keep:
            yield rec
    L = T
    mean_ready = False          # the previous stage's last launch stored the MRF mean itself
    for i in range(cfg.num_upsamples):
        u, C = cfg.upsample_rates[i], cfg.stage_channels(i)
        stage = by_where[f"mrf.{i}"]
        r = by_where[f"ups.{i}"][0]
        if id(r) in keep or own:
            wb = W[f"ups.{i}"]
            c_in = wb[0].shape[0]
            chunk = co.chunk_of(r["kernel"], c_in)
            srcs = [prov.get(("pre",))] if i == 0 else prov.get(("y", i - 1, nd - 1))
            assert len(srcs) == (1 if (i == 0 or mean_ready) else nk), (len(srcs), mean_ready)
            taps = -(-wb[0].shape[2] // u)
            rows = rows_for(L * u, wb[0].shape[1] * c_in * taps)
            touches = {"ascending", "bias_first"} | ({"tap_major"} if c_in > chunk else set()) | \
                      ({"mean_mul", "mean_assoc"} if len(srcs) == 3 else set())

            def restate(wrong, wb=wb, srcs=srcs, u=u, chunk=chunk, rows=rows):
                x = srcs[0] if len(srcs) == 1 else mean_of(srcs, wrong)
                return co.chain_conv_transpose1d(co.lrelu32(x), wb[0], wb[1], u, chunk, rows, variant=_VARIANT.get(wrong, 0))
            rec = record(r, f"ups.{i}", chunk, rows, L * u, restate, touches, None if own else prov.get(("up", i)))
            if own:
                prov.t[("up", i)] = rec["want"]
            if id(r) in keep:
                yield rec
        L *= u
        for r in stage:
            if not (id(r) in keep or own):
                continue
            m, form = r["pair"], r["form"]
            xs = [prov.get(("up", i))] * nk if m == 0 else prov.get(("y", i, m - 1))
            assert len(xs) == nk
            chunk = co.chunk_of(r["kernel"], C)
            wb1 = [W[f"resblocks.{i * nk + j}.convs1.{m}"] for j in range(nk)]
            wb2 = [W[f"resblocks.{i * nk + j}.convs2.{m}"] for j in range(nk)]
            dil = [cfg.resblock_dilation_sizes[j][m] for j in range(nk)]
            ksum = sum(w[0].shape[2] for w in wb1)        # (a launch: all branches)
            base = {"ascending", "bias_first"} | ({"tap_major"} if C > chunk else set())
            if form == "step1":
                rows = rows_for(L, C * C * ksum)
                got = [None] * nk if own else prov.get(("xt", i, m))
                outs = []
                for j in range(nk):
                    def restate(wrong, j=j, xs=xs, wb1=wb1, dil=dil, chunk=chunk, rows=rows):
                        return conv(co.lrelu32(xs[j]), wb1[j], dil[j], chunk, rows, None, wrong)
                    rec = record(r, f"stage {i} step {2 * m} branch {j}", chunk, rows, L, restate, base, got[j])
                    outs.append(rec["want"])
                    yield rec
                if own:
                    prov.t[("xt", i, m)] = outs
                continue
            fused = form in ("pair", "pair_sum")
            summing = form in ("step2_sum", "pair_sum")
            rows = rows_for(L, C * C * ksum * (2.2 if fused else 1))
            if fused:
                def one(j, wrong, xs=xs, wb1=wb1, wb2=wb2, dil=dil, chunk=chunk, rows=rows):
                    return pair(xs[j], wb1[j], wb2[j], dil[j], chunk, rows, wrong)
            else:
                xts = prov.get(("xt", i, m))

                def one(j, wrong, xs=xs, xts=xts, wb2=wb2, chunk=chunk, rows=rows):
                    return conv(co.lrelu32(xts[j]), wb2[j], 1, chunk, rows, xs[j], wrong)
            touches = base | {"res_first"}
            got = None if own else prov.get(("y", i, m))
            if summing:
                assert got is None or len(got) == 1, "the plan says this launch stores the MRF mean"
                touches = touches | ({"mean_mul", "mean_assoc"} if nk == 3 else set())
                rec = record(r, f"stage {i} step {2 * m + 1} mean", chunk, rows, L,
                             lambda wrong, one=one: mean_of([one(j, wrong) for j in range(nk)], wrong), touches,
                             None if own else got[0])
                outs = [rec["want"]]
                yield rec
            else:
                assert got is None or len(got) == nk
                outs = []
                for j in range(nk):
                    rec = record(r, f"stage {i} step {2 * m + 1} branch {j}", chunk, rows, L,
                                 lambda wrong, j=j, one=one: one(j, wrong), touches, None if own else got[j])
                    outs.append(rec["want"])
                    yield rec
            if own:
                prov.t[("y", i, m)] = outs
        mean_ready = stage[-1]["form"] in ("step2_sum", "pair_sum")
    r = by_where["post"][0]
    if id(r) in keep:
        wb = W["conv_post"]
        srcs = prov.get(("y", cfg.num_upsamples - 1, nd - 1))
        assert len(srcs) == (1 if mean_ready else nk)
        rows = [(0, L)]

        def restate(wrong, srcs=srcs, wb=wb, rows=rows):
            x = srcs[0] if len(srcs) == 1 else mean_of(srcs, wrong)
            return co.chain_conv_post_preact(co.lrelu32(x), wb[0], wb[1], rows)
        rec = record(r, "conv_post + tanh", None, rows, L, restate, {"mean_mul", "mean_assoc"} if len(srcs) == 3 else set(),
                     None if own else prov.get(("wav",)), kind="wav")
        yield rec
