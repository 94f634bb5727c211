// iris_hifigan_bf16.hip -- the bf16-storage generator forward (dtype IRIS_HIFIGAN_BF16) behind
// iris_hifigan_forward.  Same launch plan as the fp32 path (iris_hifigan.hip; reference
// HiFiGANModel.forward, src/iris/hifigan_pretrained.py:123-143):
//   conv_pre (reads the fp32 channels-first mel) -> per stage { upsample (u phases), 2*num_dilations
//   grouped MRF launches } -> conv_post + tanh (fp32 waveform out).
// The MRF mean is formed by the consumer of a stage while it stages its input (SURVEY.md 8d accounting L).
#include "generator_internal.h"
#include "host_parallel.h"
#include "conv_mfma_bf16.h"
#include "convt_mfma_bf16.h"
#include "mrf_pair_bf16.h"
#include "conv_mfma_f32s.h"
#include "conv_post.h"

namespace iris {

using namespace b16;

namespace {

// ---- launch descriptors: one builder per kind, shared by the forward and the single-layer entry points ----
Problem conv_problem(const void* x, const void* w, const float* bias, const uint16_t* res, uint16_t* y, int k, int dil) {
    Problem p; memset(&p, 0, sizeof(p));
    p.x = x; p.wp = w; p.bias = bias; p.res = res; p.y = y;
    p.ks = k; p.dil = dil; p.pad_left = dil * (k - 1) / 2;
    return p;
}

// nz 'same'-padding convs [B, L, C_in] -> [B, L, C_out] in one launch: a single layer, or one conv step of all MRF branches
Launch conv_launch(const Problem* p, int nz, int B, int L, int C_in, int C_out, int in_act, float slope) {
    Launch a; memset(&a, 0, sizeof(a));
    for (int j = 0; j < nz; ++j) a.p[j] = p[j];
    a.B = B; a.L_in = L; a.L_out = L; a.C_in = C_in; a.C_out = C_out; a.n_idx = L; a.out_stride = 1;
    a.in_act = in_act; a.slope = slope;
    return a;
}

// ConvTranspose1d [B, L, C_in] -> [B, L * u, C_out] of x[0] (in_act IN_ACT_NONE / IN_ACT_LRELU) or of LeakyReLU(mean of the
// n_in branch outputs x[]) (IN_ACT_MRF_LRELU): the u phases as one grid; launch_convt_bf16 takes the GEMM kernel where it applies
Launch convt_launch(const uint16_t* const* x, int n_in, int in_act, const void* w, const float* bias, uint16_t* y, int B, int L,
                    int C_in, int C_out, int k, int u, float slope) {
    const int taps = convt_taps(k, u);
    Problem p = conv_problem(x[0], w, bias, nullptr, y, taps, 1);
    p.pad_left = taps - 1;
    Launch a = conv_launch(&p, 1, B, L, C_in, C_out, in_act, slope);
    a.L_out = L * u; a.n_idx = L + taps - 1; a.out_stride = u; a.out_off = -(k - u) / 2;
    a.z_is_phase = 1;
    a.phase_wp_bytes = (unsigned)(packed_convt_phase_halfs(C_in, C_out, k, u) * 2);
    if (in_act == IN_ACT_MRF_LRELU) { a.n_mrf = n_in; for (int j = 0; j < n_in; ++j) a.xmrf[j] = x[j]; }
    return a;
}

// conv1 -> conv2 + residual of all branches in one launch (mrf_pair_bf16.h)
PairLaunch pair_launch(const PairProblem* p, int nz, int B, int L, int C, float slope) {
    PairLaunch pa; memset(&pa, 0, sizeof(pa));
    for (int j = 0; j < nz && j < kMaxGroup; ++j) pa.p[j] = p[j];
    pa.B = B; pa.L = L; pa.C = C; pa.slope = slope;
    return pa;
}

// a packed weight blob of create / prepare onto the device; *dev stays null when it fails
int upload_blob(uint16_t** dev, const std::vector<uint16_t>& host, const char* what) {
    hipError_t e = hipMalloc(dev, host.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(*dev, host.data(), host.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (*dev) (void)hipFree(*dev);
        *dev = nullptr;
        return fail(e == hipErrorOutOfMemory ? IRIS_HIFIGAN_OUT_OF_MEMORY : IRIS_HIFIGAN_HIP_ERROR,
                    "%s weight upload failed: %s", what, hipGetErrorString(e));
    }
    return IRIS_HIFIGAN_OK;
}

}  // namespace

int bf16_build_blob(iris_hifigan_handle* h, const float* weights_host) {
    // every channel count of the bf16 path must be a multiple of 8 (16-byte bf16 pieces)
    bool ok = h->cfg.num_kernels <= kMaxGroup && (h->pre.C_out % 8) == 0;
    for (const auto& st : h->stages) ok = ok && (st.C % 8) == 0;
    if (!ok) { h->blob16 = nullptr; h->blob16_halfs = 0; return IRIS_HIFIGAN_OK; }   // bf16 forward reports UNSUPPORTED
    size_t off = 0;
    for_each_layer(h, [&](ConvLayer& l) {
        if (l.kind == 2)      l.w16_halfs = 0;                      // conv_post keeps fp32 weights
        else if (l.kind == 1) l.w16_halfs = packed_convt_phase_halfs(l.C_in, l.C_out, l.k, l.u) * l.u;
        else                  l.w16_halfs = packed_conv1d_halfs(l.C_in, l.C_out, l.k);
        l.w16_off = off;
        off += (l.w16_halfs + 127) & ~(size_t)127;
    });
    h->blob16_halfs = off;
    if (h->host_only) { h->blob16 = reinterpret_cast<uint16_t*>((uintptr_t)0x20000000); return IRIS_HIFIGAN_OK; }   // offsets only
    std::vector<uint16_t> host(off, 0);
    const float* src = weights_host;
    std::vector<std::function<void()>> jobs;          // one per layer, on a few host threads (host_parallel.h)
    for_each_layer(h, [&](ConvLayer& l) {
        uint16_t* dst = host.data() + l.w16_off;
        const ConvLayer* lp = &l;
        if (l.kind == 1)      jobs.push_back([=] { pack_convt_bf16(src, lp->C_in, lp->C_out, lp->k, lp->u, dst); });
        else if (l.kind == 0) jobs.push_back([=] { pack_conv1d_bf16(src, lp->C_in, lp->C_out, lp->k, dst); });
        src += l.ref_w_floats + l.C_out;
    });
    run_host_jobs(jobs);
    return upload_blob(&h->blob16, host, "bf16");
}

// ---- split-product mode: hi/mid planes of every ResBlock conv -------------------------------------------
int f32s_build_blob(iris_hifigan_handle* h, const float* weights_host) {
    h->blob_s3 = nullptr;
    for (const auto& st : h->stages)
        if (st.C < 32 || (st.C & 31)) return IRIS_HIFIGAN_OK;          // mode unavailable for this config
    size_t off = 0;
    for (auto& st : h->stages) {
        for (size_t j = 0; j < st.c1.size(); ++j)
            for (int half = 0; half < 2; ++half)
                for (auto& l : (half == 0 ? st.c1[j] : st.c2[j])) {
                    l.ws3_off = off;
                    off += (2 * s3::packed_plane_halfs(l.C_in, l.C_out, l.k) + 127) & ~(size_t)127;
                }
    }
    if (h->host_only) { h->blob_s3 = reinterpret_cast<uint16_t*>((uintptr_t)0x30000000); return IRIS_HIFIGAN_OK; }   // offsets only
    std::vector<uint16_t> host(off, 0);
    const float* src = weights_host;
    std::vector<std::function<void()>> jobs;
    for_each_layer(h, [&](ConvLayer& l) {
        uint16_t* dst = host.data() + l.ws3_off;
        const ConvLayer* lp = &l;
        if (l.kind == 0 && &l != &h->pre) jobs.push_back([=] { s3::pack_conv1d_split(src, lp->C_in, lp->C_out, lp->k, dst); });
        src += l.ref_w_floats + l.C_out;
    });
    run_host_jobs(jobs);
    return upload_blob(&h->blob_s3, host, "split-product");
}

bool f32s_step_applicable(const iris_hifigan_handle* h, int C, int L, int nk) {
    if (!h->blob_s3 || nk > s3::kMaxGroup) return false;
    s3::Launch a; memset(&a, 0, sizeof(a));
    a.C = C; a.L = L;
    return s3::applicable(a, nk);
}

int f32s_launch_step(iris_hifigan_handle* h, const F32sStep& st, int nk, int B, int L, int C, float* sum_y, hipStream_t stream) {
    s3::Launch a; memset(&a, 0, sizeof(a));
    for (int j = 0; j < nk; ++j) {
        const ConvLayer& l = *st.layer[j];
        s3::Problem& p = a.p[j];
        p.x = st.x[j]; p.res = st.res[j]; p.y = st.y[j];
        p.wp = h->blob_s3 + l.ws3_off; p.bias = h->blob + l.b_off;
        p.ks = l.k; p.dil = l.dil; p.pad_left = l.dil * (l.k - 1) / 2;
    }
    a.B = B; a.L = L; a.C = C; a.slope = h->cfg.lrelu_slope; a.sum_y = sum_y;
    HIP_TRY(s3::launch(a, nk, stream));
    return IRIS_HIFIGAN_OK;
}

namespace {
// LeakyReLU + ConvTranspose1d of one stage as u phase launches in one grid (split products)
void fill_ups(s3::Launch& a, const ConvLayer& l, const float* x, const void* wp, const float* bias, float* y,
              int B, int L_in, float slope) {
    memset(&a, 0, sizeof(a));
    const int taps = b16::convt_taps(l.k, l.u);
    a.p[0].x = x; a.p[0].wp = wp; a.p[0].bias = bias; a.p[0].res = nullptr; a.p[0].y = y;
    a.p[0].ks = taps; a.p[0].dil = 1; a.p[0].pad_left = taps - 1;
    a.B = B; a.L = L_in * l.u; a.C = l.C_out; a.slope = slope;
    a.C_in = l.C_in; a.L_in = L_in; a.n_idx = L_in + taps - 1;
    a.out_stride = l.u; a.out_off = -(l.k - l.u) / 2; a.z_is_phase = 1;
    a.phase_bytes = (unsigned)(b16::packed_convt_phase_halfs(l.C_in, l.C_out, l.k, l.u) * 2);
    a.plane_bytes[0] = (unsigned)(s3::packed_convt_plane_halfs(l.C_in, l.C_out, l.k, l.u) * 2);
}

// ---- MRF: the launches of one stage, decided once (MrfStep / MrfStagePlan: generator_internal.h) ----
struct StageCtx16 {         // what the MRF launches of stage i share
    const iris_hifigan_handle* h;
    int i, B, L;            // L: rows per item after the stage's upsample
    uint16_t* ws;           // the workspace and its layout
    const WsLayout* w;
    const Stage& st() const { return h->stages[i]; }
    uint16_t* buf(WsBuf r, int j) const {
        return r == WS_UP ? ws + w->up : r == WS_Y ? ws + w->y[j] : r == WS_XT ? ws + w->xt[j] : nullptr;
    }
    double n_el() const { return (double)B * L * st().C; }
};

// the pair of dilation s.m in one launch; algorithmic FLOP / bytes (accounting L) are those of both steps
PairLaunch stage_pair_launch(const StageCtx16& c, const MrfStep& s, double& flops, double& bytes) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const int nk = h->cfg.num_kernels;
    PairProblem p[kMaxGroup];
    flops = 0; bytes = 2.0 * c.n_el() * nk * 5;
    for (int j = 0; j < nk; ++j) {
        const ConvLayer& l1 = st.c1[j][s.m];
        const ConvLayer& l2 = st.c2[j][s.m];
        // (a summing pair has no branch outputs: its one tensor is the launch's sum_y)
        p[j] = PairProblem{c.buf(s.x, j), h->blob16 + l1.w16_off, h->blob16 + l2.w16_off, h->blob + l1.b_off, h->blob + l2.b_off,
                           s.mean == MEAN_NONE ? c.buf(s.y, j) : nullptr, l1.k, l1.dil};
        flops += 2.0 * c.n_el() * (l1.C_in * l1.k + l2.C_in * l2.k);
        bytes += 2.0 * (double)(l1.ref_w_floats + l2.ref_w_floats) + 4.0 * (l1.C_out + l2.C_out);
    }
    return pair_launch(p, nk, c.B, c.L, st.C, h->cfg.lrelu_slope);
}

// one conv step (half 0: convs1[m], half 1: convs2[m] + residual) of all branches
Launch stage_conv_launch(const StageCtx16& c, const MrfStep& s, double& flops, double& bytes) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const int nk = h->cfg.num_kernels;
    Problem p[kMaxGroup];
    flops = 0; bytes = 2.0 * c.n_el() * nk * (s.half == 0 ? 2 : 3);
    for (int j = 0; j < nk; ++j) {
        const ConvLayer& l = s.half == 0 ? st.c1[j][s.m] : st.c2[j][s.m];
        p[j] = conv_problem(c.buf(s.x, j), h->blob16 + l.w16_off, h->blob + l.b_off, c.buf(s.res, j), c.buf(s.y, j), l.k, l.dil);
        flops += 2.0 * c.n_el() * l.C_in * l.k;
        bytes += 2.0 * (double)l.ref_w_floats + 4.0 * l.C_out;
    }
    return conv_launch(p, nk, c.B, c.L, st.C, st.C, IN_ACT_LRELU, h->cfg.lrelu_slope);
}

// The steps of stage c.i, in order, with the buffers each reads and writes.  Pure: nothing is launched or recorded here, and no
// buffer is resolved to an address (of the context it reads the handle, the stage, B, L and the layout's offsets).
MrfStagePlan plan_mrf_stage_bf16(const StageCtx16& c, const ForwardStop& stop) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const WsLayout& w = *c.w;
    const int i = c.i, nk = h->cfg.num_kernels, nd = h->cfg.num_dilations[0];
    const bool last_stage = i + 1 == (int)h->stages.size();
    MrfStagePlan pl;
    pl.n = 0;
    auto add = [&](StepKind kind, int m, int half, WsBuf x, WsBuf res, WsBuf y, StepMean mean) {
        pl.s[pl.n++] = MrfStep{kind, false, m, half, x, res, y, mean};
    };
    WsBuf cur = WS_UP;          // where the running x of every branch lies
    for (int m = 0; m < nd; ++m) {
        // C <= 128: conv1 and conv2 of the pair in ONE launch, xt stays in LDS (mrf_pair_bf16.h): two tensor passes over HBM
        // instead of five.  It cannot work in place (a block's input window overlaps its neighbours' output rows), so its
        // output alternates between the y and the xt buffer of the branch.
        const WsBuf to = cur == WS_Y ? WS_XT : WS_Y;
        double f, by;
        const PairLaunch pa = stage_pair_launch(c, MrfStep{STEP_PAIR, false, m, 1, WS_NONE, WS_NONE, WS_NONE, MEAN_NONE}, f, by);
        bool same_k = true;     // what the pair kernels take: equal kernel sizes, conv2 undilated
        for (int j = 0; j < nk; ++j) same_k = same_k && st.c1[j][m].k == st.c2[j][m].k && st.c2[j][m].dil == 1;
        // The stage's LAST pair: one block runs the three branches of its rows and stores only the MRF mean, as the operand of
        // the layer that follows (bf16, activated) or -- last stage -- as the fp32 mean conv_post takes.  Not when the caller
        // asked for a state of this stage (forward_until returns branch tensors).
        if (m == nd - 1 && stop.stage != i && same_k && nk == 3) {
            bool room = true;
            if (last_stage) {
                // The fp32 mean is twice a bf16 tensor: it goes over `up` + y[0], which must be adjacent and both free, i.e. the
                // pair reads xt[j] (so after an odd number of pairs; otherwise conv_post reads three tensors), and conv_post
                // must take one fp32 input of this shape.
                const size_t n_el = (size_t)c.n_el();
                room = w.y[0] >= w.up && (w.y[0] - w.up) * 2 >= n_el * 2 && (w.y[0] - w.up) <= n_el + 128 && cur == WS_XT;
                post::ConvPostLaunch probe; memset(&probe, 0, sizeof(probe));
                probe.B = c.B; probe.L = c.L; probe.C = st.C; probe.n_in = 1; probe.k = h->post.k;
                room = room && h->post.C_in == st.C && post::conv_post_rows_ok(probe, false);
            }
            if (room && pair_sum_applicable(pa, nk, last_stage)) {
                add(STEP_PAIR_SUM, m, 1, cur, WS_NONE, last_stage ? WS_UP : to, last_stage ? MEAN_F32_IN_UP : MEAN_IN_Y);
                continue;
            }
        }
        // (forward_until asking for the state after conv1 gets the two separate launches for that pair)
        const bool want_xt = stop.stage == i && stop.step == 2 * m;
        if (!want_xt && same_k && pair_applicable(pa, nk)) {
            add(STEP_PAIR, m, 1, cur, WS_NONE, to, MEAN_NONE);
            cur = to;
            continue;
        }
        // conv1 writes the branch's other buffer; conv2 (own rows only: in place is safe) writes back over x, or to y[j]
        // when x is the shared upsample output
        const WsBuf tmp = cur == WS_XT ? WS_Y : WS_XT, dst = cur == WS_UP ? WS_Y : cur;
        add(STEP_CONV1, m, 0, cur, WS_NONE, tmp, MEAN_NONE);
        add(STEP_CONV2, m, 1, tmp, cur, dst, MEAN_NONE);
        cur = dst;
    }
    return pl;
}
}  // namespace

int bf16_forward(iris_hifigan_handle* h, const void* mel_dev, int B, int T, const ForwardOut& out,
                 void* workspace_dev, uint64_t workspace_bytes, hipStream_t stream, const ForwardStop& stop,
                 int32_t* until_flags) {
    if (!h->blob16)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "bf16 path needs channel counts that are multiples of 8 and at most %d MRF kernels", kMaxGroup);
    {   // the bf16 kernels address one batch item's tensor with 32-bit byte offsets and have no wider fallback
        double per_item = (double)T * h->pre.C_out, L = T;
        for (const auto& st : h->stages) { L *= st.rate; if (L * st.C > per_item) per_item = L * st.C; }
        if (per_item * 2.0 >= 2147483648.0)
            return fail(IRIS_HIFIGAN_UNSUPPORTED, "bf16 path: %d frames make a single item's activations 2^31 bytes or more; "
                        "split the utterance (iris.streaming) or use fp32", T);
    }
    const WsLayout w = ws_layout(h, B, T, IRIS_HIFIGAN_BF16);
    if (workspace_bytes < w.bytes())
        return fail(IRIS_HIFIGAN_WORKSPACE_TOO_SMALL, "workspace has %llu bytes, need %llu",
                    (unsigned long long)workspace_bytes, (unsigned long long)w.bytes());
    uint16_t* ws = (uint16_t*)workspace_dev;
    const uint16_t* wb = h->blob16;
    const float* blob = h->blob;
    const float slope = h->cfg.lrelu_slope;
    const int nk = h->cfg.num_kernels;
    Prof prof{h, stream, h->profiling ? h->n_rec : 0};
    const double fB = (double)B;

    // ---- conv_pre (hifigan_pretrained.py:124): fp32 mel in, bf16 out ----
    {
        const ConvLayer& l = h->pre;
        const Problem p = conv_problem(mel_dev, wb + l.w16_off, blob + l.b_off, nullptr, ws + w.pre, l.k, 1);
        Launch a = conv_launch(&p, 1, B, T, l.C_in, l.C_out, IN_ACT_NONE, slope);
        a.x_f32_cf = 1;
        TRY(prof.begin(0, -1, 0, 2.0 * fB * T * l.C_in * l.C_out * l.k,
                       fB * T * (4.0 * l.C_in + 2.0 * l.C_out) + 2.0 * (double)l.ref_w_floats + 4.0 * l.C_out));
        HIP_TRY(launch_conv_bf16(a, 1, stream));
        TRY(prof.end());
    }

    StageCtx16 c{h, 0, B, T, ws, &w};
    StageOut prev{MEAN_NONE, WS_NONE};      // what the previous stage handed over (stage 0 reads conv_pre's output)
    for (c.i = 0; c.i < (int)h->stages.size(); ++c.i) {
        const Stage& st = c.st();
        const int L = c.L, L_out = L * st.rate;
        // ---- LeakyReLU + ConvTranspose1d (hifigan_pretrained.py:127-128) ----
        {
            const ConvLayer& l = st.up;
            const int n_in = c.i == 0 ? 1 : nk;     // (accounting L counts the reference's three branch tensors whatever was fused)
            // the branch tensors (the kernel forms their mean), or ONE tensor: conv_pre's, or the summing pair's mean, which is
            // already activated and rounded
            const bool mrf = c.i > 0 && prev.mean == MEAN_NONE;
            const uint16_t* x[IRIS_HIFIGAN_MAX_KERNELS];
            for (int j = 0; j < nk; ++j) x[j] = c.i == 0 ? ws + w.pre : c.buf(prev.buf, j);
            Launch a = convt_launch(x, nk, mrf ? IN_ACT_MRF_LRELU : (c.i == 0 ? IN_ACT_LRELU : IN_ACT_NONE),
                                    wb + l.w16_off, blob + l.b_off, ws + w.up, B, L, l.C_in, l.C_out, l.k, l.u, slope);
            TRY(prof.begin(1, c.i, 0, 2.0 * fB * L * l.C_in * l.C_out * l.k,
                           2.0 * (fB * L * l.C_in * n_in + fB * L_out * l.C_out + (double)l.ref_w_floats) + 4.0 * l.C_out));
            HIP_TRY(launch_convt_bf16(a, l.k, l.u, stream));      // one GEMM launch (convt_mfma_bf16.h) where it applies
            TRY(prof.end());
        }
        // ---- MRF: num_kernels ResBlocks advance together (hifigan_pretrained.py:64-71,131-136) ----
        c.L = L_out;
        const MrfStagePlan plan = plan_mrf_stage_bf16(c, stop);
        for (int n = 0; n < plan.n; ++n) {
            const MrfStep& s = plan.s[n];
            double flops, bytes;
            if (s.kind == STEP_PAIR || s.kind == STEP_PAIR_SUM) {
                PairLaunch pa = stage_pair_launch(c, s, flops, bytes);
                TRY(prof.begin(2, c.i, 2 * s.m + 1, flops, bytes));      // the record carries the index of the pair's second step
                if (s.kind == STEP_PAIR_SUM) HIP_TRY(launch_pair_bf16_sum(pa, c.buf(s.y, 0), s.mean == MEAN_F32_IN_UP, stream));
                else                         HIP_TRY(launch_pair_bf16(pa, nk, stream));
            } else {
                Launch a = stage_conv_launch(c, s, flops, bytes);
                TRY(prof.begin(2, c.i, 2 * s.m + s.half, flops, bytes));
                HIP_TRY(launch_conv_bf16(a, nk, stream));
            }
            TRY(prof.end());
            if (stop.stage == c.i && stop.step == 2 * s.m + s.half) {
                // where the running x lies now: conv1 left it where it was (and xt in the branch's other buffer)
                if (until_flags) *until_flags = (s.kind == STEP_CONV1 ? s.x : s.y) == WS_XT ? IRIS_HIFIGAN_UNTIL_X_IN_XT : 0;
                return prof.finish();
            }
        }
        prev = plan.out();
    }

    // ---- LeakyReLU + conv_post + tanh (hifigan_pretrained.py:139-141): bf16 in, fp32 waveform (or what `out` asks for) out ----
    {
        const ConvLayer& l = h->post;
        const int L = c.L;
        TRY(prof.begin(3, -1, 0, 2.0 * fB * L * l.C_in * l.k,
                       2.0 * fB * L * l.C_in * nk + 4.0 * (fB * L + (double)l.ref_w_floats + 1)));
        auto fill = [&](auto& a) {        // the fields the two descriptors (conv_post.h, conv_mfma_bf16.h) share
            memset(&a, 0, sizeof(a));
            for (int j = 0; j < nk; ++j) a.x[j] = c.buf(prev.buf, j);
            a.n_in = nk; a.inv_n = 1.0f / (float)nk;
            a.w = blob + l.w_off; a.bias = blob + l.b_off; out.to_post(a);
            a.B = B; a.L = L; a.C = l.C_in; a.k = l.k; a.slope = slope;
        };
        post::ConvPostLaunch ar; fill(ar);
        if (prev.mean == MEAN_F32_IN_UP) {
            // the summing pair left the fp32 mean in `up`: conv_post as in the fp32 path (one fp32 input, LeakyReLU in fp32)
            ar.n_in = 1;
            if (!post::conv_post_rows_ok(ar, false)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "conv_post: shape not supported behind the summing pair");
            HIP_TRY(post::launch_conv_post_t<false>(ar, stream));
        } else if (post::conv_post_rows_ok(ar, true)) {
            // 16-byte staging, batch folded into the grid (conv_post.h); same arithmetic as the kernel below, which takes
            // the shapes this one cannot (other channel counts; a single item of 2^31 bytes or more)
            HIP_TRY(post::launch_conv_post_t<true>(ar, stream));
        } else {
            PostLaunch a; fill(a);
            HIP_TRY(launch_conv_post_bf16(a, stream));
        }
        TRY(prof.end());
    }
    TRY(prof.finish());
    return IRIS_HIFIGAN_OK;
}

}  // namespace iris

// ------------------------------------------------------------------------------------------------
// single-layer entry points (parity tests of the bf16 kernel)
// ------------------------------------------------------------------------------------------------
namespace {
using namespace iris;
using namespace iris::b16;

// Packs and uploads one branch's pair weights (the two pair entry points) and points `p` at them.
struct PairWeights { DevBuf w1, w2, b1, b2; };
int upload_pair_weights(PairWeights& d, PairProblem& p, const float* w1, const float* b1, const float* w2, const float* b2, int C) {
    std::vector<uint16_t> packed(packed_conv1d_halfs(C, C, p.ks));
    pack_conv1d_bf16(w1, C, C, p.ks, packed.data());
    HIP_TRY(d.w1.upload(packed));
    pack_conv1d_bf16(w2, C, C, p.ks, packed.data());
    HIP_TRY(d.w2.upload(packed));
    HIP_TRY(d.b1.upload(b1, sizeof(float) * C));
    HIP_TRY(d.b2.upload(b2, sizeof(float) * C));
    p.w1 = d.w1.p; p.w2 = d.w2.p; p.b1 = d.b1.f32(); p.b2 = d.b2.f32();
    return IRIS_HIFIGAN_OK;
}

// The per-branch argument checks of the two pair entry points, and their problems without weights.  y_dev: the branch
// outputs; null for the summing pair, which has none.
int pair_problems(PairProblem* p, int nz, const void* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                  const float* const* w2_host, const float* const* b2_host, void* const* y_dev, const int32_t* k, const int32_t* dil) {
    for (int j = 0; j < nz; ++j) {
        if (!x_dev[j] || !w1_host[j] || !b1_host[j] || !w2_host[j] || !b2_host[j] || (y_dev && !y_dev[j]))
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL branch argument");
        if (k[j] < 1 || !(k[j] & 1) || dil[j] < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad kernel size / dilation");
        p[j] = PairProblem{(const uint16_t*)x_dev[j], nullptr, nullptr, nullptr, nullptr, y_dev ? (uint16_t*)y_dev[j] : nullptr, k[j], dil[j]};
    }
    return IRIS_HIFIGAN_OK;
}
}  // namespace

extern "C" {

int32_t iris_hifigan_op_conv1d_bf16(const void* x_dev, const float* w_host, const float* bias_host,
                                    const void* res_dev, void* y_dev, int32_t B, int32_t L, int32_t C_in,
                                    int32_t C_out, int32_t k, int32_t dilation, int32_t in_act, float slope,
                                    void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || C_out < 1 || k < 1 || !(k & 1) || dilation < 1 || B > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv1d shape");
    if ((C_in & 7) || (C_out & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "bf16 conv needs C_in %% 8 == 0 and C_out %% 4 == 0");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<uint16_t> packed(packed_conv1d_halfs(C_in, C_out, k));
    pack_conv1d_bf16(w_host, C_in, C_out, k, packed.data());
    DevBuf wb, bb;
    HIP_TRY(wb.upload(packed));
    HIP_TRY(bb.upload(bias_host, sizeof(float) * C_out));
    const Problem p = conv_problem(x_dev, wb.p, bb.f32(), (const uint16_t*)res_dev, (uint16_t*)y_dev, k, dilation);
    Launch a = conv_launch(&p, 1, B, L, C_in, C_out, in_act ? IN_ACT_LRELU : IN_ACT_NONE, slope);
    HIP_TRY(launch_conv_bf16(a, 1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_mrf_pair_bf16(const void* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                      const float* const* w2_host, const float* const* b2_host, void* const* y_dev,
                                      int32_t n_branches, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                      float slope, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w1_host || !b1_host || !w2_host || !b2_host || !y_dev || !k || !dil)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (n_branches < 1 || n_branches > kMaxGroup || B < 1 || L < 1 || C < 1 || B > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad mrf_pair shape");
    hipStream_t stream = (hipStream_t)stream_;
    PairProblem p[kMaxGroup];
    TRY(pair_problems(p, n_branches, x_dev, w1_host, b1_host, w2_host, b2_host, y_dev, k, dil));
    PairLaunch a = pair_launch(p, n_branches, B, L, C, slope);
    if (!pair_applicable(a, n_branches))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the fused pair kernel takes C = 32, 64 or 128 and windows up to 64 KB");
    PairWeights wts[kMaxGroup];
    for (int j = 0; j < n_branches; ++j) TRY(upload_pair_weights(wts[j], a.p[j], w1_host[j], b1_host[j], w2_host[j], b2_host[j], C));
    HIP_TRY(launch_pair_bf16(a, n_branches, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_mrf_pair_mean_bf16(const void* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                           const float* const* w2_host, const float* const* b2_host, void* mean_dev,
                                           int32_t mean_f32, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                           float slope, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w1_host || !b1_host || !w2_host || !b2_host || !mean_dev || !k || !dil)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C < 1 || B > 65535) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad mrf_pair shape");
    const int nz = 3;
    hipStream_t stream = (hipStream_t)stream_;
    PairProblem p[kMaxGroup];
    TRY(pair_problems(p, nz, x_dev, w1_host, b1_host, w2_host, b2_host, nullptr, k, dil));
    for (int j = 0; j < nz; ++j)
        if (x_dev[j] == mean_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the mean must not overwrite an input");
    PairLaunch a = pair_launch(p, nz, B, L, C, slope);
    if (!pair_sum_applicable(a, nz, mean_f32 != 0))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the summing pair kernel takes C = 32 or 64, three branches and windows up to 64 KB");
    PairWeights wts[kMaxGroup];
    for (int j = 0; j < nz; ++j) TRY(upload_pair_weights(wts[j], a.p[j], w1_host[j], b1_host[j], w2_host[j], b2_host[j], C));
    HIP_TRY(launch_pair_bf16_sum(a, mean_dev, mean_f32 != 0, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_conv1d_f32s(const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev,
                                    float* y_dev, int32_t B, int32_t L, int32_t C, int32_t k, int32_t dilation, float slope,
                                    void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C < 1 || k < 1 || !(k & 1) || dilation < 1 || B > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv1d shape");
    s3::Launch a; memset(&a, 0, sizeof(a));
    a.B = B; a.L = L; a.C = C; a.slope = slope;
    if (!s3::applicable(a, 1)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "split-product conv needs C %% 32 == 0");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<uint16_t> packed(2 * s3::packed_plane_halfs(C, C, k));
    s3::pack_conv1d_split(w_host, C, C, k, packed.data());
    DevBuf wb, bb;
    HIP_TRY(wb.upload(packed));
    HIP_TRY(bb.upload(bias_host, sizeof(float) * C));
    a.p[0].x = x_dev; a.p[0].wp = wb.p; a.p[0].bias = bb.f32(); a.p[0].res = res_dev; a.p[0].y = y_dev;
    a.p[0].ks = k; a.p[0].dil = dilation; a.p[0].pad_left = dilation * (k - 1) / 2;
    HIP_TRY(s3::launch(a, 1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_conv_transpose1d_f32s(const float* x_dev, const float* w_host, const float* bias_host, float* y_dev,
                                              int32_t B, int32_t L, int32_t C_in, int32_t C_out, int32_t k, int32_t u,
                                              float slope, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || C_out < 1 || u < 1 || k < u || ((k - u) & 1) || B > 65535 || u > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv_transpose1d shape");
    ConvLayer l; l.kind = 1; l.C_in = C_in; l.C_out = C_out; l.k = k; l.u = u;
    s3::Launch a;
    fill_ups(a, l, nullptr, nullptr, nullptr, nullptr, B, L, slope);
    if (!s3::applicable(a, u)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "split-product upsample: channel counts not supported");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<uint16_t> packed(2 * s3::packed_convt_plane_halfs(C_in, C_out, k, u));
    s3::pack_convt_split(w_host, C_in, C_out, k, u, packed.data());
    DevBuf wb, bb;
    HIP_TRY(wb.upload(packed));
    HIP_TRY(bb.upload(bias_host, sizeof(float) * C_out));
    fill_ups(a, l, x_dev, wb.p, bb.f32(), y_dev, B, L, slope);
    HIP_TRY(s3::launch(a, u, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_conv_transpose1d_bf16(const void* x_dev, const float* w_host, const float* bias_host,
                                              void* y_dev, int32_t B, int32_t L, int32_t C_in, int32_t C_out,
                                              int32_t k, int32_t u, int32_t in_act, float slope, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || C_out < 1 || u < 1 || k < u || ((k - u) & 1) || B > 65535 || u > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv_transpose1d shape");
    if ((C_in & 7) || (C_out & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "bf16 conv needs C_in %% 8 == 0 and C_out %% 4 == 0");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t phase_halfs = packed_convt_phase_halfs(C_in, C_out, k, u);
    std::vector<uint16_t> packed(phase_halfs * u);
    pack_convt_bf16(w_host, C_in, C_out, k, u, packed.data());
    DevBuf wb, bb;
    HIP_TRY(wb.upload(packed));
    HIP_TRY(bb.upload(bias_host, sizeof(float) * C_out));
    const uint16_t* const x = (const uint16_t*)x_dev;
    Launch a = convt_launch(&x, 1, in_act ? IN_ACT_LRELU : IN_ACT_NONE, wb.p, bb.f32(), (uint16_t*)y_dev, B, L, C_in, C_out, k, u, slope);
    HIP_TRY(launch_convt_bf16(a, k, u, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

}  // extern "C"
