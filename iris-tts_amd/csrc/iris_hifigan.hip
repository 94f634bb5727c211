// iris_hifigan.hip -- C-ABI (include/iris_hifigan.h) over the gfx950 kernels.
//
// Generator dataflow follows HiFiGANModel.forward (reference src/iris/hifigan_pretrained.py:123-143,
// Keras twin src/iris/vocoder.py:103-130):
//   conv_pre -> for each stage { LeakyReLU -> ConvTranspose1d -> MRF(3 ResBlocks) / 3 } -> LeakyReLU
//   -> conv_post -> tanh.
// Launches of one forward:
//   1            conv_pre, reading the channels-first mel directly
//   per stage:   1 upsample launch (one GEMM, or all u phases as blockIdx.z; input = LeakyReLU of conv_pre's output, of the
//                MRF mean the previous stage stored, or of the mean of its branch outputs formed in the LDS staging)
//                the MRF steps plan_mrf_stage lists: per dilation a fused conv pair, or convs1[m] and convs2[m] + residual
//                as two grouped launches of ALL branches; the stage's last launch stores only the MRF mean where a block
//                holds all branch outputs of its tile (summing forms)
//   1            conv_post + tanh, reading that mean or the last stage's branch outputs.
// Where no summing form runs, the MRF sum and the division by num_kernels (hifigan_pretrained.py:131-137) are never
// materialised: the consumer of a stage reads the branch outputs and forms ((b0+b1)+b2)/3 itself.  DESIGN.md sections 2, 5.
// Host structure: entry point (own argument checks) -> run_forward (device, weight packing, passes) -> forward_f32 /
// bf16_forward; launch descriptors come from one builder per kind, shared with the single-layer entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <new>
#include <utility>
#include <vector>

#include "generator_internal.h"
#include "stage_host.h"
#include "host_parallel.h"
#include "conv_mfma_f32.h"
#include "mrf_conv_mfma_f32.h"
#include "convt_mfma_f32.h"
#include "mrf_small_f32.h"
#include "mrf_pair_f32.h"
#include "mrf_pair_f32_pf.h"
#include "conv_post.h"
#include "postnet.h"
#include "resample.h"

using namespace iris;

namespace iris {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace iris

namespace {

int validate(const iris_hifigan_config* c) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->in_channels < 1 || c->upsample_initial_channel < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "channel counts must be positive");
    if (c->num_upsamples < 1 || c->num_upsamples > IRIS_HIFIGAN_MAX_STAGES)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "num_upsamples %d out of range", c->num_upsamples);
    if (c->num_kernels < 1 || c->num_kernels > IRIS_HIFIGAN_MAX_KERNELS)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "num_kernels %d out of range", c->num_kernels);
    if ((c->upsample_initial_channel >> c->num_upsamples) < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "upsample_initial_channel too small for %d stages",
                    c->num_upsamples);
    for (int i = 0; i < c->num_upsamples; ++i) {
        const int u = c->upsample_rates[i], k = c->upsample_kernel_sizes[i];
        if (u < 1 || k < u || ((k - u) & 1))
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT,
                        "stage %d: need kernel >= rate and (kernel - rate) even, got k=%d u=%d", i, k, u);
        if (u > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "upsample rate too large");
    }
    for (int j = 0; j < c->num_kernels; ++j) {
        const int k = c->resblock_kernel_sizes[j];
        if (k < 1 || !(k & 1))
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "resblock kernel size %d must be odd", k);
        if (c->num_dilations[j] < 1 || c->num_dilations[j] > IRIS_HIFIGAN_MAX_DILATIONS)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "num_dilations[%d] out of range", j);
        if (c->num_dilations[j] != c->num_dilations[0])
            return fail(IRIS_HIFIGAN_UNSUPPORTED, "MRF branches must have the same number of dilations");
        for (int m = 0; m < c->num_dilations[j]; ++m)
            if (c->resblock_dilations[j][m] < 1)
                return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "dilations must be >= 1");
    }
    if (c->pre_kernel_size < 1 || !(c->pre_kernel_size & 1) || c->post_kernel_size < 1 ||
        !(c->post_kernel_size & 1))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "pre/post kernel sizes must be odd");
    return IRIS_HIFIGAN_OK;
}

void build_layers(iris_hifigan_handle* h) {
    const iris_hifigan_config& c = h->cfg;
    h->pre.kind = 0;
    h->pre.C_in = c.in_channels; h->pre.C_out = c.upsample_initial_channel; h->pre.k = c.pre_kernel_size;
    h->stages.resize(c.num_upsamples);
    h->hop = 1;
    int ch = c.upsample_initial_channel;
    for (int i = 0; i < c.num_upsamples; ++i) {
        Stage& st = h->stages[i];
        st.up.kind = 1;
        st.up.C_in = ch; st.up.C_out = ch / 2; st.up.k = c.upsample_kernel_sizes[i];
        st.up.u = c.upsample_rates[i];
        st.rate = st.up.u;
        ch /= 2;
        st.C = ch;
        h->hop *= st.rate;
        st.c1.resize(c.num_kernels); st.c2.resize(c.num_kernels);
        for (int j = 0; j < c.num_kernels; ++j) {
            for (int m = 0; m < c.num_dilations[j]; ++m) {
                ConvLayer l1; l1.C_in = ch; l1.C_out = ch; l1.k = c.resblock_kernel_sizes[j];
                l1.dil = c.resblock_dilations[j][m];
                ConvLayer l2 = l1; l2.dil = 1;
                st.c1[j].push_back(l1); st.c2[j].push_back(l2);
            }
        }
    }
    h->post.kind = 2;
    h->post.C_in = ch; h->post.C_out = 1; h->post.k = c.post_kernel_size;
    // device blob layout
    size_t off = 0;
    for_each_layer(h, [&](ConvLayer& l) {
        l.ref_w_floats = (size_t)l.C_in * l.C_out * l.k;
        if (l.kind == 2)      l.w_floats = (size_t)l.k * l.C_in;
        else if (l.kind == 1) l.w_floats = packed_convt_phase_floats(l.C_in, l.C_out, l.k, l.u) * l.u;
        else                  l.w_floats = packed_conv1d_floats(l.C_in, l.C_out, l.k);
    });
    for_each_layer(h, [&](ConvLayer& l) {
        l.w_off = off; off += (l.w_floats + 3) & ~(size_t)3;
        l.b_off = off; off += ((size_t)l.C_out + 3) & ~(size_t)3;
    });
    h->blob_floats = off;
}

uint64_t ref_weight_count(iris_hifigan_handle* h) {
    uint64_t n = 0;
    for_each_layer(h, [&](ConvLayer& l) { n += l.ref_w_floats + l.C_out; });
    return n;
}

// ---- launch descriptors: one builder per kind, shared by the forwards and the single-layer entry points ----
ConvProblem conv_problem(const float* x, const float* w, const float* bias, const float* res, float* y, int k, int dil,
                         const float* w16 = nullptr) {
    ConvProblem p; memset(&p, 0, sizeof(p));
    p.x = x; p.wp = (const f32x4*)w; p.bias = bias; p.res = res; p.y = y;
    p.ks = k; p.dil = dil; p.pad_left = dil * (k - 1) / 2;
    p.wp16 = (const f32x4*)w16;
    return p;
}

// nz 'same'-padding convs [B, L, C_in] -> [B, L, C_out] in one launch: a single layer (conv_pre, PostNet), or one conv step
// of all MRF branches.  `lengths` / `row_scale`: the ragged forward's bounds (ConvLaunch).
ConvLaunch conv_launch(const ConvProblem* p, int nz, int B, int L, int C_in, int C_out, int in_act, float slope,
                       const int32_t* lengths = nullptr, int row_scale = 1) {
    ConvLaunch a; memset(&a, 0, sizeof(a));
    for (int j = 0; j < nz; ++j) a.p[j] = p[j];
    a.B = B; a.L_in = L; a.L_out = L; a.C_in = C_in; a.C_out = C_out; a.n_idx = L; a.out_stride = 1;
    a.in_act = in_act; a.slope = slope;
    a.lengths = lengths; a.row_scale = row_scale;
    return a;
}

// The grouped step `a` as the MRF kernel's summing launch, which forms mean_j(y_j) itself: it processes p[2], p[1], p[0];
// passing the branches reversed makes that resblock 0, 1, 2 -- the reference's summation order
// (hifigan_pretrained.py:131-137).
void to_summing(ConvLaunch& a, float* mean, int nk) {
    std::swap(a.p[0], a.p[2]);
    a.sum_y = mean; a.sum_div = (float)nk;
}

// ConvTranspose1d [B, L, C_in] -> [B, L * u, C_out] of x[0] (in_act IN_ACT_NONE / IN_ACT_LRELU) or of LeakyReLU(mean of the
// n_in branch outputs x[]) (IN_ACT_MRF_LRELU), and which kernel takes it.
struct ConvtF32 { bool gemm; ConvtLaunch c; ConvLaunch a; int k, u; };

ConvtF32 convt_launch(const float* const* x, int n_in, int in_act, const float* w, const float* bias, float* y, int B, int L,
                      int C_in, int C_out, int k, int u, float slope, const int32_t* lengths = nullptr, int row_scale = 1) {
    ConvtF32 d; memset(&d, 0, sizeof(d));
    d.k = k; d.u = u;
    const bool mrf = in_act == IN_ACT_MRF_LRELU;
    // (split-product mode keeps the upsamplers in fp32: split as well, they grew the worst observed waveform error
    //  from 2e-5 to 5e-5 -- still inside 1e-4, but the mode keeps the wider margin)
    d.gemm = (in_act == IN_ACT_LRELU || (mrf && n_in == 3)) && convt_gemm_applicable(C_in, C_out, k, u, L, L * u, slope);
    if (d.gemm) {
        // the whole layer as ONE GEMM [L + 1, 2 C_in] x [2 C_in, u C_out] (convt_mfma_f32.h), bit for bit the polyphase
        // launches below; its input is one tensor (conv_pre's output, or the MRF mean the previous stage's last step
        // stored) or the previous stage's three branch outputs, whose mean is then formed while the window is staged
        ConvtLaunch& c = d.c;
        c.x = x[0]; c.wp = (const f32x4*)w; c.bias = bias; c.y = y;
        if (mrf) { c.x1 = x[1]; c.x2 = x[2]; }
        c.B = B; c.L_in = L; c.L_out = L * u; c.C_in = C_in; c.C_out = C_out; c.u = u; c.slope = slope;
        c.lengths = lengths; c.row_scale = row_scale;
        return d;
    }
    // all u phases in one grid (blockIdx.z), each a conv of `taps` taps over the input
    const int taps = convt_taps(k, u);
    ConvProblem p = conv_problem(x[0], w, bias, nullptr, y, taps, 1);
    p.pad_left = taps - 1;
    ConvLaunch& a = d.a;
    a = conv_launch(&p, 1, B, L, C_in, C_out, in_act, slope, lengths, row_scale);
    a.L_out = L * u; a.n_idx = L + taps - 1; a.out_stride = u; a.out_off = -(k - u) / 2;
    a.z_is_phase = 1;
    a.phase_wp_stride = (int64_t)(packed_convt_phase_floats(C_in, C_out, k, u) / 4);
    if (mrf) { a.n_mrf = n_in; for (int j = 0; j < n_in; ++j) a.xmrf[j] = x[j]; }
    return d;
}

hipError_t launch_convt(ConvtF32& d, hipStream_t stream) {
    return d.gemm ? launch_convt_gemm(d.c, d.k, stream) : launch_conv(d.a, d.u, stream);
}

// conv1 -> conv2 + residual of all branches in one launch (mrf_pair_f32.h)
PairLaunchF32 pair_launch(const PairProblemF32* p, int nk, int B, int L, int C, float slope, const int32_t* lengths = nullptr,
                          int row_scale = 1) {
    PairLaunchF32 pa; memset(&pa, 0, sizeof(pa));
    for (int j = 0; j < nk && j < kMaxGroup; ++j) pa.p[j] = p[j];
    pa.B = B; pa.L = L; pa.C = C; pa.slope = slope;
    pa.lengths = lengths; pa.row_scale = row_scale;
    return pa;
}

// second packing of the ResBlock conv weights for the small-problem kernel (mrf_small_f32.h): float offsets of each layer's
// 16 x 16 fragments in blob_w16 (layers whose channel counts are not multiples of 16 keep -1: they never take that kernel)
size_t assign_w16_offsets(iris_hifigan_handle* h) {
    size_t off16 = 0;
    for (auto& st : h->stages)
        for (size_t j = 0; j < st.c1.size(); ++j)
            for (int half = 0; half < 2; ++half)
                for (auto& l : (half == 0 ? st.c1[j] : st.c2[j]))
                    if ((l.C_in & 15) == 0 && (l.C_out & 15) == 0) { l.w16f_off = off16; off16 += packed16_conv1d_floats(l.C_in, l.C_out, l.k); }
    return off16;
}


}  // namespace

namespace iris {
// Batch items one pass of a forward processes.  Batch items are independent, so a forward of a large batch runs as
// consecutive passes over sub-batches that share ONE workspace: the workspace is bounded by kPassFrames mel frames
// (229 KB per frame in fp32: 15 GB) instead of growing with the batch (58 GB at 256 x 1000 frames), at no cost in
// throughput -- the kernels are at their large-batch efficiency from ~16,000 frames on.
int pass_items(int B, int T) {
    if (B <= 1 || T <= 0) return B;
    const long long fit = kPassFrames / T;
    return (int)(fit < 1 ? 1 : (fit < B ? fit : B));
}
}  // namespace iris

extern "C" {

int32_t iris_hifigan_abi_version(void) { return IRIS_HIFIGAN_ABI_VERSION; }
const char* iris_hifigan_last_error(void) { return iris::g_err; }

int32_t iris_hifigan_weight_count(const iris_hifigan_config* cfg, uint64_t* count) {
    IRIS_ABI_BEGIN
    TRY(validate(cfg));
    if (!count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "count is NULL");
    iris_hifigan_handle tmp;
    tmp.cfg = *cfg;
    build_layers(&tmp);
    *count = ref_weight_count(&tmp);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_create(const iris_hifigan_config* cfg, const float* weights_host,
                            uint64_t n_weights, iris_hifigan_handle** out) {
    IRIS_ABI_BEGIN
    TRY(validate(cfg));
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    struct Owner {                      // frees a half-built generator on every early return, exceptions included
        iris_hifigan_handle* h = nullptr;
        ~Owner() { if (h) (void)iris_hifigan_destroy(h); }
    } owner;
    iris_hifigan_handle* h = new (std::nothrow) iris_hifigan_handle;
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    owner.h = h;
    h->cfg = *cfg;
    build_layers(h);
    const uint64_t expect = ref_weight_count(h);
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, config needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    // Repacking: the MFMA fragment order of the persistent kernels (32 x 32 tiles) and, for the ResBlock convs, the 16 x 16
    // fragments of the short-input kernel (mrf_small_f32.h) -- two gathers over 13.9 M weights.  (layer, tap) pieces write
    // disjoint ranges, so they run on a few host threads (host_parallel.h): the reference's caller loads a model to vocode ONE
    // utterance (scripts/synthesize.py:197-198), so this is time that caller waits for.
    std::vector<float> host(h->blob_floats, 0.f);
    const size_t off16 = assign_w16_offsets(h);
    std::vector<float> host16(off16);
    std::vector<std::function<void()>> jobs;
    {
        const float* src = weights_host;
        for_each_layer(h, [&](ConvLayer& l) {
            float* dst = host.data() + l.w_off;
            const ConvLayer* lp = &l;
            if (l.kind == 2) {
                jobs.push_back([=] {            // [1][C][k] -> [k][C]
                    for (int c = 0; c < lp->C_in; ++c)
                        for (int kap = 0; kap < lp->k; ++kap) dst[(size_t)kap * lp->C_in + c] = src[(size_t)c * lp->k + kap];
                });
            } else if (l.kind == 1) {
                for (int ph = 0; ph < l.u; ++ph)
                    jobs.push_back([=] { pack_convt_weights(src, lp->C_in, lp->C_out, lp->k, lp->u, dst, ph, ph + 1); });
            } else {
                for (int kap = 0; kap < l.k; ++kap)
                    jobs.push_back([=] { pack_conv1d_weights(src, lp->C_in, lp->C_out, lp->k, dst, kap, kap + 1); });
                if (l.w16f_off != (size_t)-1) {
                    float* dst16 = host16.data() + l.w16f_off;
                    for (int kap = 0; kap < l.k; ++kap)
                        jobs.push_back([=] { pack_conv1d_weights16(src, lp->C_in, lp->C_out, lp->k, dst16, kap, kap + 1); });
                }
            }
            src += l.ref_w_floats;
            memcpy(host.data() + l.b_off, src, sizeof(float) * l.C_out);
            src += l.C_out;
        });
    }
    // the reference-layout weights stay on the host for the packings of the other dtypes (bf16 fragments, split-bf16 planes),
    // which are built by iris_hifigan_prepare / the first forward of that dtype; iris_hifigan_release_host_weights drops them
    jobs.push_back([=] { h->ref_weights.assign(weights_host, weights_host + n_weights); });
    run_host_jobs(jobs);
    // the generator lives on the device that is current now; every later call runs under that device
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->blob, h->blob_floats * sizeof(float));
    if (e == hipSuccess)
        e = hipMemcpy(h->blob, host.data(), h->blob_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && off16 > 0) e = hipMalloc(&h->blob_w16, off16 * sizeof(float));
    if (e == hipSuccess && off16 > 0)
        e = hipMemcpy(h->blob_w16, host16.data(), off16 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? IRIS_HIFIGAN_OUT_OF_MEMORY : IRIS_HIFIGAN_HIP_ERROR,
                    "weight upload failed: %s", hipGetErrorString(e));
    if (hipMalloc(&h->tile_counters, kTileCounterWords * sizeof(unsigned)) != hipSuccess) h->tile_counters = nullptr;   // optional
    owner.h = nullptr;
    *out = h;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_destroy(iris_hifigan_handle* h) {
    if (!h) return IRIS_HIFIGAN_OK;
    if (h->host_only) { delete h; return IRIS_HIFIGAN_OK; }
    DeviceGuard guard(h->device);       // the allocations belong to the handle's device, whatever is current now
    for (hipEvent_t ev : h->ev) (void)hipEventDestroy(ev);
    if (h->blob) (void)hipFree(h->blob);
    if (h->blob16) (void)hipFree(h->blob16);
    if (h->blob_s3) (void)hipFree(h->blob_s3);
    if (h->blob_w16) (void)hipFree(h->blob_w16);
    if (h->tile_counters) (void)hipFree(h->tile_counters);
    delete h;
    return IRIS_HIFIGAN_OK;
}

}  // extern "C"

namespace {

// Builds the weight packing `dtype` needs beyond what create uploaded (bf16 fragments / split-bf16 planes), once.
// Synchronous (packs on the host, allocates, uploads).  A packing counts as built only when its build SUCCEEDED or the
// configuration genuinely cannot have it (then the forward of that dtype reports UNSUPPORTED): a transient failure -- out
// of memory -- is reported and retried by the next call.  `stream` non-null-checked: inside a stream capture nothing may
// allocate or synchronise, so a forward that still needs a packing there is refused with NOT_PREPARED.
int ensure_prepared(iris_hifigan_handle* h, int32_t dtype, hipStream_t stream, bool from_forward) {
    const bool want_bf16 = dtype == IRIS_HIFIGAN_BF16 && !h->built_bf16;
    const bool want_s3 = dtype == IRIS_HIFIGAN_F32_SPLIT && !h->built_s3;
    if (!want_bf16 && !want_s3) return IRIS_HIFIGAN_OK;
    if (from_forward) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(IRIS_HIFIGAN_NOT_PREPARED, "the weight packing of dtype %d is not built yet and the stream is being captured: "
                        "call iris_hifigan_prepare(h, %d) before capturing forwards of this dtype", dtype, dtype);
    }
    if (h->ref_weights.empty())
        return fail(IRIS_HIFIGAN_NOT_PREPARED, "the host copy of the weights was released (iris_hifigan_release_host_weights) before "
                    "dtype %d was prepared", dtype);
    if (want_bf16) { TRY(bf16_build_blob(h, h->ref_weights.data())); h->built_bf16 = true; }
    if (want_s3)   { TRY(f32s_build_blob(h, h->ref_weights.data())); h->built_s3 = true; }
    if (h->built_bf16 && h->built_s3) std::vector<float>().swap(h->ref_weights);   // every packing exists
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_hifigan_prepare(iris_hifigan_handle* h, int32_t dtype) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (dtype != IRIS_HIFIGAN_F32 && dtype != IRIS_HIFIGAN_BF16 && dtype != IRIS_HIFIGAN_F32_SPLIT)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "dtype %d not supported", dtype);
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    return ensure_prepared(h, dtype, nullptr, false);
    IRIS_ABI_END
}

int32_t iris_hifigan_release_host_weights(iris_hifigan_handle* h) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    std::vector<float>().swap(h->ref_weights);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_hifigan_hop_length(const iris_hifigan_handle* h, int32_t* hop) {
    if (!h || !hop) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    *hop = h->hop;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_hifigan_workspace_bytes(const iris_hifigan_handle* h, int32_t B, int32_t T,
                                     int32_t dtype, uint64_t* bytes) {
    if (!h || !bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (dtype != IRIS_HIFIGAN_F32 && dtype != IRIS_HIFIGAN_BF16 && dtype != IRIS_HIFIGAN_F32_SPLIT)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "dtype %d not supported", dtype);
    *bytes = ws_layout(h, pass_items(B, T), T, dtype).bytes();   // a large batch runs as passes over sub-batches sharing the workspace
    return IRIS_HIFIGAN_OK;
}

int32_t iris_hifigan_set_profiling(iris_hifigan_handle* h, int32_t enabled) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    h->profiling = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
    h->profiling_paused = 0;
    h->n_rec = 0;
    h->n_ev = 0;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_hifigan_pause_profiling(iris_hifigan_handle* h, int32_t paused) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    h->profiling_paused = paused != 0;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_hifigan_read_profile(iris_hifigan_handle* h, iris_hifigan_launch_record* out,
                                  int32_t capacity, int32_t* n_launches) {
    IRIS_ABI_BEGIN
    if (!h || !n_launches) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    *n_launches = h->n_rec;
    for (int i = 0; i < h->n_rec; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->rec_ev[i].first, h->rec_ev[i].second));
        h->recs[i].ms = ms;
        if (out && i < capacity) out[i] = h->recs[i];
    }
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

}  // extern "C"

namespace {

// ---- MRF: the launches of one stage, decided once (MrfStep / MrfStagePlan: generator_internal.h) ----
struct StageCtx {           // what the MRF launches of stage i share in one pass
    const iris_hifigan_handle* h;
    int i, B, L;            // L: rows per item after the stage's upsample
    float *up, *y[IRIS_HIFIGAN_MAX_KERNELS], *xt[IRIS_HIFIGAN_MAX_KERNELS];
    const int32_t* lengths; int row_scale;
    bool dyn_tiles;
    const Stage& st() const { return h->stages[i]; }
    float* buf(WsBuf r, int j) const { return r == WS_UP ? up : r == WS_Y ? y[j] : r == WS_XT ? xt[j] : nullptr; }
    double n_el() const { return (double)B * L * st().C; }
};

// one conv step (half 0: convs1[m], half 1: convs2[m] + residual) of all branches, separate launches
ConvLaunch step_launch(const StageCtx& c, const MrfStep& s, double& flops, double& wbytes) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const int nk = h->cfg.num_kernels;
    ConvProblem p[kMaxGroup];
    flops = 0; wbytes = 0;
    for (int j = 0; j < nk; ++j) {
        const ConvLayer& l = s.half == 0 ? st.c1[j][s.m] : st.c2[j][s.m];
        p[j] = conv_problem(c.buf(s.x, j), h->blob + l.w_off, h->blob + l.b_off, c.buf(s.res, j), c.buf(s.y, j), l.k, l.dil,
                            (h->blob_w16 && l.w16f_off != (size_t)-1) ? h->blob_w16 + l.w16f_off : nullptr);
        flops += 2.0 * c.n_el() * l.C_in * l.k;
        wbytes += 4.0 * ((double)l.ref_w_floats + l.C_out);
    }
    ConvLaunch a = conv_launch(p, nk, c.B, c.L, st.C, st.C, IN_ACT_LRELU, h->cfg.lrelu_slope, c.lengths, c.row_scale);
    a.dyn_counter = c.dyn_tiles ? h->tile_counters + (c.i * 2 * h->cfg.num_dilations[0] + 2 * s.m + s.half) : nullptr;
    return a;
}

// the pair of dilation s.m; *ok: the layers are what the pair kernels take (equal kernel sizes, conv2 undilated)
PairLaunchF32 stage_pair_launch(const StageCtx& c, const MrfStep& s, double& flops, double& wbytes, bool* ok = nullptr) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const int nk = h->cfg.num_kernels;
    PairProblemF32 p[kMaxGroup];
    flops = 0; wbytes = 0;
    bool good = nk <= kMaxGroup;
    for (int j = 0; j < nk && good; ++j) {
        const ConvLayer& c1 = st.c1[j][s.m];
        const ConvLayer& c2 = st.c2[j][s.m];
        good = c1.k == c2.k && c2.dil == 1 && c1.C_in == st.C && c1.C_out == st.C && c2.C_in == st.C && c2.C_out == st.C;
        p[j] = PairProblemF32{c.buf(s.x, j), (const f32x4*)(h->blob + c1.w_off), (const f32x4*)(h->blob + c2.w_off),
                              h->blob + c1.b_off, h->blob + c2.b_off, c.buf(s.y, j), c1.k, c1.dil};
        flops += 2.0 * c.n_el() * st.C * (c1.k + c2.k);
        wbytes += 4.0 * ((double)c1.ref_w_floats + c1.C_out + (double)c2.ref_w_floats + c2.C_out);
    }
    if (ok) *ok = good;
    return pair_launch(p, good ? nk : 0, c.B, c.L, st.C, h->cfg.lrelu_slope, c.lengths, c.row_scale);
}

// The steps of stage c.i, in order, with the buffers each reads and writes.  Pure: nothing is launched or recorded here.
MrfStagePlan plan_mrf_stage(const StageCtx& c, int32_t dtype, const ForwardStop& stop) {
    const iris_hifigan_handle* h = c.h;
    const Stage& st = c.st();
    const int nk = h->cfg.num_kernels, nd = h->cfg.num_dilations[0];
    double f, wb;
    // fp32 storage, split-bf16 products (conv_mfma_f32s.h): every step separate; at the last step of the stage the kernel
    // folds the branch mean (written to y[0]; a lane overwrites only elements it has read itself as branch 0's residual)
    const bool split = dtype == IRIS_HIFIGAN_F32_SPLIT && f32s_step_applicable(h, st.C, c.L, nk);
    // The stage's last step as the MRF kernel's summing launch (to_summing).  The mean goes to y[0] (in place: each lane
    // overwrites only elements it read itself as branch 0's residual).  Small problems run one branch per block -- mrf_plan's
    // latency modes -- and cannot sum.
    bool sums = split;
    if (!split && nk == 3) {
        const ConvLaunch a = step_launch(c, MrfStep{STEP_CONV2, false, nd - 1, 1, WS_XT, WS_Y, WS_Y, MEAN_NONE}, f, wb);
        if (mrf_kernel_applicable(a, nk)) {
            const MrfPlan pq = mrf_plan(a, true);
            ConvLaunch b = a;
            to_summing(b, c.y[0], nk);
            sums = mrf_kernel_applicable(b, nk) && !pq.zpar && !pq.small;
        }
    }
    // ---- fused conv pairs (mrf_pair_f32.h; C = 32 / 64, exact fp32): conv1 -> xt in LDS -> conv2 + residual in ONE launch,
    // bit for bit the two separate launches.  A fused pair cannot run in place, so the running x of a branch alternates
    // between its y and xt buffers, arranged so that the last fused pair leaves it in y (where the separate launches and
    // the next layer expect it).  The last pair of the stage stays separate when its second step is the persistent
    // kernel's summing launch (which forms the MRF mean; large problems).  forward_until asking for a state after a
    // conv1 gets the separate launches for that stage.
    int n_fused = 0;
    bool fused_sum = false;     // the stage's last pair forms the MRF mean itself (mrf_pair_f32_pf.h; no persistent summing launches)
    if (dtype == IRIS_HIFIGAN_F32 && !(stop.stage == c.i && !(stop.step & 1))) {
        bool all_ok = true;
        PairLaunchF32 pa;
        for (int m = 0; m < nd && all_ok; ++m) {
            pa = stage_pair_launch(c, MrfStep{STEP_PAIR, false, m, 1, WS_UP, WS_NONE, WS_Y, MEAN_NONE}, f, wb, &all_ok);
            all_ok = all_ok && pair_f32_applicable(pa, nk);
        }
        if (all_ok) {
            // The stage's LAST pair on the persistent summing kernel (mrf_pair_f32_pf.h: a block runs the three branches of
            // its tile and stores only the MRF mean -- no xt, no per-branch outputs, one launch instead of the persistent
            // kernel's two): taken where its whole-tile jobs fill at least four rounds of the chip well.  Measured
            // (profiles/r03_notes.md): +3 % on the C = 32 stage and +0.6 % on the step at batch 32 x 500, neutral at
            // batch 1 x 1000, a loss where a launch is one or two rounds (its jobs are 21 tap-units against 11 / 7 / 3).
            // The non-summing pairs stay on the one-job-per-block kernel: as persistent, prefetching blocks they
            // were 3-5 % slower at every size.
            const PairPfTileF32 pt = pair_pf_f32_tile(st.C);
            const long long tiles_pf = (long long)((c.L + (pt.M - 10) - 1) / (pt.M - 10)) * c.B;
            if (pair_pf_f32_applicable(pa, nk)) {
                const PairPfPlanF32 sp = pair_pf_f32_plan(tiles_pf, device_cu_count(), pt.MINB);
                fused_sum = sp.efficiency >= 0.85 && tiles_pf >= 4LL * device_cu_count() * sp.per_cu;
            }
            n_fused = (fused_sum || !sums) ? nd : nd - 1;
        }
    }
    MrfStagePlan pl;
    pl.n = 0;
    auto add = [&](StepKind kind, int m, int half, WsBuf x, WsBuf res, WsBuf y) {
        pl.s[pl.n++] = MrfStep{kind, split, m, half, x, res, y, kind == STEP_PAIR_SUM || kind == STEP_CONV2_SUM ? MEAN_IN_Y : MEAN_NONE};
    };
    // never in place: the running x of a branch alternates between its y and xt buffers, arranged so that the last
    // fused pair ends in y -- or, in front of the summing pair (which writes the mean to y[0]), in xt
    const int last_pair = fused_sum ? nd - 2 : n_fused - 1;
    const WsBuf last_to = fused_sum ? WS_XT : WS_Y, other = fused_sum ? WS_Y : WS_XT;
    WsBuf cur = WS_UP;          // where the running x of every branch lies
    for (int m = 0; m < nd; ++m) {
        if (m < n_fused && fused_sum && m == nd - 1) {
            add(STEP_PAIR_SUM, m, 1, cur, WS_NONE, WS_Y);
        } else if (m < n_fused) {
            const WsBuf to = ((last_pair - m) & 1) ? other : last_to;
            add(STEP_PAIR, m, 1, cur, WS_NONE, to);
            cur = to;
        } else {
            add(STEP_CONV1, m, 0, cur, WS_NONE, WS_XT);
            add(m == nd - 1 && sums ? STEP_CONV2_SUM : STEP_CONV2, m, 1, WS_XT, cur, WS_Y);
            cur = WS_Y;
        }
    }
    return pl;
}

// The fp32 / split-product forward.  `stop` (forward_until only): return after MRF step stop.step of stage
// stop.stage has been queued; *until_flags then says where that stage's result lies (forward_until's contract).
// `lengths` (iris_hifigan_forward_ragged, fp32 only; nullptr otherwise): mel frames of each batch item on the device.
// Every launch carries it with its rows per mel frame (`row_scale`), and every kernel bounds the item's reads and stores
// by them: the plan is the one of (B, T), each item is computed as a forward of its own length would compute it.
int forward_f32(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T, const ForwardOut& out, void* workspace_dev,
                uint64_t workspace_bytes, int32_t dtype, hipStream_t stream, const ForwardStop& stop, int32_t* until_flags,
                const int32_t* lengths) {
    const WsLayout w = ws_layout(h, B, T, dtype);
    if (workspace_bytes < w.bytes())
        return fail(IRIS_HIFIGAN_WORKSPACE_TOO_SMALL, "workspace has %llu bytes, need %llu",
                    (unsigned long long)workspace_bytes, (unsigned long long)w.bytes());
    float* ws = (float*)workspace_dev;
    const float* blob = h->blob;
    const float slope = h->cfg.lrelu_slope;
    const int nk = h->cfg.num_kernels, nd = h->cfg.num_dilations[0];
    Prof prof{h, stream, (h->profiling && !h->profiling_paused) ? h->n_rec : 0};
    const double fB = (double)B;
    // large batches: the MRF kernel's blocks draw tiles from per-launch counters (mrf_conv_mfma_f32.h); one
    // memset per forward zeroes them.  Below ~2000 frames no launch has enough tiles per block to use them.
    const bool dyn_tiles = h->tile_counters && (long long)B * T >= 2000 &&
                           (int)h->stages.size() * 2 * nd <= kTileCounterWords / 2;
    // the persistent pair kernels draw jobs from one counter word per launch (upper half of the array); a forward too short
    // to use either kind of counter skips the memset
    const bool pf_counters = h->tile_counters && (long long)B * T >= 100 &&
                             (int)h->stages.size() * nd <= kTileCounterWords / 2;
    // (zeroed where the first launch that reads them is about to be issued: a batch-1 forward of a few hundred frames has none)
    bool counters_zeroed = false;
    auto zero_counters = [&]() -> hipError_t {
        if (counters_zeroed || h->host_only) return hipSuccess;
        counters_zeroed = true;
        return hipMemsetAsync(h->tile_counters, 0, kTileCounterWords * sizeof(unsigned), stream);
    };
    if (dyn_tiles) HIP_TRY(zero_counters());

    // ---- conv_pre (hifigan_pretrained.py:124) ----
    {
        const ConvLayer& l = h->pre;
        const ConvProblem p = conv_problem((const float*)mel_dev, blob + l.w_off, blob + l.b_off, nullptr, ws + w.pre, l.k, 1);
        ConvLaunch a = conv_launch(&p, 1, B, T, l.C_in, l.C_out, IN_ACT_NONE, slope, lengths, 1);
        a.x_channels_first = 1;
        TRY(prof.begin(0, -1, 0, 2.0 * fB * T * l.C_in * l.C_out * l.k,
                       4.0 * (fB * T * (l.C_in + l.C_out) + (double)l.ref_w_floats + l.C_out)));
        HIP_TRY(launch_conv(a, 1, stream));
        TRY(prof.end());
    }

    StageCtx c;
    c.h = h; c.B = B; c.L = T; c.lengths = lengths; c.row_scale = 1; c.dyn_tiles = dyn_tiles;
    c.up = ws + w.up;
    for (int j = 0; j < nk; ++j) { c.y[j] = ws + w.y[j]; c.xt[j] = ws + w.xt[j]; }
    bool prev_summed = false;   // the previous stage left mean(branches) in y[0]
    for (c.i = 0; c.i < (int)h->stages.size(); ++c.i) {
        const Stage& st = c.st();
        const int L = c.L, L_out = L * st.rate;
        // ---- LeakyReLU + ConvTranspose1d (hifigan_pretrained.py:127-128) ----
        {
            const ConvLayer& l = st.up;
            // bytes are reported in accounting L (the MRF accumulation costs one extra read
            // per additional branch) whether or not the summing step already folded the mean
            const int n_in = c.i == 0 ? 1 : nk;
            const float* const one = c.i == 0 ? ws + w.pre : c.y[0];
            const bool mrf = c.i > 0 && !prev_summed;
            ConvtF32 d = convt_launch(mrf ? c.y : &one, nk, mrf ? IN_ACT_MRF_LRELU : IN_ACT_LRELU, blob + l.w_off, blob + l.b_off,
                                      c.up, B, L, l.C_in, l.C_out, l.k, l.u, slope, lengths, c.row_scale);
            TRY(prof.begin(1, c.i, 0, 2.0 * fB * L * l.C_in * l.C_out * l.k,
                           4.0 * (fB * L * l.C_in * n_in + fB * L_out * l.C_out + (double)l.ref_w_floats + l.C_out)));
            HIP_TRY(launch_convt(d, stream));
            TRY(prof.end());
        }
        // ---- MRF: num_kernels ResBlocks advance together (hifigan_pretrained.py:64-71,131-136) ----
        c.L = L_out;
        c.row_scale *= st.rate;
        const MrfStagePlan plan = plan_mrf_stage(c, dtype, stop);
        for (int n = 0; n < plan.n; ++n) {
            const MrfStep& s = plan.s[n];
            double flops, wbytes;
            if (s.kind == STEP_PAIR || s.kind == STEP_PAIR_SUM) {
                PairLaunchF32 pa = stage_pair_launch(c, s, flops, wbytes);
                // algorithmic FLOP / bytes (accounting L) are those of both steps; the record carries the second step's index
                TRY(prof.begin(2, c.i, 2 * s.m + 1, flops, 4.0 * c.n_el() * nk * 5 + wbytes));
                if (s.kind == STEP_PAIR_SUM) {
                    // (a zeroed counter word per persistent launch: the upper half of the per-forward counters)
                    unsigned* const ctr = pf_counters ? h->tile_counters + kTileCounterWords / 2 + (c.i * nd + s.m) : nullptr;
                    if (ctr) HIP_TRY(zero_counters());
                    HIP_TRY(launch_pair_f32_pf(pa, nk, c.y[0], ctr, stream));
                } else
                    HIP_TRY(launch_pair_f32(pa, nk, stream));
            } else {
                ConvLaunch a = step_launch(c, s, flops, wbytes);
                TRY(prof.begin(2, c.i, 2 * s.m + s.half, flops, 4.0 * c.n_el() * nk * (s.half == 0 ? 2 : 3) + wbytes));
                if (s.split) {
                    F32sStep step;
                    for (int j = 0; j < nk; ++j) {
                        step.x[j] = a.p[j].x; step.res[j] = a.p[j].res; step.y[j] = a.p[j].y;
                        step.layer[j] = s.half == 0 ? &st.c1[j][s.m] : &st.c2[j][s.m];
                    }
                    TRY(f32s_launch_step(h, step, nk, B, L_out, st.C, s.mean == MEAN_IN_Y ? c.y[0] : nullptr, stream));
                } else {
                    if (s.mean == MEAN_IN_Y) to_summing(a, c.y[0], nk);
                    if (mrf_kernel_applicable(a, nk)) HIP_TRY(launch_mrf_conv(a, nk, stream));
                    else                              HIP_TRY(launch_conv(a, nk, stream));
                }
            }
            TRY(prof.end());
            prev_summed = s.mean == MEAN_IN_Y;
            if (stop.stage == c.i && stop.step == 2 * s.m + s.half) {
                if (until_flags)
                    *until_flags = s.mean == MEAN_IN_Y ? IRIS_HIFIGAN_UNTIL_MEAN_IN_Y0
                                                : (s.kind == STEP_PAIR && s.y == WS_XT ? IRIS_HIFIGAN_UNTIL_X_IN_XT : 0);
                TRY(prof.finish());
                return IRIS_HIFIGAN_OK;
            }
        }
    }

    // ---- LeakyReLU + conv_post + tanh (hifigan_pretrained.py:139-141) ----
    {
        post::ConvPostLaunch a; memset(&a, 0, sizeof(a));
        const ConvLayer& l = h->post;
        const int L = c.L;
        if (prev_summed) { a.x[0] = c.y[0]; a.n_in = 1; }
        else { for (int j = 0; j < nk; ++j) a.x[j] = c.y[j]; a.n_in = nk; }
        a.w = blob + l.w_off; a.bias = blob + l.b_off; out.to_post(a);
        a.B = B; a.L = L; a.C = l.C_in; a.k = l.k; a.slope = slope; a.inv_n = 1.0f / (float)nk;
        a.lengths = lengths; a.row_scale = c.row_scale;
        TRY(prof.begin(3, -1, 0, 2.0 * fB * L * l.C_in * l.k,
                       4.0 * (fB * L * l.C_in * nk + fB * L + (double)l.ref_w_floats + 1)));
        HIP_TRY(post::launch_conv_post(a, stream));
        TRY(prof.end());
    }
    TRY(prof.finish());
    return IRIS_HIFIGAN_OK;
}

// Checks shared by the forwards, forward_until and describe_plan.
int check_forward_args(const iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T, const void* workspace_dev,
                       int32_t dtype) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (dtype != IRIS_HIFIGAN_F32 && dtype != IRIS_HIFIGAN_BF16 && dtype != IRIS_HIFIGAN_F32_SPLIT)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "dtype %d not supported", dtype);
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (!mel_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.y)", B);
    if ((int64_t)T * h->hop > (int64_t)1 << 30)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "T*hop = %lld exceeds 2^30 rows", (long long)T * h->hop);
    return IRIS_HIFIGAN_OK;
}

// What every forward does once its own argument checks have passed: the handle's device, the weight packing of the dtype,
// then the passes (pass_items).  `lengths_dev`: the ragged forward's; `stop` / `until_flags`: forward_until's (one pass).
// `out`: what the forward leaves behind (ForwardOut); a normalising pass zeroes its items' peaks in front of the forward and
// converts its waveform behind it (pcm_out.h), all on `stream`.
// A host-only handle (describe_plan) has no device and every packing's offsets.
int run_forward(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T, const int32_t* lengths_dev, const ForwardOut& out,
                void* workspace_dev, uint64_t workspace_bytes, int32_t dtype, hipStream_t stream, const ForwardStop& stop,
                int32_t* until_flags) {
    DeviceGuard guard(h->device, !h->host_only);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    TRY(ensure_prepared(h, dtype, stream, true));
    if (dtype == IRIS_HIFIGAN_F32_SPLIT && !h->blob_s3)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "split-product mode needs ResBlock channel counts that are multiples of 32");
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    const int Bp = pass_items(B, T);
    for (int b0 = 0; b0 < B; b0 += Bp) {
        const int nb = B - b0 < Bp ? B - b0 : Bp;
        const float* mel_p = (const float*)mel_dev + (size_t)b0 * h->cfg.in_channels * T;
        const ForwardOut out_p = out.advanced((size_t)b0, (size_t)h->hop * T);
        const int32_t* const lengths_p = lengths_dev ? lengths_dev + b0 : nullptr;
        if (out_p.normalize() && !h->host_only) HIP_TRY(hipMemsetAsync(out_p.peak, 0, sizeof(float) * nb, stream));
        if (dtype == IRIS_HIFIGAN_BF16)
            TRY(bf16_forward(h, mel_p, nb, T, out_p, workspace_dev, workspace_bytes, stream, stop, until_flags));
        else
            TRY(forward_f32(h, mel_p, nb, T, out_p, workspace_dev, workspace_bytes, dtype, stream, stop, until_flags, lengths_p));
        if (out_p.normalize()) {
            const pcm::PcmLaunch q{out_p.wav, lengths_p, h->hop, out_p.pcm, out_p.peak, nb, h->hop * T, out_p.target};
            HIP_TRY(pcm::launch_pcm_normalize(q, true, stream));
        }
    }
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_hifigan_forward(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                             void* wav_dev, void* workspace_dev, uint64_t workspace_bytes,
                             int32_t dtype, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_forward_args(h, mel_dev, B, T, workspace_dev, dtype));
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;  // empty batch / empty mel -> empty waveform
    if (!wav_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardOut out; out.wav = (float*)wav_dev;
    return run_forward(h, mel_dev, B, T, nullptr, out, workspace_dev, workspace_bytes, dtype, (hipStream_t)stream_,
                       ForwardStop{-1, -1}, nullptr);
    IRIS_ABI_END
}

int32_t iris_hifigan_forward_ragged(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                    const int32_t* lengths_dev, void* wav_dev, void* workspace_dev,
                                    uint64_t workspace_bytes, int32_t dtype, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_forward_args(h, mel_dev, B, T, workspace_dev, dtype));
    if (dtype != IRIS_HIFIGAN_F32)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the ragged forward supports fp32 (dtype 0) only, got dtype %d: the bf16-storage "
                    "and split-product paths have no per-item lengths", dtype);
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (!lengths_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "lengths_dev is NULL");
    if (!wav_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    // the plan of (B, T), as iris_hifigan_forward: the lengths are never read on the host (fp32 plans are bitwise
    // plan-independent, so each item still gets the bits of a forward of its own length)
    ForwardOut out; out.wav = (float*)wav_dev;
    return run_forward(h, mel_dev, B, T, lengths_dev, out, workspace_dev, workspace_bytes, dtype, (hipStream_t)stream_,
                       ForwardStop{-1, -1}, nullptr);
    IRIS_ABI_END
}

int32_t iris_hifigan_forward_pcm16(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                   const int32_t* lengths_dev, int16_t* pcm_dev, float* wav_dev, float* peak_dev,
                                   int32_t normalize, float peak_target, void* workspace_dev, uint64_t workspace_bytes,
                                   int32_t dtype, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_forward_args(h, mel_dev, B, T, workspace_dev, dtype));
    if (lengths_dev && dtype != IRIS_HIFIGAN_F32)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "per-item lengths are supported in fp32 (dtype 0) only, got dtype %d: the bf16-storage "
                    "and split-product paths have no per-item lengths", dtype);
    if (normalize && !(peak_target > 0.f && peak_target <= 1.f))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "peak_target must lie in (0, 1], got %g", (double)peak_target);
    if (normalize && (!wav_dev || !peak_dev))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "normalize needs wav_dev and peak_dev");
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (!pcm_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardOut out;
    out.pcm = pcm_dev;
    if (normalize) { out.wav = wav_dev; out.peak = peak_dev; out.target = peak_target; }
    return run_forward(h, mel_dev, B, T, lengths_dev, out, workspace_dev, workspace_bytes, dtype, (hipStream_t)stream_,
                       ForwardStop{-1, -1}, nullptr);
    IRIS_ABI_END
}

int32_t iris_hifigan_forward_until(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                   void* workspace_dev, uint64_t workspace_bytes, int32_t dtype,
                                   int32_t stop_stage, int32_t stop_step, int32_t* flags, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_forward_args(h, mel_dev, B, T, workspace_dev, dtype));
    if (B == 0 || T == 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "forward_until needs a non-empty input");
    if (stop_stage < 0 || stop_stage >= (int)h->stages.size() || stop_step < 0 || stop_step >= 2 * h->cfg.num_dilations[0])
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "no MRF step %d in stage %d", stop_step, stop_stage);
    if (pass_items(B, T) != B)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "forward_until takes shapes that run in one pass (B * T <= %d frames)", kPassFrames);
    return run_forward(h, mel_dev, B, T, nullptr, ForwardOut{}, workspace_dev, workspace_bytes, dtype, (hipStream_t)stream_,
                       ForwardStop{stop_stage, stop_step}, flags);
    IRIS_ABI_END
}

int32_t iris_hifigan_describe_plan(const iris_hifigan_config* cfg, int32_t B, int32_t T, int32_t dtype, int32_t cu_count,
                                   iris_hifigan_plan* out) {
    IRIS_ABI_BEGIN
    TRY(validate(cfg));
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out is NULL");
    memset(out, 0, sizeof(*out));
    // a generator without a device: the layer table, the offsets of every weight packing and fake (never dereferenced)
    // base pointers -- then the forward itself, with every launch recorded instead of issued
    iris_hifigan_handle h;
    h.cfg = *cfg;
    h.host_only = true;
    build_layers(&h);
    h.blob = reinterpret_cast<float*>((uintptr_t)0x10000000);
    h.tile_counters = reinterpret_cast<unsigned*>((uintptr_t)0x08000000);
    if (assign_w16_offsets(&h) > 0) h.blob_w16 = reinterpret_cast<float*>((uintptr_t)0x18000000);
    TRY(bf16_build_blob(&h, nullptr)); h.built_bf16 = true;
    TRY(f32s_build_blob(&h, nullptr)); h.built_s3 = true;
    void* const mel = reinterpret_cast<void*>((uintptr_t)0x40000000);
    void* const wav = reinterpret_cast<void*>((uintptr_t)0x50000000);
    void* const ws = reinterpret_cast<void*>((uintptr_t)0x100000000ull);
    TRY(check_forward_args(&h, mel, B, T, ws, dtype));
    DryRunLaunch recs[IRIS_HIFIGAN_MAX_PLAN_LAUNCHES];
    DryRun dry{recs, IRIS_HIFIGAN_MAX_PLAN_LAUNCHES, 0, cu_count > 0 ? cu_count : 256};
    struct Scope { DryRun* prev; Scope(DryRun* d) : prev(dry_run_slot()) { dry_run_slot() = d; } ~Scope() { dry_run_slot() = prev; } } scope(&dry);
    const int Bp = pass_items(B, T);
    out->workspace_bytes = ws_layout(&h, Bp, T, dtype).bytes();
    out->cu_count = dry.cu_count;
    if (B > 0 && T > 0) out->passes = (B + Bp - 1) / Bp;
    ForwardOut fo; fo.wav = (float*)wav;
    const int rc = run_forward(&h, mel, B, T, nullptr, fo, ws, out->workspace_bytes, dtype, nullptr, ForwardStop{-1, -1}, nullptr);
    out->n_launches = dry.n;                                    // (the launches of every pass are recorded)
    for (int i = 0; i < dry.n && i < IRIS_HIFIGAN_MAX_PLAN_LAUNCHES; ++i) {
        iris_hifigan_plan_launch& o = out->launches[i];
        strncpy(o.kernel, recs[i].kernel ? recs[i].kernel : "", sizeof(o.kernel) - 1);
        o.grid[0] = recs[i].grid[0]; o.grid[1] = recs[i].grid[1]; o.grid[2] = recs[i].grid[2];
        o.block = recs[i].block; o.lds_bytes = recs[i].lds_bytes;
    }
    return rc;
    IRIS_ABI_END
}

int32_t iris_hifigan_workspace_layout(const iris_hifigan_handle* h, int32_t B, int32_t T, int32_t dtype,
                                      iris_hifigan_workspace_map* out) {
    if (!h || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    memset(out, 0, sizeof(*out));
    if (dtype != IRIS_HIFIGAN_F32 && dtype != IRIS_HIFIGAN_BF16 && dtype != IRIS_HIFIGAN_F32_SPLIT)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "dtype %d not supported", dtype);
    const WsLayout w = ws_layout(h, pass_items(B, T), T, dtype);   // (the layout of one pass; forward_until takes single-pass shapes only)
    const uint64_t e = w.elem_bytes;
    out->element_bytes = (int32_t)e;
    out->pre_offset = w.pre * e; out->up_offset = w.up * e; out->total_bytes = w.total * e;
    for (int j = 0; j < h->cfg.num_kernels; ++j) { out->y_offset[j] = w.y[j] * e; out->xt_offset[j] = w.xt[j] * e; }
    return IRIS_HIFIGAN_OK;
}

// ------------------------------------------------------------------------------------------------
// single-layer entry points
// ------------------------------------------------------------------------------------------------
int32_t iris_hifigan_op_conv1d(const float* x_dev, const float* w_host, const float* bias_host,
                               const float* res_dev, float* y_dev, int32_t B, int32_t L,
                               int32_t C_in, int32_t C_out, int32_t k, int32_t dilation,
                               int32_t in_act, float slope, int32_t x_channels_first, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || C_out < 1 || k < 1 || !(k & 1) || dilation < 1 || B > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv1d shape");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<float> packed(packed_conv1d_floats(C_in, C_out, k) + C_out);
    pack_conv1d_weights(w_host, C_in, C_out, k, packed.data());
    const size_t boff = packed.size() - C_out;
    memcpy(packed.data() + boff, bias_host, sizeof(float) * C_out);
    DevBuf wb;
    HIP_TRY(wb.upload(packed));
    const ConvProblem p = conv_problem(x_dev, wb.f32(), wb.f32() + boff, res_dev, y_dev, k, dilation);
    ConvLaunch a = conv_launch(&p, 1, B, L, C_in, C_out, in_act ? IN_ACT_LRELU : IN_ACT_NONE, slope);
    a.x_channels_first = x_channels_first;
    HIP_TRY(launch_conv(a, 1, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_conv_transpose1d(const float* x_dev, const float* w_host,
                                         const float* bias_host, float* y_dev, int32_t B, int32_t L,
                                         int32_t C_in, int32_t C_out, int32_t k, int32_t u,
                                         int32_t in_act, float slope, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || C_out < 1 || u < 1 || k < u || ((k - u) & 1) || B > 65535 || u > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv_transpose1d shape");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t phase_floats = packed_convt_phase_floats(C_in, C_out, k, u);
    std::vector<float> packed(phase_floats * u + C_out);
    pack_convt_weights(w_host, C_in, C_out, k, u, packed.data());
    const size_t boff = packed.size() - C_out;
    memcpy(packed.data() + boff, bias_host, sizeof(float) * C_out);
    DevBuf wb;
    HIP_TRY(wb.upload(packed));
    ConvtF32 d = convt_launch(&x_dev, 1, in_act ? IN_ACT_LRELU : IN_ACT_NONE, wb.f32(), wb.f32() + boff, y_dev, B, L, C_in, C_out,
                              k, u, slope);
    HIP_TRY(launch_convt(d, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_conv_post(const float* x0_dev, const float* x1_dev, const float* x2_dev,
                                  const float* w_host, const float* bias_host, float* y_dev,
                                  int32_t B, int32_t L, int32_t C_in, int32_t k, float slope,
                                  void* stream_) {
    IRIS_ABI_BEGIN
    if (!x0_dev || !w_host || !bias_host || !y_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C_in < 1 || k < 1 || !(k & 1) || B > 65535)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad conv_post shape");
    if ((x1_dev == nullptr) != (x2_dev == nullptr))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "x1 and x2 must both be given or both be NULL");
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<float> wv((size_t)k * C_in + 1);
    for (int c = 0; c < C_in; ++c)
        for (int kap = 0; kap < k; ++kap) wv[(size_t)kap * C_in + c] = w_host[(size_t)c * k + kap];
    wv[(size_t)k * C_in] = bias_host[0];
    DevBuf wb;
    HIP_TRY(wb.upload(wv));
    post::ConvPostLaunch a; memset(&a, 0, sizeof(a));
    a.x[0] = x0_dev; a.n_in = 1;
    if (x1_dev) { a.x[1] = x1_dev; a.x[2] = x2_dev; a.n_in = 3; }
    a.w = wb.f32(); a.bias = wb.f32() + (size_t)k * C_in; a.y = y_dev;
    a.B = B; a.L = L; a.C = C_in; a.k = k; a.slope = slope; a.inv_n = 1.0f / (float)a.n_in;
    HIP_TRY(post::launch_conv_post(a, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_pcm16(const float* wav_dev, const int32_t* lengths_dev, int32_t row_scale, int16_t* pcm_dev,
                              float* peak_dev, int32_t B, int32_t L, int32_t normalize, float peak_target, void* stream_) {
    IRIS_ABI_BEGIN
    if (!wav_dev || !pcm_dev || (normalize && !peak_dev)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || B > 65535 || row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad pcm16 shape");
    if (normalize && !(peak_target > 0.f && peak_target <= 1.f))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "peak_target must lie in (0, 1], got %g", (double)peak_target);
    hipStream_t stream = (hipStream_t)stream_;
    const pcm::PcmLaunch q{wav_dev, lengths_dev, row_scale, pcm_dev, peak_dev, B, L, peak_target};
    if (normalize) {
        HIP_TRY(hipMemsetAsync(peak_dev, 0, sizeof(float) * B, stream));
        HIP_TRY(pcm::launch_pcm_peak(q, stream));
    }
    HIP_TRY(pcm::launch_pcm_normalize(q, normalize != 0, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_g711(const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale, int32_t law,
                             uint8_t* out_u8_dev, void* stream_) {
    IRIS_ABI_BEGIN
    if (!wav_dev || !out_u8_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || B > 65535 || row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad g711 shape");
    if (law != IRIS_OUT_ULAW && law != IRIS_OUT_ALAW)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "law must be IRIS_OUT_ULAW or IRIS_OUT_ALAW, got %d", law);
    hipStream_t stream = (hipStream_t)stream_;
    const pcm::G711Launch q{wav_dev, lengths_dev, row_scale, out_u8_dev, B, L};
    HIP_TRY(pcm::launch_g711(q, law, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_mrf_step(const float* const* x_dev, const float* const* w_host, const float* const* bias_host,
                                 const float* const* res_dev, float* const* y_dev, float* mean_dev,
                                 int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                 float slope, int32_t plan, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w_host || !bias_host || !k || !dil || (!y_dev && !mean_dev))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C < 1 || plan < 0 || plan > 6) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad mrf_step shape or plan");
    const int nk = 3;
    for (int j = 0; j < nk; ++j) {
        if (!x_dev[j] || !w_host[j] || !bias_host[j] || (!mean_dev && !y_dev[j])) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL branch argument");
        if (k[j] < 1 || !(k[j] & 1) || dil[j] < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad branch kernel size / dilation");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DevBuf wb[3], wb16[3];
    ConvProblem p[3];
    for (int j = 0; j < nk; ++j) {
        std::vector<float> packed(packed_conv1d_floats(C, C, k[j]) + ((size_t)C + 3 & ~(size_t)3));
        pack_conv1d_weights(w_host[j], C, C, k[j], packed.data());
        const size_t boff = packed_conv1d_floats(C, C, k[j]);
        memcpy(packed.data() + boff, bias_host[j], sizeof(float) * C);
        HIP_TRY(wb[j].upload(packed));
        if ((C & 15) == 0) {
            std::vector<float> p16(packed16_conv1d_floats(C, C, k[j]));
            pack_conv1d_weights16(w_host[j], C, C, k[j], p16.data());
            HIP_TRY(wb16[j].upload(p16));
        }
        p[j] = conv_problem(x_dev[j], wb[j].f32(), wb[j].f32() + boff, res_dev ? res_dev[j] : nullptr, y_dev ? y_dev[j] : nullptr,
                            k[j], dil[j], wb16[j].f32());
    }
    ConvLaunch a = conv_launch(p, nk, B, L, C, C, IN_ACT_LRELU, slope);
    if (mean_dev) {
        to_summing(a, mean_dev, nk);
        for (int j = 0; j < nk; ++j) if (!a.p[j].y) a.p[j].y = mean_dev;     // never written; keeps descriptors valid
    }
    if (!mrf_kernel_applicable(a, nk)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "shape cannot take the MRF kernel");
    const int force = plan == 0 ? -1 : (plan >= 4 ? plan : plan - 1);
    if (mean_dev && (force == 2 || force >= 4)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "the one-branch-per-block modes cannot form the mean");
    if (force == 4 && !mrf_small_applicable(a, nk)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "the small-problem kernel needs C %% 32 == 0");
    if (force >= 5 && !mrf_plan(a, true, force).zdyn) return fail(IRIS_HIFIGAN_UNSUPPORTED, "the job mode needs two or more C_in chunks (C >= 128)");
    HIP_TRY(launch_mrf_conv(a, nk, stream, force));
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_hifigan_op_mrf_pair(const float* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                 const float* const* w2_host, const float* const* b2_host, float* const* y_dev,
                                 float* mean_dev, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                 float slope, int32_t mode, void* stream_) {
    IRIS_ABI_BEGIN
    if (!x_dev || !w1_host || !b1_host || !w2_host || !b2_host || (!y_dev && !mean_dev) || !k || !dil)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 1 || L < 1 || C < 1 || mode < 0 || mode > 2) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad mrf_pair shape or mode");
    if (mean_dev && mode == 0) return fail(IRIS_HIFIGAN_UNSUPPORTED, "only the persistent kernel (modes 1, 2) forms the mean");
    const int nk = 3;
    hipStream_t stream = (hipStream_t)stream_;
    DevBuf wb[3];
    PairProblemF32 p[3];
    for (int j = 0; j < nk; ++j) {
        if (!x_dev[j] || !w1_host[j] || !b1_host[j] || !w2_host[j] || !b2_host[j] || (!mean_dev && !y_dev[j]))
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL branch argument");
        if (k[j] < 1 || !(k[j] & 1) || dil[j] < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad branch kernel size / dilation");
        const size_t wf = packed_conv1d_floats(C, C, k[j]), cpad = ((size_t)C + 3) & ~(size_t)3;
        std::vector<float> packed(2 * wf + 2 * cpad);
        pack_conv1d_weights(w1_host[j], C, C, k[j], packed.data());
        pack_conv1d_weights(w2_host[j], C, C, k[j], packed.data() + wf);
        memcpy(packed.data() + 2 * wf, b1_host[j], sizeof(float) * C);
        memcpy(packed.data() + 2 * wf + cpad, b2_host[j], sizeof(float) * C);
        HIP_TRY(wb[j].upload(packed));
        const float* const w = wb[j].f32();
        p[j] = PairProblemF32{x_dev[j], (const f32x4*)w, (const f32x4*)(w + wf), w + 2 * wf, w + 2 * wf + cpad,
                              mean_dev ? mean_dev : y_dev[j],      // (summing launch: the branch outputs are never written)
                              k[j], dil[j]};
    }
    PairLaunchF32 pa = pair_launch(p, nk, B, L, C, slope);
    if (!pair_f32_applicable(pa, nk)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "shape cannot take the fused fp32 pair kernel");
    if (mode == 1 || mode == 2) {
        if (!mean_dev) return fail(IRIS_HIFIGAN_UNSUPPORTED, "the persistent pair kernel exists in its summing form only (mean_dev)");
        if (!pair_pf_f32_applicable(pa, nk)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "shape cannot take the persistent pair kernel");
        struct Word { unsigned* p = nullptr; ~Word() { if (p) (void)hipFree(p); } } ctr;
        if (mode == 1) {                                    // blocks draw their jobs from a counter (mode 2: fixed stride)
            HIP_TRY(hipMalloc(&ctr.p, sizeof(unsigned)));
            HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(unsigned), stream));
        }
        HIP_TRY(launch_pair_f32_pf(pa, nk, mean_dev, ctr.p, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    } else {
        HIP_TRY(launch_pair_f32(pa, nk, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

// ------------------------------------------------------------------------------------------------
// PostNet (src/iris/postnet.py:48-67)
// ------------------------------------------------------------------------------------------------
}  // extern "C"

struct iris_postnet_handle : StageHandle {
    int n_mels = 0, num_layers = 0, channels = 0, k = 0;
    std::vector<PackedGemm> layers;
};

namespace {

// workspace: two ping-pong hidden buffers [B, T, channels] and the residual [B, T, n_mels]
struct PostnetWs { size_t hid[2], res, total; };   // float offsets; every buffer starts on 256 bytes

PostnetWs postnet_ws(const iris_postnet_handle* h, int B, int T) {
    const size_t frames = (size_t)B * T;
    PostnetWs w;
    WsTaker t;
    w.hid[0] = t.take(frames * h->channels); w.hid[1] = t.take(frames * h->channels);
    w.res = t.take(frames * h->n_mels);
    w.total = t.off;
    return w;
}

}  // namespace

extern "C" {

int32_t iris_postnet_create(int32_t n_mels, int32_t num_layers, int32_t channels, int32_t kernel_size,
                            const float* weights_host, uint64_t n_weights, iris_postnet_handle** out) {
    IRIS_ABI_BEGIN
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (n_mels < 1 || channels < 1 || num_layers < 2 || num_layers > 64 || kernel_size < 1 || !(kernel_size & 1))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "PostNet needs n_mels, channels >= 1, 2 <= num_layers <= 64, odd kernel_size");
    std::unique_ptr<iris_postnet_handle> h(new (std::nothrow) iris_postnet_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->n_mels = n_mels; h->num_layers = num_layers; h->channels = channels; h->k = kernel_size;
    h->layers.resize(num_layers);
    uint64_t expect = 0;
    for (int i = 0; i < num_layers; ++i) {
        PackedGemm& l = h->layers[i];
        l.C_in = i == 0 ? n_mels : channels;
        l.C_out = i == num_layers - 1 ? n_mels : channels;
        l.k = kernel_size;
        expect += (uint64_t)l.C_in * l.C_out * l.k + l.C_out;
    }
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, PostNet needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    BlobBuilder bb(weights_host);
    for (PackedGemm& l : h->layers) bb.dense(l, l.C_in, l.C_out, l.k);
    TRY(upload(bb.host, h.get(), "PostNet"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_postnet_destroy(iris_postnet_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_postnet_workspace_bytes(const iris_postnet_handle* h, int32_t B, int32_t T, uint64_t* bytes) {
    if (!h || !bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    *bytes = (uint64_t)postnet_ws(h, B, T).total * sizeof(float);
    return IRIS_HIFIGAN_OK;
}

}  // extern "C"

namespace {

// The PostNet forward.  `lengths` (iris_postnet_forward_ragged; nullptr otherwise): frames of each batch item on the device.
// `ragged` says which entry point is calling: the plan is that of (B, T) either way, every conv bounds the item's reads and
// stores by its length (row_scale 1: 'same' convolutions keep one row per frame), and the residual kernel zeroes the rest.
int postnet_forward(iris_postnet_handle* h, const void* mel_dev, int32_t B, int32_t T, bool ragged, const int32_t* lengths,
                    void* out_dev, void* workspace_dev, uint64_t workspace_bytes, hipStream_t stream) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (ragged && !lengths) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "lengths_dev is NULL");
    if (!mel_dev || !out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.y)", B);
    const PostnetWs w = postnet_ws(h, B, T);
    ForwardScope scope(*h, workspace_bytes, w.total);
    TRY(scope.rc);
    float* ws = (float*)workspace_dev;
    float* hbuf[2] = {ws + w.hid[0], ws + w.hid[1]};
    float* res = ws + w.res;
    const float* x = (const float*)mel_dev;
    for (int i = 0; i < h->num_layers; ++i) {
        const PackedGemm& l = h->layers[i];
        const bool last = i == h->num_layers - 1;
        const ConvProblem p = conv_problem(x, h->blob + l.w_off, h->blob + l.b_off, nullptr, last ? res : hbuf[i & 1], l.k, 1);
        ConvLaunch a = conv_launch(&p, 1, B, T, l.C_in, l.C_out, IN_ACT_NONE, 0.f, lengths, 1);
        a.x_channels_first = i == 0 ? 1 : 0;                            // the mel arrives [B, n_mels, T]
        a.out_act = last ? 0 : 1;                                       // tanh (postnet.py:59)
        HIP_TRY(launch_conv(a, 1, stream));
        x = p.y;
    }
    dim3 grid((unsigned)((T + 255) / 256), (unsigned)B), block(256);
    HIP_TRY(launch_kernel(postnet_residual_kernel, grid, block, 0, stream, (const float*)mel_dev, (const float*)res,
                          (float*)out_dev, h->n_mels, T, lengths));     // x + res (postnet.py:67)
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_postnet_forward(iris_postnet_handle* h, const void* mel_dev, int32_t B, int32_t T,
                             void* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    return postnet_forward(h, mel_dev, B, T, false, nullptr, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream_);
    IRIS_ABI_END
}

int32_t iris_postnet_forward_ragged(iris_postnet_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                    const int32_t* lengths_dev, void* out_dev, void* workspace_dev,
                                    uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    return postnet_forward(h, mel_dev, B, T, true, lengths_dev, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream_);
    IRIS_ABI_END
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Sample-rate conversion behind conv_post (csrc/resample.h)
// ------------------------------------------------------------------------------------------------
struct iris_resampler_handle {
    resample::Design d;
    float* bank = nullptr;      // [up][row_stride(taps)] on the device
    int device = 0;
};

namespace {

int resampler_plan(int32_t rate_in, int32_t rate_out, int32_t zeros, double beta, double rolloff, resample::Design* d) {
    const int rc = resample::plan(rate_in, rate_out, zeros, beta, rolloff, d);
    if (rc == IRIS_HIFIGAN_INVALID_ARGUMENT)
        return fail(rc, "resampler needs rate_in != rate_out, both >= 1, zeros >= 0, beta >= 0, 0 <= rolloff <= 1 (0 = default), "
                        "got %d -> %d Hz, zeros %d, beta %g, rolloff %g", rate_in, rate_out, zeros, beta, rolloff);
    if (rc != 0 || resample::lds_floats(d->up, d->down, d->taps) * sizeof(float) > 64 * 1024)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "resampler %d -> %d Hz (zeros %d) is outside %d <= rate_out <= %d, up <= %d, taps <= %d "
                    "or needs more than 64 KB of LDS", rate_in, rate_out, zeros, resample::kMinRateOut, resample::kMaxRateOut,
                    resample::kMaxUp, resample::kMaxTaps);
    return IRIS_HIFIGAN_OK;
}

static_assert(IRIS_OUT_F32 == pcm::OUT_F32 && IRIS_OUT_PCM16 == pcm::OUT_PCM16 && IRIS_OUT_ULAW == pcm::OUT_ULAW &&
              IRIS_OUT_ALAW == pcm::OUT_ALAW, "the public output forms are pcm_out.h's");

// What every device entry of the stage asks of its shape before it looks at anything else.
int resampler_check(const iris_resampler_handle* h, int32_t B, int32_t L, int64_t origin) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (origin < 0 || origin > resample::kMaxOrigin)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin must lie in [0, 2^40], got %lld", (long long)origin);
    return IRIS_HIFIGAN_OK;
}

int resampler_check_size(int32_t B, int32_t L, long long n_count) {
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.y)", B);
    if (L > (1 << 30)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "%d samples per item exceed 2^30", L);
    if (n_count > 0x7fffffffll) return fail(IRIS_HIFIGAN_UNSUPPORTED, "%lld outputs per item exceed 2^31 - 1", n_count);
    return IRIS_HIFIGAN_OK;
}

// The one launch builder of the stage: the outputs [n_lo, n_lo + N) of wav [B, L], whose first sample is `origin` of its
// utterance.  The caller names ONE output form afterwards (y, pcm, y + peak, or g711 + law).
resample::ResampleLaunch resampler_launch(const iris_resampler_handle* h, const float* wav_dev, int B, int L, const int32_t* lengths_dev,
                                          int row_scale, long long origin, long long n_lo, long long N) {
    resample::ResampleLaunch a;
    a.wav = wav_dev; a.lengths = lengths_dev; a.row_scale = lengths_dev ? row_scale : 1; a.bank = h->bank;
    a.y = nullptr; a.pcm = nullptr; a.g711 = nullptr; a.law = 0; a.peak = nullptr;
    a.B = B; a.L = L; a.N = (int)N;
    a.up = h->d.up; a.down = h->d.down; a.taps = h->d.taps; a.half_width = h->d.half_width;
    a.origin = origin; a.n_lo = n_lo;
    return a;
}

// origin, Lw and n_next of a window, checked; *win is the rule's answer (csrc/resample.h: struct Window).
int resampler_window(const iris_resampler_handle* h, int64_t origin, int64_t Lw, int64_t n_next, int32_t final, resample::Window* win) {
    if (origin < 0 || Lw < 0 || origin > resample::kMaxOrigin || Lw > resample::kMaxOrigin)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin and Lw must lie in [0, 2^40], got %lld and %lld", (long long)origin, (long long)Lw);
    const long long n_end = resample::ceil_div_ll((origin + Lw) * h->d.up, h->d.down);
    if (n_next < 0 || n_next > n_end)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "n_next = %lld lies outside [0, %lld], the outputs up to the window's end", (long long)n_next, n_end);
    *win = resample::Window(h->d, origin, Lw, n_next, final != 0);
    if (!win->ok)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the window starts at sample %lld, but output %lld reads from sample %lld on: keep the "
                    "samples from the previous window's keep_from", (long long)origin, (long long)n_next,
                    (long long)n_next * h->d.down / h->d.up - h->d.half_width + 1);
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_resampler_design(int32_t rate_in, int32_t rate_out, int32_t zeros, double beta, double rolloff,
                              int32_t* up, int32_t* down, int32_t* taps, float* bank_host, uint64_t capacity) {
    IRIS_ABI_BEGIN
    if (!up || !down || !taps) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    resample::Design d;
    TRY(resampler_plan(rate_in, rate_out, zeros, beta, rolloff, &d));
    *up = d.up; *down = d.down; *taps = d.taps;
    if (!bank_host) return IRIS_HIFIGAN_OK;
    if (capacity < (uint64_t)d.up * d.taps)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bank_host holds %llu values, the bank has %llu",
                    (unsigned long long)capacity, (unsigned long long)d.up * d.taps);
    resample::fill_bank(d, bank_host);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_create(int32_t rate_in, int32_t rate_out, int32_t zeros, double beta, double rolloff,
                              iris_resampler_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    resample::Design d;
    TRY(resampler_plan(rate_in, rate_out, zeros, beta, rolloff, &d));
    std::vector<float> bank((size_t)d.up * d.taps);
    resample::fill_bank(d, bank.data());
    const int stride = resample::row_stride(d.taps);
    std::vector<float> padded((size_t)d.up * stride, 0.f);             // rows start on 16-byte boundaries
    for (int p = 0; p < d.up; ++p) memcpy(padded.data() + (size_t)p * stride, bank.data() + (size_t)p * d.taps, sizeof(float) * d.taps);
    iris_resampler_handle* h = new (std::nothrow) iris_resampler_handle;
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->d = d;
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->bank, padded.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->bank, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->bank) (void)hipFree(h->bank);
        delete h;
        return fail(IRIS_HIFIGAN_HIP_ERROR, "resampler bank upload failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_destroy(iris_resampler_handle* h) {
    if (!h) return IRIS_HIFIGAN_OK;
    if (h->bank) (void)hipFree(h->bank);
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_resampler_info(const iris_resampler_handle* h, int32_t* up, int32_t* down, int32_t* taps, int32_t* half_width) {
    if (!h || !up || !down || !taps || !half_width) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    *up = h->d.up; *down = h->d.down; *taps = h->d.taps; *half_width = h->d.half_width;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_resampler_out_range(const iris_resampler_handle* h, int64_t origin, int64_t L, int64_t* n_lo, int64_t* n_count) {
    if (!h || !n_lo || !n_count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (origin < 0 || L < 0 || origin > resample::kMaxOrigin || L > resample::kMaxOrigin)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin and L must lie in [0, 2^40], got %lld and %lld", (long long)origin, (long long)L);
    long long lo = 0, count = 0;
    resample::out_range(h->d, origin, L, &lo, &count);
    *n_lo = lo; *n_count = count;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_resampler_forward(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev,
                               int32_t row_scale, int64_t origin, float* out_f32_dev, int16_t* out_pcm_dev, float* peak_dev,
                               int32_t normalize, float peak_target, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(resampler_check(h, B, L, origin));
    if (normalize && !(peak_target > 0.f && peak_target <= 1.f))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "peak_target must lie in (0, 1], got %g", (double)peak_target);
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "wav_dev is NULL");
    if (normalize && (!out_f32_dev || !out_pcm_dev || !peak_dev))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "normalising needs out_f32_dev, out_pcm_dev and peak_dev");
    if (!normalize && !out_f32_dev && !out_pcm_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "no output: out_f32_dev and out_pcm_dev are NULL");
    if (!normalize && out_f32_dev && out_pcm_dev)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "one output form per call: fp32 or int16 (both only when normalising)");
    if (lengths_dev && row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "row_scale must be >= 1, got %d", row_scale);
    // the whole call is the final window that starts its own outputs: n_next = ceil(origin * up / down)
    const long long n_lo = resample::ceil_div_ll(origin * h->d.up, h->d.down);
    const long long n_count = resample::Window(h->d, origin, L, n_lo, true).count;
    TRY(resampler_check_size(B, L, n_count));
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    hipStream_t stream = (hipStream_t)stream_;
    if (normalize) HIP_TRY(hipMemsetAsync(peak_dev, 0, sizeof(float) * B, stream));
    if (n_count == 0) return IRIS_HIFIGAN_OK;                       // (a short window between two output positions)
    resample::ResampleLaunch a = resampler_launch(h, wav_dev, B, L, lengths_dev, row_scale, origin, n_lo, n_count);
    a.y = out_f32_dev; a.pcm = normalize ? nullptr : out_pcm_dev; a.peak = normalize ? reinterpret_cast<unsigned*>(peak_dev) : nullptr;
    HIP_TRY(resample::launch_resample(a, stream));
    if (normalize) {
        // every item's row is already 0 past its own outputs, so the plain form of the output stage converts it
        const pcm::PcmLaunch q{out_f32_dev, nullptr, 1, out_pcm_dev, peak_dev, B, (int)n_count, peak_target};
        HIP_TRY(pcm::launch_pcm_normalize(q, true, stream));
    }
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_forward_g711(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev,
                                    int32_t row_scale, int64_t origin, int32_t law, uint8_t* out_u8_dev, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(resampler_check(h, B, L, origin));
    if (law != IRIS_OUT_ULAW && law != IRIS_OUT_ALAW)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "law must be IRIS_OUT_ULAW or IRIS_OUT_ALAW, got %d", law);
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev || !out_u8_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    if (lengths_dev && row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "row_scale must be >= 1, got %d", row_scale);
    const long long n_lo = resample::ceil_div_ll(origin * h->d.up, h->d.down);
    const long long n_count = resample::Window(h->d, origin, L, n_lo, true).count;
    TRY(resampler_check_size(B, L, n_count));
    if (n_count == 0) return IRIS_HIFIGAN_OK;
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    resample::ResampleLaunch a = resampler_launch(h, wav_dev, B, L, lengths_dev, row_scale, origin, n_lo, n_count);
    a.g711 = out_u8_dev; a.law = law;
    HIP_TRY(resample::launch_resample(a, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_window_plan(const iris_resampler_handle* h, int64_t origin, int64_t Lw, int64_t n_next, int32_t final,
                                   int64_t* n_hi, int64_t* keep_from) {
    IRIS_ABI_BEGIN
    if (!h || !n_hi || !keep_from) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    resample::Window win(h->d, 0, 0, 0, false);
    TRY(resampler_window(h, origin, Lw, n_next, final, &win));
    *n_hi = win.n_hi; *keep_from = win.keep_from;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_forward_window(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t Lw, int64_t origin,
                                      int64_t n_next, int32_t final, void* out_dev, int32_t out_form, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(resampler_check(h, B, Lw, origin));
    if (out_form != IRIS_OUT_F32 && out_form != IRIS_OUT_PCM16 && out_form != IRIS_OUT_ULAW && out_form != IRIS_OUT_ALAW)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_form must be IRIS_OUT_F32, _PCM16, _ULAW or _ALAW, got %d (a window has no "
                    "normalised form: the peak is the whole item's)", out_form);
    resample::Window win(h->d, 0, 0, 0, false);
    TRY(resampler_window(h, origin, Lw, n_next, final, &win));
    TRY(resampler_check_size(B, Lw, win.count));
    if (B == 0 || Lw == 0 || win.count == 0) return IRIS_HIFIGAN_OK;            // nothing is final yet: no launch
    if (!wav_dev || !out_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    const uintptr_t align = out_form == IRIS_OUT_F32 ? 4 : out_form == IRIS_OUT_PCM16 ? 2 : 1;
    if ((uintptr_t)out_dev % align) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev is off its type's %d bytes", (int)align);
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    resample::ResampleLaunch a = resampler_launch(h, wav_dev, B, Lw, nullptr, 1, origin, n_next, win.count);
    if (out_form == IRIS_OUT_F32)        a.y = static_cast<float*>(out_dev);
    else if (out_form == IRIS_OUT_PCM16) a.pcm = static_cast<int16_t*>(out_dev);
    else                                 { a.g711 = static_cast<uint8_t*>(out_dev); a.law = out_form; }
    HIP_TRY(resample::launch_resample(a, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_resampler_forward_windows(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t in_stride,
                                       const iris_resampler_window_item* items_host, void* out_dev, int32_t out_stride, int32_t out_form,
                                       void* stream_) {
    IRIS_ABI_BEGIN
    TRY(resampler_check(h, B, in_stride, 0));
    if (out_stride < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (out_form != IRIS_OUT_F32 && out_form != IRIS_OUT_PCM16 && out_form != IRIS_OUT_ULAW && out_form != IRIS_OUT_ALAW)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_form must be IRIS_OUT_F32, _PCM16, _ULAW or _ALAW, got %d (a window has no "
                    "normalised form: the peak is the whole item's)", out_form);
    if (B > resample::kGroupMax)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "a group call takes at most %d windows, got %d: split the group", resample::kGroupMax, B);
    if ((long long)B * in_stride > 0x7fffffffll || (long long)B * out_stride > 0x7fffffffll)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d rows of %d and %d samples exceed 2^31 - 1", B, in_stride, out_stride);
    if (B > 0 && !items_host) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "items_host is NULL");
    resample::ResampleItem items[resample::kGroupMax];
    long long most = 0;
    for (int b = 0; b < B; ++b) {                                   // every row is a window of its own: the rule is struct Window's
        const iris_resampler_window_item& it = items_host[b];
        if (it.Lw < 0 || it.Lw > in_stride)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "item %d: Lw = %d lies outside [0, in_stride = %d]", b, it.Lw, in_stride);
        TRY(resampler_check(h, 1, it.Lw, it.origin));
        resample::Window win(h->d, 0, 0, 0, false);
        TRY(resampler_window(h, it.origin, it.Lw, it.n_next, it.final, &win));
        TRY(resampler_check_size(1, it.Lw, win.count));
        if (win.count > out_stride)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "item %d emits %lld outputs, out_stride = %d holds fewer", b, win.count, out_stride);
        items[b] = resample::ResampleItem{it.origin, it.n_next, (int)win.count, it.Lw};
        if (win.count > most) most = win.count;
    }
    if (B == 0 || most == 0) return IRIS_HIFIGAN_OK;                // nothing is final yet: no launch
    if (!wav_dev || !out_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    const uintptr_t align = out_form == IRIS_OUT_F32 ? 4 : out_form == IRIS_OUT_PCM16 ? 2 : 1;
    if ((uintptr_t)out_dev % align) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev is off its type's %d bytes", (int)align);
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    resample::ResampleLaunch a = resampler_launch(h, wav_dev, B, in_stride, nullptr, 1, 0, 0, out_stride);
    if (out_form == IRIS_OUT_F32)        a.y = static_cast<float*>(out_dev);
    else if (out_form == IRIS_OUT_PCM16) a.pcm = static_cast<int16_t*>(out_dev);
    else                                 { a.g711 = static_cast<uint8_t*>(out_dev); a.law = out_form; }
    HIP_TRY(resample::launch_resample_group(a, items, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

}  // extern "C"
