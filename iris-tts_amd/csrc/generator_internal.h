// generator_internal.h -- state shared by the translation units behind include/iris_hifigan.h
// (iris_hifigan.hip: C-ABI + fp32 path; iris_hifigan_bf16.hip: bf16-storage path).  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <utility>
#include <vector>

#include "../../include/iris_hifigan.h"
#include "device_info.h"
#include <new>

namespace iris {

constexpr int kPassFrames = 65536;       // mel frames (batch x frames) one pass of a forward processes: bounds the workspace
int pass_items(int B, int T);             // batch items of one pass
constexpr int kTileCounterWords = 256;   // per-launch next-tile counters of one forward (MRF kernel, large batches)

// forward_until: stop after MRF step `step` of stage `stage` has been queued (stage < 0: run the whole forward)
struct ForwardStop { int stage; int step; };

// What one forward leaves behind, i.e. what its conv_post stores (pcm_out.h).  The plain forward: `wav` alone.
// iris_hifigan_forward_pcm16: `pcm` alone (conv_post stores int16 in place of the waveform), or -- normalising -- all three:
// conv_post stores `wav` and reduces `peak`, and a second kernel writes `pcm` from them.  forward_until: nothing.
struct ForwardOut {
    float* wav = nullptr;       // [B, hop*T] fp32
    int16_t* pcm = nullptr;     // [B, hop*T]
    float* peak = nullptr;      // [B] per-item max |wav|; non-null = peak-normalised PCM
    float target = 0.f;         // the peak's value after normalisation, in (0, 1]
    bool normalize() const { return peak != nullptr; }
    ForwardOut advanced(size_t items, size_t samples_per_item) const {      // the same buffers from batch item `items` on
        ForwardOut o = *this;
        if (wav) o.wav += items * samples_per_item;
        if (pcm) o.pcm += items * samples_per_item;
        if (peak) o.peak += items;
        return o;
    }
    // fills the output fields of a conv_post launch descriptor (post::ConvPostLaunch, b16::PostLaunch)
    template <class A> void to_post(A& a) const {
        a.y = wav;
        a.pcm = normalize() ? nullptr : pcm;
        a.peak = normalize() ? reinterpret_cast<unsigned*>(peak) : nullptr;
    }
};

// Runs the rest of the scope under the handle's device and restores the caller's (a process may hold generators on
// several GPUs; launches, events and the CU-count-based launch plans must all refer to the handle's device).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev, bool active = true) {      // (!active: a host-only handle has no device to select)
        if (!active) return;
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// records the message for iris_hifigan_last_error() and returns `code`
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ::iris::fail(IRIS_HIFIGAN_HIP_ERROR, "%s failed: %s (%s:%d)", #expr,      \
                                hipGetErrorString(e__), __FILE__, __LINE__);                 \
    } while (0)

#define TRY(expr) do { int rc__ = (expr); if (rc__ != IRIS_HIFIGAN_OK) return rc__; } while (0)

// Every extern "C" body that can allocate runs between these: no C++ exception crosses the ABI (include/iris_hifigan.h).
#define IRIS_ABI_BEGIN try {
#define IRIS_ABI_END                                                                                              \
    } catch (const std::bad_alloc&) {                                                                             \
        return ::iris::fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed (%s)", __func__);                 \
    } catch (...) {                                                                                               \
        return ::iris::fail(IRIS_HIFIGAN_HIP_ERROR, "unexpected C++ exception in %s", __func__);                  \
    }

struct ConvLayer {       // one Conv1d / ConvTranspose1d, weights resident on the device
    int kind = 0;                                     // 0 Conv1d, 1 ConvTranspose1d, 2 conv_post
    int C_in = 0, C_out = 0, k = 0, dil = 1, u = 1;  // u = stride of a ConvTranspose1d
    size_t w_off = 0, b_off = 0;                      // float offsets into the device blob
    size_t w_floats = 0;                              // packed size
    size_t ref_w_floats = 0;                          // size in the reference layout
    size_t w16_off = 0, w16_halfs = 0;                // bf16 path: offset/size (bf16 elements) in blob16
    size_t ws3_off = 0;                               // split path (ResBlock convs): offset (bf16 elements) of the hi plane in blob_s3
    size_t w16f_off = (size_t)-1;                     // small-problem kernel: float offset of the 16x16x4 packing in blob_w16, or -1
};

struct Stage {
    ConvLayer up;
    int C = 0;             // channels after the upsample
    int rate = 1;
    // convs[j][m][0|1] = resblocks[i*nk + j].convs{1,2}[m]
    std::vector<std::vector<ConvLayer>> c1, c2;
};

}  // namespace iris

struct iris_hifigan_handle {
    iris_hifigan_config cfg;
    iris::ConvLayer pre, post;
    std::vector<iris::Stage> stages;
    float* blob = nullptr;   // device: packed fp32 weights + biases
    size_t blob_floats = 0;
    unsigned* tile_counters = nullptr;  // device: one next-tile counter per MRF launch of a forward (zeroed per forward)
    uint16_t* blob16 = nullptr;  // device: packed bf16 weights (biases stay fp32 in `blob`)
    size_t blob16_halfs = 0;
    uint16_t* blob_s3 = nullptr; // device: hi/mid bf16 planes of the ResBlock conv weights (split-product mode), or null
    float* blob_w16 = nullptr;   // device: ResBlock conv weights in v_mfma_f32_16x16x4_f32 fragment order (small-problem kernel), or null
    int hop = 1;
    int device = 0;
    // create uploads both fp32 packings; those of the other dtypes are built on first use (iris_hifigan_prepare, or the
    // first forward of the dtype): the reference-layout weights are kept on the host until both exist or the caller
    // releases them (iris_hifigan_release_host_weights).  built_* = the build succeeded, or the config cannot have it.
    std::vector<float> ref_weights;
    bool built_bf16 = false, built_s3 = false;
    bool host_only = false;     // iris_hifigan_describe_plan: no device memory behind the pointers, nothing is launched
    // profiling
    int profiling = 0;          // 0 off, 1 one record per launch, 2 the MRF launches of a stage share one record
    int profiling_paused = 0;   // records are kept, forwards add none (hipGraph capture)
    std::vector<hipEvent_t> ev;          // event pool, n_ev in use
    size_t n_ev = 0;
    std::vector<iris_hifigan_launch_record> recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> rec_ev;  // (start, end) event of each record
    int n_rec = 0;
};

namespace iris {

// Walks the layers in blob order; fn(layer&) for each.
template <class Fn>
void for_each_layer(iris_hifigan_handle* h, Fn fn) {
    fn(h->pre);
    for (auto& st : h->stages) {
        fn(st.up);
        for (size_t j = 0; j < st.c1.size(); ++j) {
            for (auto& l : st.c1[j]) fn(l);
            for (auto& l : st.c2[j]) fn(l);
        }
    }
    fn(h->post);
}

// Launch timing with ONE event per launch boundary: event e_k sits between launch k-1 and launch k
// of a forward, so launch k lasted elapsed(e_k, e_{k+1}) (its start-up gap included).  A forward of
// n launches records n + 1 events.
struct Prof {
    iris_hifigan_handle* h;
    hipStream_t stream;
    int idx = 0;        // next record
    bool open = false;  // a start event for the next launch is already on the stream
    bool pending = false;  // grouped mode: record idx covers the MRF launches of a stage so far and has no end event yet
    int mark(hipEvent_t* out) {
        if (h->n_ev >= h->ev.size()) {
            const size_t old = h->ev.size();
            h->ev.resize(old + 64);
            for (size_t i = old; i < h->ev.size(); ++i) HIP_TRY(hipEventCreate(&h->ev[i]));
        }
        *out = h->ev[h->n_ev++];
        HIP_TRY(hipEventRecord(*out, stream));
        return IRIS_HIFIGAN_OK;
    }
    // grouped mode (set_profiling(h, 2)): the MRF launches of a stage share ONE record (flops and bytes summed,
    // `launches` counted), so a forward carries 11 events instead of 31 -- an event costs ~3 us of stream time
    int close_group() {
        if (!pending) return IRIS_HIFIGAN_OK;
        int rc = mark(&h->rec_ev[idx].second);
        if (rc != IRIS_HIFIGAN_OK) return rc;
        pending = false;
        open = true;
        ++idx;
        return IRIS_HIFIGAN_OK;
    }
    bool on() const { return h->profiling && !h->profiling_paused; }
    int begin(int kind, int stage, int step, double flops, double bytes) {
        if (!on()) return IRIS_HIFIGAN_OK;
        const bool grouped = h->profiling == 2 && kind == 2;
        if (pending) {
            iris_hifigan_launch_record& g = h->recs[idx];
            if (grouped && g.stage == stage) { g.flops += flops; g.bytes += bytes; g.launches += 1; return IRIS_HIFIGAN_OK; }
            int rc = close_group();
            if (rc != IRIS_HIFIGAN_OK) return rc;
        }
        if ((size_t)idx >= h->recs.size()) { h->recs.resize(idx + 64); h->rec_ev.resize(idx + 64); }
        iris_hifigan_launch_record& r = h->recs[idx];
        memset(&r, 0, sizeof(r));
        r.kind = kind; r.stage = stage; r.step = step; r.launches = 1; r.flops = flops; r.bytes = bytes;
        if (!open) {
            int rc = mark(&h->rec_ev[idx].first);
            if (rc != IRIS_HIFIGAN_OK) return rc;
        } else {
            h->rec_ev[idx].first = h->rec_ev[idx - 1].second;
        }
        pending = grouped;
        return IRIS_HIFIGAN_OK;
    }
    int end() {
        if (!on() || pending) return IRIS_HIFIGAN_OK;
        int rc = mark(&h->rec_ev[idx].second);
        if (rc != IRIS_HIFIGAN_OK) return rc;
        open = true;
        ++idx;
        return IRIS_HIFIGAN_OK;
    }
    // end of a forward (or of forward_until): closes an open group and publishes the record count
    int finish() {
        if (!on()) return IRIS_HIFIGAN_OK;
        int rc = close_group();
        if (rc != IRIS_HIFIGAN_OK) return rc;
        h->n_rec = idx;
        return IRIS_HIFIGAN_OK;
    }
};

// ---- workspace layout of one pass of B x T mel frames, in elements of the dtype's storage ----
struct WsLayout {
    size_t pre;   // conv_pre output                [B, T, C0]
    size_t up;    // upsample output of a stage     [B, L, C]     (max over stages)
    size_t y[IRIS_HIFIGAN_MAX_KERNELS];   // running x of branch j
    size_t xt[IRIS_HIFIGAN_MAX_KERNELS];  // conv1 output of branch j
    size_t total;
    size_t elem_bytes;                    // 2 (bf16 storage) or 4; every buffer starts on a multiple of 256 bytes
    uint64_t bytes() const { return (uint64_t)total * elem_bytes; }
};

inline WsLayout ws_layout(const iris_hifigan_handle* h, int B, int T, int32_t dtype) {
    WsLayout w;
    w.elem_bytes = dtype == IRIS_HIFIGAN_BF16 ? 2 : 4;
    const size_t round = 256 / w.elem_bytes - 1;
    const size_t frames = (size_t)B * T;
    size_t per_frame_max = 0, L = 1;
    for (const auto& st : h->stages) {
        L *= st.rate;
        const size_t e = L * st.C;
        if (e > per_frame_max) per_frame_max = e;
    }
    size_t off = 0;
    auto take = [&](size_t elems) { size_t o = off; off += (elems + round) & ~round; return o; };
    w.pre = take(frames * h->pre.C_out);
    w.up = take(frames * per_frame_max);
    for (int j = 0; j < h->cfg.num_kernels; ++j) {
        w.y[j] = take(frames * per_frame_max);
        w.xt[j] = take(frames * per_frame_max);
    }
    w.total = off;
    return w;
}

// ---- MRF: the launches of one stage as data (plan_mrf_stage, iris_hifigan.hip; plan_mrf_stage_bf16, iris_hifigan_bf16.hip) ----
enum WsBuf : uint8_t { WS_NONE, WS_UP, WS_Y, WS_XT };        // the stage's upsample output; y[j] / xt[j] of branch j
enum StepKind : uint8_t {
    STEP_PAIR,        // conv1 -> conv2 + residual of one dilation in ONE launch (mrf_pair_f32.h, mrf_pair_bf16.h)
    STEP_PAIR_SUM,    // ... the stage's last pair on a kernel that stores only the MRF mean (mrf_pair_f32_pf.h, mrf_pair_bf16.h)
    STEP_CONV1,       // convs1[m] of all branches
    STEP_CONV2,       // convs2[m] + residual of all branches
    STEP_CONV2_SUM,   // ... the stage's last step, storing only the MRF mean (fp32 storage)
};
enum StepMean : uint8_t {
    MEAN_NONE,        // the step writes every branch's output to `y`
    MEAN_IN_Y,        // it leaves mean_j(branch j) in `y` of branch 0 and no branch outputs (bf16 storage: activated and rounded)
    MEAN_F32_IN_UP,   // bf16 storage, last stage: the fp32 mean over `up` + y[0], adjacent in the workspace (`y` is WS_UP)
};
struct MrfStep {
    StepKind kind;
    bool split;             // the conv steps on split-bf16 products (conv_mfma_f32s.h)
    int m, half;            // MRF step 2 * m + half of the stage (a pair carries its second step's index)
    WsBuf x, res, y;        // per branch: what the step reads, adds as the residual (conv2) and writes
    StepMean mean;
};
// What a stage hands to the next layer: every branch's output in `buf` (MEAN_NONE; the consumer forms the mean), or the mean.
struct StageOut { StepMean mean; WsBuf buf; };
struct MrfStagePlan {
    int n;
    MrfStep s[2 * IRIS_HIFIGAN_MAX_DILATIONS];
    StageOut out() const { return StageOut{s[n - 1].mean, s[n - 1].y}; }
};

// Device memory of a single-layer entry point (packed weights, a bias): freed when the call returns.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t upload(const void* src, size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    template <class T> hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size() * sizeof(T)); }
    const float* f32() const { return (const float*)p; }
};

// ---- bf16-storage path (iris_hifigan_bf16.hip) ----
int bf16_build_blob(iris_hifigan_handle* h, const float* weights_host);   // packs + uploads blob16 (host_only: packs only)
int bf16_forward(iris_hifigan_handle* h, const void* mel_dev, int B, int T, const ForwardOut& out,
                 void* workspace_dev, uint64_t workspace_bytes, hipStream_t stream, const ForwardStop& stop,
                 int32_t* until_flags);

// ---- fp32 storage with split-bf16 products for the ResBlock convs (conv_mfma_f32s.h; iris_hifigan_bf16.hip) ----
int f32s_build_blob(iris_hifigan_handle* h, const float* weights_host);   // packs + uploads blob_s3 (null if unsupported)
// one grouped MRF step (all branches): x/res/y pointers per branch as in the fp32 path
struct F32sStep { const float* x[IRIS_HIFIGAN_MAX_KERNELS]; const float* res[IRIS_HIFIGAN_MAX_KERNELS];
                  float* y[IRIS_HIFIGAN_MAX_KERNELS]; const ConvLayer* layer[IRIS_HIFIGAN_MAX_KERNELS]; };
bool f32s_step_applicable(const iris_hifigan_handle* h, int C, int L, int nk);
// sum_y: when set, the step stores only the mean of the branch outputs there (last conv step of a stage)
int f32s_launch_step(iris_hifigan_handle* h, const F32sStep& st, int nk, int B, int L, int C, float* sum_y, hipStream_t stream);

}  // namespace iris
