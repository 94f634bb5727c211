// stage_host.h -- the host scaffold of the stages around the vocoder: the PostNet (iris_hifigan.hip), the VAE decoder
// (iris_vae_decoder.hip), the text stage (iris_text_encoder.hip) and the DSP stages (stft_f32.h).  Each of them packs a weight blob, uploads it, lays
// out a workspace, checks it in front of a forward and counts its launches in a dry run; that is written here once.
// The waveform stages (iris_mel_frontend.hip, iris_griffin_lim.hip, iris_denoiser.hip, iris_time_stretch.hip, iris_assemble.hip,
// iris_loudness.hip, iris_limiter.hip, iris_spectral_distance.hip) also take from here what their entry points repeat: the handle's allocation, the bytes
// of a workspace, the launch count of a forward that may be empty, the overlap test, the plain [B, L] shape check, and the
// whole prologue of a forward on a ragged batch of waveforms (run_ragged_wave).
// The vocoder's own create and forward (iris_hifigan.hip, generator_internal.h) do not use it.  Not installed.
#pragma once
#include <string.h>
#include <memory>
#include <new>
#include <vector>

#include "generator_internal.h"
#include "packed_conv_f32.h"

namespace iris {

// One Conv1d / Dense that runs as an MFMA GEMM: its shape and where its packed weights and its bias lie in the blob.
struct PackedGemm { int C_in = 0, C_out = 0, k = 1; size_t w_off = 0, b_off = 0; };   // float offsets into the device blob

// Builds the host image of a stage's device blob from the caller's weights (`src` walks them in order): GEMM weights in
// fragment order, everything else as it comes.  Every tensor starts on 4 floats (16 bytes); the padding is zero.
struct BlobBuilder {
    std::vector<float> host;
    const float* src;
    explicit BlobBuilder(const float* weights_host) : src(weights_host) {}
    size_t reserve(size_t n) { size_t o = host.size(); host.resize(o + ((n + 3) & ~(size_t)3), 0.f); return o; }
    void take(float* dst, size_t n) { memcpy(dst, src, sizeof(float) * n); src += n; }      // the next n values, to anywhere
    size_t raw(size_t n) { const size_t o = reserve(n); take(host.data() + o, n); return o; }
    // w [C_out][C_in][k] and its bias from anywhere (C_out may be 0: nothing is read)
    void dense(PackedGemm& l, const float* w, const float* bias, int C_in, int C_out, int k) {
        l.C_in = C_in; l.C_out = C_out; l.k = k;
        l.w_off = reserve(packed_conv1d_floats(C_in, C_out, k));
        pack_conv1d_weights(w, C_in, C_out, k, host.data() + l.w_off);
        l.b_off = reserve(C_out);
        if (C_out) memcpy(host.data() + l.b_off, bias, sizeof(float) * C_out);
    }
    void dense(PackedGemm& l, int C_in, int C_out, int k) {     // the next tensor of src, followed by its bias
        const size_t nw = (size_t)C_in * C_out * k;
        dense(l, src, src + nw, C_in, C_out, k);
        src += nw + C_out;
    }
};

// What every stage handle owns: the device blob and the device it lives on.  `delete h` frees both.
struct StageHandle {
    float* blob = nullptr;
    int device = 0;
    StageHandle() = default;
    StageHandle(const StageHandle&) = delete;
    StageHandle& operator=(const StageHandle&) = delete;
    ~StageHandle() { if (blob) (void)hipFree(blob); }
};

// Uploads the image to the current device, which becomes the handle's.  `what` names the stage in the error text.
inline int upload(const std::vector<float>& host, StageHandle* h, const char* what) {
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = hipMalloc(&h->blob, host.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->blob, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "%s weight upload failed: %s", what, hipGetErrorString(e));
    return IRIS_HIFIGAN_OK;
}

// Lays the buffers of a workspace out one behind the other, in floats; every buffer starts on 256 bytes.
struct WsTaker {
    size_t off = 0;
    size_t take(size_t n) { const size_t o = off; off += (n + 63) & ~(size_t)63; return o; }
};

// The last check of every forward, behind the entry point's own argument checks: the workspace is large enough, and the
// rest of the caller's scope runs under the handle's device.  Use:  ForwardScope scope(*h, workspace_bytes, need_floats); TRY(scope.rc);
struct ForwardScope {
    int rc;
    DeviceGuard guard;          // selects nothing when the workspace is too small
    ForwardScope(const StageHandle& h, uint64_t workspace_bytes, size_t need_floats)
        : rc(check_workspace(workspace_bytes, (uint64_t)need_floats * sizeof(float))), guard(h.device, rc == IRIS_HIFIGAN_OK) {
        if (guard.err != hipSuccess) rc = fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h.device, hipGetErrorString(guard.err));
    }
    static int check_workspace(uint64_t have, uint64_t need) {
        if (have >= need) return IRIS_HIFIGAN_OK;
        return fail(IRIS_HIFIGAN_WORKSPACE_TOO_SMALL, "workspace has %llu bytes, need %llu", (unsigned long long)have, (unsigned long long)need);
    }
};

// A stage whose grid.y is the batch takes at most 65535 items.
inline int check_batch(int32_t B) {
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.y)", B);
    return IRIS_HIFIGAN_OK;
}

// Counts the launches of `run` instead of issuing them: the forward's own code in a dry run.  `run` gets a pointer to pass
// wherever the forward wants device memory (no pointer is dereferenced).
template <class Fn> int count_launches(Fn run, int32_t* n) {
    DryRun d{nullptr, 0, 0, 256};
    DryRun* const prev = dry_run_slot();
    dry_run_slot() = &d;
    const int rc = run(reinterpret_cast<float*>(uintptr_t(256)));
    dry_run_slot() = prev;
    TRY(rc);
    *n = d.n;
    return IRIS_HIFIGAN_OK;
}

// ---- the waveform stages (mel front-end, Griffin-Lim, denoiser, time stretch, assemble, loudness, limiter) ----------------------

// What a *_launch_count answers behind its config and shape checks: 0 for a forward that returns before its first launch
// (`empty`), else the launches of `run`, the forward in a dry run.
template <class Fn> int count_forward_launches(bool empty, Fn run, int32_t* n) {
    *n = 0;
    if (empty) return IRIS_HIFIGAN_OK;
    return count_launches(run, n);
}

// A handle of a stage, or the failure of the host allocation.
template <class H> int new_handle(std::unique_ptr<H>* h) {
    h->reset(new (std::nothrow) H);
    if (!*h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    return IRIS_HIFIGAN_OK;
}

// What a *_workspace_bytes answers for a layout of `floats`: no workspace is smaller than one buffer's alignment.
inline uint64_t workspace_bytes_of(size_t floats) {
    const uint64_t bytes = (uint64_t)floats * sizeof(float);
    return bytes < 256 ? 256 : bytes;
}

// Do the na floats at a and the nb floats at b share a byte?
inline bool overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb * sizeof(float) && y < x + na * sizeof(float);
}

// A batch of B waveforms of L samples each whose kernels index the B L samples in 32 bits, one item per grid.y.
inline int check_wave_shape(int32_t B, int32_t L) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    TRY(check_batch(B));
    if ((long long)B * L > 0x7fffffffll) return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d, L = %d: %lld samples exceed 32-bit offsets", B, L, (long long)B * L);
    return IRIS_HIFIGAN_OK;
}

// The arguments of a forward on a ragged batch of waveforms (wav [B, L], item b owning lengths[b] * row_scale samples) that the
// assemble, loudness and limiter stages check alike.  `stats`: the per-item results (statistics, or the join's integers);
// `stats_align`, `workspace_align`: the bytes each must lie on, 0 for no demand beyond its type's.
struct RaggedWaveCall {
    const float* wav;
    int32_t B, L, row_scale;
    const float* out;
    bool want_out;                  // false: a measuring call, `out` is not looked at
    const void* stats;
    int stats_align;
    const void* workspace;
    int workspace_align;
    uint64_t workspace_bytes;
};

// Every check of such a forward in one order -- handle, row_scale, `shape`, the empty batch (OK, nothing is launched), NULL
// pointers, alignment, overlap, workspace -- and then `forward` under the handle's device.  `shape(&out_floats, &ws_floats)`
// is the stage's shape check; it says how many floats `out` holds and how many the workspace needs.
template <class Shape, class Forward>
int run_ragged_wave(const StageHandle* h, const RaggedWaveCall& c, Shape shape, Forward forward) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (c.row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "row_scale >= 1 is required, got %d", c.row_scale);
    size_t out_floats = 0, ws_floats = 0;
    TRY(shape(&out_floats, &ws_floats));
    if (c.B == 0 || c.L == 0) return IRIS_HIFIGAN_OK;
    if (!c.wav || (c.want_out && !c.out) || !c.stats || !c.workspace) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (c.stats_align && ((uintptr_t)c.stats & (uintptr_t)(c.stats_align - 1)))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "stats_out_dev must lie on %d bytes", c.stats_align);
    if (c.workspace_align && ((uintptr_t)c.workspace & (uintptr_t)(c.workspace_align - 1)))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "workspace_dev must lie on %d bytes", c.workspace_align);
    if (c.want_out && overlap(c.wav, (size_t)c.B * c.L, c.out, out_floats)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev overlaps wav_dev");
    ForwardScope scope(*h, c.workspace_bytes, ws_floats);
    TRY(scope.rc);
    return forward();
}

}  // namespace iris
