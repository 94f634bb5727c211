// stage_host.h -- the host scaffold of the stages around the vocoder: the PostNet (iris_hifigan.hip), the VAE decoder
// (iris_vae_decoder.hip), the text stage (iris_text_encoder.hip) and the DSP stages (stft_f32.h).  Each of them packs a weight blob, uploads it, lays
// out a workspace, checks it in front of a forward and counts its launches in a dry run; that is written here once.
// The vocoder's own create and forward (iris_hifigan.hip, generator_internal.h) do not use it.  Not installed.
#pragma once
#include <string.h>
#include <memory>
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

}  // namespace iris
