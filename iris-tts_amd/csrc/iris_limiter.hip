// iris_limiter.hip -- the iris_limiter_* entry points of include/iris_hifigan.h: a look-ahead true-peak limiter per item of a
// ragged batch of waveforms (csrc/limiter.h holds the rules and the kernels).  forward_ragged is 2 launches: the fused tile
// kernel, which stores the samples and every tile's (max p, min g), and the per-item reduction of those into stats.
// measure_ragged is the same two without the samples.  The handle owns the design table (the interpolation bank and the
// smoothing weights); the host never reads a length.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "limiter.h"
#include "stage_host.h"

using namespace iris;

namespace {

// A checked config.
struct LmPlan {
    float ceiling = 0.f;
    int A = 0;
};

}  // namespace

struct iris_limiter_handle : StageHandle {
    LmPlan p;
};

namespace {

int lm_validate(const iris_limiter_config* c, LmPlan* p) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (!isfinite(c->ceiling) || !(c->ceiling > 0.f) || c->ceiling > 1.f)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "ceiling must be an amplitude in (0, 1], got %g", (double)c->ceiling);
    if (c->lookahead < 1 || c->lookahead > limiter::kMaxLookahead)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "lookahead must lie in 1 .. %d samples, got %d", limiter::kMaxLookahead, c->lookahead);
    p->ceiling = c->ceiling; p->A = c->lookahead;
    return IRIS_HIFIGAN_OK;
}

int lm_check_shape(int32_t B, int32_t L) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    TRY(check_batch(B));
    if ((long long)B * L > 0x7fffffffll) return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d, L = %d: %lld samples exceed 32-bit offsets", B, L, (long long)B * L);
    return IRIS_HIFIGAN_OK;
}

int lm_design(const LmPlan& p, float* out) {
    if (!limiter::fill_design(p.A, out)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "the resampler's bank builder does not give 4 : 1 with 12 taps");
    return IRIS_HIFIGAN_OK;
}

// parts [B][tiles][2] (fp32), starting on 256 bytes.
struct LmWorkspace {
    size_t parts, floats;
    int tiles;
    LmWorkspace(int B, int L) {
        tiles = (int)(((long long)L + limiter::kTile - 1) / limiter::kTile);
        WsTaker ws;
        parts = ws.take((size_t)B * tiles * 2);
        floats = ws.off;
    }
};

// Queues the launches (or, in a dry run, counts them).  out == nullptr: measure only.
int lm_forward(const LmPlan& p, const float* table, const float* wav, int B, int L, const int32_t* lengths, int row_scale, float* out, float* stats,
               float* ws, hipStream_t stream) {
    const LmWorkspace lay(B, L);
    limiter::TileLaunch tl; memset(&tl, 0, sizeof(tl));
    tl.wav = wav; tl.lengths = lengths; tl.row_scale = row_scale; tl.table = table; tl.out = out; tl.parts = ws + lay.parts;
    tl.L = L; tl.tiles = lay.tiles; tl.A = p.A; tl.ceiling = p.ceiling;
    HIP_TRY(limiter::launch_tile(tl, B, stream));

    limiter::StatsLaunch st; memset(&st, 0, sizeof(st));
    st.lengths = lengths; st.row_scale = row_scale; st.parts = tl.parts; st.stats = stats; st.L = L; st.tiles = lay.tiles;
    HIP_TRY(limiter::launch_stats(st, B, stream));
    return IRIS_HIFIGAN_OK;
}

bool overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb * sizeof(float) && y < x + na * sizeof(float);
}

int lm_run(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale, float* out_dev, bool apply,
           float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (row_scale < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "row_scale >= 1 is required, got %d", row_scale);
    TRY(lm_check_shape(B, L));
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev || (apply && !out_dev) || !stats_out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if ((uintptr_t)stats_out_dev & 3) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "stats_out_dev must lie on 4 bytes");
    if ((uintptr_t)workspace_dev & 7) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "workspace_dev must lie on 8 bytes");
    if (apply && overlap(wav_dev, (size_t)B * L, out_dev, (size_t)B * L)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev overlaps wav_dev");
    ForwardScope scope(*h, workspace_bytes, LmWorkspace(B, L).floats);
    TRY(scope.rc);
    return lm_forward(h->p, h->blob, wav_dev, B, L, lengths_dev, row_scale, apply ? out_dev : nullptr, stats_out_dev, (float*)workspace_dev,
                      (hipStream_t)stream);
}

}  // namespace

extern "C" {

int32_t iris_limiter_design(const iris_limiter_config* cfg, float* out, uint64_t n) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    if (n != (uint64_t)limiter::design_floats(p.A))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the design table has %d floats, got room for %llu", limiter::design_floats(p.A), (unsigned long long)n);
    return lm_design(p, out);
    IRIS_ABI_END
}

int32_t iris_limiter_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t L, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    TRY(lm_check_shape(B, L));
    *bytes = (uint64_t)LmWorkspace(B, L).floats * sizeof(float);
    if (*bytes < 256) *bytes = 256;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_limiter_launch_count(const iris_limiter_config* cfg, int32_t B, int32_t L, int32_t measure_only, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    TRY(lm_check_shape(B, L));
    *n = 0;
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    return count_launches([&](float* fake) { return lm_forward(p, fake, fake, B, L, nullptr, 1, measure_only ? nullptr : fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_limiter_create(const iris_limiter_config* cfg, iris_limiter_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    std::unique_ptr<iris_limiter_handle> h(new (std::nothrow) iris_limiter_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->p = p;
    std::vector<float> host((size_t)limiter::design_floats(p.A));
    TRY(lm_design(p, host.data()));
    TRY(upload(host, h.get(), "limiter"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_limiter_destroy(iris_limiter_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_limiter_forward_ragged(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                                    float* out_dev, float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return lm_run(h, wav_dev, B, L, lengths_dev, row_scale, out_dev, true, stats_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_limiter_measure_ragged(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                                    float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return lm_run(h, wav_dev, B, L, lengths_dev, row_scale, nullptr, false, stats_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

}  // extern "C"
