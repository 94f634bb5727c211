// iris_limiter.hip -- the iris_limiter_* entry points of include/iris_hifigan.h: a look-ahead true-peak limiter per item of a
// ragged batch of waveforms (csrc/limiter.h holds the rules and the kernels).  forward_ragged is 2 launches: the fused tile
// kernel, which stores the samples and every tile's (max p, min g), and the per-item reduction of those into stats.
// measure_ragged is the same two without the samples.  forward_window is the same two on a window of an utterance, storing the
// samples the window settles (limiter::Window in csrc/limiter.h) as fp32 or as 16-bit PCM: a session that pushes consecutive
// windows reproduces the whole-item call bit for bit.  The handle owns the design table (the interpolation bank and the
// smoothing weights); the host never reads a length.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
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

// What a call runs on: a ragged batch of whole items [B, L], a window [B, Lw] of B utterances (limiter::Window), or a group of
// windows of B utterances, one per row (`items`).
struct LmRows {
    int in_len;                 // L, or Lw; a group: the rows' stride, in_stride
    int offset, n_out;          // the row's sample that is output 0, and the outputs of a row: 0 and L, or the window's settled range;
                                // a group: 0 and the largest count of its rows
    const int32_t* lengths;     // whole items only (device, or NULL); the host never reads it
    int row_scale;
    bool pcm16;                 // out is int16: windows only
    const limiter::TileItem* items = nullptr;   // a group: what each row names itself (host)
    int out_stride = 0;         // a group: the output rows' stride; otherwise n_out
};

// Queues the launches (or, in a dry run, counts them).  out == nullptr: measure only.
int lm_forward(const LmPlan& p, const float* table, const float* wav, int B, const LmRows& r, void* out, float* stats, float* ws, hipStream_t stream) {
    const LmWorkspace lay(B, r.n_out);
    limiter::TileLaunch tl; memset(&tl, 0, sizeof(tl));
    tl.wav = wav; tl.lengths = r.lengths; tl.row_scale = r.row_scale; tl.table = table; tl.out = out; tl.parts = ws + lay.parts;
    tl.in_len = tl.in_stride = r.in_len; tl.offset = r.offset; tl.n_out = r.n_out; tl.out_stride = r.items ? r.out_stride : r.n_out;
    tl.tiles = lay.tiles; tl.A = p.A; tl.ceiling = p.ceiling;
    HIP_TRY(limiter::launch_tile(tl, r.items, B, r.pcm16, stream));

    limiter::StatsLaunch st; memset(&st, 0, sizeof(st));
    st.lengths = r.lengths; st.row_scale = r.row_scale; st.parts = tl.parts; st.stats = stats;
    st.in_len = r.in_len; st.offset = r.offset; st.n_out = r.n_out; st.tiles = lay.tiles;
    HIP_TRY(limiter::launch_stats(st, r.items, B, stream));
    return IRIS_HIFIGAN_OK;
}

int lm_run(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale, float* out_dev, bool apply,
           float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    const RaggedWaveCall call = {wav_dev, B, L, row_scale, out_dev, apply, stats_out_dev, 4, workspace_dev, 8, workspace_bytes};
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            TRY(check_wave_shape(B, L));
            *out_floats = (size_t)B * L; *ws_floats = LmWorkspace(B, L).floats;
            return IRIS_HIFIGAN_OK; },
        [&] { const LmRows rows = {L, 0, L, lengths_dev, row_scale, false};
              return lm_forward(h->p, h->blob, wav_dev, B, rows, apply ? out_dev : nullptr, stats_out_dev, (float*)workspace_dev, (hipStream_t)stream); });
}

// A window's shape and place: [B, Lw] in 32-bit offsets, one item per grid.y, and origin + Lw an int64 sample index.
int lm_check_window(int32_t B, int32_t Lw, int64_t origin) {
    TRY(check_wave_shape(B, Lw));
    if (origin < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin = %lld is negative", (long long)origin);
    if (origin > INT64_MAX - (int64_t)Lw)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "origin = %lld, Lw = %d: the window's end exceeds int64 sample indexing", (long long)origin, Lw);
    return IRIS_HIFIGAN_OK;
}

LmRows lm_window_rows(int32_t Lw, const limiter::Window& w, bool pcm16) {
    return LmRows{Lw, w.offset, (int)w.out_count, nullptr, 1, pcm16};
}

// The rows of a group call, each checked as a window of its own and planned by limiter::Window; max_count: the largest count.
int lm_group_items(const LmPlan& p, int32_t B, const iris_limiter_window_item* items_host, limiter::TileItem* items, int* max_count) {
    TRY(check_wave_shape(B, 0));
    if (B > limiter::kGroupMax)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "a group call takes at most %d windows, got %d: split the group", limiter::kGroupMax, B);
    if (B > 0 && !items_host) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "items_host is NULL");
    *max_count = 0;
    for (int b = 0; b < B; ++b) {
        const iris_limiter_window_item& it = items_host[b];
        if (it.Lw < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "item %d: Lw = %d is negative", b, it.Lw);
        TRY(lm_check_window(1, it.Lw, it.origin));
        const limiter::Window w(p.A, it.origin, it.Lw, it.final != 0);
        items[b] = limiter::TileItem{w.offset, (int)w.out_count, it.Lw, (int)((w.out_count + limiter::kTile - 1) / limiter::kTile)};
        if (items[b].n_out > *max_count) *max_count = items[b].n_out;
    }
    return IRIS_HIFIGAN_OK;
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
    TRY(check_wave_shape(B, L));
    *bytes = workspace_bytes_of(LmWorkspace(B, L).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_limiter_launch_count(const iris_limiter_config* cfg, int32_t B, int32_t L, int32_t measure_only, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    TRY(check_wave_shape(B, L));
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
        const LmRows rows = {L, 0, L, nullptr, 1, false};
        return lm_forward(p, fake, fake, B, rows, measure_only ? nullptr : fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_limiter_create(const iris_limiter_config* cfg, iris_limiter_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    std::unique_ptr<iris_limiter_handle> h;
    TRY(new_handle(&h));
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

int32_t iris_limiter_window_range(const iris_limiter_config* cfg, int64_t origin, int32_t Lw, int32_t final, int64_t* out_lo, int64_t* out_count) {
    IRIS_ABI_BEGIN
    if (!out_lo || !out_count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    TRY(lm_check_window(1, Lw, origin));
    const limiter::Window w(p.A, origin, Lw, final != 0);
    *out_lo = w.out_lo; *out_count = w.out_count;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_limiter_window_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t Lw, uint64_t* bytes) {
    return iris_limiter_workspace_bytes(cfg, B, Lw, bytes);                  // the partials of at most ceil(Lw / kTile) tiles per item
}

int32_t iris_limiter_window_launch_count(const iris_limiter_config* cfg, int32_t B, int32_t Lw, int64_t origin, int32_t final, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    TRY(lm_check_window(B, Lw, origin));
    const limiter::Window w(p.A, origin, Lw, final != 0);
    return count_forward_launches(B == 0 || w.out_count == 0, [&](float* fake) {
        return lm_forward(p, fake, fake, B, lm_window_rows(Lw, w, false), fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_limiter_forward_window(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t Lw, int64_t origin, int32_t final, void* out_dev,
                                    int32_t out_is_pcm16, float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(lm_check_window(B, Lw, origin));
    const limiter::Window w(h->p.A, origin, Lw, final != 0);
    if (w.out_count == 0) return IRIS_HIFIGAN_OK;                            // nothing is settled: nothing is looked at or launched
    const bool pcm16 = out_is_pcm16 != 0;
    if (out_dev && ((uintptr_t)out_dev & (pcm16 ? 1u : 3u))) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev must lie on %d bytes", pcm16 ? 2 : 4);
    const RaggedWaveCall call = {wav_dev, B, Lw, 1, (const float*)out_dev, true, stats_out_dev, 4, workspace_dev, 8, workspace_bytes};
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            const size_t n = (size_t)B * (size_t)w.out_count;
            *out_floats = pcm16 ? (n + 1) / 2 : n; *ws_floats = LmWorkspace(B, Lw).floats;      // what window_workspace_bytes states
            return IRIS_HIFIGAN_OK; },
        [&] { return lm_forward(h->p, h->blob, wav_dev, B, lm_window_rows(Lw, w, pcm16), out_dev, stats_out_dev, (float*)workspace_dev,
                                (hipStream_t)stream); });
    IRIS_ABI_END
}

int32_t iris_limiter_windows_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t in_stride, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (B > limiter::kGroupMax && in_stride >= 0)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "a group call takes at most %d windows, got %d: split the group", limiter::kGroupMax, B);
    return iris_limiter_workspace_bytes(cfg, B, in_stride, bytes);          // no row has more tiles than ceil(in_stride / kTile)
    IRIS_ABI_END
}

int32_t iris_limiter_windows_launch_count(const iris_limiter_config* cfg, int32_t B, const iris_limiter_window_item* items_host, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LmPlan p;
    TRY(lm_validate(cfg, &p));
    limiter::TileItem items[limiter::kGroupMax];
    int max_count = 0;
    TRY(lm_group_items(p, B, items_host, items, &max_count));
    return count_forward_launches(max_count == 0, [&](float* fake) {
        LmRows rows = {0, 0, max_count, nullptr, 1, false};
        rows.items = items; rows.out_stride = max_count;
        return lm_forward(p, fake, fake, B, rows, fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_limiter_forward_windows(iris_limiter_handle* h, const float* wav_dev, int32_t B, int32_t in_stride,
                                     const iris_limiter_window_item* items_host, void* out_dev, int32_t out_stride, int32_t out_is_pcm16,
                                     float* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(check_wave_shape(B, in_stride));
    TRY(check_wave_shape(B, out_stride));
    limiter::TileItem items[limiter::kGroupMax];
    int max_count = 0;
    TRY(lm_group_items(h->p, B, items_host, items, &max_count));
    for (int b = 0; b < B; ++b) {
        if (items[b].in_len > in_stride)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "item %d: Lw = %d exceeds in_stride = %d", b, items[b].in_len, in_stride);
        if (items[b].n_out > out_stride)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "item %d settles %d samples, out_stride = %d holds fewer", b, items[b].n_out, out_stride);
    }
    if (max_count == 0) return IRIS_HIFIGAN_OK;                              // nothing is settled: nothing is looked at or launched
    const bool pcm16 = out_is_pcm16 != 0;
    if (out_dev && ((uintptr_t)out_dev & (pcm16 ? 1u : 3u))) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev must lie on %d bytes", pcm16 ? 2 : 4);
    const RaggedWaveCall call = {wav_dev, B, in_stride, 1, (const float*)out_dev, true, stats_out_dev, 4, workspace_dev, 8, workspace_bytes};
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            const size_t n = (size_t)B * (size_t)out_stride;
            *out_floats = pcm16 ? (n + 1) / 2 : n; *ws_floats = LmWorkspace(B, in_stride).floats;   // what windows_workspace_bytes states
            return IRIS_HIFIGAN_OK; },
        [&] { LmRows rows = {in_stride, 0, max_count, nullptr, 1, pcm16};
              rows.items = items; rows.out_stride = out_stride;
              return lm_forward(h->p, h->blob, wav_dev, B, rows, out_dev, stats_out_dev, (float*)workspace_dev, (hipStream_t)stream); });
    IRIS_ABI_END
}

}  // extern "C"
