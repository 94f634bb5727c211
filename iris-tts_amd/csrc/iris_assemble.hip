// iris_assemble.hip -- the iris_assemble_* entry points of include/iris_hifigan.h: silence trim and sentence join of a ragged
// batch of waveforms (csrc/assemble.h holds the rules and the kernels).  A forward is 3 launches: the frames' energies, the
// items' bounds, and the gather that lays the trimmed items end to end (forward) or each in its own row (trim_ragged).  The
// handle owns the fade ramp; the host never reads a length.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "assemble.h"
#include "stage_host.h"

using namespace iris;

namespace {

// A checked config: the config's integers, k and the squared absolute reference.
struct AsPlan {
    int F = 0, H = 0, pad = 0, fade = 0, pause = 0;
    float k = 0.f, ref_sq = 0.f;
};

}  // namespace

struct iris_assemble_handle : StageHandle {
    AsPlan p;
    size_t ramp_off = 0;
};

namespace {

int as_validate(const iris_assemble_config* c, AsPlan* p) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->frame_length < 2 || c->frame_length % 2 || c->hop_length < 1 || (c->frame_length / 2) % c->hop_length)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "frame_length %d must be even and hop_length %d must divide its half (a frame is whole hop_length blocks)",
                    c->frame_length, c->hop_length);
    if (!isfinite(c->top_db) || !(c->top_db > 0.f)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "top_db must be finite and above 0, got %g", (double)c->top_db);
    if (!isfinite(c->ref) || c->ref < 0.f) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "ref must be finite and at least 0 (0: the item's own maximum), got %g", (double)c->ref);
    if (c->pad_samples < 0 || c->fade_samples < 0 || c->pause_samples < 0)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "pad_samples, fade_samples and pause_samples must not be negative");
    if (c->frame_length > assemble::kMaxFrame) return fail(IRIS_HIFIGAN_UNSUPPORTED, "frame_length %d exceeds %d", c->frame_length, assemble::kMaxFrame);
    if (c->fade_samples > assemble::kMaxFade) return fail(IRIS_HIFIGAN_UNSUPPORTED, "fade_samples %d exceeds %d", c->fade_samples, assemble::kMaxFade);
    p->F = c->frame_length; p->H = c->hop_length; p->pad = c->pad_samples; p->fade = c->fade_samples; p->pause = c->pause_samples;
    p->k = (float)pow(10.0, -(double)c->top_db / 10.0);
    p->ref_sq = c->ref * c->ref;
    return IRIS_HIFIGAN_OK;
}

// cap of the join (rows == 0) or of the rows form, which has no pause
int as_check_shape(const AsPlan& p, int32_t B, int32_t L, int rows, long long* cap) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (B > assemble::kMaxBatch) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds %d (the join stages the items' offsets in LDS)", B, assemble::kMaxBatch);
    const long long BL = (long long)B * L, c = BL + (rows || B == 0 ? 0 : (long long)p.pause * (B - 1));
    if (BL > 0x7fffffffll || c > 0x7fffffffll)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d, L = %d, pause = %d: %lld samples exceed 32-bit offsets", B, L, p.pause, c);
    *cap = c;
    return IRIS_HIFIGAN_OK;
}

// mse [B][T], then spans [B][2] (int32), each starting on 256 bytes.
struct AsWorkspace {
    size_t mse, spans, floats;
    int T;
    AsWorkspace(const AsPlan& p, int B, int L) {
        T = L / p.H + 1;
        WsTaker ws;
        mse = ws.take((size_t)B * T);
        spans = ws.take((size_t)B * 2);
        floats = ws.off;
    }
};

// Queues the three launches (or, in a dry run, counts them).  `ints_out`: offsets [B + 1] of the join, counts [B] of the rows form.
int as_forward(const AsPlan& p, const float* ramp, const float* wav, int B, int L, const int32_t* lengths, int row_scale, float* out, int cap,
               int rows, int32_t* spans_out, int32_t* ints_out, float* ws, hipStream_t stream) {
    const AsWorkspace lay(p, B, L);
    int32_t* spans = reinterpret_cast<int32_t*>(ws + lay.spans);

    assemble::EnergyLaunch en; memset(&en, 0, sizeof(en));
    en.wav = wav; en.lengths = lengths; en.row_scale = row_scale; en.mse = ws + lay.mse; en.L = L; en.T = lay.T; en.F = p.F; en.H = p.H;
    HIP_TRY(assemble::launch_energy(en, B, stream));

    assemble::BoundsLaunch bo; memset(&bo, 0, sizeof(bo));
    bo.mse = ws + lay.mse; bo.lengths = lengths; bo.row_scale = row_scale; bo.spans = spans; bo.L = L; bo.T = lay.T; bo.H = p.H; bo.pad = p.pad;
    bo.ref_sq = p.ref_sq; bo.k = p.k;
    HIP_TRY(assemble::launch_bounds(bo, B, stream));

    assemble::GatherLaunch ga; memset(&ga, 0, sizeof(ga));
    ga.wav = wav; ga.spans = spans; ga.ramp = ramp; ga.out = out; ga.spans_out = spans_out; ga.offsets_out = ints_out;
    ga.B = B; ga.L = L; ga.cap = cap; ga.fade = p.fade; ga.pause = rows ? 0 : p.pause; ga.rows = rows;
    HIP_TRY(assemble::launch_gather(ga, stream));
    return IRIS_HIFIGAN_OK;
}

int as_run(iris_assemble_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale, float* out_dev, int rows,
           int32_t* spans_out_dev, int32_t* ints_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    const RaggedWaveCall call = {wav_dev, B, L, row_scale, out_dev, true, ints_out_dev, 0, workspace_dev, 0, workspace_bytes};
    long long cap = 0;
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            TRY(as_check_shape(h->p, B, L, rows, &cap));
            *out_floats = (size_t)cap; *ws_floats = AsWorkspace(h->p, B, L).floats;
            return IRIS_HIFIGAN_OK; },
        [&] { return as_forward(h->p, h->blob + h->ramp_off, wav_dev, B, L, lengths_dev, row_scale, out_dev, (int)cap, rows, spans_out_dev,
                                ints_out_dev, (float*)workspace_dev, (hipStream_t)stream); });
}

}  // namespace

extern "C" {

int32_t iris_assemble_out_capacity(const iris_assemble_config* cfg, int32_t B, int32_t L, int64_t* cap) {
    IRIS_ABI_BEGIN
    if (!cap) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    AsPlan p;
    TRY(as_validate(cfg, &p));
    long long c = 0;
    TRY(as_check_shape(p, B, L, 0, &c));
    *cap = c;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_assemble_workspace_bytes(const iris_assemble_config* cfg, int32_t B, int32_t L, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    AsPlan p;
    TRY(as_validate(cfg, &p));
    long long c = 0;
    TRY(as_check_shape(p, B, L, 0, &c));
    *bytes = workspace_bytes_of(AsWorkspace(p, B, L).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_assemble_launch_count(const iris_assemble_config* cfg, int32_t B, int32_t L, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    AsPlan p;
    TRY(as_validate(cfg, &p));
    long long c = 0;
    TRY(as_check_shape(p, B, L, 0, &c));
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
        return as_forward(p, fake, fake, B, L, nullptr, 1, fake, (int)c, 0, nullptr, reinterpret_cast<int32_t*>(fake), fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_assemble_create(const iris_assemble_config* cfg, iris_assemble_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    AsPlan p;
    TRY(as_validate(cfg, &p));
    std::unique_ptr<iris_assemble_handle> h;
    TRY(new_handle(&h));
    h->p = p;
    BlobBuilder bb(nullptr);
    h->ramp_off = bb.reserve(p.fade ? p.fade : 1);                 // (fade == 0: one unread word, so that there is a blob)
    assemble::fill_ramp(p.fade, bb.host.data() + h->ramp_off);
    TRY(upload(bb.host, h.get(), "assemble"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_assemble_destroy(iris_assemble_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_assemble_forward(iris_assemble_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                              float* out_dev, int32_t* spans_out_dev, int32_t* offsets_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                              void* stream) {
    IRIS_ABI_BEGIN
    return as_run(h, wav_dev, B, L, lengths_dev, row_scale, out_dev, 0, spans_out_dev, offsets_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_assemble_trim_ragged(iris_assemble_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                                  float* out_dev, int32_t* spans_out_dev, int32_t* counts_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                  void* stream) {
    IRIS_ABI_BEGIN
    return as_run(h, wav_dev, B, L, lengths_dev, row_scale, out_dev, 1, spans_out_dev, counts_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

}  // extern "C"
