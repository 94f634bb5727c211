// iris_loudness.hip -- the iris_loudness_* entry points of include/iris_hifigan.h: BS.1770-4 integrated loudness per item of a
// ragged batch of waveforms and the gain to a target (csrc/loudness.h holds the rules and the kernels).  normalize_ragged is 4
// launches: the segments' end states from zero with the scan inside each chunk, the rerun from the true start states that
// accumulates the squares, the gates and the gain (one block per item), and the product.  measure_ragged stops after the third.
// The handle owns the design table (coefficients, thresholds, the powers of the transition matrix); the host never reads a length.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "loudness.h"
#include "stage_host.h"

using namespace iris;

namespace {

// A checked config.
struct LdPlan {
    int rate = 0, step = 0;
    double target = 0.0, max_gain = 0.0, ceiling = 0.0;
};

}  // namespace

struct iris_loudness_handle : StageHandle {
    LdPlan p;
};

namespace {

int ld_validate(const iris_loudness_config* c, LdPlan* p) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->sample_rate < 8000 || c->sample_rate > 48000 || c->sample_rate % 10)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "sample_rate %d must lie in 8000 .. 48000 and be a multiple of 10 (a gating step is sample_rate / 10 samples)",
                    c->sample_rate);
    if (!isfinite(c->target_lufs) || c->target_lufs > 0.f || c->target_lufs < -70.f)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "target_lufs must lie in -70 .. 0, got %g", (double)c->target_lufs);
    if (!isfinite(c->max_gain_db) || c->max_gain_db < 0.f || c->max_gain_db > 120.f)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "max_gain_db must lie in 0 .. 120, got %g", (double)c->max_gain_db);
    if (!isfinite(c->peak_ceiling) || c->peak_ceiling < 0.f || c->peak_ceiling > 1.f)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "peak_ceiling must be an amplitude in (0, 1], or 0 for none, got %g", (double)c->peak_ceiling);
    p->rate = c->sample_rate; p->step = c->sample_rate / 10;
    p->target = (double)c->target_lufs; p->max_gain = (double)c->max_gain_db; p->ceiling = (double)c->peak_ceiling;
    return IRIS_HIFIGAN_OK;
}

// ends [B][segs][4], parts [B][segs][2], hops [B][hop_cap] (doubles), then seg_peak [B][segs] (fp32); each starts on 256 bytes.
struct LdWorkspace {
    size_t ends, parts, hops, seg_peak, floats;
    int segs, hop_cap;
    LdWorkspace(const LdPlan& p, int B, int L) {
        segs = (int)(((long long)L + loudness::kChunk - 1) / loudness::kChunk) * loudness::kChunkSegs;
        hop_cap = L / p.step + 1;
        WsTaker ws;
        ends = ws.take((size_t)B * segs * 8);
        parts = ws.take((size_t)B * segs * 4);
        hops = ws.take((size_t)B * hop_cap * 2);
        seg_peak = ws.take((size_t)B * segs);
        floats = ws.off;
    }
};

// Queues the launches (or, in a dry run, counts them).  out == nullptr: measure only.
int ld_forward(const LdPlan& p, const double* design, const float* wav, int B, int L, const int32_t* lengths, int row_scale, float* out, double* stats,
               float* ws, hipStream_t stream) {
    const LdWorkspace lay(p, B, L);
    loudness::SegLaunch sg; memset(&sg, 0, sizeof(sg));
    sg.wav = wav; sg.lengths = lengths; sg.row_scale = row_scale; sg.design = design;
    sg.ends = reinterpret_cast<double*>(ws + lay.ends); sg.parts = reinterpret_cast<double*>(ws + lay.parts); sg.seg_peak = ws + lay.seg_peak;
    sg.L = L; sg.segs = lay.segs; sg.step = p.step;
    HIP_TRY(loudness::launch_local(sg, B, stream));
    HIP_TRY(loudness::launch_rerun(sg, B, stream));

    loudness::GateLaunch ga; memset(&ga, 0, sizeof(ga));
    ga.lengths = lengths; ga.row_scale = row_scale; ga.design = design; ga.parts = sg.parts; ga.seg_peak = sg.seg_peak;
    ga.hops = reinterpret_cast<double*>(ws + lay.hops); ga.stats = stats; ga.L = L; ga.segs = lay.segs; ga.step = p.step; ga.hop_cap = lay.hop_cap;
    HIP_TRY(loudness::launch_gate(ga, B, stream));
    if (!out) return IRIS_HIFIGAN_OK;

    loudness::ApplyLaunch ap; memset(&ap, 0, sizeof(ap));
    ap.wav = wav; ap.lengths = lengths; ap.row_scale = row_scale; ap.stats = stats; ap.out = out; ap.B = B; ap.L = L;
    HIP_TRY(loudness::launch_apply(ap, stream));
    return IRIS_HIFIGAN_OK;
}

int ld_run(iris_loudness_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale, float* out_dev, bool apply,
           double* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    const RaggedWaveCall call = {wav_dev, B, L, row_scale, out_dev, apply, stats_out_dev, 8, workspace_dev, 8, workspace_bytes};
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            TRY(check_wave_shape(B, L));
            *out_floats = (size_t)B * L; *ws_floats = LdWorkspace(h->p, B, L).floats;
            return IRIS_HIFIGAN_OK; },
        [&] { return ld_forward(h->p, reinterpret_cast<const double*>(h->blob), wav_dev, B, L, lengths_dev, row_scale, apply ? out_dev : nullptr,
                                stats_out_dev, (float*)workspace_dev, (hipStream_t)stream); });
}

}  // namespace

extern "C" {

int32_t iris_loudness_design(const iris_loudness_config* cfg, double* out, uint64_t n) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LdPlan p;
    TRY(ld_validate(cfg, &p));
    if (n != (uint64_t)loudness::kDesign) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the design table has %d doubles, got room for %llu", loudness::kDesign, (unsigned long long)n);
    loudness::fill_design(p.rate, p.target, p.max_gain, p.ceiling, out);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_loudness_workspace_bytes(const iris_loudness_config* cfg, int32_t B, int32_t L, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LdPlan p;
    TRY(ld_validate(cfg, &p));
    TRY(check_wave_shape(B, L));
    *bytes = workspace_bytes_of(LdWorkspace(p, B, L).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_loudness_launch_count(const iris_loudness_config* cfg, int32_t B, int32_t L, int32_t measure_only, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LdPlan p;
    TRY(ld_validate(cfg, &p));
    TRY(check_wave_shape(B, L));
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
        return ld_forward(p, reinterpret_cast<const double*>(fake), fake, B, L, nullptr, 1, measure_only ? nullptr : fake, reinterpret_cast<double*>(fake),
                          fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_loudness_create(const iris_loudness_config* cfg, iris_loudness_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    LdPlan p;
    TRY(ld_validate(cfg, &p));
    std::unique_ptr<iris_loudness_handle> h;
    TRY(new_handle(&h));
    h->p = p;
    double design[loudness::kDesign];
    loudness::fill_design(p.rate, p.target, p.max_gain, p.ceiling, design);
    std::vector<float> host(2 * loudness::kDesign);                 // the doubles' bytes: the blob starts on 256 bytes
    memcpy(host.data(), design, sizeof(design));
    TRY(upload(host, h.get(), "loudness"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_loudness_destroy(iris_loudness_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_loudness_normalize_ragged(iris_loudness_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                                       float* out_dev, double* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return ld_run(h, wav_dev, B, L, lengths_dev, row_scale, out_dev, true, stats_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_loudness_measure_ragged(iris_loudness_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                                     double* stats_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return ld_run(h, wav_dev, B, L, lengths_dev, row_scale, nullptr, false, stats_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

}  // extern "C"
