// iris_mel_frontend.hip -- the iris_mel_frontend_* entry points of include/iris_hifigan.h: waveform [B, L] (fp32 or int16) to
// log-mel [B, n_mels, 1 + L / hop] in one launch of mel_kernel (csrc/mel_frontend.h), the reference's compute_mel_spectrogram
// (src/iris/data.py:25-67) in front of the posterior encoder.  The handle owns the packed windowed-DFT table and the packed
// filterbank; iris_mel_frontend_design hands out the same fp32 tables unpacked, on the host alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define IRIS_STFT_NO_INVERSE             // this stage launches no inverse transform
#include "stage_host.h"
#include "mel_frontend.h"

using namespace iris;

struct iris_mel_frontend_handle : StageHandle {
    mel::Design d;
    stft::Tables t;
    PackedGemm fb;
};

namespace iris {

// declared in mel_frontend.h: iris_griffin_lim.hip holds its config to the same rules
int mel_validate(const iris_mel_frontend_config* c, mel::Design* d) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->sample_rate < 1 || c->n_fft < 2 || c->hop_length < 1 || c->win_length < 1 || c->n_mels < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "mel front-end sizes must be positive (n_fft >= 2)");
    const double nyquist = 0.5 * c->sample_rate, fmax = c->fmax > 0.0 ? c->fmax : nyquist;
    if (!(c->fmin >= 0.0) || !(fmax > c->fmin) || fmax > nyquist)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "0 <= fmin < fmax <= sample_rate / 2 is required, got fmin %g fmax %g", c->fmin, fmax);
    if (c->n_fft > mel::kMaxFft) return fail(IRIS_HIFIGAN_UNSUPPORTED, "n_fft %d exceeds %d", c->n_fft, mel::kMaxFft);
    if (c->n_fft % c->hop_length)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "hop_length %d does not divide n_fft %d (a frame is n_fft / hop_length rows of hop_length samples)",
                    c->hop_length, c->n_fft);
    if (c->hop_length % 4) return fail(IRIS_HIFIGAN_UNSUPPORTED, "hop_length %d is not a multiple of 4 (16-byte rows)", c->hop_length);
    if (c->win_length > c->n_fft) return fail(IRIS_HIFIGAN_UNSUPPORTED, "win_length %d exceeds n_fft %d", c->win_length, c->n_fft);
    if (c->n_mels > 1024) return fail(IRIS_HIFIGAN_UNSUPPORTED, "n_mels %d exceeds 1024", c->n_mels);
    d->sample_rate = c->sample_rate; d->n_fft = c->n_fft; d->hop = c->hop_length; d->win = c->win_length; d->n_mels = c->n_mels;
    d->fmin = c->fmin; d->fmax = fmax;
    if (d->lds_bytes() > stft::kMaxLdsBytes)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the sample window and the magnitude tile of n_fft %d, hop_length %d need %llu bytes of LDS, "
                    "more than %llu: the single-launch form does not fit and no two-launch form is built", c->n_fft, c->hop_length,
                    (unsigned long long)d->lds_bytes(), (unsigned long long)stft::kMaxLdsBytes);
    return IRIS_HIFIGAN_OK;
}

}  // namespace iris

namespace {

int mel_check_shape(int32_t B, int32_t L) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    return check_batch(B);
}

// The single launch keeps nothing in HBM between its two GEMMs; a forward still takes a workspace like every stage, of the
// smallest size a buffer has here.
constexpr uint64_t kWorkspaceBytes = 256;

// Queues the forward's launch (or, in a dry run, counts it).  n_samples != nullptr selects the ragged kernel.
int mel_forward(const mel::Design& d, const float* blob, const PackedGemm& dft, const PackedGemm& fb, const void* audio, bool i16,
                int B, int L, const int32_t* n_samples, const int32_t* max_frames, float* mel_out, int32_t* frames, hipStream_t stream) {
    mel::MelLaunch a; memset(&a, 0, sizeof(a));
    a.audio = audio; a.mel = mel_out;
    a.wdft = (const f32x4*)(blob + dft.w_off); a.wfb = (const f32x4*)(blob + fb.w_off);
    a.L = L; a.T = 1 + L / d.hop; a.hop = d.hop; a.taps = d.taps(); a.n_fft = d.n_fft; a.bins = d.bins(); a.n_mels = d.n_mels;
    a.n_samples = n_samples; a.max_frames = max_frames; a.frames = frames;
    HIP_TRY(mel::launch_mel(a, d, B, i16, stream));
    return IRIS_HIFIGAN_OK;
}

int32_t mel_forward_checked(iris_mel_frontend_handle* h, const void* audio_dev, int32_t sample_format, int32_t B, int32_t L, bool ragged,
                            const int32_t* n_samples_dev, const int32_t* max_frames_dev, float* mel_out_dev, int32_t* frames_out_dev,
                            void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(mel_check_shape(B, L));
    if (sample_format != IRIS_MEL_SAMPLES_F32 && sample_format != IRIS_MEL_SAMPLES_I16)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "unknown sample format %d", sample_format);
    if (B == 0) return IRIS_HIFIGAN_OK;
    if ((L > 0 && !audio_dev) || !mel_out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (ragged && (!n_samples_dev || !frames_out_dev)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "n_samples_dev or frames_out_dev is NULL");
    ForwardScope scope(*h, workspace_bytes, kWorkspaceBytes / sizeof(float));
    TRY(scope.rc);
    return mel_forward(h->d, h->blob, h->t.dft, h->fb, audio_dev, sample_format == IRIS_MEL_SAMPLES_I16, B, L,
                       ragged ? n_samples_dev : nullptr, ragged ? max_frames_dev : nullptr, mel_out_dev, frames_out_dev, (hipStream_t)stream_);
    IRIS_ABI_END
}

}  // namespace

extern "C" {

int32_t iris_mel_frontend_design(const iris_mel_frontend_config* cfg, int32_t* n_bins, float* dft_host, uint64_t dft_floats,
                                 float* fb_host, uint64_t fb_floats) {
    IRIS_ABI_BEGIN
    mel::Design d;
    TRY(mel_validate(cfg, &d));
    if (n_bins) *n_bins = d.bins();
    if (dft_host) {
        const uint64_t need = (uint64_t)2 * d.bins() * d.n_fft;
        if (dft_floats < need) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the DFT table has %llu floats, dft_host holds %llu",
                                           (unsigned long long)need, (unsigned long long)dft_floats);
        stft::fill_dft(d, dft_host);
    }
    if (fb_host) {
        const uint64_t need = (uint64_t)d.n_mels * d.bins();
        if (fb_floats < need) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "the filterbank has %llu floats, fb_host holds %llu",
                                          (unsigned long long)need, (unsigned long long)fb_floats);
        mel::fill_filterbank(d, fb_host);
    }
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_mel_frontend_create(const iris_mel_frontend_config* cfg, iris_mel_frontend_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(mel_validate(cfg, &d));
    std::unique_ptr<iris_mel_frontend_handle> h;
    TRY(new_handle(&h));
    h->d = d;
    std::vector<float> fbank((size_t)d.n_mels * d.bins());
    mel::fill_filterbank(d, fbank.data());
    const std::vector<float> no_bias(d.n_mels, 0.f);
    BlobBuilder bb(nullptr);
    stft::pack_tables(bb, d, false, h->t);
    bb.dense(h->fb, fbank.data(), no_bias.data(), d.bins(), d.n_mels, 1);
    TRY(upload(bb.host, h.get(), "mel front-end"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_mel_frontend_destroy(iris_mel_frontend_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_mel_frontend_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(mel_validate(cfg, &d));
    TRY(mel_check_shape(B, L));
    *bytes = kWorkspaceBytes;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_mel_frontend_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(mel_validate(cfg, &d));
    TRY(mel_check_shape(B, L));
    const PackedGemm none;
    return count_forward_launches(B == 0, [&](float* fake) {
        return mel_forward(d, fake, none, none, fake, false, B, L, nullptr, nullptr, fake, nullptr, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_mel_frontend_forward(iris_mel_frontend_handle* h, const void* audio_dev, int32_t sample_format, int32_t B, int32_t L,
                                  float* mel_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    return mel_forward_checked(h, audio_dev, sample_format, B, L, false, nullptr, nullptr, mel_out_dev, nullptr, workspace_dev,
                               workspace_bytes, stream);
}

int32_t iris_mel_frontend_forward_ragged(iris_mel_frontend_handle* h, const void* audio_dev, int32_t sample_format, int32_t B, int32_t L,
                                         const int32_t* n_samples_dev, const int32_t* max_frames_dev, float* mel_out_dev,
                                         int32_t* frames_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    return mel_forward_checked(h, audio_dev, sample_format, B, L, true, n_samples_dev, max_frames_dev, mel_out_dev, frames_out_dev,
                               workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
