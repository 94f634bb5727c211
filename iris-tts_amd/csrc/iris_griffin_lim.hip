// iris_griffin_lim.hip -- the iris_griffin_lim_* entry points of include/iris_hifigan.h: log-mel [B, n_mels, T] to a waveform
// [B, hop (T - 1)] by mel inversion and Griffin-Lim phase retrieval (csrc/griffin_lim.h), the reference's --use_griffin_lim
// path (scripts/synthesize.py:174-194); iris_griffin_lim_forward_ragged adds per-item frame counts and a start phase drawn on
// the device, through the same host routine.  2 * n_iter + 2 launches: the inversion, n_iter times (inverse STFT, STFT with the phase
// update), and the last inverse STFT.  The handle owns the packed tables: P = pinv(fb) from the caller, fb both ways round, the
// front-end's windowed DFT and the windowed inverse DFT, and w^2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define IRIS_MEL_NO_KERNEL               // this stage takes the front-end's design and filterbank, not mel_kernel
#include "stage_host.h"
#include "griffin_lim.h"

using namespace iris;

struct iris_griffin_lim_handle : StageHandle {
    gl::Design d;
    PackedGemm p, fb, fbt;
    stft::Tables t;
};

// the layout iris._native.GriffinLimConfig restates (tests/test_griffin_lim.py holds the two together)
static_assert(sizeof(iris_griffin_lim_config) == 64 && offsetof(iris_griffin_lim_config, n_iter) == 20 &&
              offsetof(iris_griffin_lim_config, fmin) == 24 && offsetof(iris_griffin_lim_config, nnls_iters) == 40 &&
              offsetof(iris_griffin_lim_config, momentum) == 48 && offsetof(iris_griffin_lim_config, nnls_step) == 56,
              "iris_griffin_lim_config layout");

namespace {

int gl_validate(const iris_griffin_lim_config* c, gl::Design* d) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    const iris_mel_frontend_config mc = {c->sample_rate, c->n_fft, c->hop_length, c->win_length, c->n_mels, 0, c->fmin, c->fmax};
    TRY(mel_validate(&mc, d));
    if (c->n_iter < 0 || c->nnls_iters < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "n_iter and nnls_iters must not be negative");
    if (!(c->momentum >= 0.0) || !(c->momentum < 1.0))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "0 <= momentum < 1 is required, got %g", c->momentum);
    if (!(c->nnls_step > 0.0) || !isfinite(c->nnls_step))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "nnls_step must be positive and finite, got %g", c->nnls_step);
    TRY(stft::validate_bin_tiles(*d));
    d->n_iter = c->n_iter; d->nnls_iters = c->nnls_iters; d->momentum = c->momentum; d->nnls_step = c->nnls_step;
    if (d->invert_lds_bytes() > stft::kMaxLdsBytes)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the mel inversion of n_mels %d, n_fft %d needs %llu bytes of LDS, more than %llu", c->n_mels,
                    c->n_fft, (unsigned long long)d->invert_lds_bytes(), (unsigned long long)stft::kMaxLdsBytes);
    return stft::validate_frame_window(*d);
}

int gl_check_shape(int32_t B, int32_t T) {
    if (B < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative batch");
    if (T < 2) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "T = %d: Griffin-Lim needs at least 2 frames (the output has hop (T - 1) samples)", T);
    return check_batch(B);
}

// S first (tests read it there), then c, r and the waveform between the passes.
struct GlWorkspace {
    size_t S, c, r, y, floats;
    GlWorkspace(const gl::Design& d, int B, int T) {
        WsTaker ws;
        const size_t frames = (size_t)B * T;
        S = ws.take(frames * d.ks());
        c = ws.take(frames * d.qp());
        r = ws.take(frames * d.qp());
        y = ws.take((size_t)B * d.hop * (T - 1));
        floats = ws.off;
    }
};

struct GlTables { const float *p, *fb, *fbt, *dft, *idft, *wsq; };

// Queues the forward's launches (or, in a dry run, counts them).  `lengths` (device, or NULL: dense) is handed to every launch
// and never read here; `seed` and `item0` matter when `phase0` is NULL.
int gl_forward(const gl::Design& d, const GlTables& tb, const float* logmel, const float* phase0, uint64_t seed, int32_t item0,
               int B, int T, const int32_t* lengths, float* wav_out, float* ws, hipStream_t stream) {
    const GlWorkspace lay(d, B, T);
    gl::InvertLaunch inv; memset(&inv, 0, sizeof(inv));
    inv.logmel = logmel; inv.phase0 = phase0; inv.lengths = lengths; inv.T = T;
    inv.seed_lo = (uint32_t)seed; inv.seed_hi = (uint32_t)(seed >> 32); inv.item0 = (uint32_t)item0;
    inv.wp = (const f32x4*)tb.p; inv.wfb = (const f32x4*)tb.fb; inv.wfbt = (const f32x4*)tb.fbt;
    inv.S = ws + lay.S; inv.c = ws + lay.c;
    HIP_TRY(gl::launch_invert(inv, d, B, stream));
    stft::IstftLaunch is; memset(&is, 0, sizeof(is));
    is.c = ws + lay.c; is.widft = (const f32x4*)tb.idft; is.wsq = tb.wsq; is.lengths = lengths; is.T = T;
    gl::StftLaunch st; memset(&st, 0, sizeof(st));
    st.wdft = (const f32x4*)tb.dft; st.S = ws + lay.S; st.c = ws + lay.c; st.r = ws + lay.r; st.y = ws + lay.y; st.T = T;
    st.lengths = lengths;
    for (int it = 0; it < d.n_iter; ++it) {
        is.y = ws + lay.y;
        HIP_TRY(stft::launch_istft(is, d, B, stream));
        st.first = it == 0;
        HIP_TRY(gl::launch_stft_update(st, d, B, stream));
    }
    is.y = wav_out; is.zero_tail = lengths != nullptr;
    HIP_TRY(stft::launch_istft(is, d, B, stream));
    return IRIS_HIFIGAN_OK;
}

// What both forwards check, in one order, before anything is launched.
int gl_forward_checked(iris_griffin_lim_handle* h, const float* logmel, const float* phase0, bool need_phase, uint64_t seed,
                       int32_t item0, int32_t B, int32_t T, const int32_t* lengths, float* wav_out, void* workspace,
                       uint64_t workspace_bytes, void* stream) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(gl_check_shape(B, T));
    if (item0 < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative item0");
    if (B == 0) return IRIS_HIFIGAN_OK;
    if (!logmel || (need_phase && !phase0) || !wav_out || !workspace) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardScope scope(*h, workspace_bytes, GlWorkspace(h->d, B, T).floats);
    TRY(scope.rc);
    const GlTables tb = {h->blob + h->p.w_off, h->blob + h->fb.w_off, h->blob + h->fbt.w_off, h->blob + h->t.dft.w_off,
                         h->blob + h->t.idft.w_off, h->blob + h->t.wsq_off};
    return gl_forward(h->d, tb, logmel, phase0, seed, item0, B, T, lengths, wav_out, (float*)workspace, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int32_t iris_griffin_lim_design(const iris_griffin_lim_config* cfg, int32_t* n_bins, float* dft_host, uint64_t dft_floats,
                                float* idft_host, uint64_t idft_floats, float* fb_host, uint64_t fb_floats, float* wsq_host,
                                uint64_t wsq_floats) {
    IRIS_ABI_BEGIN
    gl::Design d;
    TRY(gl_validate(cfg, &d));
    if (n_bins) *n_bins = d.bins();
    const uint64_t table = (uint64_t)2 * d.bins() * d.n_fft;
    if ((dft_host && dft_floats < table) || (idft_host && idft_floats < table) || (fb_host && fb_floats < (uint64_t)d.n_mels * d.bins()) ||
        (wsq_host && wsq_floats < (uint64_t)d.n_fft))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "a table does not fit its array: the DFT tables have %llu floats each, the filterbank "
                    "%llu, the squared window %d", (unsigned long long)table, (unsigned long long)d.n_mels * d.bins(), d.n_fft);
    if (dft_host) stft::fill_dft(d, dft_host);
    if (idft_host) stft::fill_idft(d, idft_host);
    if (fb_host) mel::fill_filterbank(d, fb_host);
    if (wsq_host) stft::fill_wsq(d, wsq_host);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_griffin_lim_create(const iris_griffin_lim_config* cfg, const float* pinv_host, uint64_t n_pinv, iris_griffin_lim_handle** out) {
    IRIS_ABI_BEGIN
    if (!out || !pinv_host) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    gl::Design d;
    TRY(gl_validate(cfg, &d));
    const int nb = d.bins(), M = d.n_mels;
    if (n_pinv != (uint64_t)nb * M)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "pinv(fb) [n_bins][n_mels] has %llu values, got %llu", (unsigned long long)nb * M,
                    (unsigned long long)n_pinv);
    std::unique_ptr<iris_griffin_lim_handle> h;
    TRY(new_handle(&h));
    h->d = d;
    std::vector<float> fbank((size_t)M * nb), fbt((size_t)nb * M);
    mel::fill_filterbank(d, fbank.data());
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < nb; ++k) fbt[(size_t)k * M + i] = fbank[(size_t)i * nb + k];
    const std::vector<float> no_bias(M > nb ? M : nb, 0.f);                  // no GEMM here has one
    BlobBuilder bb(nullptr);
    bb.dense(h->p, pinv_host, no_bias.data(), M, nb, 1);
    bb.dense(h->fb, fbank.data(), no_bias.data(), nb, M, 1);
    bb.dense(h->fbt, fbt.data(), no_bias.data(), M, nb, 1);
    stft::pack_tables(bb, d, true, h->t);
    TRY(upload(bb.host, h.get(), "Griffin-Lim"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_griffin_lim_destroy(iris_griffin_lim_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_griffin_lim_workspace_bytes(const iris_griffin_lim_config* cfg, int32_t B, int32_t T, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    gl::Design d;
    TRY(gl_validate(cfg, &d));
    TRY(gl_check_shape(B, T));
    *bytes = workspace_bytes_of(GlWorkspace(d, B, T).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_griffin_lim_launch_count(const iris_griffin_lim_config* cfg, int32_t B, int32_t T, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    gl::Design d;
    TRY(gl_validate(cfg, &d));
    TRY(gl_check_shape(B, T));
    return count_forward_launches(B == 0, [&](float* fake) {
        const GlTables tb = {fake, fake, fake, fake, fake, fake};
        return gl_forward(d, tb, fake, fake, 0, 0, B, T, nullptr, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_griffin_lim_forward(iris_griffin_lim_handle* h, const float* logmel_dev, const float* phase0_dev, int32_t B, int32_t T,
                                 float* wav_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return gl_forward_checked(h, logmel_dev, phase0_dev, true, 0, 0, B, T, nullptr, wav_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_griffin_lim_forward_ragged(iris_griffin_lim_handle* h, const float* logmel_dev, const float* phase0_dev, uint64_t seed,
                                        int32_t item0, int32_t B, int32_t T, const int32_t* lengths_dev, float* wav_out_dev,
                                        void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return gl_forward_checked(h, logmel_dev, phase0_dev, false, seed, item0, B, T, lengths_dev, wav_out_dev, workspace_dev,
                              workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_griffin_lim_draw_phase(iris_griffin_lim_handle* h, uint64_t seed, int32_t item0, int32_t B, int32_t T, float* phase_out_dev,
                                    void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(gl_check_shape(B, T));
    if (item0 < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative item0");
    if (B == 0) return IRIS_HIFIGAN_OK;
    if (!phase_out_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    DeviceGuard guard(h->device, true);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    gl::DrawLaunch a; memset(&a, 0, sizeof(a));
    a.phase = phase_out_dev; a.T = T; a.bins = h->d.bins();
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.item0 = (uint32_t)item0;
    HIP_TRY(gl::launch_draw_phase(a, B, (hipStream_t)stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

}  // extern "C"
