// iris_time_stretch.hip -- the iris_time_stretch_* entry points of include/iris_hifigan.h: tempo without pitch on a waveform
// [B, L] (csrc/time_stretch.h), librosa.effects.time_stretch on the transforms of stft_f32.h.  A forward is 4 launches: the STFT
// that stores the plain spectrum and the items' counts, the phase vocoder's step and scan, and the Griffin-Lim stage's
// inverse STFT bounded by the items' sample counts.  The handle owns the packed windowed DFT, the packed windowed inverse DFT
// and w^2; the rate is an argument of the forward.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "stage_host.h"
#include "stft_f32.h"
#include "time_stretch.h"

using namespace iris;

struct iris_time_stretch_handle : StageHandle {
    stft::Sizes d;
    stft::Tables t;
};

namespace {

constexpr int kMaxFft = 4096;                                            // the front-end's bound (mel_frontend.h): the tables stay small

// The transform fields of the front-end's config by the front-end's rules for them, then the transforms' own; sample_rate,
// n_mels, fmin and fmax are not read.
int ts_validate(const iris_mel_frontend_config* c, stft::Sizes* d) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->n_fft < 2 || c->hop_length < 1 || c->win_length < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "n_fft >= 2, hop_length >= 1 and win_length >= 1 are required");
    if (c->n_fft > kMaxFft) return fail(IRIS_HIFIGAN_UNSUPPORTED, "n_fft %d exceeds %d", c->n_fft, kMaxFft);
    if (c->n_fft % c->hop_length)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "hop_length %d does not divide n_fft %d (a frame is n_fft / hop_length rows of hop_length samples)",
                    c->hop_length, c->n_fft);
    if (c->hop_length % 4) return fail(IRIS_HIFIGAN_UNSUPPORTED, "hop_length %d is not a multiple of 4 (16-byte rows)", c->hop_length);
    if (c->win_length > c->n_fft) return fail(IRIS_HIFIGAN_UNSUPPORTED, "win_length %d exceeds n_fft %d", c->win_length, c->n_fft);
    d->n_fft = c->n_fft; d->hop = c->hop_length; d->win = c->win_length;
    return stft::transform_validate(*d);
}

int ts_check_rate(double rate) {
    if (!isfinite(rate) || rate < ts::kMinRate || rate > ts::kMaxRate)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "rate must lie in [%g, %g], got %g", ts::kMinRate, ts::kMaxRate, rate);
    return IRIS_HIFIGAN_OK;
}

// What a forward of shape (B, L) at `rate` is laid out by: T, T_out and n_out of a whole row.
struct TsShape {
    int T = 0, T_out = 0, n_out = 0;
};

int ts_check_shape(const stft::Sizes& d, int32_t B, int32_t L, double rate, TsShape* s) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (L % d.hop) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "L = %d is not a multiple of hop_length %d (a vocoder emits hop_length samples per mel frame)", L, d.hop);
    TRY(ts_check_rate(rate));
    TRY(check_batch(B));
    const long long T = L / d.hop + 1, T_out = L ? ts::frames_out((int)T, rate) : 0, n_out = ts::samples_out(L, rate);
    const long long rows = T > T_out ? T : T_out;
    // kernels index a buffer's floats and a grid's threads in 32 bits
    if ((unsigned long long)(B ? B : 1) * rows * d.qp() >= (1ull << 31) || (unsigned long long)(B ? B : 1) * n_out >= (1ull << 31))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d, L = %d at rate %g: %lld frames of %d columns or %lld samples per item exceed 32-bit offsets",
                    B, L, rate, rows, d.qp(), n_out);
    s->T = (int)T; s->T_out = (int)T_out; s->n_out = (int)n_out;
    return IRIS_HIFIGAN_OK;
}

// c first, then mag, inc, acc and out_c (the order tests read them in), then the three per-item counts.
struct TsWorkspace {
    size_t c, mag, inc, acc, out_c, frames, frames_out, counts, floats;
    TsWorkspace(const stft::Sizes& d, int B, const TsShape& s) {
        WsTaker ws;
        c = ws.take((size_t)B * s.T * d.qp());
        mag = ws.take((size_t)B * s.T_out * d.ks());
        inc = ws.take((size_t)B * s.T_out * d.ks());
        acc = ws.take((size_t)B * s.T_out * d.ks());
        out_c = ws.take((size_t)B * s.T_out * d.qp());
        frames = ws.take((size_t)B);
        frames_out = ws.take((size_t)B);
        counts = ws.take((size_t)B);
        floats = ws.off;
    }
};

struct TsTables { const float *dft, *idft, *wsq; };

// Queues the forward's four launches (or, in a dry run, counts them).  `lengths` (device, or NULL: dense) is never read here.
int ts_forward(const stft::Sizes& d, const TsTables& tb, const float* wav, int B, int L, const TsShape& s, const int32_t* lengths, double rate,
               float* out, int32_t* counts_user, float* ws, hipStream_t stream) {
    const TsWorkspace lay(d, B, s);
    int32_t* frames = reinterpret_cast<int32_t*>(ws + lay.frames);
    int32_t* frames_out = reinterpret_cast<int32_t*>(ws + lay.frames_out);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + lay.counts);
    uint32_t* inc = reinterpret_cast<uint32_t*>(ws + lay.inc);
    uint32_t* acc = reinterpret_cast<uint32_t*>(ws + lay.acc);

    stft::StftLaunch st; memset(&st, 0, sizeof(st));
    st.y = wav; st.wdft = (const f32x4*)tb.dft; st.lengths = lengths; st.L = L; st.T = s.T;
    const ts::Spectrum spec = {ws + lay.c, frames, frames_out, counts, counts_user, rate, d.hop};
    HIP_TRY(stft::launch_stft(st, spec, d, B, stream));

    ts::StepLaunch sp; memset(&sp, 0, sizeof(sp));
    sp.c = ws + lay.c; sp.frames = frames; sp.frames_out = frames_out; sp.mag = ws + lay.mag; sp.inc = inc; sp.rate = rate;
    sp.T = s.T; sp.T_out = s.T_out; sp.Ks = d.ks(); sp.Qp = d.qp(); sp.bins = d.bins(); sp.hop = d.hop; sp.n_fft = d.n_fft;
    HIP_TRY(ts::launch_step(sp, B, stream));

    ts::ScanLaunch sc; memset(&sc, 0, sizeof(sc));
    sc.c = ws + lay.c; sc.mag = ws + lay.mag; sc.inc = inc; sc.frames_out = frames_out; sc.acc = acc; sc.out_c = ws + lay.out_c;
    sc.T = s.T; sc.T_out = s.T_out; sc.Ks = d.ks(); sc.Qp = d.qp(); sc.bins = d.bins();
    HIP_TRY(ts::launch_scan(sc, B, stream));

    stft::IstftLaunch is; memset(&is, 0, sizeof(is));
    is.c = ws + lay.out_c; is.widft = (const f32x4*)tb.idft; is.wsq = tb.wsq; is.lengths = frames_out; is.sample_counts = counts;
    is.T = s.T_out; is.y = out; is.zero_tail = 1; is.Ly = s.n_out; is.s_org = 0;
    HIP_TRY(stft::launch_istft_slice(is, d, B, stream));
    return IRIS_HIFIGAN_OK;
}

bool overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb * sizeof(float) && y < x + na * sizeof(float);
}

int ts_run(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, double rate, float* out_dev,
           int32_t* counts_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TsShape s;
    TRY(ts_check_shape(h->d, B, L, rate, &s));
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev || !out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (overlap(wav_dev, (size_t)B * L, out_dev, (size_t)B * s.n_out)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev aliases wav_dev");
    ForwardScope scope(*h, workspace_bytes, TsWorkspace(h->d, B, s).floats);
    TRY(scope.rc);
    const TsTables tb = {h->blob + h->t.dft.w_off, h->blob + h->t.idft.w_off, h->blob + h->t.wsq_off};
    return ts_forward(h->d, tb, wav_dev, B, L, s, lengths_dev, rate, out_dev, counts_out_dev, (float*)workspace_dev, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int32_t iris_time_stretch_create(const iris_mel_frontend_config* cfg, iris_time_stretch_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    std::unique_ptr<iris_time_stretch_handle> h(new (std::nothrow) iris_time_stretch_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->d = d;
    BlobBuilder bb(nullptr);
    stft::pack_tables(bb, d, true, h->t);
    TRY(upload(bb.host, h.get(), "time stretch"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_destroy(iris_time_stretch_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_time_stretch_out_samples(const iris_mel_frontend_config* cfg, int32_t L, double rate, int32_t* frames_out, int32_t* samples_out) {
    IRIS_ABI_BEGIN
    if (!frames_out || !samples_out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TsShape s;
    TRY(ts_check_shape(d, 1, L, rate, &s));
    *frames_out = s.T_out; *samples_out = s.n_out;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, double rate, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TsShape s;
    TRY(ts_check_shape(d, B, L, rate, &s));
    *bytes = (uint64_t)TsWorkspace(d, B, s).floats * sizeof(float);
    if (*bytes < 256) *bytes = 256;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, double rate, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TsShape s;
    TRY(ts_check_shape(d, B, L, rate, &s));
    *n = 0;
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    return count_launches([&](float* fake) {
        const TsTables tb = {fake, fake, fake};
        return ts_forward(d, tb, fake, B, L, s, nullptr, rate, fake, nullptr, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_time_stretch_forward(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t L, double rate, float* out_dev,
                                  void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    return ts_run(h, wav_dev, B, L, nullptr, rate, out_dev, nullptr, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

int32_t iris_time_stretch_forward_ragged(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev,
                                         double rate, float* out_dev, int32_t* counts_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                         void* stream) {
    IRIS_ABI_BEGIN
    return ts_run(h, wav_dev, B, L, lengths_dev, rate, out_dev, counts_out_dev, workspace_dev, workspace_bytes, stream);
    IRIS_ABI_END
}

}  // extern "C"
