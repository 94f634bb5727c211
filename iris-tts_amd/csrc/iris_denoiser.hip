// iris_denoiser.hip -- the iris_denoiser_* entry points of include/iris_hifigan.h: spectral bias subtraction on a waveform
// [B, L] (csrc/denoiser.h), the post-processing step HiFiGAN users run behind the vocoder.  A forward is 2 launches: the STFT
// whose epilogue subtracts strength * bias from the magnitudes, and the Griffin-Lim stage's inverse STFT as it stands.  The
// estimator is 2 launches: the same STFT storing magnitudes, and the fp64 mean over the interior frames.  The handle owns the
// front-end's packed windowed DFT, the packed windowed inverse DFT, w^2 and the bias row.
// forward_window is the same two launches on a window of an utterance, storing the samples that the window settles
// (dn::Window in csrc/denoiser.h): a session that pushes consecutive windows reproduces the whole-utterance forward bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define IRIS_MEL_NO_KERNEL               // this stage takes the front-end's config rules (mel_validate), not mel_kernel
#include "stage_host.h"
#include "mel_frontend.h"
#include "denoiser.h"

using namespace iris;

struct iris_denoiser_handle : StageHandle {
    mel::Design d;
    stft::Tables t;
    size_t bias_off = 0;
};

namespace {

// The front-end's rules (its config is this stage's), then the transforms'.
int dn_validate(const iris_mel_frontend_config* c, mel::Design* d) {
    TRY(mel_validate(c, d));
    return stft::transform_validate(*d);
}

int dn_check_shape(const mel::Design& d, int32_t B, int32_t L) {
    if (B < 0 || L < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (L % d.hop) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "L = %d is not a multiple of hop_length %d (a vocoder emits hop_length samples per mel frame)", L, d.hop);
    return check_batch(B);
}

// c first (tests read it there; the estimator keeps its magnitudes [T][Ks] in the same place), then the items' frame counts.
struct DnWorkspace {
    size_t c, frames, floats;
    DnWorkspace(const mel::Design& d, int B, int L) {
        WsTaker ws;
        c = ws.take((size_t)B * (L / d.hop + 1) * d.qp());
        frames = ws.take((size_t)B);
        floats = ws.off;
    }
};

struct DnTables { const float *dft, *idft, *wsq, *bias; };

// Queues the forward's two launches (or, in a dry run, counts them).  `lengths` (device, or NULL: dense) is never read here.
int dn_forward(const mel::Design& d, const DnTables& tb, const float* wav, int B, int L, const int32_t* lengths, float strength,
               float* out, float* ws, hipStream_t stream) {
    const DnWorkspace lay(d, B, L);
    const int T = L / d.hop + 1;
    int32_t* frames = reinterpret_cast<int32_t*>(ws + lay.frames);
    stft::StftLaunch st; memset(&st, 0, sizeof(st));
    st.y = wav; st.wdft = (const f32x4*)tb.dft; st.lengths = lengths; st.L = L; st.T = T;
    const dn::Subtract sub = {tb.bias, ws + lay.c, frames, strength};
    HIP_TRY(stft::launch_stft(st, sub, d, B, stream));
    stft::IstftLaunch is; memset(&is, 0, sizeof(is));
    is.c = ws + lay.c; is.widft = (const f32x4*)tb.idft; is.wsq = tb.wsq; is.lengths = frames; is.T = T; is.y = out; is.zero_tail = 1;
    HIP_TRY(stft::launch_istft(is, d, B, stream));
    return IRIS_HIFIGAN_OK;
}

// The window's two launches (or their count): the computable frames [f_lo, f_hi) of wav [B, Lw] into c [B, f_hi - f_lo, Qp], then
// the final samples of its inverse transform into out [B, out_count].  The caller has checked that out_count > 0.
int dn_forward_window(const mel::Design& d, const DnTables& tb, const float* wav, int B, int Lw, const dn::Window& w, long long origin,
                      float strength, float* out, float* ws, hipStream_t stream) {
    const DnWorkspace lay(d, B, Lw);                                         // f_hi - f_lo <= Lw / hop + 1
    const int frames = (int)(w.f_hi - w.f_lo);
    stft::StftLaunch st; memset(&st, 0, sizeof(st));
    st.y = wav; st.wdft = (const f32x4*)tb.dft; st.L = Lw; st.T = frames; st.y_org = (int)(w.f_lo * d.hop - origin);
    const dn::Subtract sub = {tb.bias, ws + lay.c, reinterpret_cast<int32_t*>(ws + lay.frames), strength};
    HIP_TRY(stft::launch_stft(st, sub, d, B, stream));
    stft::IstftLaunch is; memset(&is, 0, sizeof(is));
    is.c = ws + lay.c; is.widft = (const f32x4*)tb.idft; is.wsq = tb.wsq; is.T = frames; is.y = out;
    is.Ly = (int)w.out_count; is.s_org = (int)(w.out_lo - w.f_lo * d.hop);
    HIP_TRY(stft::launch_istft_slice(is, d, B, stream));
    return IRIS_HIFIGAN_OK;
}

int dn_check_window(const mel::Design& d, int32_t B, int32_t Lw, int64_t origin) {
    TRY(dn_check_shape(d, B, Lw));
    if (origin < 0 || origin % d.hop)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin = %lld is not a multiple of hop_length %d at or above 0", (long long)origin, d.hop);
    if (origin > ((int64_t)1 << 60)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "origin = %lld exceeds 2^60", (long long)origin);
    return IRIS_HIFIGAN_OK;
}

// Queues the estimator's two launches (or counts them); the caller has checked that an interior frame exists.
int dn_estimate(const mel::Design& d, const float* dft, const float* wav, int L, float* bias_out, float* ws, hipStream_t stream) {
    const int T = L / d.hop + 1, edge = dn::edge_frames(d);
    stft::StftLaunch st; memset(&st, 0, sizeof(st));
    st.y = wav; st.wdft = (const f32x4*)dft; st.L = L; st.T = T;
    HIP_TRY(stft::launch_stft(st, dn::Magnitude{ws}, d, 1, stream));
    dn::ReduceLaunch rd; memset(&rd, 0, sizeof(rd));
    rd.mag = ws; rd.bias = bias_out; rd.t_lo = edge; rd.t_hi = T - edge; rd.Ks = d.ks(); rd.bins = d.bins();
    HIP_TRY(dn::launch_bias_reduce(rd, stream));
    return IRIS_HIFIGAN_OK;
}

int dn_check_interior(const mel::Design& d, int32_t L) {
    const int T = L / d.hop + 1, edge = dn::edge_frames(d);
    if (T - edge <= edge)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "L = %d: no frame of n_fft %d, hop_length %d lies wholly inside the signal (at least %d samples are needed)",
                    L, d.n_fft, d.hop, 2 * edge * d.hop);
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_denoiser_create(const iris_mel_frontend_config* cfg, const float* bias_host, iris_denoiser_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    const int nb = d.bins();
    if (bias_host)
        for (int k = 0; k < nb; ++k)
            if (!(bias_host[k] >= 0.f) || !isfinite(bias_host[k]))
                return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bias[%d] = %g: a magnitude spectrum is finite and not negative", k, (double)bias_host[k]);
    std::unique_ptr<iris_denoiser_handle> h;
    TRY(new_handle(&h));
    h->d = d;
    BlobBuilder bb(nullptr);
    stft::pack_tables(bb, d, true, h->t);
    h->bias_off = bb.reserve(d.ks());                                        // zeros behind the last bin
    if (bias_host) memcpy(bb.host.data() + h->bias_off, bias_host, sizeof(float) * nb);
    TRY(upload(bb.host, h.get(), "denoiser"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_denoiser_destroy(iris_denoiser_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_denoiser_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    TRY(dn_check_shape(d, B, L));
    *bytes = workspace_bytes_of(DnWorkspace(d, B, L).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_denoiser_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    TRY(dn_check_shape(d, B, L));
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
        const DnTables tb = {fake, fake, fake, fake};
        return dn_forward(d, tb, fake, B, L, nullptr, 0.f, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_denoiser_set_bias(iris_denoiser_handle* h, const float* bias_dev, void* stream) {
    IRIS_ABI_BEGIN
    if (!h || !bias_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(h->device, true);
    if (guard.err != hipSuccess) return fail(IRIS_HIFIGAN_HIP_ERROR, "cannot select device %d: %s", h->device, hipGetErrorString(guard.err));
    HIP_TRY(hipMemcpyAsync(h->blob + h->bias_off, bias_dev, sizeof(float) * h->d.bins(), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_denoiser_estimate_bias(iris_denoiser_handle* h, const float* wav_dev, int32_t L, float* bias_out_dev, void* workspace_dev,
                                    uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(dn_check_shape(h->d, 1, L));
    TRY(dn_check_interior(h->d, L));
    if (!wav_dev || !bias_out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardScope scope(*h, workspace_bytes, DnWorkspace(h->d, 1, L).floats);
    TRY(scope.rc);
    return dn_estimate(h->d, h->blob + h->t.dft.w_off, wav_dev, L, bias_out_dev, (float*)workspace_dev, (hipStream_t)stream);
    IRIS_ABI_END
}

int32_t iris_denoiser_estimate_launch_count(const iris_mel_frontend_config* cfg, int32_t L, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    TRY(dn_check_shape(d, 1, L));
    TRY(dn_check_interior(d, L));
    return count_launches([&](float* fake) { return dn_estimate(d, fake, fake, L, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_denoiser_forward(iris_denoiser_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, float strength,
                              float* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(dn_check_shape(h->d, B, L));
    if (!(strength >= 0.f) || !isfinite(strength)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "strength must be finite and not negative, got %g", (double)strength);
    if (B == 0 || L == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev || !out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (overlap(wav_dev, (size_t)B * L, out_dev, (size_t)B * L)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev aliases wav_dev");
    ForwardScope scope(*h, workspace_bytes, DnWorkspace(h->d, B, L).floats);
    TRY(scope.rc);
    const DnTables tb = {h->blob + h->t.dft.w_off, h->blob + h->t.idft.w_off, h->blob + h->t.wsq_off, h->blob + h->bias_off};
    return dn_forward(h->d, tb, wav_dev, B, L, lengths_dev, strength, out_dev, (float*)workspace_dev, (hipStream_t)stream);
    IRIS_ABI_END
}

int32_t iris_denoiser_window_range(const iris_mel_frontend_config* cfg, int64_t origin, int32_t Lw, int32_t final, int64_t* out_lo,
                                   int64_t* out_count) {
    IRIS_ABI_BEGIN
    if (!out_lo || !out_count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    TRY(dn_check_window(d, 1, Lw, origin));
    const dn::Window w(d, origin / d.hop, Lw / d.hop, final != 0);
    *out_lo = w.out_lo; *out_count = w.out_count;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_denoiser_window_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, uint64_t* bytes) {
    return iris_denoiser_workspace_bytes(cfg, B, Lw, bytes);                 // c of at most Lw / hop + 1 frames, and the frame counts
}

int32_t iris_denoiser_window_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, int64_t origin, int32_t final, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    mel::Design d;
    TRY(dn_validate(cfg, &d));
    TRY(dn_check_window(d, B, Lw, origin));
    const dn::Window w(d, origin / d.hop, Lw / d.hop, final != 0);
    return count_forward_launches(B == 0 || w.out_count == 0, [&](float* fake) {
        const DnTables tb = {fake, fake, fake, fake};
        return dn_forward_window(d, tb, fake, B, Lw, w, origin, 0.f, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_denoiser_forward_window(iris_denoiser_handle* h, const float* wav_dev, int32_t B, int32_t Lw, int64_t origin, int32_t final,
                                     float strength, float* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(dn_check_window(h->d, B, Lw, origin));
    if (!(strength >= 0.f) || !isfinite(strength)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "strength must be finite and not negative, got %g", (double)strength);
    const dn::Window w(h->d, origin / h->d.hop, Lw / h->d.hop, final != 0);
    if (B == 0 || w.out_count == 0) return IRIS_HIFIGAN_OK;
    if (!wav_dev || !out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (overlap(wav_dev, (size_t)B * Lw, out_dev, (size_t)B * w.out_count)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev aliases wav_dev");
    ForwardScope scope(*h, workspace_bytes, DnWorkspace(h->d, B, Lw).floats);
    TRY(scope.rc);
    const DnTables tb = {h->blob + h->t.dft.w_off, h->blob + h->t.idft.w_off, h->blob + h->t.wsq_off, h->blob + h->bias_off};
    return dn_forward_window(h->d, tb, wav_dev, B, Lw, w, origin, strength, out_dev, (float*)workspace_dev, (hipStream_t)stream);
    IRIS_ABI_END
}

}  // extern "C"
