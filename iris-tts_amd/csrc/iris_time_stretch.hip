// iris_time_stretch.hip -- the iris_time_stretch_* entry points of include/iris_hifigan.h: tempo without pitch on a waveform
// [B, L] (csrc/time_stretch.h), librosa.effects.time_stretch on the transforms of stft_f32.h.  A forward is 4 launches: the STFT
// that stores the plain spectrum and the items' counts, the phase vocoder's step and scan, and the Griffin-Lim stage's
// inverse STFT bounded by the items' sample counts.  The handle owns the packed windowed DFT, the packed windowed inverse DFT
// and w^2; the rate is an argument of the forward.
// forward_window is the same launches on a window of an utterance, with the phase and the last taps - 1 output frames carried
// in a caller-owned state (ts::WindowPlan in csrc/time_stretch.h): a session that pushes consecutive windows reproduces the
// whole-utterance forward bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
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

// ---- windows -----------------------------------------------------------------------------------------------------------
// The state: acc [B, Ks] (uint32), then tail [B, taps - 1, Qp], each starting on 256 bytes.
struct TsState {
    size_t acc, tail, floats;
    TsState(const stft::Sizes& d, int B) {
        WsTaker ws;
        acc = ws.take((size_t)B * d.ks());
        tail = ws.take((size_t)B * (d.taps() - 1) * d.qp());
        floats = ws.off;
    }
};

// The most output frames a window of Mw mel frames computes: its rows span at most Mw + 1 values of i(t), each of which at most
// ceil(1 / rate) frames share, and one more frame may straddle the front.
long long ts_window_frames(long long Mw, double rate) { return (long long)ceil((double)(Mw + 1) / rate) + 1; }

// A window's buffers in the forward's order, sized by what any window of (B, Lw) at `rate` can hold, so that the layout does
// not depend on u; each is dense in the rows the window has.
struct TsWindowWorkspace {
    size_t c, mag, inc, acc, out_c, floats;
    TsWindowWorkspace(const stft::Sizes& d, int B, int Lw, double rate) {
        const size_t F = (size_t)(Lw / d.hop + 1), n = (size_t)ts_window_frames(Lw / d.hop, rate);
        WsTaker ws;
        c = ws.take((size_t)B * F * d.qp());
        mag = ws.take((size_t)B * n * d.ks());
        inc = ws.take((size_t)B * n * d.ks());
        acc = ws.take((size_t)B * n * d.ks());
        out_c = ws.take((size_t)B * (n + d.taps() - 1) * d.qp());
        floats = ws.off;
    }
};

int ts_check_window(const stft::Sizes& d, int32_t B, int32_t Lw, double rate, int64_t origin, int64_t u) {
    if (B < 0 || Lw < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (Lw % d.hop) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "Lw = %d is not a multiple of hop_length %d", Lw, d.hop);
    if (origin < 0 || origin % d.hop)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "origin = %lld is not a multiple of hop_length %d at or above 0", (long long)origin, d.hop);
    if (u < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "u = %lld is negative", (long long)u);
    TRY(ts_check_rate(rate));
    TRY(check_batch(B));
    if (origin > ((int64_t)1 << 60)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "origin = %lld exceeds 2^60", (long long)origin);
    if (u > ((int64_t)1 << 61) / d.hop) return fail(IRIS_HIFIGAN_UNSUPPORTED, "u = %lld: its samples exceed 2^61", (long long)u);
    if (d.taps() < 2)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "hop_length %d equals n_fft: frames that do not overlap carry no tail, and no window form is built for them", d.hop);
    const unsigned long long rows = (unsigned long long)ts_window_frames(Lw / d.hop, rate) + d.taps();
    if ((unsigned long long)(B ? B : 1) * rows * d.qp() >= (1ull << 31))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B = %d, Lw = %d at rate %g: %llu frames of %d columns per item exceed 32-bit offsets", B, Lw, rate, rows, d.qp());
    return IRIS_HIFIGAN_OK;
}

// The plan of a checked window, or the refusal of a u whose first row the window no longer holds.
int ts_plan_window(const stft::Sizes& d, double rate, int64_t origin, int32_t Lw, int32_t final, int64_t u, ts::WindowPlan* out) {
    const ts::WindowPlan p(d, rate, origin / d.hop, Lw / d.hop, final != 0, u);
    if (p.dropped)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "frame u = %lld reads input row %lld, but the window [%lld, %lld) holds rows from %lld on: samples were dropped "
                    "before keep_from", (long long)u, ts::source_row(u, rate), (long long)origin, (long long)origin + Lw, p.f_lo);
    *out = p;
    return IRIS_HIFIGAN_OK;
}

// Queues a window's launches (or, in a dry run, counts them): 4; 3 where frames advance but no sample is emitted yet; 2 (the
// scan, which then only lays the tail out, and the inverse transform) where a final window has samples left and no frame.
// The caller has checked that there is a frame or a sample.  `state` may be NULL only when u == 0.
int ts_forward_window(const stft::Sizes& d, const TsTables& tb, const float* wav, int B, int Lw, const ts::WindowPlan& p, long long origin,
                      long long u, double rate, float* state, float* out, float* ws, hipStream_t stream) {
    const TsWindowWorkspace lay(d, B, Lw, rate);
    const TsState sl(d, B);
    const int F = (int)(p.f_hi - p.f_lo), n_new = (int)(p.u_hi - u), n_tail = (int)p.n_tail;
    uint32_t* inc = reinterpret_cast<uint32_t*>(ws + lay.inc);
    uint32_t* acc = reinterpret_cast<uint32_t*>(ws + lay.acc);
    if (n_new > ts_window_frames(Lw / d.hop, rate)) return fail(IRIS_HIFIGAN_UNSUPPORTED, "a window of %d samples plans %d frames, past its workspace", Lw, n_new);
    uint32_t* acc_state = state ? reinterpret_cast<uint32_t*>(state + sl.acc) : nullptr;
    float* tail_state = state ? state + sl.tail : nullptr;

    if (n_new > 0) {
        stft::StftLaunch st; memset(&st, 0, sizeof(st));
        st.y = wav; st.wdft = (const f32x4*)tb.dft; st.L = Lw; st.T = F; st.y_org = (int)(p.f_lo * d.hop - origin);
        ts::WindowSpectrum spec; memset(&spec, 0, sizeof(spec));
        spec.c = ws + lay.c; spec.rate = rate; spec.hop = d.hop;
        HIP_TRY(stft::launch_stft(st, spec, d, B, stream));

        ts::StepLaunch sp; memset(&sp, 0, sizeof(sp));
        sp.c = ws + lay.c; sp.mag = ws + lay.mag; sp.inc = inc; sp.rate = rate;
        sp.T = F; sp.T_out = n_new; sp.Ks = d.ks(); sp.Qp = d.qp(); sp.bins = d.bins(); sp.hop = d.hop; sp.n_fft = d.n_fft;
        sp.t_org = u; sp.f_lo = p.f_lo;
        HIP_TRY(ts::launch_step(sp, B, stream));
    }

    ts::ScanLaunch sc; memset(&sc, 0, sizeof(sc));
    sc.c = ws + lay.c; sc.mag = ws + lay.mag; sc.inc = inc; sc.acc = acc; sc.out_c = ws + lay.out_c;
    sc.T = F; sc.T_out = n_new; sc.Ks = d.ks(); sc.Qp = d.qp(); sc.bins = d.bins();
    sc.acc_in = u ? acc_state : nullptr; sc.acc_out = acc_state;
    sc.tail_in = tail_state; sc.tail_out = n_new > 0 ? tail_state : nullptr;
    sc.row_off = n_tail; sc.tail_rows = d.taps() - 1; sc.tail_keep = (int)p.n_keep;
    HIP_TRY(ts::launch_scan(sc, B, stream));

    if (p.out_count > 0) {
        stft::IstftLaunch is; memset(&is, 0, sizeof(is));
        is.c = ws + lay.out_c; is.widft = (const f32x4*)tb.idft; is.wsq = tb.wsq; is.T = n_tail + n_new; is.y = out;
        is.Ly = (int)p.out_count; is.s_org = (int)(p.out_lo - (u - n_tail) * d.hop);
        HIP_TRY(stft::launch_istft_slice(is, d, B, stream));
    }
    return IRIS_HIFIGAN_OK;
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
    std::unique_ptr<iris_time_stretch_handle> h;
    TRY(new_handle(&h));
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
    *bytes = workspace_bytes_of(TsWorkspace(d, B, s).floats);
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
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
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

int32_t iris_time_stretch_state_bytes(const iris_mel_frontend_config* cfg, int32_t B, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TRY(ts_check_window(d, B, 0, 1.0, 0, 0));
    *bytes = workspace_bytes_of(TsState(d, B).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_window_plan(const iris_mel_frontend_config* cfg, double rate, int64_t origin, int32_t Lw, int32_t final, int64_t u,
                                      int64_t* u_hi, int64_t* out_lo, int64_t* out_count, int64_t* keep_from) {
    IRIS_ABI_BEGIN
    if (!u_hi || !out_lo || !out_count || !keep_from) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TRY(ts_check_window(d, 1, Lw, rate, origin, u));
    ts::WindowPlan p;
    TRY(ts_plan_window(d, rate, origin, Lw, final, u, &p));
    *u_hi = p.u_hi; *out_lo = p.out_lo; *out_count = p.out_count; *keep_from = p.keep_from;
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_window_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, double rate, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TRY(ts_check_window(d, B, Lw, rate, 0, 0));
    *bytes = workspace_bytes_of(TsWindowWorkspace(d, B, Lw, rate).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_time_stretch_window_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, double rate, int64_t origin, int32_t final,
                                              int64_t u, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    stft::Sizes d;
    TRY(ts_validate(cfg, &d));
    TRY(ts_check_window(d, B, Lw, rate, origin, u));
    ts::WindowPlan p;
    TRY(ts_plan_window(d, rate, origin, Lw, final, u, &p));
    return count_forward_launches(B == 0 || (p.u_hi == u && p.out_count == 0), [&](float* fake) {
        const TsTables tb = {fake, fake, fake};
        return ts_forward_window(d, tb, fake, B, Lw, p, origin, u, rate, fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_time_stretch_forward_window(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t Lw, int64_t origin, int32_t final,
                                         double rate, int64_t u, void* state_dev, float* out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                         void* stream) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(ts_check_window(h->d, B, Lw, rate, origin, u));
    ts::WindowPlan p;
    TRY(ts_plan_window(h->d, rate, origin, Lw, final, u, &p));
    if (!state_dev && (u > 0 || !final))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "no state: only a final window that starts at frame 0 (a whole utterance) carries nothing over");
    if (B == 0 || (p.u_hi == u && p.out_count == 0)) return IRIS_HIFIGAN_OK;
    if ((p.u_hi > u && !wav_dev) || !workspace_dev || (p.out_count && !out_dev)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (p.out_count && wav_dev && overlap(wav_dev, (size_t)B * Lw, out_dev, (size_t)B * p.out_count)) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "out_dev aliases wav_dev");
    ForwardScope scope(*h, workspace_bytes, TsWindowWorkspace(h->d, B, Lw, rate).floats);
    TRY(scope.rc);
    const TsTables tb = {h->blob + h->t.dft.w_off, h->blob + h->t.idft.w_off, h->blob + h->t.wsq_off};
    return ts_forward_window(h->d, tb, wav_dev, B, Lw, p, origin, u, rate, (float*)state_dev, out_dev, (float*)workspace_dev, (hipStream_t)stream);
    IRIS_ABI_END
}

}  // extern "C"
