// iris_spectral_distance.hip -- the iris_spectral_distance_* entry points of include/iris_hifigan.h: the sums behind the
// multi-resolution STFT distance and the SNR of two ragged batches of waveforms (csrc/spectral_distance.h holds the rules and the
// kernels).  A forward is 3 R + 2 launches: per resolution the forward STFT of ref and of test with magnitudes as the epilogue
// and the tile sums over the two magnitude buffers, then the sample-domain chunk sums and the kernel that adds an item's
// partials in order.  The handle owns one packed windowed DFT per resolution and no inverse table; the host never reads a length.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define IRIS_STFT_NO_INVERSE             // a forward-only stage
#define IRIS_DN_POLICIES_ONLY            // dn::Magnitude, not the bias estimator
#include "stage_host.h"
#include "spectral_distance.h"

using namespace iris;

namespace {

// A checked list of resolutions.
struct SdPlan {
    int R = 0;
    stft::Sizes d[sd::kMaxRes];
};

}  // namespace

struct iris_spectral_distance_handle : StageHandle {
    SdPlan p;
    stft::Tables t[sd::kMaxRes];
};

namespace {

constexpr int kMaxFft = 4096;            // the mel front-end's limit

int sd_validate(const int32_t* res, int32_t n_res, SdPlan* p) {
    if (!res) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "resolutions is NULL");
    if (n_res < 1 || n_res > sd::kMaxRes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "1 .. %d resolutions are taken, got %d", sd::kMaxRes, n_res);
    p->R = n_res;
    for (int r = 0; r < n_res; ++r) {
        const int n_fft = res[3 * r], hop = res[3 * r + 1], win = res[3 * r + 2];
        if (n_fft < 2 || hop < 1 || win < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "resolution %d: sizes must be positive (n_fft >= 2)", r);
        if (win > n_fft) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "resolution %d: win %d exceeds n_fft %d", r, win, n_fft);
        if (n_fft % hop)
            return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "resolution %d: hop %d does not divide n_fft %d (a frame is n_fft / hop rows of hop samples)", r, hop, n_fft);
        if (n_fft > kMaxFft) return fail(IRIS_HIFIGAN_UNSUPPORTED, "resolution %d: n_fft %d exceeds %d", r, n_fft, kMaxFft);
        if (hop % 4) return fail(IRIS_HIFIGAN_UNSUPPORTED, "resolution %d: hop %d is not a multiple of 4", r, hop);
        stft::Sizes& d = p->d[r];
        d.n_fft = n_fft; d.hop = hop; d.win = win;
        TRY(stft::validate_bin_tiles(d));
        if (d.stft_lds_bytes() > stft::kMaxLdsBytes)         // forward only: the inverse transform's window is nobody's here
            return fail(IRIS_HIFIGAN_UNSUPPORTED, "resolution %d: the frame window of n_fft %d, hop %d needs %llu bytes of LDS, more than %llu", r, n_fft,
                        hop, (unsigned long long)d.stft_lds_bytes(), (unsigned long long)stft::kMaxLdsBytes);
    }
    return IRIS_HIFIGAN_OK;
}

// magA and magB [B][T_r][Ks_r] (fp32; one pair, sized for the largest resolution and used by each in turn), then the tile sums
// of every resolution [B][tiles_r][3] and the chunk sums [B][chunks][3] (doubles); each starts on 256 bytes.
struct SdWorkspace {
    size_t magA, magB, spec_part[sd::kMaxRes], wave_part, floats;
    int T[sd::kMaxRes], tiles[sd::kMaxRes], chunks;
    SdWorkspace(const SdPlan& p, int B, int L) {
        size_t mag = 0;
        for (int r = 0; r < p.R; ++r) {
            T[r] = L / p.d[r].hop + 1;
            tiles[r] = sd::tiles_of(T[r]);
            const size_t n = (size_t)B * T[r] * p.d[r].ks();
            if (n > mag) mag = n;
        }
        chunks = sd::chunks_of(L);
        WsTaker ws;
        magA = ws.take(mag);
        magB = ws.take(mag);
        for (int r = 0; r < p.R; ++r) spec_part[r] = ws.take((size_t)B * tiles[r] * 3 * 2);
        wave_part = ws.take((size_t)B * chunks * 3 * 2);
        floats = ws.off;
    }
};

int sd_check_shape(int32_t B, int32_t L) { return check_wave_shape(B, L); }

// Queues the launches (or, in a dry run, counts them).  dft[r]: the packed table of resolution r.
int sd_forward(const SdPlan& p, const float* const* dft, const float* ref, const float* test, int B, int L, const int32_t* lengths, int row_scale,
               double* spec, double* wave, int32_t* frames, float* ws, hipStream_t stream) {
    const SdWorkspace lay(p, B, L);
    sd::FinishLaunch fin; memset(&fin, 0, sizeof(fin));
    for (int r = 0; r < p.R; ++r) {
        const stft::Sizes& d = p.d[r];
        for (int side = 0; side < 2; ++side) {
            stft::StftLaunch st; memset(&st, 0, sizeof(st));
            st.y = side ? test : ref; st.wdft = (const f32x4*)dft[r]; st.L = L; st.T = lay.T[r];
            const sd::Magnitude mg = {{ws + (side ? lay.magB : lay.magA)}, lengths, row_scale, side ? nullptr : frames + r, p.R};
            HIP_TRY(stft::launch_stft(st, mg, d, B, stream));
        }
        sd::TileLaunch tl; memset(&tl, 0, sizeof(tl));
        tl.A = ws + lay.magA; tl.Bm = ws + lay.magB; tl.lengths = lengths; tl.row_scale = row_scale;
        tl.part = reinterpret_cast<double*>(ws + lay.spec_part[r]);
        tl.L = L; tl.T = lay.T[r]; tl.hop = d.hop; tl.Ks = d.ks(); tl.bins = d.bins(); tl.tiles = lay.tiles[r];
        HIP_TRY(sd::launch_tiles(tl, B, stream));
        fin.spec_part[r] = tl.part; fin.hop[r] = d.hop; fin.tiles[r] = lay.tiles[r];
    }
    sd::WaveLaunch wv; memset(&wv, 0, sizeof(wv));
    wv.ref = ref; wv.test = test; wv.lengths = lengths; wv.row_scale = row_scale;
    wv.part = reinterpret_cast<double*>(ws + lay.wave_part); wv.L = L; wv.chunks = lay.chunks;
    HIP_TRY(sd::launch_wave(wv, B, stream));
    fin.lengths = lengths; fin.row_scale = row_scale; fin.wave_part = wv.part; fin.spec = spec; fin.wave = wave;
    fin.L = L; fin.R = p.R; fin.chunks = lay.chunks;
    HIP_TRY(sd::launch_finish(fin, B, stream));
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_spectral_distance_workspace_bytes(const int32_t* resolutions, int32_t n_res, int32_t B, int32_t L, uint64_t* bytes) {
    IRIS_ABI_BEGIN
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    SdPlan p;
    TRY(sd_validate(resolutions, n_res, &p));
    TRY(sd_check_shape(B, L));
    *bytes = workspace_bytes_of(SdWorkspace(p, B, L).floats);
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_spectral_distance_launch_count(const int32_t* resolutions, int32_t n_res, int32_t B, int32_t L, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    SdPlan p;
    TRY(sd_validate(resolutions, n_res, &p));
    TRY(sd_check_shape(B, L));
    return count_forward_launches(B == 0 || L == 0, [&](float* fake) {
        const float* dft[sd::kMaxRes] = {fake, fake, fake, fake};
        return sd_forward(p, dft, fake, fake, B, L, nullptr, 1, reinterpret_cast<double*>(fake), reinterpret_cast<double*>(fake),
                          reinterpret_cast<int32_t*>(fake), fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_spectral_distance_create(const int32_t* resolutions, int32_t n_res, iris_spectral_distance_handle** out) {
    IRIS_ABI_BEGIN
    if (!out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    SdPlan p;
    TRY(sd_validate(resolutions, n_res, &p));
    std::unique_ptr<iris_spectral_distance_handle> h;
    TRY(new_handle(&h));
    h->p = p;
    BlobBuilder bb(nullptr);
    for (int r = 0; r < p.R; ++r) stft::pack_tables(bb, p.d[r], false, h->t[r]);     // forward halves only
    TRY(upload(bb.host, h.get(), "spectral distance"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_spectral_distance_destroy(iris_spectral_distance_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_spectral_distance_forward(iris_spectral_distance_handle* h, const float* ref_dev, const float* test_dev, int32_t B, int32_t L,
                                       const int32_t* lengths_dev, int32_t row_scale, double* spec_out_dev, double* wave_out_dev,
                                       int32_t* frames_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream) {
    IRIS_ABI_BEGIN
    // run_ragged_wave's `out` is the second waveform: it is required and, as nothing is stored to it, may overlap the first
    // (a signal against itself), so want_out stays false and the NULL check is made here.
    const RaggedWaveCall call = {ref_dev, B, L, row_scale, nullptr, false, spec_out_dev, 8, workspace_dev, 8, workspace_bytes};
    return run_ragged_wave(h, call,
        [&](size_t* out_floats, size_t* ws_floats) -> int {
            TRY(sd_check_shape(B, L));
            *out_floats = 0; *ws_floats = SdWorkspace(h->p, B, L).floats;
            return IRIS_HIFIGAN_OK; },
        [&]() -> int {
            if (!test_dev || !wave_out_dev || !frames_out_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
            if ((uintptr_t)wave_out_dev & 7) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "wave_out_dev must lie on 8 bytes");
            const float* dft[sd::kMaxRes] = {};
            for (int r = 0; r < h->p.R; ++r) dft[r] = h->blob + h->t[r].dft.w_off;
            return sd_forward(h->p, dft, ref_dev, test_dev, B, L, lengths_dev, row_scale, spec_out_dev, wave_out_dev, frames_out_dev,
                              (float*)workspace_dev, (hipStream_t)stream); });
    IRIS_ABI_END
}

}  // extern "C"
