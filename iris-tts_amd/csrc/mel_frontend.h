// mel_frontend.h -- waveform to log-mel on the device (iris_mel_frontend_*): the reference's compute_mel_spectrogram
// (src/iris/data.py:25-67), i.e. librosa 0.11's melspectrogram(power=1.0) followed by log(max(mel, 1e-5)).  Frames, window,
// the windowed DFT table and the forward transform as a GEMM (tiles, column order, staging, decode) are stft_f32.h's.
//
//   mag      |stft(x)[t, k]|, k = 0 .. n_fft / 2
//   mel      fb [n_mels][n_fft / 2 + 1] (Slaney scale and Slaney area normalisation) times mag
//   out      log(max(mel, 1e-5f)) taken in double and rounded once to fp32, channels-first [B, n_mels, T]
//
// design(): host only.  The windowed DFT table is stft::fill_dft's; the filterbank is evaluated in double by librosa's own
// steps and rounded once to fp32.  These are the bits the kernel multiplies by.
//
// mel_kernel: ONE launch.  A block owns 32 frames, stages their window (stft::stage_window) and spreads the ceil(n_fft / 32)
// column tiles over its 8 waves.  Its DFT is ONE long chain per column: mma_loop over all taps, no partial sums -- a different,
// deliberate summation from stft_kernel's short chains.  The epilogue (stft::decode_bins) takes sqrtf(re * re + im * im) into
// an LDS tile of 32 frames x (n_fft / 2 + 1) bins behind the sample window -- magnitudes never go to HBM -- and after one
// barrier the filterbank runs over that tile as a second GEMM, the way the VAE's fused res_proj does.
//
// LDS: (31 + k) * (hop8 + 4) + 32 * (bins8 + 4) floats (x8 = rounded up to 8): 36 400 + 67 072 = 103 472 bytes at the
// defaults (n_fft 1024, hop 256), one block per CU.  A config whose two tiles exceed 160 KB is unsupported.
//
// Input form: fp32 samples, or int16 samples converted as x * (1.0f / 32768) while staging (SAMPLE_I16; stft::load_sample).
//
// Ragged form (RAGGED, "Ragged form" in vae_decoder.h): n_samples[B] on the device, clamped to [0, L], bounds what is fetched
// -- samples at or past it read 0 -- and gives the item's frames 1 + n_b / hop, capped by max_frames[b] when that array is
// given.  Strides and the block partition come from the padded shape, so inside its frames item b runs the dense form's
// loads and MFMAs in the dense form's order: bit for bit its batch-of-one result.  Frames past the item's are stored as
// 0.0f, the item's frame count goes to frames[b], and a block wholly past its item stores its zeros and returns before
// the first barrier.
#pragma once
#include "stft_f32.h"

struct iris_mel_frontend_config;

namespace iris {
namespace mel {

constexpr int kFrames = stft::kRows;
constexpr int kWaves = stft::kWaves;
constexpr int kMaxFft = 4096;
constexpr float kClip = 1e-5f;

struct Design : stft::Sizes {
    int sample_rate = 0, n_mels = 0;
    double fmin = 0.0, fmax = 0.0;          // fmax resolved (sample_rate / 2 when the caller gave none)
    int bins8() const { return (bins() + 7) & ~7; }
    size_t lds_bytes() const { return stft_lds_bytes() + (size_t)kFrames * (bins8() + 4) * sizeof(float); }
};

// Slaney's scale (librosa hz_to_mel / mel_to_hz, htk=False)
inline double hz_to_mel(double f) {
    const double min_log_hz = 1000.0, min_log_mel = 15.0, logstep = log(6.4) / 27.0;     // 200 / 3 Hz per mel below 1000 Hz
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : 3.0 * f / 200.0;
}
inline double mel_to_hz(double m) {
    const double min_log_hz = 1000.0, min_log_mel = 15.0, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : 200.0 * m / 3.0;
}

// fb [n_mels][bins]: librosa.filters.mel(htk=False, norm="slaney")
inline void fill_filterbank(const Design& d, float* fb) {
    const int nb = d.bins(), M = d.n_mels;
    std::vector<double> mel_f(M + 2);
    const double lo = hz_to_mel(d.fmin), hi = hz_to_mel(d.fmax), step = (hi - lo) / (M + 1);
    for (int i = 0; i < M + 2; ++i) mel_f[i] = mel_to_hz(i == M + 1 ? hi : lo + i * step);        // np.linspace
    const double val = 1.0 / (d.n_fft * (1.0 / d.sample_rate));                                   // np.fft.rfftfreq
    for (int i = 0; i < M; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < nb; ++k) {
            const double f = k * val;
            const double lower = -(mel_f[i] - f) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
            const double t = lower < upper ? lower : upper;
            fb[(size_t)i * nb + k] = (float)((t > 0.0 ? t : 0.0) * enorm);
        }
    }
}

}  // namespace mel

// Checks a config and fills the design (iris_mel_frontend.hip): IRIS_HIFIGAN_OK, or the status of the rule it breaks.
int mel_validate(const ::iris_mel_frontend_config* c, mel::Design* d);

}  // namespace iris

#if defined(__HIPCC__) && !defined(IRIS_MEL_NO_KERNEL)
namespace iris {
namespace mel {

struct MelLaunch {
    const void* audio;        // [B, L] fp32 or int16
    const f32x4* wdft;        // packed windowed DFT: `taps` taps, Gp groups, n_ct column tiles
    const f32x4* wfb;         // packed filterbank, 1x1: Gp2 groups, n_ct2 tiles
    float* mel;               // [B, n_mels, T]
    int L, T, hop, taps, n_fft, bins, n_mels;
    int Gp, n_ct, Gp2, n_ct2;
    // RAGGED only
    const int32_t* n_samples; // [B] (device)
    const int32_t* max_frames;// [B] (device) or nullptr
    int32_t* frames;          // [B] out
};

template <bool SAMPLE_I16, bool RAGGED>
__global__ void __launch_bounds__(64 * kWaves) mel_kernel(const MelLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = 64 * kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y;
    const int i0 = blockIdx.x * kFrames;
    const int H = a.hop, Cp = (H + 7) & ~7, S = Cp + 4, R = kFrames - 1 + a.taps;
    const int half = a.n_fft >> 1, Kb = (a.bins + 7) & ~7, S2 = Kb + 4;
    int nb = a.L, Tb = a.T;                                  // the item's samples and frames: bounds, never strides
    if constexpr (RAGGED) {
        nb = __builtin_amdgcn_readfirstlane(a.n_samples[b]);
        nb = nb < 0 ? 0 : (nb > a.L ? a.L : nb);
        Tb = 1 + nb / H;
        if (a.max_frames) {
            int cap = __builtin_amdgcn_readfirstlane(a.max_frames[b]);
            cap = cap < 0 ? 0 : cap;
            Tb = cap < Tb ? cap : Tb;
        }
        if (blockIdx.x == 0 && tid == 0) a.frames[b] = Tb;
        if (i0 >= Tb) {                                      // block-uniform, before the first barrier
            const int cnt = a.T - i0 < kFrames ? a.T - i0 : kFrames;
            for (int idx = tid; idx < a.n_mels * cnt; idx += nthr) {
                const int m = idx / cnt, t = idx - m * cnt;
                a.mel[((size_t)b * a.n_mels + m) * a.T + i0 + t] = 0.f;
            }
            return;
        }
    }

    // the window's first sample is i0 * hop - n_fft / 2 of the item; 0 outside [0, nb)
    if constexpr (SAMPLE_I16) stft::stage_window(lds, reinterpret_cast<const int16_t*>(a.audio) + (size_t)b * a.L, (long long)i0 * H - half, nb, H, a.taps);
    else stft::stage_window(lds, reinterpret_cast<const float*>(a.audio) + (size_t)b * a.L, (long long)i0 * H - half, nb, H, a.taps);
    float* mag = lds + R * S;                                // [32][S2]: the magnitudes, bins [0, a.bins), then zeros up to Kb
    for (int idx = tid; idx < kFrames * (Kb - a.bins); idx += nthr) {
        const int r = idx / (Kb - a.bins), c = idx - r * (Kb - a.bins);
        mag[r * S2 + a.bins + c] = 0.f;
    }
    __syncthreads();

    for (int ct = wave; ct < a.n_ct; ct += kWaves) {         // wave-uniform
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        mma_loop(acc, lds + lo * S + 4 * hi, S, a.wdft + (size_t)ct * 64 + lane, (size_t)a.n_ct * 64, a.Gp, a.taps, Cp >> 3);
        stft::decode_bins(acc, ct, hi, half, [&](int bin0, const float (&re)[4], const float (&im)[4], float nyq) {
            if (bin0 == 0) mag[lo * S2 + half] = fabsf(nyq);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (bin0 + e == 0) mag[lo * S2] = fabsf(re[e]);
                else if (bin0 + e < half) mag[lo * S2 + bin0 + e] = sqrtf(re[e] * re[e] + im[e] * im[e]);
            }
        });
    }
    __syncthreads();

    const int t = i0 + lo;
    for (int ct = wave; ct < a.n_ct2; ct += kWaves) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        mma_loop(acc, mag + lo * S2 + 4 * hi, 0, a.wfb + (size_t)ct * 64 + lane, (size_t)a.n_ct2 * 64, a.Gp2, 1, Kb >> 3);
        if (t < a.T) {                                       // the 32 lanes of a half-wave store 32 consecutive frames
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int m = ct * 32 + 8 * g + 4 * hi + e;
                    // the logarithm in double, rounded once: logf is 2 ulp off at the clip value itself (16 per lane: nothing)
                    if (m < a.n_mels) a.mel[((size_t)b * a.n_mels + m) * a.T + t] = t < Tb ? (float)log((double)fmaxf(acc[4 * g + e], kClip)) : 0.f;
                }
        }
    }
}

inline hipError_t launch_mel(MelLaunch& a, const Design& d, int B, bool i16, hipStream_t stream) {
    if (B < 1 || B > 65535 || a.T < 1) return hipErrorInvalidValue;
    a.Gp = packed_groups(d.hop);
    a.n_ct = d.dft_tiles();
    a.Gp2 = packed_groups(d.bins());
    a.n_ct2 = packed_cotiles(d.n_mels);
    const dim3 grid((unsigned)((a.T + kFrames - 1) / kFrames), (unsigned)B), block(64 * kWaves);
    const size_t lds_bytes = d.lds_bytes();
    if (a.n_samples) {
        if (i16) return launch_kernel_named("mel_kernel_ragged<i16>", mel_kernel<true, true>, grid, block, lds_bytes, stream, a);
        return launch_kernel_named("mel_kernel_ragged", mel_kernel<false, true>, grid, block, lds_bytes, stream, a);
    }
    if (i16) return launch_kernel_named("mel_kernel<i16>", mel_kernel<true, false>, grid, block, lds_bytes, stream, a);
    return launch_kernel_named("mel_kernel", mel_kernel<false, false>, grid, block, lds_bytes, stream, a);
}

}  // namespace mel
}  // namespace iris
#endif
