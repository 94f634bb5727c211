// mel_frontend.h -- waveform to log-mel on the device (iris_mel_frontend_*): the reference's compute_mel_spectrogram
// (src/iris/data.py:25-67), i.e. librosa 0.11's melspectrogram(power=1.0) followed by log(max(mel, 1e-5)).
//
//   frames   center=True, pad_mode="constant": frame t covers samples [t * hop - n_fft / 2, t * hop + n_fft / 2), 0 outside
//            the item's own [0, n); an item of n samples has 1 + n / hop frames
//   window   periodic Hann of win_length, (n_fft - win_length) / 2 zeros in front of it and the rest behind
//   mag      |sum_n x[n] w[n] e^(-2 pi i k n / n_fft)|, k = 0 .. n_fft / 2
//   mel      fb [n_mels][n_fft / 2 + 1] (Slaney scale and Slaney area normalisation) times mag
//   out      log(max(mel, 1e-5f)) taken in double and rounded once to fp32, channels-first [B, n_mels, T]
//
// design(): host only.  The windowed DFT table  w[n] cos(2 pi k n / n_fft), w[n] sin(2 pi k n / n_fft)  is evaluated in
// double with the angle reduced by (k n) mod n_fft first (one table of n_fft cosines and sines serves every entry), the
// filterbank in double by librosa's own steps; both are rounded once to fp32.  These are the bits the kernel multiplies by.
//
// mel_kernel: ONE launch.  View an item's samples as rows of `hop` floats: the windowed DFT of frame t is a
// k = n_fft / hop tap, C_in = hop implicit-GEMM convolution over rows t .. t + k - 1 of the window that starts n_fft / 2
// samples before frame t's centre -- the formulation of vae_gemm_kernel, on the MFMA loop of gemm_tile_f32.h.  A block owns
// 32 frames and stages their 31 + k rows once (rows padded to hop + 4 floats: conflict-free 16-byte reads).  Output columns
// come in 32-wide tiles that pair Re and Im of the same 16 bins in one lane:
//     column j of tile ct:  bin = 16 ct + 8 ((j >> 3) & 1) + (j & 7),  Re for j < 16, Im for j >= 16
// Im of bin 0 is identically 0, so that column carries Re of bin n_fft / 2 instead (whose Im is 0 as well): n_fft / 2 bin
// pairs, ceil(n_fft / 32) tiles, spread over the block's 8 waves.  The epilogue takes sqrtf(re * re + im * im) into an LDS
// tile of 32 frames x (n_fft / 2 + 1) bins behind the sample window -- magnitudes never go to HBM -- and after one barrier
// the filterbank runs over that tile as a second GEMM, the way the VAE's fused res_proj does.
//
// LDS: (31 + k) * (hop8 + 4) + 32 * (bins8 + 4) floats (x8 = rounded up to 8): 36 400 + 67 072 = 103 472 bytes at the
// defaults (n_fft 1024, hop 256), one block per CU.  A config whose two tiles exceed 160 KB is unsupported.
//
// Input form: fp32 samples, or int16 samples converted as x * (1.0f / 32768) while staging (SAMPLE_I16).
//
// Ragged form (RAGGED, "Ragged form" in vae_decoder.h): n_samples[B] on the device, clamped to [0, L], bounds what is fetched
// -- samples at or past it read 0 -- and gives the item's frames 1 + n_b / hop, capped by max_frames[b] when that array is
// given.  Strides and the block partition come from the padded shape, so inside its frames item b runs the dense form's
// loads and MFMAs in the dense form's order: bit for bit its batch-of-one result.  Frames past the item's are stored as
// 0.0f, the item's frame count goes to frames[b], and a block wholly past its item stores its zeros and returns before
// the first barrier.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "packed_conv_f32.h"

struct iris_mel_frontend_config;

namespace iris {
namespace mel {

constexpr int kFrames = 32;          // frames of a block (the MFMA's rows)
constexpr int kWaves = 8;
constexpr int kMaxFft = 4096;
constexpr size_t kMaxLdsBytes = 160 * 1024;
constexpr float kClip = 1e-5f;

struct Design {
    int sample_rate = 0, n_fft = 0, hop = 0, win = 0, n_mels = 0;
    double fmin = 0.0, fmax = 0.0;          // fmax resolved (sample_rate / 2 when the caller gave none)
    int taps() const { return n_fft / hop; }
    int bins() const { return n_fft / 2 + 1; }
    int dft_tiles() const { return (n_fft / 2 + 15) / 16; }
    int hop8() const { return (hop + 7) & ~7; }
    int bins8() const { return (bins() + 7) & ~7; }
    int window_rows() const { return kFrames - 1 + taps(); }
    size_t lds_bytes() const {
        return ((size_t)window_rows() * (hop8() + 4) + (size_t)kFrames * (bins8() + 4)) * sizeof(float);
    }
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

// periodic Hann of `win`, centred in n_fft (librosa pad_center)
inline void fill_window(const Design& d, std::vector<double>& w) {
    const double two_pi = 6.283185307179586476925286766559;
    w.assign(d.n_fft, 0.0);
    const int lpad = (d.n_fft - d.win) / 2;
    for (int n = 0; n < d.win; ++n) w[lpad + n] = 0.5 - 0.5 * cos(two_pi * n / d.win);
}

// dft [2][bins][n_fft]: w[n] cos(2 pi k n / n_fft), then w[n] sin(2 pi k n / n_fft)
inline void fill_dft(const Design& d, float* dft) {
    const double two_pi = 6.283185307179586476925286766559;
    const int N = d.n_fft, nb = d.bins();
    std::vector<double> w, c(N), s(N);
    fill_window(d, w);
    for (int j = 0; j < N; ++j) { c[j] = cos(two_pi * j / N); s[j] = sin(two_pi * j / N); }
    s[0] = 0.0;
    if (!(N & 1)) s[N / 2] = 0.0;                       // sin(pi): exactly 0, not 1.2e-16
    for (int k = 0; k < nb; ++k)
        for (int n = 0; n < N; ++n) {
            const int j = (int)(((long long)k * n) % N);
            dft[(size_t)k * N + n] = (float)(w[n] * c[j]);
            dft[((size_t)nb + k) * N + n] = (float)(w[n] * s[j]);
        }
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

// The DFT table as the [C_out][C_in = hop][k] Conv1d weight the kernel's column order asks for (see the head of the file).
inline void conv_weight_from_dft(const Design& d, const float* dft, std::vector<float>& w) {
    const int N = d.n_fft, H = d.hop, K = d.taps(), nb = d.bins(), half = N / 2, C_out = 32 * d.dft_tiles();
    w.assign((size_t)C_out * H * K, 0.f);
    for (int co = 0; co < C_out; ++co) {
        const int j = co & 31, bin = 16 * (co >> 5) + 8 * ((j >> 3) & 1) + (j & 7), im = j >> 4;
        if (bin >= half) continue;
        const float* row = (bin == 0 && im) ? dft + (size_t)half * N : dft + ((size_t)(im ? nb : 0) + bin) * N;
        for (int ci = 0; ci < H; ++ci)
            for (int kap = 0; kap < K; ++kap) w[((size_t)co * H + ci) * K + kap] = row[kap * H + ci];
    }
}

}  // namespace mel

// Checks a config and fills the design (iris_mel_frontend.hip): IRIS_HIFIGAN_OK, or the status of the rule it breaks.
int mel_validate(const ::iris_mel_frontend_config* c, mel::Design* d);

}  // namespace iris

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "device_info.h"
#include "gemm_tile_f32.h"

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
    const int H = a.hop, Cp = (H + 7) & ~7, S = Cp + 4;
    const int R = kFrames - 1 + a.taps;
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

    // stage the window: row r, column c is sample i0 * hop - n_fft / 2 + r * hop + c of the item; 0 outside [0, nb)
    {
        const long long s0 = (long long)i0 * H - half;
        const size_t item = (size_t)b * a.L;
        const int total = R * Cp;
        for (int idx = tid; idx < total; idx += nthr) {
            const int r = idx / Cp, c = idx - r * Cp;
            const long long s = s0 + (long long)r * H + c;
            float v = 0.f;
            if (c < H && s >= 0 && s < nb) {
                if constexpr (SAMPLE_I16) v = (float)reinterpret_cast<const int16_t*>(a.audio)[item + (size_t)s] * (1.0f / 32768);
                else v = reinterpret_cast<const float*>(a.audio)[item + (size_t)s];
            }
            lds[r * S + c] = v;
        }
    }
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
        // D[col][frame]: lane & 31 = frame, registers 4g .. 4g + 3 = columns 8g + 4 (lane >> 5) + {0..3}; g < 2 Re, g >= 2 Im
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bin = 16 * ct + 8 * g + 4 * hi + e;
                const float re = acc[4 * g + e], im = acc[4 * (g + 2) + e];
                if (bin == 0) {                              // its Im column is Re of bin n_fft / 2
                    mag[lo * S2] = fabsf(re);
                    mag[lo * S2 + half] = fabsf(im);
                } else if (bin < half) {
                    mag[lo * S2 + bin] = sqrtf(re * re + im * im);
                }
            }
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
