// denoiser.h -- spectral bias subtraction on a waveform (iris_denoiser_*): the bias denoiser HiFiGAN users run behind the
// vocoder, fp32, on the Griffin-Lim stage's transforms (griffin_lim.h: the mel front-end's window, frames and DFT tables).
// N = n_fft, H = hop, K = N / 2 + 1 bins.  A waveform of L = H M samples (M mel frames) has T = M + 1 frames, and
// H (T - 1) = L, so the inverse transform is gl_istft_kernel as it stands.
//
//   forward   a = stft(y)[t, k];  mag = sqrtf(re re + im im);  g = fmaxf(fmaf(-strength, bias[k], mag), 0);
//             scale = mag > 0 ? g / mag : 0;  c = (scale re, scale im);  out = istft(c) (zero_tail set: out[b, L_b:] = 0)
//             Bins 0 and N / 2 are real.  strength = 0 gives scale == 1 exactly, so c is the plain STFT; a strength at or
//             above max(mag / bias) gives c == 0 and an output of exactly 0.
//   estimate  bias[k] = the mean of mag[t, k] over the interior frames of a waveform [1, L], those whose window lies wholly
//             inside the signal: e <= t < T - e with e = ceil(N / 2 / H) (= taps / 2 for an even taps = N / H).  The terms
//             are fp32, summed in fp64 in ascending t by one thread per bin and rounded once (the rule of vae_losses.h):
//             the same bits on every run.
//
// dn_stft_kernel: tiling, LDS staging and summation are gl_stft_update_kernel's -- a block owns 32 frames and stages their
// 31 + taps rows of H samples, a wave runs one 32-column tile that pairs Re and Im of 16 bins in one lane, one chain per tap
// and 64 samples with the partial sums added -- restated here so that griffin_lim.h stays as it is.  The epilogue is the
// template parameter: SUBTRACT stores c [B][T][Qp] (interleaved complex, the inverse kernel's input), MAGNITUDE stores
// mag [B][T][Ks] for the estimator.  A lane holds 16 accumulators and, per group of 4 bins, 4 bias values.
//
// Ragged batches: `lengths` (device [B], or NULL) holds MEL frames M_b.  The kernel takes M_b = min(max(lengths[b], 0), T - 1),
// T_b = M_b + 1 (0 if M_b == 0) and L_b = H M_b, bounds its loads and stores by them and writes T_b to frames[b], which the
// inverse kernel then reads as its `lengths`.  Strides stay those of (B, T) and the tiling does not depend on T, so every
// chain of item b has the terms and the order of its batch-of-one call at M = M_b.  Nothing at t >= T_b is read or written.
#pragma once
#include "griffin_lim.h"

namespace iris {
namespace dn {

constexpr int kRows = gl::kRows;
constexpr int kWaves = gl::kWaves;
constexpr int kReduceThreads = 256;

// frames on either side whose window leaves the signal
inline int edge_frames(const mel::Design& d) { return (d.n_fft / 2 + d.hop - 1) / d.hop; }

}  // namespace dn
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace dn {

enum Epilogue { SUBTRACT = 0, MAGNITUDE = 1 };

struct StftLaunch {
    const float* y;           // [B, L]
    const f32x4* wdft;        // the front-end's packed windowed DFT
    const float* bias;        // [Ks] (SUBTRACT)
    float* out;               // SUBTRACT: c [B, T, Qp]; MAGNITUDE: mag [B, T, Ks]
    const int* lengths;       // [B] mel frames, or NULL
    int* frames;              // [B] out: T_b (SUBTRACT)
    int L, T, hop, taps, n_fft, Ks, Qp, Gp, n_ct;
    float strength;
};

__device__ __forceinline__ float magnitude(float re, float im) { return sqrtf(re * re + im * im); }

__device__ __forceinline__ float subtract_scale(float mag, float bias, float strength) {
    const float g = fmaxf(fmaf(-strength, bias, mag), 0.f);
    return mag > 0.f ? g / mag : 0.f;
}

template <int EPI>
__global__ void __launch_bounds__(64 * kWaves) dn_stft_kernel(const StftLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = 64 * kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * kRows;
    const int ct = blockIdx.z * kWaves + wave;               // wave-uniform
    const int H = a.hop, Cp = (H + 7) & ~7, S = Cp + 4, R = kRows - 1 + a.taps, half = a.n_fft >> 1;
    int Tb = a.T;
    if (a.lengths) {
        int m = a.lengths[b];
        m = m < 0 ? 0 : (m > a.T - 1 ? a.T - 1 : m);
        Tb = m ? m + 1 : 0;
    }
    if (EPI == SUBTRACT && blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) a.frames[b] = Tb;
    if (i0 >= Tb) return;                                    // block-uniform: all 32 frames lie past the item
    const int Lb = H * (Tb - 1);                             // a.L of a dense call

    {   // the front-end's window: row r, column c is sample i0 * hop - n_fft / 2 + r * hop + c; 0 outside [0, Lb)
        const long long s0 = (long long)i0 * H - half;
        const size_t item = (size_t)b * a.L;
        for (int idx = tid; idx < R * Cp; idx += nthr) {
            const int r = idx / Cp, c = idx - r * Cp;
            const long long s = s0 + (long long)r * H + c;
            lds[r * S + c] = (c < H && s >= 0 && s < Lb) ? a.y[item + (size_t)s] : 0.f;
        }
    }
    __syncthreads();
    const int t = i0 + lo;
    if (ct >= a.n_ct) return;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kk = 0; kk < a.taps; ++kk)                      // one chain per tap and 64 samples ("Summation" in griffin_lim.h)
        for (int g0 = 0; g0 < Cp >> 3; g0 += 8) {
            f32x16 part;
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.f;
            mma_loop(part, lds + (lo + kk) * S + 4 * hi + 8 * g0, 0, a.wdft + ((size_t)kk * a.Gp + g0) * a.n_ct * 64 + (size_t)ct * 64 + lane,
                     (size_t)a.n_ct * 64, a.Gp, 1, (Cp >> 3) - g0 < 8 ? (Cp >> 3) - g0 : 8);
            acc += part;
        }
    if (t >= Tb) return;

    // registers 4g + e: g < 2 Re, g >= 2 Im of bin 16 ct + 8 g + 4 (lane >> 5) + e; the Im column of bin 0 is Re of bin n_fft / 2
    const size_t row = (size_t)b * a.T + t;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int bin0 = 16 * ct + 8 * g + 4 * hi;           // 4 bins
        if (bin0 >= half) continue;
        if (EPI == SUBTRACT) {
            float* crow = a.out + row * a.Qp;                // 8 consecutive floats of c
            const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + bin0);
            float cn[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float re = acc[4 * g + e];
                float im = -acc[4 * (g + 2) + e];             // the table holds +sin: the sum is minus the imaginary part
                if (bin0 + e == 0) {                          // one lane of tile 0: bins 0 and n_fft / 2 are real
                    const float nyq = acc[4 * (g + 2) + e];
                    crow[2 * half] = subtract_scale(magnitude(nyq, 0.f), a.bias[half], a.strength) * nyq;
                    crow[2 * half + 1] = 0.f;
                    im = 0.f;
                }
                const float scale = subtract_scale(magnitude(re, im), bv[e], a.strength);
                cn[2 * e] = scale * re; cn[2 * e + 1] = scale * im;
            }
            *reinterpret_cast<f32x4*>(crow + 2 * bin0) = f32x4{cn[0], cn[1], cn[2], cn[3]};
            *reinterpret_cast<f32x4*>(crow + 2 * bin0 + 4) = f32x4{cn[4], cn[5], cn[6], cn[7]};
        } else {
            float* mrow = a.out + row * a.Ks;
            f32x4 mv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float re = acc[4 * g + e];
                float im = -acc[4 * (g + 2) + e];
                if (bin0 + e == 0) {
                    mrow[half] = magnitude(acc[4 * (g + 2) + e], 0.f);
                    im = 0.f;
                }
                mv[e] = magnitude(re, im);
            }
            *reinterpret_cast<f32x4*>(mrow + bin0) = mv;
        }
    }
}

struct ReduceLaunch {
    const float* mag;         // [T, Ks]
    float* bias;              // [bins] out
    int t_lo, t_hi, Ks, bins; // the interior frames [t_lo, t_hi)
};

__global__ void __launch_bounds__(kReduceThreads) dn_bias_reduce_kernel(const ReduceLaunch a) {
    const int k = blockIdx.x * kReduceThreads + threadIdx.x;
    if (k >= a.bins) return;
    double sum = 0.0;
    for (int t = a.t_lo; t < a.t_hi; ++t) sum += (double)a.mag[(size_t)t * a.Ks + k];      // ascending t, consecutive threads: consecutive bins
    a.bias[k] = (float)(sum / (double)(a.t_hi - a.t_lo));
}

inline hipError_t launch_stft(StftLaunch& a, const gl::Design& d, int B, bool magnitude_only, hipStream_t stream) {
    a.L = d.m.hop * (a.T - 1); a.hop = d.m.hop; a.taps = d.m.taps(); a.n_fft = d.m.n_fft; a.Ks = d.ks(); a.Qp = d.qp();
    a.Gp = packed_groups(d.m.hop); a.n_ct = d.m.dft_tiles();
    const dim3 grid((unsigned)((a.T + kRows - 1) / kRows), (unsigned)B, (unsigned)((a.n_ct + kWaves - 1) / kWaves)), block(64 * kWaves);
    if (magnitude_only) return launch_kernel_named("dn_stft_kernel<magnitude>", dn_stft_kernel<MAGNITUDE>, grid, block, d.stft_lds_bytes(), stream, a);
    return launch_kernel_named("dn_stft_kernel<subtract>", dn_stft_kernel<SUBTRACT>, grid, block, d.stft_lds_bytes(), stream, a);
}

inline hipError_t launch_bias_reduce(const ReduceLaunch& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.bins + kReduceThreads - 1) / kReduceThreads)), block(kReduceThreads);
    return launch_kernel_named("dn_bias_reduce_kernel", dn_bias_reduce_kernel, grid, block, 0, stream, a);
}

}  // namespace dn
}  // namespace iris
#endif
