// denoiser.h -- spectral bias subtraction on a waveform (iris_denoiser_*): the bias denoiser HiFiGAN users run behind the
// vocoder, fp32, on the transforms of stft_f32.h (window, frames, tables, buffers, summation).
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
// dn_stft_kernel<subtract | magnitude>: stft::stft_kernel with Subtract or Magnitude as its epilogue.  Subtract stores
// c [B][T][Qp] (interleaved complex, the inverse kernel's input), Magnitude stores mag [B][T][Ks] for the estimator.  A lane
// holds 16 accumulators and, per group of 4 bins, 4 bias values.
//
// Ragged batches: `lengths` (device [B], or NULL) holds MEL frames M_b: stft::item_frames with extra = 1, so M_b =
// min(max(lengths[b], 0), T - 1), T_b = M_b + 1 (0 if M_b == 0) and L_b = H M_b.  Subtract writes T_b to frames[b], which the
// inverse kernel then reads as its `lengths`.
//
// Windows (iris_denoiser_forward_window): a dense call on samples [o, o + Lw) of an utterance, o = H m0, Lw = H Mw, `final`
// when o + Lw is the utterance's end.  Frame t exists when t >= 0 and, if final, t <= m0 + Mw; it is computable when every
// sample of its span inside the utterance lies inside the window; a sample is final when each of its `taps` frames is
// computable or does not exist.  `Window` below is that rule in closed form, the only place it is written down.  A frame's
// chain depends on its own n_fft samples alone and a row's on its own `taps` frames alone, not on the block or lane either
// falls into, so both launches run in coordinates that start at the window's first computable frame f_lo: the STFT reads its
// samples `y_org` = H f_lo - o into the window (StftLaunch::y_org) and stores c [B, frames, Qp]; the inverse transform sees
// c as a whole utterance's -- a final sample's frames outside [f_lo, f_hi) do not exist, so "staged as 0, no w^2 term" is
// the one-shot's own treatment of them -- and stores the samples from `s_org` = out_lo - H f_lo on (IstftLaunch::s_org).
// With both origins 0 and L = H (T - 1) the launches are the whole-utterance ones.
#pragma once
#include "stft_f32.h"

namespace iris {
namespace dn {

constexpr int kReduceThreads = 256;

// edge_frames and Window -- the finality rule of "Windows" above in closed form, the only place it is written down -- live in
// stft_f32.h, where the time stretch's windows (time_stretch.h) reach them too.
using stft::edge_frames;
using stft::Window;

}  // namespace dn
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace dn {

__device__ __forceinline__ float magnitude(float re, float im) { return sqrtf(re * re + im * im); }

__device__ __forceinline__ float subtract_scale(float mag, float bias, float strength) {
    const float g = fmaxf(fmaf(-strength, bias, mag), 0.f);
    return mag > 0.f ? g / mag : 0.f;
}

// The two epilogues of dn_stft_kernel (stft::stft_kernel policies).
struct Subtract {
    const float* bias;        // [Ks]
    float* c;                 // [B, T, Qp] out
    int* frames;              // [B] out: T_b
    float strength;
    static constexpr const char* kName = "dn_stft_kernel<subtract>";
    static constexpr int kExtraFrames = 1;
    __device__ __forceinline__ void item(int b, int Tb) const { frames[b] = Tb; }
    __device__ __forceinline__ void bins4(const stft::StftLaunch& a, size_t row, int bin0, const float (&re)[4], const float (&im)[4], float nyq) const {
        float* crow = c + row * a.Qp + 2 * bin0;             // 4 bins, 8 consecutive floats of c
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + bin0);
        if (bin0 == 0) nyquist(a, row, nyq);
        float cn[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float scale = subtract_scale(magnitude(re[e], im[e]), bv[e], strength);
            cn[2 * e] = scale * re[e]; cn[2 * e + 1] = scale * im[e];
        }
        *reinterpret_cast<f32x4*>(crow) = f32x4{cn[0], cn[1], cn[2], cn[3]};
        *reinterpret_cast<f32x4*>(crow + 4) = f32x4{cn[4], cn[5], cn[6], cn[7]};
    }
    __device__ __forceinline__ void nyquist(const stft::StftLaunch& a, size_t row, float nyq) const {
        float* crow = c + row * a.Qp + a.n_fft;               // column 2 (n_fft / 2)
        crow[0] = subtract_scale(magnitude(nyq, 0.f), bias[a.n_fft >> 1], strength) * nyq;
        crow[1] = 0.f;
    }
};

struct Magnitude {
    float* mag;               // [B, T, Ks] out
    static constexpr const char* kName = "dn_stft_kernel<magnitude>";
    static constexpr int kExtraFrames = 1;
    __device__ __forceinline__ void item(int, int) const {}
    __device__ __forceinline__ void bins4(const stft::StftLaunch& a, size_t row, int bin0, const float (&re)[4], const float (&im)[4], float nyq) const {
        if (bin0 == 0) nyquist(a, row, nyq);
        f32x4 mv;
#pragma unroll
        for (int e = 0; e < 4; ++e) mv[e] = magnitude(re[e], im[e]);
        *reinterpret_cast<f32x4*>(mag + row * a.Ks + bin0) = mv;
    }
    __device__ __forceinline__ void nyquist(const stft::StftLaunch& a, size_t row, float nyq) const {
        mag[row * a.Ks + (a.n_fft >> 1)] = magnitude(nyq, 0.f);
    }
};

#ifndef IRIS_DN_POLICIES_ONLY            // a translation unit that takes the policies alone (spectral_distance.h) carries no estimator
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

inline hipError_t launch_bias_reduce(const ReduceLaunch& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.bins + kReduceThreads - 1) / kReduceThreads)), block(kReduceThreads);
    return launch_kernel_named("dn_bias_reduce_kernel", dn_bias_reduce_kernel, grid, block, 0, stream, a);
}
#endif

}  // namespace dn
}  // namespace iris
#endif
