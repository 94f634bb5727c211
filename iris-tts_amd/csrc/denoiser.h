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
// and 64 samples with the partial sums added -- restated here, not templated into griffin_lim.h.  The epilogue is the
// template parameter: SUBTRACT stores c [B][T][Qp] (interleaved complex, the inverse kernel's input), MAGNITUDE stores
// mag [B][T][Ks] for the estimator.  A lane holds 16 accumulators and, per group of 4 bins, 4 bias values.
//
// Ragged batches: `lengths` (device [B], or NULL) holds MEL frames M_b.  The kernel takes M_b = min(max(lengths[b], 0), T - 1),
// T_b = M_b + 1 (0 if M_b == 0) and L_b = H M_b, bounds its loads and stores by them and writes T_b to frames[b], which the
// inverse kernel then reads as its `lengths`.  Strides stay those of (B, T) and the tiling does not depend on T, so every
// chain of item b has the terms and the order of its batch-of-one call at M = M_b.  Nothing at t >= T_b is read or written.
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
#include "griffin_lim.h"

namespace iris {
namespace dn {

constexpr int kRows = gl::kRows;
constexpr int kWaves = gl::kWaves;
constexpr int kReduceThreads = 256;

// frames on either side whose window leaves the signal
inline int edge_frames(const mel::Design& d) { return (d.n_fft / 2 + d.hop - 1) / d.hop; }

// The finality rule of "Windows" above for the window [H m0, H (m0 + Mw)): frames [f_lo, f_hi) are computable (f_lo is
// clamped to f_hi when there is none) and samples [out_lo, out_lo + out_count) are final.  Frames before f_lo exist unless
// m0 == 0, frames from f_hi on exist unless `final`, so a row j = floor((s + n_fft / 2) / H) is final when
// j - taps + 1 >= f_lo (or m0 == 0) and j < f_hi (or final).
struct Window {
    long long f_lo, f_hi, out_lo, out_count;
    Window(const mel::Design& d, long long m0, long long Mw, bool final) {
        const long long H = d.hop, half = d.n_fft / 2, e = edge_frames(d), o = H * m0, end = o + H * Mw;
        f_lo = m0 ? m0 + e : 0;
        f_hi = final ? m0 + Mw + 1 : m0 + Mw - e + 1;
        if (f_hi < f_lo) f_hi = f_lo;
        long long lo = o, hi = end;
        if (m0 && (f_lo + d.taps() - 1) * H - half > lo) lo = (f_lo + d.taps() - 1) * H - half;
        if (!final && f_hi * H - half < hi) hi = f_hi * H - half;
        out_count = f_hi > f_lo && hi > lo ? hi - lo : 0;
        out_lo = out_count ? lo : o;
    }
};

}  // namespace dn
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace dn {

enum Epilogue { SUBTRACT = 0, MAGNITUDE = 1 };

struct StftLaunch {
    const float* y;           // [B, L]; frame 0 is centred on sample y_org
    const f32x4* wdft;        // the front-end's packed windowed DFT
    const float* bias;        // [Ks] (SUBTRACT)
    float* out;               // SUBTRACT: c [B, T, Qp]; MAGNITUDE: mag [B, T, Ks]
    const int* lengths;       // [B] mel frames, or NULL
    int* frames;              // [B] out: T_b (SUBTRACT)
    int L, T, hop, taps, n_fft, Ks, Qp, Gp, n_ct;
    int y_org;                // a window: H f_lo - o ("Windows" above); 0 for a whole utterance, where L = H (T - 1)
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
    const int Lb = a.lengths ? H * (Tb - 1) : a.L;           // H (T - 1) of a dense whole utterance as well

    {   // the front-end's window: row r, column c is sample y_org + i0 * hop - n_fft / 2 + r * hop + c; 0 outside [0, Lb)
        const long long s0 = (long long)a.y_org + (long long)i0 * H - half;
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

// The caller sets y, L, T and y_org (a whole utterance: L = hop * (T - 1), y_org = 0).
inline hipError_t launch_stft(StftLaunch& a, const gl::Design& d, int B, bool magnitude_only, hipStream_t stream) {
    a.hop = d.m.hop; a.taps = d.m.taps(); a.n_fft = d.m.n_fft; a.Ks = d.ks(); a.Qp = d.qp();
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
