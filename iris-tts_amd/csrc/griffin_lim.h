// griffin_lim.h -- log-mel to waveform on the device without a trained vocoder (iris_griffin_lim_*): the reference's
// --use_griffin_lim path (scripts/synthesize.py:174-194), i.e. exp(clip(logmel, -11.513, 2)), librosa 0.11's
// mel_to_stft(power=1.0) and griffinlim(n_iter, hop_length, win_length), fp32.  The filterbank is the mel front-end's
// (mel_frontend.h); window, frames, both transforms, their buffers (S, c, r, y), their summation and the ragged rule
// (`lengths` holds frame counts: extra = 0) are stft_f32.h's.  N = n_fft, H = hop, K = N / 2 + 1 bins, T frames,
// Ly = H (T - 1) samples.
//
//   invert   m = exp(clip(logmel)) (exp in double, rounded once);  x0 = max(P m, 0), P = pinv(fb) from the caller;
//            nnls_iters steps  x <- max(x - s fb^T (fb x - m), 0),  s = 1 / lambda_max(fb fb^T) from the caller;  S = x
//   phase    c0 = S (cos phi0, sin phi0);  n_iter times:  y = istft(c);  r = stft(y);  a = r - alpha r_prev (alpha =
//            momentum / (1 + momentum); r_prev = 0 in the first pass);  c = S a / (|a| + FLT_MIN);  then out = istft(c)
//            (in a ragged forward with zero_tail set: wav[b, Ly_b:] = 0.f)
//
// gl_invert_kernel: ONE launch.  A block owns 32 frames; m (32 x n_mels), the residual and x (32 x K) stay in LDS and the
// three products run on the MFMA loop of gemm_tile_f32.h against P, fb and fb^T in fragment order.  It stores S and c0 and
// bounds item b by stft::item_frames (extra = 0) like the transforms.
//
// gl_stft_update_kernel: the forward transform of stft_f32.h (same packed table, same column order, same staging, chain loop
// and decode as stft::stft_kernel) written out with the phase update as its epilogue; it stores the new c and keeps r for the
// next pass.  It is not an instantiation of stft::stft_kernel: with the update as a policy the compiler schedules the epilogue
// differently and a 60-pass forward measured 0.3 % slower (profiles/dsp_stft_refactor.md), so a change to the transform's
// body is made in both.  The normalisation a / |a| amplifies what the transform's summation leaves where |a| is small.
//
// Start phase: with phase0 == NULL the inversion draws it in its epilogue -- Philox4x32-10, key (seed & 0xffffffff, seed >> 32),
// counter (k >> 2, t, stream, 0) with output word k & 3 for bin k of frame t; u = (x >> 8) 2^-24, angle = 6.2831855f * u (one
// fp32 product), phase = (cosf, sinf) of it.  A counter-based draw depends on no grid shape or batch position: item b of a call
// uses stream item0 + b.  gl_draw_phase_kernel stores the same numbers as a packed [B][T][bins][2] tensor.
//
// The kernels have internal linkage, like stft::gl_istft_kernel.
#pragma once
#include "mel_frontend.h"

namespace iris {
namespace gl {

constexpr int kRows = stft::kRows;   // frames of a block
constexpr int kWaves = stft::kWaves;
constexpr double kLogLo = -11.513, kLogHi = 2.0;

struct Design : mel::Design {
    int n_iter = 0, nnls_iters = 0;
    double momentum = 0.0, nnls_step = 0.0;
    static int row_floats(int C) { return ((C + 7) & ~7) + 4; }
    size_t invert_lds_bytes() const { return (size_t)kRows * (2 * row_floats(n_mels) + row_floats(bins())) * sizeof(float); }
};

}  // namespace gl
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace gl {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// The start phase of bins 4 k4 .. 4 k4 + 3 of frame t of item stream `stream`: (cos, sin) per bin.
__device__ __forceinline__ void draw_phase4(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, int t, int k4, float2 (&ph)[4]) {
    uint32_t c[4] = {(uint32_t)k4, (uint32_t)t, stream, 0u};
    philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = (float)(c[e] >> 8) * 0x1p-24f;
        const float ang = 6.2831855f * u;
        ph[e] = make_float2(cosf(ang), sinf(ang));
    }
}

struct DrawLaunch {
    float* phase;             // [B, T, bins, 2] out
    int T, bins;
    uint32_t seed_lo, seed_hi, item0;
};

static __global__ void __launch_bounds__(256) gl_draw_phase_kernel(const DrawLaunch a) {
    const int b = blockIdx.y, i0 = blockIdx.x * kRows, groups = (a.bins + 3) >> 2;
    for (int idx = threadIdx.x; idx < kRows * groups; idx += 256) {
        const int r = idx / groups, k4 = idx - r * groups, t = i0 + r;
        if (t >= a.T) break;
        float2 ph[4];
        draw_phase4(a.seed_lo, a.seed_hi, a.item0 + (uint32_t)b, t, k4, ph);
        float2* row = reinterpret_cast<float2*>(a.phase) + ((size_t)b * a.T + t) * a.bins;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * k4 + e < a.bins) row[4 * k4 + e] = ph[e];
    }
}

struct InvertLaunch {
    const float* logmel;      // [B, n_mels, T]
    const float* phase0;      // [B, T, bins, 2]: cos, sin; NULL: drawn here from (seed, item0 + b)
    const int* lengths;       // [B] or NULL
    const f32x4* wp;          // packed P: C_in n_mels, C_out bins
    const f32x4* wfb;         // packed fb: C_in bins, C_out n_mels
    const f32x4* wfbt;        // packed fb^T: C_in n_mels, C_out bins
    float* S;                 // [B, T, Ks]
    float* c;                 // [B, T, Qp]
    int T, n_mels, bins, Ks, Qp, nnls_iters;
    float step;
    int GpM, nctK, GpK, nctM;
    uint32_t seed_lo, seed_hi, item0;
};

static __global__ void __launch_bounds__(64 * kWaves) gl_invert_kernel(const InvertLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = 64 * kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * kRows;
    const int Mp = (a.n_mels + 7) & ~7, SM = Mp + 4, Kb = (a.bins + 7) & ~7, SX = Kb + 4;
    float* m = lds;                       // [32][SM]  exp(clip(logmel)); columns from n_mels on are 0
    float* res = m + kRows * SM;          // [32][SM]  fb x - m
    float* x = res + kRows * SM;          // [32][SX]  the solution; columns from bins on are 0
    const int Tb = stft::item_frames(a.lengths, b, a.T, 0);
    if (i0 >= Tb) return;                 // block-uniform: all 32 frames lie past the item

    for (int idx = tid; idx < kRows * Mp; idx += nthr) {             // consecutive threads: consecutive frames of one channel
        const int ch = idx / kRows, r = idx - ch * kRows, t = i0 + r;
        float v = 0.f;
        if (ch < a.n_mels && t < Tb) {
            double l = (double)a.logmel[((size_t)b * a.n_mels + ch) * a.T + t];
            l = l < kLogLo ? kLogLo : (l > kLogHi ? kLogHi : l);
            v = (float)exp(l);                                       // in double, rounded once (as the front-end takes its log)
        }
        m[r * SM + ch] = v;
        res[r * SM + ch] = 0.f;
    }
    for (int idx = tid; idx < kRows * (Kb - a.bins); idx += nthr) {
        const int r = idx / (Kb - a.bins), cc = idx - r * (Kb - a.bins);
        x[r * SX + a.bins + cc] = 0.f;
    }
    __syncthreads();

    for (int ct = wave; ct < a.nctK; ct += kWaves) {                 // x0 = max(P m, 0)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        mma_loop(acc, m + lo * SM + 4 * hi, 0, a.wp + (size_t)ct * 64 + lane, (size_t)a.nctK * 64, a.GpM, 1, Mp >> 3);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bin = ct * 32 + 8 * g + 4 * hi + e;
                if (bin < a.bins) x[lo * SX + bin] = fmaxf(acc[4 * g + e], 0.f);
            }
    }
    __syncthreads();

    for (int it = 0; it < a.nnls_iters; ++it) {
        for (int ct = wave; ct < a.nctM; ct += kWaves) {             // res = fb x - m
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            mma_loop(acc, x + lo * SX + 4 * hi, 0, a.wfb + (size_t)ct * 64 + lane, (size_t)a.nctM * 64, a.GpK, 1, Kb >> 3);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ch = ct * 32 + 8 * g + 4 * hi + e;
                    if (ch < a.n_mels) res[lo * SM + ch] = acc[4 * g + e] - m[lo * SM + ch];
                }
        }
        __syncthreads();
        for (int ct = wave; ct < a.nctK; ct += kWaves) {             // x = max(x - s fb^T res, 0)
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            mma_loop(acc, res + lo * SM + 4 * hi, 0, a.wfbt + (size_t)ct * 64 + lane, (size_t)a.nctK * 64, a.GpM, 1, Mp >> 3);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int bin = ct * 32 + 8 * g + 4 * hi + e;
                    if (bin < a.bins) x[lo * SX + bin] = fmaxf(x[lo * SX + bin] - a.step * acc[4 * g + e], 0.f);
                }
        }
        __syncthreads();
    }

    if (!a.phase0) {                                                 // S and c0 from the drawn phase, four bins at a time
        const int groups = (a.bins + 3) >> 2;
        for (int idx = tid; idx < kRows * groups; idx += nthr) {
            const int r = idx / groups, k4 = idx - r * groups, t = i0 + r;
            if (t >= Tb) break;
            const size_t row = (size_t)b * a.T + t;
            float2 ph[4];
            draw_phase4(a.seed_lo, a.seed_hi, a.item0 + (uint32_t)b, t, k4, ph);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * k4 + e;
                if (k >= a.bins) break;
                const float s = x[r * SX + k];
                a.S[row * a.Ks + k] = s;
                reinterpret_cast<float2*>(a.c)[(row * a.Qp >> 1) + k] = make_float2(s * ph[e].x, s * ph[e].y);
            }
        }
        return;
    }
    for (int idx = tid; idx < kRows * a.bins; idx += nthr) {         // S and c0 = S (cos, sin)
        const int r = idx / a.bins, k = idx - r * a.bins, t = i0 + r;
        if (t >= Tb) break;
        const size_t row = (size_t)b * a.T + t;
        const float s = x[r * SX + k];
        const float2 ph = reinterpret_cast<const float2*>(a.phase0)[row * a.bins + k];
        a.S[row * a.Ks + k] = s;
        reinterpret_cast<float2*>(a.c)[(row * a.Qp >> 1) + k] = make_float2(s * ph.x, s * ph.y);
    }
}

struct StftLaunch {
    const float* y;           // [B, Ly]
    const f32x4* wdft;        // the front-end's packed windowed DFT
    const float* S;           // [B, T, Ks]
    float* c;                 // [B, T, Qp] out
    float* r;                 // [B, T, Qp] r_prev in (unless first), r out
    const int* lengths;       // [B] or NULL
    int Ly, T, hop, taps, n_fft, Ks, Qp, Gp, n_ct, first;
    float alpha;
};

__device__ __forceinline__ void phase_update(float re, float im, float pr, float pi, float alpha, float s, float& cre, float& cim) {
    const float ar = re - alpha * pr, ai = im - alpha * pi;
    const float den = sqrtf(ar * ar + ai * ai) + FLT_MIN;
    cre = s * ar / den;
    cim = s * ai / den;
}

static __global__ void __launch_bounds__(64 * kWaves) gl_stft_update_kernel(const StftLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = 64 * kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * kRows;
    const int ct = blockIdx.z * kWaves + wave;               // wave-uniform
    const int H = a.hop, Cp = (H + 7) & ~7, S = Cp + 4, R = kRows - 1 + a.taps, half = a.n_fft >> 1;
    const int Tb = stft::item_frames(a.lengths, b, a.T, 0);
    if (i0 >= Tb) return;                                    // block-uniform: all 32 frames lie past the item
    const int Lyb = H * (Tb - 1);                            // a.Ly of a dense call

    {   // the front-end's window: row r, column c is sample i0 * hop - n_fft / 2 + r * hop + c; 0 outside [0, Ly)
        const long long s0 = (long long)i0 * H - half;
        const size_t item = (size_t)b * a.Ly;
        for (int idx = tid; idx < R * Cp; idx += nthr) {
            const int r = idx / Cp, c = idx - r * Cp;
            const long long s = s0 + (long long)r * H + c;
            lds[r * S + c] = (c < H && s >= 0 && s < Lyb) ? a.y[item + (size_t)s] : 0.f;
        }
    }
    __syncthreads();
    const int t = i0 + lo;
    if (ct >= a.n_ct) return;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kk = 0; kk < a.taps; ++kk)                      // one chain per tap and 64 samples (see "Summation" above)
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
    float* crow = a.c + row * a.Qp;
    float* rrow = a.r + row * a.Qp;
    const float* srow = a.S + row * a.Ks;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int bin0 = 16 * ct + 8 * g + 4 * hi;           // 4 bins, 8 consecutive floats of c and r
        if (bin0 >= half) continue;
        const f32x4 sv = *reinterpret_cast<const f32x4*>(srow + bin0);
        f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0;
        if (!a.first) {
            p0 = *reinterpret_cast<const f32x4*>(rrow + 2 * bin0);
            p1 = *reinterpret_cast<const f32x4*>(rrow + 2 * bin0 + 4);
        }
        const float prev[8] = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
        float cn[8], rn[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float re = acc[4 * g + e];
            float im = -acc[4 * (g + 2) + e];                 // the table holds +sin: the sum is minus the imaginary part
            if (bin0 + e == 0) {                              // one lane of tile 0: bins 0 and n_fft / 2 are real
                const float nyq = acc[4 * (g + 2) + e], pn = a.first ? 0.f : rrow[2 * half];
                float cre, unused;
                phase_update(nyq, 0.f, pn, 0.f, a.alpha, srow[half], cre, unused);
                rrow[2 * half] = nyq; rrow[2 * half + 1] = 0.f;
                crow[2 * half] = cre; crow[2 * half + 1] = 0.f;
                im = 0.f;
            }
            rn[2 * e] = re; rn[2 * e + 1] = im;
            phase_update(re, im, prev[2 * e], bin0 + e == 0 ? 0.f : prev[2 * e + 1], a.alpha, sv[e], cn[2 * e], cn[2 * e + 1]);
        }
        *reinterpret_cast<f32x4*>(rrow + 2 * bin0) = f32x4{rn[0], rn[1], rn[2], rn[3]};
        *reinterpret_cast<f32x4*>(rrow + 2 * bin0 + 4) = f32x4{rn[4], rn[5], rn[6], rn[7]};
        *reinterpret_cast<f32x4*>(crow + 2 * bin0) = f32x4{cn[0], cn[1], cn[2], cn[3]};
        *reinterpret_cast<f32x4*>(crow + 2 * bin0 + 4) = f32x4{cn[4], cn[5], cn[6], cn[7]};
    }
}

inline hipError_t launch_invert(InvertLaunch& a, const Design& d, int B, hipStream_t stream) {
    a.n_mels = d.n_mels; a.bins = d.bins(); a.Ks = d.ks(); a.Qp = d.qp(); a.nnls_iters = d.nnls_iters; a.step = (float)d.nnls_step;
    a.GpM = packed_groups(d.n_mels); a.nctK = packed_cotiles(d.bins());
    a.GpK = packed_groups(d.bins()); a.nctM = packed_cotiles(d.n_mels);
    const dim3 grid((unsigned)((a.T + kRows - 1) / kRows), (unsigned)B), block(64 * kWaves);
    return launch_kernel_named("gl_invert_kernel", gl_invert_kernel, grid, block, d.invert_lds_bytes(), stream, a);
}

inline hipError_t launch_draw_phase(const DrawLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)((a.T + kRows - 1) / kRows), (unsigned)B), block(256);
    return launch_kernel_named("gl_draw_phase_kernel", gl_draw_phase_kernel, grid, block, 0, stream, a);
}

inline hipError_t launch_stft_update(StftLaunch& a, const Design& d, int B, hipStream_t stream) {
    a.Ly = d.hop * (a.T - 1); a.hop = d.hop; a.taps = d.taps(); a.n_fft = d.n_fft; a.Ks = d.ks(); a.Qp = d.qp();
    a.Gp = packed_groups(d.hop); a.n_ct = d.dft_tiles();
    a.alpha = (float)(d.momentum / (1.0 + d.momentum));
    const dim3 grid((unsigned)((a.T + kRows - 1) / kRows), (unsigned)B, (unsigned)((a.n_ct + kWaves - 1) / kWaves)), block(64 * kWaves);
    return launch_kernel_named("gl_stft_update_kernel", gl_stft_update_kernel, grid, block, d.stft_lds_bytes(), stream, a);
}

}  // namespace gl
}  // namespace iris
#endif
