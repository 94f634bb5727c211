// time_stretch.h -- the phase vocoder between the two transforms of stft_f32.h (iris_time_stretch_*): tempo without pitch,
// librosa.effects.time_stretch(y, rate=, n_fft=, hop_length=, win_length=) under that file's frame rules, fp32.
// N = n_fft, H = hop, K = N / 2 + 1 bins.  A waveform of L = H M samples has T = M + 1 frames c[t, k] = stft(y).
//
//   T_out     = ceil(T / rate) in double                    (len(np.arange(0, T, rate)))
//   step_t    = t * rate in double;  i = floor(step_t);  alpha = (float)(step_t - i);  a column >= T reads as 0
//   mag[t,k]  = fmaf(alpha, |c[i+1,k]|, (1 - alpha) |c[i,k]|)          |c| = sqrtf(re re + im im)
//   dphi      = turns(c[i+1,k]) - turns(c[i,k]) - adv_k;  dphi -= rintf(dphi)
//   acc[0,k]  = fixed(turns(c[0,k]));  acc[t+1,k] = acc[t,k] + inc[t,k],  inc = adv_fixed_k + fixed(dphi)
//   out_c[t,k]= mag[t,k] (cos, sin)(2 pi acc[t,k] / 2^32)
//   n_out     = rint(L / rate) in double (half to even)
//   y_out     = istft(out_c, length = n_out): samples below min(n_out, H (T_out - 1) + N / 2) are the overlap-add value over the
//               window-sum-square of the frames that exist, the rest are 0
//
// Phase is accumulated in 32-bit fixed-point turns, 2^32 = one turn: the advance of the top bin is pi H radians a frame, and
// an fp32 sum of radians would stand near 8e5 after 1000 frames at hop 256, where one ulp is 0.06 rad.  A uint32 sum wraps
// for free and is associative, so the scan along t may run in any order and every run gives the same bits.  The
// conversions, written down here once:
//   turns(c)      atan2f(im, re) * (1 / (2 pi)) in fp32: [-0.5, 0.5]
//   wrap          x - rintf(x): the nearest representative of x turns, [-0.5, 0.5]
//   fixed(x)      (uint32)(int64)llrintf(x * 4294967296.f): half a turn is 2^31 either way round
//   adv_k         r = (k H) mod N;  adv_fixed_k = (uint32)(((uint64)r << 32) / N);  in fp32 turns (float)r / (float)N
//   unfixed(a)    (float)(int32)a * 2^-32: [-0.5, 0.5)
//
// Four launches: stft_kernel<ts::Spectrum> (the plain interleaved spectrum c [B, T, Qp] and the items' counts), ts_step_kernel
// (mag and inc [B, T_out, Ks]), ts_scan_kernel (the exclusive scan of inc along t, acc [B, T_out, Ks], and the phasor
// out_c [B, T_out, Qp]) and gl_istft_kernel bounded by the items' sample counts (IstftLaunch::sample_counts).
//
// ts_scan_kernel is two-level: a block owns kScanBins bins of one item and splits the item's T_out_b frames into kScanRuns
// runs of ceil(T_out_b / kScanRuns) frames; a thread sums its run of one bin, the run sums go to LDS, a thread adds those
// in front of its own, and walks its run again.  Integer sums: no order matters, no atomics.
//
// Ragged batches: `lengths` (device [B], or NULL) holds MEL frames M_b as in denoiser.h: T_b = M_b + 1 (0 if M_b == 0),
// L_b = H M_b.  Spectrum::item computes T_out_b = ceil(T_b / rate) and n_out_b = rint(L_b / rate) on the device, in double, and
// stores them with T_b; every later launch bounds item b by them.  Strides are those of the dense call (T, T_out, n_out of
// the whole L), a thread's work depends on its own (b, t, k) alone, and so item b is bit for bit its batch-of-one call.
// out_samples() is the same arithmetic on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "stft_f32.h"

namespace iris {
namespace ts {

constexpr double kMinRate = 0.25, kMaxRate = 4.0;
constexpr int kStepThreads = 256;
constexpr int kScanBins = 32, kScanRuns = 32;            // a block of ts_scan_kernel: 32 runs of 32 consecutive bins

// T_out and n_out of an item of T frames and L samples (T == 0: an empty item).  Host and device run these same lines.
__host__ __device__ inline int frames_out(int T, double rate) { return T > 0 ? (int)ceil((double)T / rate) : 0; }
__host__ __device__ inline long long samples_out(long long L, double rate) { return (long long)rint((double)L / rate); }

// adv_k in fixed-point turns and in fp32 turns
__host__ __device__ inline uint32_t advance_fixed(int k, int hop, int n_fft) {
    const uint64_t r = (uint64_t)(((long long)k * hop) % n_fft);
    return (uint32_t)((r << 32) / (uint64_t)n_fft);
}
__host__ __device__ inline float advance_turns(int k, int hop, int n_fft) {
    return (float)(((long long)k * hop) % n_fft) / (float)n_fft;
}

}  // namespace ts
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace ts {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// every product and sum below is a rounding of its own: nothing is contracted into an fma that the text does not name
#pragma clang fp contract(off)
__device__ __forceinline__ float magnitude(float re, float im) { return sqrtf(re * re + im * im); }
__device__ __forceinline__ float turns(float re, float im) { return atan2f(im, re) * 0.15915494309189535f; }
__device__ __forceinline__ float wrap(float x) { return x - rintf(x); }
__device__ __forceinline__ uint32_t fixed(float x) { return (uint32_t)(long long)llrintf(x * 4294967296.f); }
__device__ __forceinline__ float unfixed(uint32_t a) { return (float)(int32_t)a * 2.3283064365386963e-10f; }

// The epilogue of launch 1 (a stft::stft_kernel policy): the plain spectrum, and per item T_b, T_out_b and n_out_b.
struct Spectrum {
    float* c;                 // [B, T, Qp] out
    int* frames;              // [B] out: T_b
    int* frames_out;          // [B] out: T_out_b
    int* counts;              // [B] out: n_out_b
    int* counts_user;         // [B] out, or NULL: the same, for the caller's next stage
    double rate;
    int hop;                  // item() gets no launch arguments
    static constexpr const char* kName = "stft_kernel<ts::Spectrum>";
    static constexpr int kExtraFrames = 1;
    __device__ __forceinline__ void item(int b, int Tb) const {
        const int n = (int)samples_out(Tb ? (long long)hop * (Tb - 1) : 0, rate);
        frames[b] = Tb;
        frames_out[b] = ts::frames_out(Tb, rate);
        counts[b] = n;
        if (counts_user) counts_user[b] = n;
    }
    __device__ __forceinline__ void bins4(const stft::StftLaunch& a, size_t row, int bin0, const float (&re)[4], const float (&im)[4], float nyq) const {
        float* crow = c + row * a.Qp + 2 * bin0;             // 4 bins, 8 consecutive floats of c
        if (bin0 == 0) {
            float* nrow = c + row * a.Qp + a.n_fft;           // column 2 (n_fft / 2)
            nrow[0] = nyq; nrow[1] = 0.f;
        }
        *reinterpret_cast<f32x4*>(crow) = f32x4{re[0], im[0], re[1], im[1]};
        *reinterpret_cast<f32x4*>(crow + 4) = f32x4{re[2], im[2], re[3], im[3]};
    }
};

struct StepLaunch {
    const float* c;           // [B, T, Qp]
    const int* frames;        // [B] T_b
    const int* frames_out;    // [B] T_out_b
    float* mag;               // [B, T_out, Ks] out
    uint32_t* inc;            // [B, T_out, Ks] out
    double rate;
    int T, T_out, Ks, Qp, bins, hop, n_fft;
};

// Launch 2.  A thread owns 4 consecutive bins of one output frame: 8 consecutive floats of source rows i and i + 1 (two 16-byte
// loads each), 4 magnitudes and 4 increments (one 16-byte store each).  Consecutive lanes are consecutive groups of bins.
// Columns of c from 2 K on were never written: they are loaded with their group and replaced by 0.
__global__ void __launch_bounds__(kStepThreads) ts_step_kernel(const StepLaunch a) {
    const int b = blockIdx.y, G = a.Ks >> 2;
    const int Tb = a.frames[b], To = a.frames_out[b];
    const long long idx = (long long)blockIdx.x * kStepThreads + threadIdx.x;
    const int t = (int)(idx / G), g = (int)(idx - (long long)t * G);
    if (t >= To) return;
    const double step = (double)t * a.rate;
    const double fl = floor(step);
    const int i = (int)fl;
    const float alpha = (float)(step - fl);
    const int bin0 = 4 * g;
    float v0[8], v1[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
        if (i < Tb) x0 = *reinterpret_cast<const f32x4*>(a.c + ((size_t)b * a.T + i) * a.Qp + 2 * bin0 + 4 * h);
        if (i + 1 < Tb) x1 = *reinterpret_cast<const f32x4*>(a.c + ((size_t)b * a.T + i + 1) * a.Qp + 2 * bin0 + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v0[4 * h + e] = x0[e]; v1[4 * h + e] = x1[e]; }
    }
    f32x4 mv;
    u32x4 iv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = bin0 + e;
        const bool live = k < a.bins;
        const float re0 = live ? v0[2 * e] : 0.f, im0 = live ? v0[2 * e + 1] : 0.f;
        const float re1 = live ? v1[2 * e] : 0.f, im1 = live ? v1[2 * e + 1] : 0.f;
        mv[e] = fmaf(alpha, magnitude(re1, im1), (1.f - alpha) * magnitude(re0, im0));
        const float dphi = wrap(turns(re1, im1) - turns(re0, im0) - advance_turns(k, a.hop, a.n_fft));
        iv[e] = live ? advance_fixed(k, a.hop, a.n_fft) + fixed(dphi) : 0u;
    }
    const size_t o = ((size_t)b * a.T_out + t) * a.Ks + bin0;
    *reinterpret_cast<f32x4*>(a.mag + o) = mv;
    *reinterpret_cast<u32x4*>(a.inc + o) = iv;
}

inline hipError_t launch_step(const StepLaunch& a, int B, hipStream_t stream) {
    const long long work = (long long)a.T_out * (a.Ks >> 2);
    const dim3 grid((unsigned)((work + kStepThreads - 1) / kStepThreads), (unsigned)B), block(kStepThreads);
    return launch_kernel_named("ts_step_kernel", ts_step_kernel, grid, block, 0, stream, a);
}

struct ScanLaunch {
    const float* c;           // [B, T, Qp]: row 0 gives the start phase
    const float* mag;         // [B, T_out, Ks]
    const uint32_t* inc;      // [B, T_out, Ks]
    const int* frames_out;    // [B] T_out_b
    uint32_t* acc;            // [B, T_out, Ks] out
    float* out_c;             // [B, T_out, Qp] out
    int T, T_out, Ks, Qp, bins;
};

// Launch 3.  Thread (run r = threadIdx.x / kScanBins, bin k = kScanBins blockIdx.x + threadIdx.x % kScanBins) of item b: frames
// [r len, (r + 1) len) with len = ceil(T_out_b / kScanRuns).  2 Ks == Qp, so the bins of a row fill every column of out_c.
__global__ void __launch_bounds__(kScanBins * kScanRuns) ts_scan_kernel(const ScanLaunch a) {
    __shared__ uint32_t sums[kScanRuns][kScanBins];
    const int b = blockIdx.y, lane = threadIdx.x % kScanBins, r = threadIdx.x / kScanBins;
    const int k = blockIdx.x * kScanBins + lane;
    const int To = a.frames_out[b];
    if (To <= 0) return;                                     // block-uniform
    const int len = (To + kScanRuns - 1) / kScanRuns;
    const int t0 = r * len < To ? r * len : To, t1 = t0 + len < To ? t0 + len : To;
    const bool live = k < a.Ks;
    const size_t base = (size_t)b * a.T_out * a.Ks + k;
    uint32_t sum = 0;
    if (live)
        for (int t = t0; t < t1; ++t) sum += a.inc[base + (size_t)t * a.Ks];
    sums[r][lane] = sum;
    __syncthreads();
    if (!live) return;
    uint32_t acc = 0;
    if (k < a.bins) {
        const float* c0 = a.c + (size_t)b * a.T * a.Qp + 2 * k;
        acc = fixed(turns(c0[0], c0[1]));
    }
    for (int q = 0; q < r; ++q) acc += sums[q][lane];
    for (int t = t0; t < t1; ++t) {
        const size_t o = base + (size_t)t * a.Ks;
        const float m = a.mag[o], x = 2.f * unfixed(acc);
        float s, co;
        sincospif(x, &s, &co);
        a.acc[o] = acc;
        *reinterpret_cast<float2*>(a.out_c + ((size_t)b * a.T_out + t) * a.Qp + 2 * k) = float2{m * co, m * s};
        acc += a.inc[o];
    }
}

inline hipError_t launch_scan(const ScanLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)((a.Ks + kScanBins - 1) / kScanBins), (unsigned)B), block(kScanBins * kScanRuns);
    return launch_kernel_named("ts_scan_kernel", ts_scan_kernel, grid, block, 0, stream, a);
}

}  // namespace ts
}  // namespace iris
#endif
