// pcm_out.h -- the output stage on the device: 16-bit PCM and per-item peak normalisation.
//
// What a caller does with the fp32 waveform before it writes a file (reference: scripts/synthesize.py writes a 16-bit WAV;
// demo_vocoder.py first scales to 0.95 / (max|w| + 1e-8)), restated in fp32 so that the host formula
// (iris.synthesis_output.pcm16_from_float) and the device produce the same bits:
//
//   plain        pcm = (int16) rintf(clamp(w, -1, 1) * 32767)                 -- conv_post's store epilogue (OUT_PCM16)
//   normalised   q   = (w / (peak[b] + 1e-8f)) * target                       -- every operation its own fp32 rounding,
//                pcm = (int16) rintf(clamp(q, -1, 1) * 32767)                    the division the correctly rounded one
//
// The peak of item b is max |w| over the item's own samples.  conv_post forms it beside its fp32 store (OUT_F32_PEAK): wave
// max -> block max -> ONE vector atomicMax per block on the uint bit pattern of the non-negative float (ordered like the
// floats; max is order-independent, so the result is deterministic) into peak[b], which the host zeroes beforehand on the
// same stream.  pcm_normalize_kernel then reads the fp32 waveform with 16-byte loads and writes int16 with 8-byte stores;
// an item whose first sample is not on such a boundary (odd hop * T) takes scalar head and tail elements.
// rintf rounds half to even (np.round); there is no add behind a multiply, so nothing contracts into an fma; a NaN clamps
// to -1 through fmaxf / fminf, so the float -> int cast is always defined.
//
// Telephony: G.711 mu-law and A-law bytes are integer functions of that int16 sample (ulaw_from_pcm16 / alaw_from_pcm16), stored
// by the resampler's kernel (OUT_ULAW / OUT_ALAW of store_sample) or by g711_kernel on a waveform that exists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_info.h"

namespace iris {
namespace pcm {       // self-contained: included by the fp32 and the bf16 translation unit

enum : int {
    OUT_F32 = 0,        // fp32 waveform (the plain forward)
    OUT_PCM16 = 1,      // int16 PCM instead of the waveform
    OUT_F32_PEAK = 2,   // fp32 waveform and the item's peak |w|
    OUT_ULAW = 3,       // G.711 mu-law, one byte per sample (the resampler and g711_kernel; conv_post has no such form)
    OUT_ALAW = 4,       // G.711 A-law
};

constexpr float kPcmScale = 32767.0f;
constexpr float kPeakEps = 1e-8f;

__device__ __forceinline__ int16_t pcm16_of(float w) {
    return (int16_t)rintf(fminf(fmaxf(w, -1.f), 1.f) * kPcmScale);
}

// G.711 from the 16-bit sample, in integers alone (the rules of include/iris_hifigan.h, restated in numpy by
// iris.synthesis_output.ulaw_from_pcm16 / alaw_from_pcm16).  floor(log2) is a count of leading zeros: m >= 132 and, where it is
// asked, a >= 32, so its argument is never 0.
__host__ __device__ inline uint8_t ulaw_from_pcm16(int s) {
    const unsigned sign = s < 0 ? 1u : 0u;
    const int mag = s < 0 ? -s : s;                                 // 32 bits: |-32768| is itself
    const unsigned m = (unsigned)(mag < 32635 ? mag : 32635) + 132u;
    const unsigned e = (unsigned)(31 - __builtin_clz(m)) - 7u;      // 0 .. 7
    const unsigned mant = (m >> (e + 3u)) & 15u;
    return (uint8_t)(~(sign << 7 | e << 4 | mant) & 0xFFu);
}

__host__ __device__ inline uint8_t alaw_from_pcm16(int s) {
    int a = s >> 3;                                                 // arithmetic
    unsigned mask = 0xD5u;
    if (a < 0) { a = ~a; mask = 0x55u; }
    const unsigned u = (unsigned)a;                                 // 0 .. 4095
    const unsigned seg = u < 32u ? 0u : (unsigned)(31 - __builtin_clz(u)) - 4u;     // 0 .. 7
    const unsigned mant = (seg < 2u ? u >> 1 : u >> seg) & 15u;
    return (uint8_t)((seg << 4 | mant) ^ mask);
}

constexpr uint8_t kUlawZero = 0xFF, kAlawZero = 0xD5;               // the codes of sample 0: what padding holds, never byte 0

__device__ __forceinline__ uint8_t ulaw_of(float w) { return ulaw_from_pcm16((int)pcm16_of(w)); }
__device__ __forceinline__ uint8_t alaw_of(float w) { return alaw_from_pcm16((int)pcm16_of(w)); }
template <int LAW>
__device__ __forceinline__ uint8_t g711_of(float w) {
    static_assert(LAW == OUT_ULAW || LAW == OUT_ALAW, "a G.711 law");
    if constexpr (LAW == OUT_ULAW) return ulaw_of(w);
    else                           return alaw_of(w);
}

__device__ __forceinline__ unsigned abs_bits(float w) { return __builtin_bit_cast(unsigned, w) & 0x7fffffffu; }

// max of `bits` over a block of 256 threads (every thread of the block calls it) -> one atomicMax into *word
__device__ __forceinline__ void block_peak_max(unsigned bits, unsigned* word) {
    __shared__ unsigned red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)bits, o);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned m01 = red[0] > red[1] ? red[0] : red[1], m23 = red[2] > red[3] ? red[2] : red[3];
        const unsigned m = m01 > m23 ? m01 : m23;
        if (m) atomicMax(word, m);          // (a vector atomic; the word was zeroed on this stream)
    }
}

// What conv_post stores for sample i of the output (w = tanh(acc), or 0 past a ragged item's length) in output form OUT.
// The peak of OUT_F32_PEAK is reduced by the caller (block_peak_max), which every thread of the block must reach.
// OUT_ULAW / OUT_ALAW (the resampler's launch alone has a.g711) store one byte; w = 0 gives the law's code for 0.
template <int OUT, class A>
__device__ __forceinline__ void store_sample(const A& a, size_t i, float w) {
    if constexpr (OUT == OUT_PCM16) a.pcm[i] = pcm16_of(w);
    else if constexpr (OUT == OUT_ULAW || OUT == OUT_ALAW) a.g711[i] = g711_of<OUT>(w);
    else                            a.y[i] = w;
}

struct PcmLaunch {
    const float* wav;           // [B, L] fp32
    const int32_t* lengths;     // ragged: frames of each item [B] (device), or nullptr
    int row_scale;              // samples per frame: item b has ragged_rows(lengths, b, row_scale, L) samples, the rest is 0
    int16_t* pcm;               // [B, L]
    float* peak;                // [B]: read by pcm_normalize_kernel<true>, written by pcm_peak_kernel
    int B, L;
    float target;
};

// peak[b] = max |wav[b, :Lb]| on its own (the single-layer entry point; a forward gets it from conv_post).  grid (x, B).
template <int UNUSED>
__global__ void __launch_bounds__(256) pcm_peak_kernel(const PcmLaunch a) {
    const int b = blockIdx.y;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const float* __restrict__ w = a.wav + (size_t)b * a.L;
    unsigned bits = 0;
    for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < Lb; i += (int)(gridDim.x * 256)) {
        const unsigned v = abs_bits(w[i]);
        bits = v > bits ? v : bits;
    }
    block_peak_max(bits, reinterpret_cast<unsigned*>(a.peak) + b);
}

typedef float pf32x4 __attribute__((ext_vector_type(4)));
typedef short pi16x4 __attribute__((ext_vector_type(4)));

// fp32 [B, L] -> int16 [B, L].  grid (x, B); a block converts 1024 consecutive samples of item b as 16-byte loads and 8-byte
// stores, from the first sample of the item whose two addresses are 16- / 8-byte aligned; the (at most three) samples in
// front of it and behind the last whole group are scalar.  Were the two alignments to disagree (a caller's own pointers),
// the whole item is scalar.
template <bool NORMALIZE>
__global__ void __launch_bounds__(256) pcm_normalize_kernel(const PcmLaunch a) {
    const int b = blockIdx.y;
    const int L = a.L;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, L);
    const float* __restrict__ w = a.wav + (size_t)b * L;
    int16_t* __restrict__ p = a.pcm + (size_t)b * L;
    float den = 1.f;
    if constexpr (NORMALIZE) den = a.peak[b] + kPeakEps;
    const float target = a.target;
    auto conv = [&](float v, int i) -> int16_t {
        if (i >= Lb) return (int16_t)0;
        if constexpr (NORMALIZE) v = (v / den) * target;
        return pcm16_of(v);
    };
    const unsigned mis_w = (unsigned)((uintptr_t)w >> 2) & 3u, mis_p = (unsigned)((uintptr_t)p >> 1) & 3u;
    int head = mis_w == mis_p ? (int)((4u - mis_w) & 3u) : L;
    if (head > L) head = L;
    const int nvec = (L - head) >> 2;
    const int tail = head + 4 * nvec;
    const int g = (int)(blockIdx.x * 256 + threadIdx.x), stride = (int)(gridDim.x * 256);
    for (int v = g; v < nvec; v += stride) {
        const int i = head + 4 * v;
        const pf32x4 x = *reinterpret_cast<const pf32x4*>(w + i);
        pi16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = conv(x[e], i + e);
        *reinterpret_cast<pi16x4*>(p + i) = o;
    }
    for (int i = g; i < head; i += stride) p[i] = conv(w[i], i);
    for (int i = tail + g; i < L; i += stride) p[i] = conv(w[i], i);
}

struct G711Launch {
    const float* wav;           // [B, L] fp32
    const int32_t* lengths;     // ragged, as in PcmLaunch
    int row_scale;
    uint8_t* out;               // [B, L]
    int B, L;
};

typedef unsigned char pu8x4 __attribute__((ext_vector_type(4)));

// fp32 [B, L] -> G.711 bytes [B, L], shaped like pcm_normalize_kernel: 16-byte loads and 4-byte stores from the first sample of
// the item whose two addresses are 16- / 4-byte aligned, scalar head and tail, the whole item scalar where the two alignments
// disagree.  Samples past the item's own hold the law's code for 0.
template <int LAW>
__global__ void __launch_bounds__(256) g711_kernel(const G711Launch a) {
    const int b = blockIdx.y;
    const int L = a.L;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, L);
    const float* __restrict__ w = a.wav + (size_t)b * L;
    uint8_t* __restrict__ p = a.out + (size_t)b * L;
    auto conv = [&](float v, int i) -> uint8_t { return g711_of<LAW>(i < Lb ? v : 0.f); };
    const unsigned mis_w = (unsigned)((uintptr_t)w >> 2) & 3u, mis_p = (unsigned)(uintptr_t)p & 3u;
    int head = mis_w == mis_p ? (int)((4u - mis_w) & 3u) : L;
    if (head > L) head = L;
    const int nvec = (L - head) >> 2;
    const int tail = head + 4 * nvec;
    const int g = (int)(blockIdx.x * 256 + threadIdx.x), stride = (int)(gridDim.x * 256);
    for (int v = g; v < nvec; v += stride) {
        const int i = head + 4 * v;
        const pf32x4 x = *reinterpret_cast<const pf32x4*>(w + i);
        pu8x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = conv(x[e], i + e);
        *reinterpret_cast<pu8x4*>(p + i) = o;
    }
    for (int i = g; i < head; i += stride) p[i] = conv(w[i], i);
    for (int i = tail + g; i < L; i += stride) p[i] = conv(w[i], i);
}

inline dim3 pcm_grid(int B, int L) {
    long long x = ((long long)L + 1023) / 1024;
    if (x < 1) x = 1;
    if (x > 65535) x = 65535;           // (the kernels stride over the rest)
    return dim3((unsigned)x, (unsigned)B);
}

// a.peak must have been zeroed on `stream`
inline hipError_t launch_pcm_peak(const PcmLaunch& a, hipStream_t stream) {
    if (a.B < 1 || a.B > 65535 || a.L < 1) return hipErrorInvalidValue;
    return ::iris::launch_kernel_named("pcm_peak_kernel", pcm_peak_kernel<0>, pcm_grid(a.B, a.L), dim3(256), 0, stream, a);
}

inline hipError_t launch_pcm_normalize(const PcmLaunch& a, bool normalize, hipStream_t stream) {
    if (a.B < 1 || a.B > 65535 || a.L < 1) return hipErrorInvalidValue;
    if (normalize)
        return ::iris::launch_kernel_named("pcm_normalize_kernel", pcm_normalize_kernel<true>, pcm_grid(a.B, a.L), dim3(256), 0, stream, a);
    return ::iris::launch_kernel_named("pcm_normalize_kernel", pcm_normalize_kernel<false>, pcm_grid(a.B, a.L), dim3(256), 0, stream, a);
}

inline hipError_t launch_g711(const G711Launch& a, int law, hipStream_t stream) {
    if (a.B < 1 || a.B > 65535 || a.L < 1 || (law != OUT_ULAW && law != OUT_ALAW)) return hipErrorInvalidValue;
    if (law == OUT_ULAW)
        return ::iris::launch_kernel_named("g711_kernel", g711_kernel<OUT_ULAW>, pcm_grid(a.B, a.L), dim3(256), 0, stream, a);
    return ::iris::launch_kernel_named("g711_kernel", g711_kernel<OUT_ALAW>, pcm_grid(a.B, a.L), dim3(256), 0, stream, a);
}

}  // namespace pcm
}  // namespace iris
