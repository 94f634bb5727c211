// resample.h -- sample-rate conversion of the waveform on the device: a polyphase Kaiser-windowed sinc resampler behind
// conv_post (iris_resampler_*).  The reference never resamples (it fixes 22 050 Hz and only labels the WAV), so the contract
// is this filter and its exact host restatement (iris.resample.resample_host), bit for bit.
//
//   g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, s = min(1, up / down), fc = rolloff * s,
//   Hw = ceil(zeros / s), taps = 2 * Hw
//   bank[p][j] = fc * sinc(fc * t) * I0(beta * sqrt(1 - (t / Hw)^2)) / I0(beta),  t = (j - Hw + 1) - p / up,  0 where |t| > Hw
//                evaluated in double (design(): host only, I0 by its power series), rounded once to fp32
//   out[n]     = the chain over j = 0 .. taps - 1, ascending, of acc = fmaf(x[i0 - Hw + 1 + j], bank[p][j], acc), acc = 0.0f at
//                the start, i0 = floor(n * down / up), p = (n * down) mod up; n and the x index are utterance-global
//
// A call sees L input samples whose first one has the global index `origin`; it produces the global outputs n with
// origin <= n * down / up < origin + L, i.e. n_lo = ceil(origin * up / down) .. ceil((origin + L) * up / down) - 1, so
// consecutive windows partition the output.  x outside the item's own samples (before `origin`, past the item's length)
// reads as 0 and is never fetched: the bound comes from ragged_rows, not from memory.  (A window of a streamed utterance emits
// another range, from another first output: struct Window below.)
//
// Kernel: grid (tiles, B); a 256-thread block computes kRun consecutive outputs of one item.  All 64-bit position
// arithmetic happens once per block (the base output's i0 and phase); a lane steps from it in 32 bits.  The block stages
// the input span of its run in LDS -- 16-byte loads from the first 16-byte boundary of the item's addresses, scalar and
// bounded at the head, the tail and wherever the span leaves the item -- and each lane walks the fmaf chain of its outputs
// (lane l owns outputs l, l + 256, ...: coalesced stores; a G.711 form stores one byte per lane, 64 bytes per wave store --
// packing four outputs per lane is not built and its worth not measured) with its phase row of the bank read as 16-byte
// loads (rows are padded to a multiple of four floats; the bank, at most 640 KB and typically < 60 KB, stays in L2).
// LDS reads are ds_read_b32 at a lane stride of down / up samples: below one when upsampling (neighbours share or
// broadcast a word), 1.4 - 5.5 when downsampling, i.e. a 2- to 6-way conflict on the 32 banks of that instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "device_info.h"
#include "pcm_out.h"

namespace iris {
namespace resample {

constexpr int kRun = 1024;              // outputs per block (four per lane)
constexpr int kMaxUp = 640, kMaxTaps = 256;
constexpr int kMinRateOut = 4000, kMaxRateOut = 192000;
constexpr int kDefaultZeros = 16;
constexpr double kDefaultBeta = 9.0, kDefaultRolloff = 0.945;
constexpr long long kMaxOrigin = 1ll << 40;     // keeps n * down and origin * up far inside 64 bits

struct Design {
    int up = 0, down = 0, taps = 0, half_width = 0;
    double fc = 0.0, beta = 0.0;
};

inline long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }
inline long long ceil_div_ll(long long a, long long b) { return (a + b - 1) / b; }      // a >= 0, b > 0

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2
inline double bessel_i0(double x) {
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= h / k;
        const double t2 = term * term;
        sum += t2;
        if (t2 < 1e-18 * sum) break;
    }
    return sum;
}

// 0 = ok, 1 = invalid argument, 4 = unsupported (the values of iris_hifigan_status).  zeros / beta / rolloff == 0 take the
// defaults.
inline int plan(int rate_in, int rate_out, int zeros, double beta, double rolloff, Design* d) {
    if (rate_in < 1 || rate_out < 1 || rate_in == rate_out) return 1;
    if (zeros < 0 || !(beta >= 0.0) || !(rolloff >= 0.0) || rolloff > 1.0) return 1;
    if (zeros == 0) zeros = kDefaultZeros;
    if (beta == 0.0) beta = kDefaultBeta;
    if (rolloff == 0.0) rolloff = kDefaultRolloff;
    if (rate_out < kMinRateOut || rate_out > kMaxRateOut) return 4;
    const long long g = gcd_ll(rate_in, rate_out);
    const long long up = rate_out / g, down = rate_in / g;
    if (up > kMaxUp) return 4;
    const double s = up < down ? (double)up / (double)down : 1.0;
    const double hw = ceil((double)zeros / s);
    if (!(hw >= 1.0) || 2.0 * hw > (double)kMaxTaps) return 4;
    d->up = (int)up; d->down = (int)down; d->half_width = (int)hw; d->taps = 2 * (int)hw;
    d->fc = rolloff * s; d->beta = beta;
    return 0;
}

// bank [up][taps], row-major, fp32
inline void fill_bank(const Design& d, float* bank) {
    const double pi = 3.14159265358979323846;
    const double inv_i0 = 1.0 / bessel_i0(d.beta), Hw = (double)d.half_width;
    for (int p = 0; p < d.up; ++p)
        for (int j = 0; j < d.taps; ++j) {
            const double t = (double)(j - d.half_width + 1) - (double)p / (double)d.up;
            double v = 0.0;
            if (fabs(t) <= Hw) {
                const double x = d.fc * t, r = t / Hw;
                const double sinc = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
                const double w2 = 1.0 - r * r;
                v = d.fc * sinc * bessel_i0(d.beta * sqrt(w2 > 0.0 ? w2 : 0.0)) * inv_i0;
            }
            bank[(size_t)p * d.taps + j] = (float)v;
        }
}

// outputs of a window of L samples at `origin`: n_lo and their number
inline void out_range(const Design& d, long long origin, long long L, long long* n_lo, long long* n_count) {
    const long long lo = ceil_div_ll(origin * d.up, d.down);
    *n_lo = lo;
    *n_count = ceil_div_ll((origin + L) * d.up, d.down) - lo;
}

// Windows (iris_resampler_window_plan / _forward_window): the utterance arrives piece by piece and a window holds its samples
// [origin, origin + Lw).  Output n reads x[i0(n) - Hw + 1 .. i0(n) + Hw], i0(n) = floor(n * down / up), and nothing else, so it is
// final once its last tap lies inside the window -- or the utterance has ended, where the whole call reads zeros too.  struct
// Window is the one place that rule is written down: the window emits [n_next, n_hi),
//     n_hi = ceil((origin + Lw) * up / down) if final, else ceil(max(0, origin + Lw - Hw) * up / down),
// provided the first tap of n_next is still held (origin == 0, or i0(n_next) - Hw + 1 >= origin: `ok`), and the next window must
// hold the samples from keep_from = max(0, i0(n_hi) - Hw + 1) on.  The kernel needs nothing new for it: a launch already names
// origin and n_lo separately and bounds every load by the row, so a window is the launch (origin, n_lo = n_next, N = count), and
// iris_resampler_forward is the final window with n_next = ceil(origin * up / down) whose `ok` nobody asks for (samples in front
// of its origin read as 0, as they always did).
struct Window {
    long long n_hi, count, keep_from;
    bool ok;
    Window(const Design& d, long long origin, long long Lw, long long n_next, bool final) {
        const long long end = origin + Lw, Hw = d.half_width;
        const long long settled = final ? end : (end > Hw ? end - Hw : 0);
        n_hi = ceil_div_ll(settled * d.up, d.down);
        count = n_hi > n_next ? n_hi - n_next : 0;
        const long long k = n_hi * d.down / d.up - Hw + 1;
        keep_from = k > 0 ? k : 0;
        ok = origin == 0 || n_next * d.down / d.up - Hw + 1 >= origin;
    }
};

__host__ __device__ inline int row_stride(int taps) { return (taps + 3) & ~3; }     // floats per bank row on the device
// floats of LDS a block needs: the span of a full run from the worst base phase, + 3 of alignment shift, whole 16-byte groups
inline size_t lds_floats(int up, int down, int taps) {
    const long long span = ((long long)(up - 1) + (long long)(kRun - 1) * down) / up + taps;
    return (size_t)((span + 3 + 3) & ~3ll);
}

struct ResampleLaunch {
    const float* wav;           // [B, L] fp32
    const int32_t* lengths;     // ragged: frames of each item [B] (device), or nullptr
    int row_scale;              // samples per frame
    const float* bank;          // [up][row_stride(taps)] fp32, 16-byte aligned
    float* y;                   // [B, N] fp32 (OUT_F32, OUT_F32_PEAK)
    int16_t* pcm;               // [B, N] int16 (OUT_PCM16)
    uint8_t* g711;              // [B, N] bytes (OUT_ULAW, OUT_ALAW: `law` says which)
    int law;
    unsigned* peak;             // [B] bit patterns of the items' max |out| (OUT_F32_PEAK), zeroed on the stream
    int B, L, N;                // N outputs per item, global indices n_lo .. n_lo + N - 1
    int up, down, taps, half_width;
    long long origin, n_lo;
};

typedef float rf32x4 __attribute__((ext_vector_type(4)));
typedef float rf32x2 __attribute__((ext_vector_type(2)));

// Groups of windows (iris_resampler_forward_windows): the rows of one launch are windows of DIFFERENT utterances.  What the launch
// names once for every row -- origin, n_lo, the row's outputs and its readable samples -- resample_kernel<OUT, true> reads per
// row from ResampleItem item[kGroupMax], which travels by value in the kernel argument behind the ResampleLaunch and is indexed
// by blockIdx.y (uniform: scalar loads from the kernarg segment; no descriptor buffer, no copy, capture-safe; 64 items are 1.5 KB
// of the 4 KB a kernel argument may have, hence the cap).  The host fills an item from struct Window and nothing else.  L and N
// stay what they were, the strides of the input and the output rows; grid.x covers the largest count of the group; a block
// behind its row's own count stores the code of sample 0 and returns, and the blocks of the last column go on to the end of the
// row, so every slot of out [B, N] is stored exactly once.  The same body: every index and operation of a row's own outputs is
// what the one-window launch does.
constexpr int kGroupMax = 64;
struct ResampleItem {
    long long origin, n_lo;     // as in ResampleLaunch, of this row
    int count, in_len;          // the row's outputs [n_lo, n_lo + count) and its readable samples [0, in_len)
};
struct ResampleGroupLaunch {
    ResampleLaunch a;           // L = in_stride, N = out_stride and what the rows share; origin and n_lo are the items'
    ResampleItem item[kGroupMax];
};
template <bool GROUP> struct ResampleArg { typedef ResampleLaunch type; };
template <> struct ResampleArg<true> { typedef ResampleGroupLaunch type; };
template <bool GROUP> __device__ __forceinline__ const ResampleLaunch& shared_of(const typename ResampleArg<GROUP>::type& arg) {
    if constexpr (GROUP) return arg.a;
    else                 return arg;
}

template <int OUT, bool GROUP>
__global__ void __launch_bounds__(256) resample_kernel(const typename ResampleArg<GROUP>::type arg) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const ResampleLaunch& a = shared_of<GROUP>(arg);
    const int b = blockIdx.y, tid = threadIdx.x;
    long long origin = a.origin, n_lo = a.n_lo;
    int n_item = a.N, in_len = a.L;                             // the row's own outputs and readable samples
    if constexpr (GROUP) { const ResampleItem it = arg.item[b]; origin = it.origin; n_lo = it.n_lo; n_item = it.count; in_len = it.in_len; }
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, in_len);
    const int run0 = (int)blockIdx.x * kRun;                    // < N < 2^31
    const int up = a.up, down = a.down, taps = a.taps;
    // the one 64-bit step: base output of the block, its integer position and phase; the item's own output count
    const long long nb = n_lo + run0;
    const long long qb = nb * down;
    const long long i0b = qb / up;
    const int pb = (int)(qb - i0b * up);
    const long long own = (origin + Lb) * (long long)up;
    long long cnt = (own + down - 1) / down - n_lo;             // outputs of this item; the rest of its row is 0
    if (cnt > n_item) cnt = n_item;
    int valid = (int)((cnt - run0 < kRun) ? cnt - run0 : kRun);  // outputs of this block that are the item's own
    if (valid < 0) valid = 0;
    int in_block = a.N - run0 < kRun ? a.N - run0 : kRun;        // slots of the row this block stores
    if constexpr (GROUP) { if (blockIdx.x + 1 == gridDim.x) in_block = a.N - run0; }     // the last column: on to the row's end

    const float* __restrict__ w = a.wav + (size_t)b * a.L;
    int shift = 0;
    if (valid > 0) {
        // LDS slot m holds item sample first + m, where first is a multiple of four floats away from a 16-byte boundary of
        // the item's addresses; the span's own first sample (item index a0, possibly negative) sits in slot `shift`.
        const int a0 = (int)(i0b - (long long)a.half_width + 1 - origin);           // >= -taps, <= L
        shift = (int)(((uintptr_t)w >> 2) + (unsigned)a0) & 3;      // (two's complement: right for a negative a0 too)
        const int first = a0 - shift;
        const int span = (int)(((long long)pb + (long long)(valid - 1) * down) / up) + taps + shift;
        const int groups = (span + 3) >> 2;
        for (int v = tid; v < groups; v += 256) {
            const int i = first + 4 * v;
            rf32x4 x;
            if (i >= 0 && i + 3 < Lb) {
                x = *reinterpret_cast<const rf32x4*>(w + i);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = (i + e >= 0 && i + e < Lb) ? w[i + e] : 0.f;
            }
            *reinterpret_cast<rf32x4*>(xs + 4 * v) = x;
        }
    }
    __syncthreads();

    unsigned bits = 0;
    const int stride = row_stride(taps);
    const size_t row = (size_t)b * a.N + run0;
    for (int r = tid; r < in_block; r += 256) {
        float acc = 0.f;
        if (r < valid) {
            const unsigned t = (unsigned)pb + (unsigned)r * (unsigned)down;      // < 640 + 1024 * down
            const unsigned di = t / (unsigned)up;
            const unsigned p = t - di * (unsigned)up;
            const float* __restrict__ x = xs + shift + di;
            const float* __restrict__ c = a.bank + (size_t)p * stride;
            int j = 0;
            for (; j + 4 <= taps; j += 4) {
                const rf32x4 cv = *reinterpret_cast<const rf32x4*>(c + j);
                acc = __builtin_fmaf(x[j + 0], cv[0], acc);
                acc = __builtin_fmaf(x[j + 1], cv[1], acc);
                acc = __builtin_fmaf(x[j + 2], cv[2], acc);
                acc = __builtin_fmaf(x[j + 3], cv[3], acc);
            }
            if (j < taps) {                                                      // taps = 2 * Hw: two left over, or none
                const rf32x2 cv = *reinterpret_cast<const rf32x2*>(c + j);
                acc = __builtin_fmaf(x[j + 0], cv[0], acc);
                acc = __builtin_fmaf(x[j + 1], cv[1], acc);
            }
            if constexpr (OUT == pcm::OUT_F32_PEAK) {
                const unsigned v = pcm::abs_bits(acc);
                bits = v > bits ? v : bits;
            }
        }
        pcm::store_sample<OUT>(a, row + r, acc);
    }
    if constexpr (OUT == pcm::OUT_F32_PEAK) pcm::block_peak_max(bits, a.peak + b);
}

// a.peak (OUT_F32_PEAK) must have been zeroed on `stream`
inline hipError_t launch_resample(const ResampleLaunch& a, hipStream_t stream) {
    if (a.B < 1 || a.B > 65535 || a.L < 1 || a.N < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((long long)a.N + kRun - 1) / kRun), (unsigned)a.B), block(256);
    const size_t lds = lds_floats(a.up, a.down, a.taps) * sizeof(float);
    if (a.peak) return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_F32_PEAK, false>, grid, block, lds, stream, a);
    if (a.pcm)  return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_PCM16, false>, grid, block, lds, stream, a);
    if (a.g711 && a.law == pcm::OUT_ULAW)
        return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_ULAW, false>, grid, block, lds, stream, a);
    if (a.g711 && a.law == pcm::OUT_ALAW)
        return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_ALAW, false>, grid, block, lds, stream, a);
    if (a.g711 || !a.y) return hipErrorInvalidValue;
    return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_F32, false>, grid, block, lds, stream, a);
}

// A group: a.B <= kGroupMax rows, a.L and a.N the strides of the input and the output rows, items[b] what row b names itself.
// One output form, as above, and no peak.  The largest count of the group must be >= 1.
inline hipError_t launch_resample_group(const ResampleLaunch& a, const ResampleItem* items, hipStream_t stream) {
    if (a.B < 1 || a.B > kGroupMax || a.L < 1 || a.N < 1 || a.peak) return hipErrorInvalidValue;
    ResampleGroupLaunch g; memset(&g, 0, sizeof(g));
    g.a = a;
    int most = 0;
    for (int b = 0; b < a.B; ++b) { g.item[b] = items[b]; if (items[b].count > most) most = items[b].count; }
    if (most < 1 || most > a.N) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((long long)most + kRun - 1) / kRun), (unsigned)a.B), block(256);
    const size_t lds = lds_floats(a.up, a.down, a.taps) * sizeof(float);
    if (a.pcm)  return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_PCM16, true>, grid, block, lds, stream, g);
    if (a.g711 && a.law == pcm::OUT_ULAW)
        return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_ULAW, true>, grid, block, lds, stream, g);
    if (a.g711 && a.law == pcm::OUT_ALAW)
        return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_ALAW, true>, grid, block, lds, stream, g);
    if (a.g711 || !a.y) return hipErrorInvalidValue;
    return ::iris::launch_kernel_named("resample_kernel", resample_kernel<pcm::OUT_F32, true>, grid, block, lds, stream, g);
}

}  // namespace resample
}  // namespace iris
