// assemble.h -- silence trim and sentence join on the device (iris_assemble_*): the last stage between a ragged batch of
// waveforms and ONE finished utterance.  Per item it is the decision of librosa.effects.trim(y, top_db=, ref=np.max,
// frame_length=F, hop_length=H) (librosa 0.11); librosa cannot be imported here, so the contract is the rules below, held by
// a float64 and an fp32 numpy restatement (tests/assemble_restatement.py).  Item b owns L_b = min(L, lengths[b] * row_scale)
// samples (ragged_rows); F is even and H divides F / 2, so a frame is R = F / H whole H-blocks.
//
//   frames     T_b = L_b / H + 1.  Frame t covers samples [t H - F / 2, t H + F / 2) of the item, i.e. the H-blocks
//              j = t - R / 2 .. t + R / 2 - 1, block j being samples [j H, (j + 1) H); a sample outside [0, L_b) reads as 0 and
//              is never fetched.  mse[t] = (sum of y^2 over the frame) / F.
//   sum order  Block j, S[j]: 256 accumulators, acc[m] = 0.0f, take the squares of the block's samples i = m, m + 256, ...
//              ascending, acc[m] = acc[m] + y[i] * y[i] (a product rounded to fp32, then a sum: nothing is contracted);
//              v[l] = ((acc[4 l] + acc[4 l + 1]) + acc[4 l + 2]) + acc[4 l + 3] for l = 0 .. 63; then for o = 32, 16, 8, 4, 2,
//              1: v[l] = v[l] + v[l + o] for l < o; S[j] = v[0].  A block that holds no sample of the item is 0.0f.
//              Frame t: s = S[t - R / 2]; s = s + S[j] for the other R - 1 blocks ascending; mse[t] = s / (float)F (a
//              correctly rounded fp32 division).  The order depends on the item's own sample indices alone, not on
//              addresses, B or the item's neighbours: item b's bounds are those of its batch-of-one call.
//   reference  ref_b = max_t mse[t]; with cfg.ref > 0 it is the fp32 product ref * ref instead.
//   decision   frame t is non-silent iff fmaxf(mse[t], amin) > fmaxf(ref_b, amin) * k, amin = 1e-10f, k = (float)pow(10.0,
//              -(double)top_db / 10.0): amplitude_to_db(rms, ref, top_db=None) > -top_db without the logarithms; the
//              product is fp32 and the comparison strict.  With ref = max an item of digital silence keeps EVERY frame,
//              because amin > amin * k -- librosa does the same.  Samples are taken to be finite.
//   bounds     t0 / t1 the first / last non-silent frame: start = t0 H, end = min(L_b, (t1 + 1) H); none: start = end = 0.
//              start' = max(0, start - pad), end' = min(L_b, end + pad), len_b = end' - start'.  L_b == 0: empty.
//   join       w_b = len_b + (len_b > 0 ? pause : 0); off_b = sum of w_a over a < b -- S_b + pause P_b with P_b the number
//              of non-empty items in front; total = off_B - (off_B > 0 ? pause : 0).  offsets_out = off_0 .. off_(B-1), total.
//              An empty item contributes neither samples nor a pause (its off_b is the next non-empty item's).
//   samples    out[off_b + n] = (y[b, start' + n] * a) * b2 for n < len_b, a = n < fade ? ramp[n] : 1.0f,
//              b2 = len_b - 1 - n < fade ? ramp[len_b - 1 - n] : 1.0f; ramp[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade) in double,
//              rounded once to fp32 at create.  Two fp32 products in that order; overlapping ramps simply multiply.  The
//              pauses and everything in [total, cap) are stored as 0.0f.  Every element of out[0, cap) is stored exactly
//              once, by one thread, without atomics: two runs give the same bits.
//   rows form  (iris_assemble_trim_ragged) the same kernel with item b stored in its own row of out [B, L] from column 0,
//              0.0f behind len_b, and counts[b] = len_b in place of the offsets; no pause.
//
// Three launches.  energy: grid (runs of kRunFrames frames, B); a wave forms one block sum at a time -- lane l owns
// acc[4 l .. 4 l + 3], a 16-byte load where the block's first sample lies on 16 bytes, four bounded 4-byte loads otherwise --
// the block keeps its run's kRunFrames + R - 1 block sums in LDS and stores mse[b][t] for t < T_b (the rest of the row is not
// touched).  bounds: one block per item, max / min reductions, stores (start', end').  gather: blocks of kGatherRun output
// positions; every block scans the B items' w_b into off[0 .. B] in LDS (at most 4097 words), finds the item of each group of
// four positions by binary search and stores 16 bytes where `out` lies on 16 bytes; block 0 also stores the integer outputs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "device_info.h"

namespace iris {
namespace assemble {

constexpr int kMaxFrame = 8192, kMaxFade = 65536, kMaxBatch = 4096;
constexpr int kRunFrames = 32;          // frames of one item an energy block owns
constexpr int kGatherRun = 4096;        // output positions of a gather block (four groups of four per lane)
constexpr float kAmin = 1e-10f;

typedef float af32x4 __attribute__((ext_vector_type(4)));

// ramp [fade], fp32
inline void fill_ramp(int fade, float* ramp) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < fade; ++j) ramp[j] = (float)(0.5 - 0.5 * cos(pi * ((double)j + 0.5) / (double)fade));
}

struct EnergyLaunch {
    const float* wav;           // [B, L] fp32
    const int32_t* lengths;     // ragged: frames of each item [B] (device), or nullptr
    int row_scale;
    float* mse;                 // [B, T] fp32
    int L, T, F, H;
};

// S[j] of the item whose samples are y[0 .. Lb): the same value in every lane.
__device__ __forceinline__ float block_sum(const float* __restrict__ y, long long j, int H, int Lb, int lane) {
#pragma clang fp contract(off)
    const long long base = j * H;
    if (j < 0 || base >= Lb) return 0.f;
    const int n = Lb - base < H ? (int)(Lb - base) : H;
    const float* __restrict__ x = y + base;
    const bool aligned = ((uintptr_t)x & 15) == 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 4 * lane; i < n; i += 256) {
        af32x4 q;
        if (aligned && i + 3 < n) {
            q = *reinterpret_cast<const af32x4*>(x + i);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = i + e < n ? x[i + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sq = q[e] * q[e];
            acc[e] = acc[e] + sq;
        }
    }
    float v = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_down(v, o, 64);        // lane l < o: v[l] + v[l + o]
    return __shfl(v, 0, 64);
}

__global__ void __launch_bounds__(256) energy_kernel(const EnergyLaunch a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float bs[];      // the run's block sums, kRunFrames + R - 1
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const int Tb = Lb / a.H + 1, R = a.F / a.H;
    const long long t0 = (long long)blockIdx.x * kRunFrames;
    if (t0 >= Tb) return;
    const int nt = Tb - t0 < kRunFrames ? (int)(Tb - t0) : kRunFrames;
    const float* __restrict__ y = a.wav + (size_t)b * a.L;
    const long long j0 = t0 - R / 2;
    for (int jj = wave; jj < nt + R - 1; jj += 4) {
        const float s = block_sum(y, j0 + jj, a.H, Lb, lane);
        if (lane == 0) bs[jj] = s;
    }
    __syncthreads();
    const float den = (float)a.F;
    for (int t = tid; t < nt; t += 256) {
        float s = bs[t];
        for (int r = 1; r < R; ++r) s = s + bs[t + r];
        a.mse[(size_t)b * a.T + t0 + t] = s / den;
    }
}

inline hipError_t launch_energy(const EnergyLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)((a.T + kRunFrames - 1) / kRunFrames), (unsigned)B), block(256);
    const size_t lds = (size_t)(kRunFrames + a.F / a.H - 1) * sizeof(float);
    return ::iris::launch_kernel(energy_kernel, grid, block, lds, stream, a);
}

struct BoundsLaunch {
    const float* mse;           // [B, T]
    const int32_t* lengths;
    int row_scale;
    int32_t* spans;             // [B][2]: start', end'
    int L, T, H, pad;
    float ref_sq;               // 0: the item's own maximum
    float k;
};

// max over the block of a value every thread brings; every thread gets it.  red: 4 words of LDS, free again on return.
__device__ __forceinline__ int block_max_int(int v, int* red) {
    for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = red[0];
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    __syncthreads();
    return m;
}

__global__ void __launch_bounds__(256) bounds_kernel(const BoundsLaunch a) {
#pragma clang fp contract(off)
    __shared__ int red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const int Tb = Lb / a.H + 1;
    const float* __restrict__ m = a.mse + (size_t)b * a.T;
    float ref = a.ref_sq;
    if (!(ref > 0.f)) {
        float mx = 0.f;                                             // mse >= 0: its bit patterns order as integers
        for (int t = tid; t < Tb; t += 256) mx = fmaxf(mx, m[t]);
        ref = __int_as_float(block_max_int(__float_as_int(mx), red));
    }
    const float thr = fmaxf(ref, kAmin) * a.k;
    int first = -0x7fffffff, last = -1;                             // `first` holds -t0, so that one max reduction serves both
    for (int t = tid; t < Tb; t += 256)
        if (fmaxf(m[t], kAmin) > thr) {
            if (-t > first) first = -t;
            last = t;                                               // t ascends within a thread
        }
    first = -block_max_int(first, red);
    last = block_max_int(last, red);
    if (tid == 0) {
        long long start = 0, end = 0;
        if (last >= 0) {
            start = (long long)first * a.H;
            end = ((long long)last + 1) * a.H;
            if (end > Lb) end = Lb;
        }
        start -= a.pad; end += a.pad;
        a.spans[2 * b] = (int32_t)(start < 0 ? 0 : start);
        a.spans[2 * b + 1] = (int32_t)(end > Lb ? Lb : end);
    }
}

inline hipError_t launch_bounds(const BoundsLaunch& a, int B, hipStream_t stream) {
    return ::iris::launch_kernel(bounds_kernel, dim3((unsigned)B), dim3(256), 0, stream, a);
}

struct GatherLaunch {
    const float* wav;           // [B, L]
    const int32_t* spans;       // [B][2], the bounds kernel's
    const float* ramp;          // [fade]
    float* out;                 // rows == 0: [cap], the join; rows != 0: [B, L] (cap = B L), item b in its own row
    int32_t* spans_out;         // [B][2] or nullptr
    int32_t* offsets_out;       // rows == 0: [B + 1], off_b and the total; rows != 0: [B], len_b
    int B, L, cap, fade, pause, rows;
};

__global__ void __launch_bounds__(256) gather_kernel(const GatherLaunch a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned off[];  // off[0 .. B]: sums of w_a (below 2^32: cap + pause)
    unsigned* const wave_sum = off + a.B + 1;                       // 4 more words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = a.B;
    const unsigned pause = (unsigned)a.pause;
    unsigned total = 0;
    if (!a.rows) {
        // thread tid owns items [lo, hi): their w summed, an exclusive scan of the 256 sums, then their off written in order
        const int per = (B + 255) / 256;
        const int lo = tid * per < B ? tid * per : B, hi = lo + per < B ? lo + per : B;
        unsigned mine = 0;
        for (int i = lo; i < hi; ++i) {
            const unsigned len = (unsigned)(a.spans[2 * i + 1] - a.spans[2 * i]);
            mine += len + (len ? pause : 0u);
        }
        unsigned incl = mine;
        for (int o = 1; o < 64; o <<= 1) { const unsigned u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned run = incl - mine;
        for (int w = 0; w < wave; ++w) run += wave_sum[w];
        for (int i = lo; i < hi; ++i) {
            off[i] = run;
            const unsigned len = (unsigned)(a.spans[2 * i + 1] - a.spans[2 * i]);
            run += len + (len ? pause : 0u);
        }
        if (tid == 255) off[B] = run;
        __syncthreads();
        total = off[B] - (off[B] ? pause : 0u);
    }
    if (blockIdx.x == 0) {
        for (int i = tid; i < B; i += 256) {
            const int s = a.spans[2 * i], e = a.spans[2 * i + 1];
            if (a.spans_out) { a.spans_out[2 * i] = s; a.spans_out[2 * i + 1] = e; }
            a.offsets_out[i] = a.rows ? e - s : (int32_t)off[i];
        }
        if (!a.rows && tid == 0) a.offsets_out[B] = (int32_t)total;
    }

    // the sample at output position p of item b, which starts at position at: 0.0f in a pause, a row's rest or the tail
    auto sample = [&](int b, unsigned at, unsigned p) -> float {
        const int s = a.spans[2 * b], len = a.spans[2 * b + 1] - s;
        const unsigned n = p - at;
        if (n >= (unsigned)len) return 0.f;
        const int back = len - 1 - (int)n;
        const float up = (int)n < a.fade ? a.ramp[n] : 1.f, down = back < a.fade ? a.ramp[back] : 1.f;
        const float v = a.wav[(size_t)b * a.L + s + n] * up;
        return v * down;
    };
    // the last b in [0, B) with off[b] <= p (an empty item shares its off with the next one: the search lands behind it)
    auto item_of = [&](unsigned p) -> int {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= p) lo = mid; else hi = mid;
        }
        return lo;
    };

    const bool vec = ((uintptr_t)a.out & 15) == 0;
    const unsigned cap = (unsigned)a.cap, p_end = blockIdx.x * (unsigned)kGatherRun + kGatherRun;
    for (unsigned p = blockIdx.x * (unsigned)kGatherRun + 4u * tid; p < p_end && p < cap; p += 1024) {
        const unsigned cnt = cap - p < 4u ? cap - p : 4u;
        af32x4 q = {0.f, 0.f, 0.f, 0.f};
        // the item of p, where its positions start and where the next item's do; a group inside one item searches once
        const int b = a.rows ? (int)(p / (unsigned)a.L) : item_of(p);
        const unsigned at = a.rows ? (unsigned)b * (unsigned)a.L : off[b];
        const unsigned next = a.rows ? at + (unsigned)a.L : (b == B - 1 ? 0xffffffffu : off[b + 1]);
        if (p + 3 < next) {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e) if (e < cnt) q[e] = sample(b, at, p + e);
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e)
                if (e < cnt) {
                    const int be = a.rows ? (int)((p + e) / (unsigned)a.L) : item_of(p + e);
                    q[e] = sample(be, a.rows ? (unsigned)be * (unsigned)a.L : off[be], p + e);
                }
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<af32x4*>(a.out + p) = q;
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e) if (e < cnt) a.out[p + e] = q[e];
        }
    }
}

inline hipError_t launch_gather(const GatherLaunch& a, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)a.cap + kGatherRun - 1) / kGatherRun)), block(256);
    const size_t lds = (size_t)(a.B + 1 + 4) * sizeof(unsigned);
    return ::iris::launch_kernel(gather_kernel, grid, block, lds, stream, a);
}

}  // namespace assemble
}  // namespace iris
