// loudness.h -- ITU-R BS.1770-4 integrated loudness per item of a ragged batch, and the gain that brings each item to a target,
// on the device (iris_loudness_*).  pyloudnorm cannot be imported here, so the contract is the rules below, held by two float64
// numpy restatements (tests/loudness_restatement.py): the plain BS.1770 loop, and the same in this file's own structure.  Item b
// of wav [B, L] fp32 owns L_b = min(L, lengths[b] * row_scale) samples (ragged_rows); mono.  Everything between the fp32 sample
// and the fp32 product that stores it is fp64, and NOTHING is contracted: a product is rounded, then a sum.
//
//   K-weighting  two biquads, derived on the host in double at create (fill_design) with K = tan(pi f0 / fs), as libebur128 and
//              pyloudnorm derive them: a high shelf (f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Q = 0.7071752369554196,
//              Vb = Vh^0.4996667741545416) and a high pass (f0 = 38.13547087602444 Hz, Q = 0.5003270373238773, b = (1, -2, 1)).  At
//              48000 Hz they are the standard's table.
//   recurrence   transposed direct form II, state (s1, s2, t1, t2) = 0 at sample 0 of every item.  Per sample x = (double)y[n],
//              shelf (b0, b1, b2, a1, a2), high pass (c0, c1, c2, d1, d2):
//                  u = b0 x + s1;   s1 = (b1 x - a1 u) + s2;   s2 = b2 x - a2 u;
//                  v = c0 u + t1;   t1 = (c1 u - d1 v) + t2;   t2 = c2 u - d2 v;            v is the filtered sample.
//              Samples are taken to be finite.
//   segments     segment k of an item is its samples [k G, min(L_b, (k + 1) G)), G = kSeg = 64; a chunk is kChunkSegs = 128
//              segments (8192 samples).  With x = 0 a step is s' = A s, so over a whole segment s_end = P_0 s_start + e with
//              P_k = A^(G 2^k) (fill_design: A^G by G - 1 products A * X, then squarings; mat_mul's order) and e the segment's end
//              state from s_start = 0.  A segment that is not whole (or holds no sample) has e = 0: nobody reads past it.
//   matvec       (P v)[r] = ((P[r][0] v[0] + P[r][1] v[1]) + P[r][2] v[2]) + P[r][3] v[3].
//   scan         inside a chunk, over its 128 e[i], for k = 0 .. 6, o = 2^k, all i at once from the values of step k - 1:
//              e[i] = i >= o ? P_k e[i - o] + e[i] : e[i]  (matvec, then one sum per row).  e[i] is then the state behind segment
//              i of a chunk entered with state 0.
//   carry        C_0 = 0, C_(c+1) = P_7 C_c + e_c[127]: the state in front of chunk c + 1.  Serial; the block of chunk c walks it
//              from 0, one dependent load per chunk in front of it (an item of 3 s at 22.05 kHz has 9 chunks).
//   start        w[0] = C_c; for k = 0 .. 6, o = 2^k: w[i] = P_k w[i - o] for o <= i < 2 o.  Segment i of the chunk starts from
//              w[0] for i = 0 and from w[i] + e[i - 1] otherwise, and is run again through the recurrence from there.
//   squares      step = sample_rate / 10; hop h is samples [h step, (h + 1) step).  G < step (sample_rate >= 8000), so a segment
//              lies in at most two hops: with m = (k G / step + 1) step - k G the samples i < m of segment k belong to hop
//              h0 = k G / step and the others to h0 + 1.  p0 = 0, p1 = 0; for i ascending, q = v v, (i < m ? p0 : p1) += q.
//              S[h] = 0; for the segments k that touch hop h, ascending: S[h] = S[h] + (k G / step == h ? p0[k] : p1[k]).
//   blocks       J_b = L_b >= 4 step ? (L_b - 4 step) / step + 1 : 0; z_j = (((S[j] + S[j+1]) + S[j+2]) + S[j+3]) / (double)(4 step).
//   block sums   (fixed_sum) 256 accumulators, acc[t] = 0, take the gated z_j of j = t, t + 256, ... ascending, acc[t] = acc[t] +
//              z_j; then for o = 128, 64, .., 1: acc[t] = acc[t] + acc[t + o] for t < o; the sum is acc[0].
//   gates        strict, no logarithm, thresholds from the host in double.  absolute: z_j > abs_thr = 10^((-70 + 0.691) / 10);
//              relative: z_j > 0.1 * (sum over the absolutely gated / their count).  ms_b = sum over the blocks passing both /
//              their count, or 0 where there is none.  Integrated loudness is -0.691 + 10 log10(ms_b), formed by the caller.
//   gain         ms_b == 0: g_b = 1.  Otherwise g_b = sqrt(target_ms / ms_b) (a correctly rounded division and square root),
//              target_ms = 10^((target_lufs + 0.691) / 10); then g_b = min(g_b, 10^(max_gain_db / 20)); then, with peak_ceiling
//              > 0, g_b = min(g_b, (double)peak_ceiling / (double)max|y_b|), the maximum being exact.
//   samples      out[b, n] = y[b, n] * (float)g_b for n < L_b, one fp32 product, and 0.0f behind L_b.  Every element of out [B, L]
//              is stored exactly once, by one thread, without atomics: two runs give the same bits.  stats_out [B][2] = (ms_b, g_b).
//   Every order above depends on the item's own sample indices alone, not on B, addresses or the item's neighbours.
//
// Four launches (three to measure).  local: grid (chunks, B), 128 threads; the chunk's samples are staged in LDS by 16-byte loads
// (4-byte ones where the row does not lie on 16 bytes) in rows of G + 1 words, so that lane i walking segment i meets no bank
// twice; every thread runs its segment from 0, the scan runs in LDS and e [B][segs][4] is stored.  rerun: the same staging, thread
// 0 walks the carry, the start states are formed in LDS, every thread reruns its segment and stores (p0, p1) and max|y|.  gate:
// one block of 256 per item: S, the two gates, the peak, ms_b and g_b.  apply: groups of four over out as ONE row of B L.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "device_info.h"

namespace iris {
namespace loudness {

constexpr int kSeg = 64, kChunkSegs = 128, kScanSteps = 7, kRow = kSeg + 1;
constexpr int kChunk = kSeg * kChunkSegs;           // samples of a chunk
constexpr int kApplyRun = 4096;                     // output positions of an apply block
// the design table [kDesign] of doubles: coefficients, thresholds, then P_0 .. P_7 row-major
constexpr int kShelf = 0, kHighPass = 5, kAbsThr = 10, kTargetMs = 11, kMaxGain = 12, kCeiling = 13, kMats = 16, kDesign = kMats + 16 * (kScanSteps + 1);

typedef float lf32x4 __attribute__((ext_vector_type(4)));

inline void mat_mul(const double* X, const double* Y, double* out) {           // out = X Y, 4 x 4 row-major, terms ascending
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = X[4 * i] * Y[j];
            for (int m = 1; m < 4; ++m) { const double p = X[4 * i + m] * Y[4 * m + j]; s = s + p; }
            r[4 * i + j] = s;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

inline void fill_design(int sample_rate, double target_lufs, double max_gain_db, double peak_ceiling, double* d) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < kDesign; ++i) d[i] = 0.0;
    {
        const double K = tan(pi * 1681.974450955533 / (double)sample_rate), Q = 0.7071752369554196;
        const double Vh = pow(10.0, 3.999843853973347 / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        d[kShelf + 0] = (Vh + Vb * K / Q + K * K) / a0;
        d[kShelf + 1] = 2.0 * (K * K - Vh) / a0;
        d[kShelf + 2] = (Vh - Vb * K / Q + K * K) / a0;
        d[kShelf + 3] = 2.0 * (K * K - 1.0) / a0;
        d[kShelf + 4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double K = tan(pi * 38.13547087602444 / (double)sample_rate), Q = 0.5003270373238773;
        const double a0 = 1.0 + K / Q + K * K;
        d[kHighPass + 0] = 1.0; d[kHighPass + 1] = -2.0; d[kHighPass + 2] = 1.0;
        d[kHighPass + 3] = 2.0 * (K * K - 1.0) / a0;
        d[kHighPass + 4] = (1.0 - K / Q + K * K) / a0;
    }
    d[kAbsThr] = pow(10.0, (-70.0 + 0.691) / 10.0);
    d[kTargetMs] = pow(10.0, (target_lufs + 0.691) / 10.0);
    d[kMaxGain] = pow(10.0, max_gain_db / 20.0);
    d[kCeiling] = peak_ceiling;
    const double a1 = d[kShelf + 3], a2 = d[kShelf + 4], c0 = d[kHighPass], c1 = d[kHighPass + 1], c2 = d[kHighPass + 2],
                 d1 = d[kHighPass + 3], d2 = d[kHighPass + 4];
    const double A[16] = {-a1, 1.0, 0.0, 0.0,   -a2, 0.0, 0.0, 0.0,   c1 - d1 * c0, 0.0, -d1, 1.0,   c2 - d2 * c0, 0.0, -d2, 0.0};
    double* P = d + kMats;
    for (int i = 0; i < 16; ++i) P[i] = A[i];
    for (int n = 1; n < kSeg; ++n) mat_mul(A, P, P);
    for (int k = 1; k <= kScanSteps; ++k) mat_mul(P + 16 * (k - 1), P + 16 * (k - 1), P + 16 * k);
}

struct State { double s1, s2, t1, t2; };

struct Coef { double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2; };

__device__ __forceinline__ Coef load_coef(const double* __restrict__ d) {
    return Coef{d[kShelf], d[kShelf + 1], d[kShelf + 2], d[kShelf + 3], d[kShelf + 4],
                d[kHighPass], d[kHighPass + 1], d[kHighPass + 2], d[kHighPass + 3], d[kHighPass + 4]};
}

// one sample through the cascade; returns v
__device__ __forceinline__ double step_sample(const Coef& c, State& s, double x) {
#pragma clang fp contract(off)
    const double u = c.b0 * x + s.s1;
    s.s1 = (c.b1 * x - c.a1 * u) + s.s2;
    s.s2 = c.b2 * x - c.a2 * u;
    const double v = c.c0 * u + s.t1;
    s.t1 = (c.c1 * u - c.d1 * v) + s.t2;
    s.t2 = c.c2 * u - c.d2 * v;
    return v;
}

__device__ __forceinline__ void matvec(const double* __restrict__ P, const double* v, double* out) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double s = P[4 * r] * v[0];
#pragma unroll
        for (int m = 1; m < 4; ++m) { const double p = P[4 * r + m] * v[m]; s = s + p; }
        out[r] = s;
    }
}

struct SegLaunch {
    const float* wav;           // [B, L] fp32
    const int32_t* lengths;     // ragged: rows of each item [B] (device), or nullptr
    int row_scale;
    const double* design;       // [kDesign]
    double* ends;               // [B][segs][4]: e, scanned inside its chunk
    double* parts;              // [B][segs][2]: p0, p1 (rerun only)
    float* seg_peak;            // [B][segs]: max|y| of the segment (rerun only)
    int L, segs, step;          // segs: kChunkSegs * chunks of L
};

// The chunk's samples into LDS rows of kRow words, 0.0f behind Lb (nothing behind Lb is fetched).
__device__ __forceinline__ void stage_chunk(const float* __restrict__ y, long long base, int Lb, float* rows, int tid) {
    const long long left = (long long)Lb - base;
    const int n = left < kChunk ? (int)left : kChunk;
    const bool aligned = ((uintptr_t)(y + base) & 15) == 0;
    for (int q = 4 * tid; q < kChunk; q += 4 * kChunkSegs) {
        lf32x4 x;
        if (aligned && q + 3 < n) {
            x = *reinterpret_cast<const lf32x4*>(y + base + q);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = q + e < n ? y[base + q + e] : 0.f;
        }
        float* dst = rows + (q / kSeg) * kRow + q % kSeg;
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = x[e];
    }
}

__global__ void __launch_bounds__(kChunkSegs) local_kernel(const SegLaunch a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];     // the staged rows; then e, twice
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const long long base = (long long)blockIdx.x * kChunk;
    if (base >= Lb) return;
    stage_chunk(a.wav + (size_t)b * a.L, base, Lb, lds, tid);
    __syncthreads();
    const Coef c = load_coef(a.design);
    State s = {0.0, 0.0, 0.0, 0.0};
    const bool whole = base + (long long)(tid + 1) * kSeg <= Lb;
    if (whole) {
        const float* __restrict__ x = lds + tid * kRow;
        for (int i = 0; i < kSeg; ++i) (void)step_sample(c, s, (double)x[i]);
    } else {
        s = State{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();                                                // the rows are read; the scan takes their place
    double* e = reinterpret_cast<double*>(lds);                     // [2][kChunkSegs][4]
    double cur[4] = {s.s1, s.s2, s.t1, s.t2};
#pragma unroll
    for (int r = 0; r < 4; ++r) e[4 * tid + r] = cur[r];
    __syncthreads();
    int from = 0;
    for (int k = 0; k < kScanSteps; ++k) {
        const int o = 1 << k;
        double* dst = e + (from ^ 1) * 4 * kChunkSegs;
        const double* src = e + from * 4 * kChunkSegs;
        if (tid >= o) {
            double pv[4];
            matvec(a.design + kMats + 16 * k, src + 4 * (tid - o), pv);
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = pv[r] + cur[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[4 * tid + r] = cur[r];
        __syncthreads();
        from ^= 1;
    }
    double* out = a.ends + ((size_t)b * a.segs + (size_t)blockIdx.x * kChunkSegs + tid) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = cur[r];
}

__global__ void __launch_bounds__(kChunkSegs) rerun_kernel(const SegLaunch a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];     // the staged rows, then w [kChunkSegs][4] doubles
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const long long base = (long long)blockIdx.x * kChunk;
    if (base >= Lb) return;
    stage_chunk(a.wav + (size_t)b * a.L, base, Lb, lds, tid);
    static_assert(kChunkSegs * kRow % 2 == 0, "w starts on 8 bytes");
    double* w = reinterpret_cast<double*>(lds + kChunkSegs * kRow);
    const double* __restrict__ ends = a.ends + (size_t)b * a.segs * 4;
    if (tid == 0) {
        double C[4] = {0.0, 0.0, 0.0, 0.0};
        for (int ch = 0; ch < (int)blockIdx.x; ++ch) {
            const double* E = ends + ((size_t)ch * kChunkSegs + kChunkSegs - 1) * 4;
            double pv[4];
            matvec(a.design + kMats + 16 * kScanSteps, C, pv);
#pragma unroll
            for (int r = 0; r < 4; ++r) C[r] = pv[r] + E[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = C[r];
    }
    __syncthreads();
    for (int k = 0; k < kScanSteps; ++k) {
        const int o = 1 << k;
        if (tid >= o && tid < 2 * o) {
            double pv[4];
            matvec(a.design + kMats + 16 * k, w + 4 * (tid - o), pv);
#pragma unroll
            for (int r = 0; r < 4; ++r) w[4 * tid + r] = pv[r];
        }
        __syncthreads();
    }
    const long long first = base + (long long)tid * kSeg;           // the segment's first sample
    const size_t seg = (size_t)b * a.segs + (size_t)blockIdx.x * kChunkSegs + tid;
    if (first >= Lb) return;                                        // no sample: nothing of this segment is read later
    State s = {w[4 * tid], w[4 * tid + 1], w[4 * tid + 2], w[4 * tid + 3]};
    if (tid > 0) {
        const double* E = ends + ((size_t)blockIdx.x * kChunkSegs + tid - 1) * 4;
        s.s1 = s.s1 + E[0]; s.s2 = s.s2 + E[1]; s.t1 = s.t1 + E[2]; s.t2 = s.t2 + E[3];
    }
    const Coef c = load_coef(a.design);
    const int cnt = Lb - first < kSeg ? (int)(Lb - first) : kSeg;
    const long long m = (first / a.step + 1) * a.step - first;      // samples of the segment in its first hop (may exceed cnt)
    const float* __restrict__ x = lds + tid * kRow;
    double p0 = 0.0, p1 = 0.0;
    float peak = 0.f;
    for (int i = 0; i < cnt; ++i) {
        const float xi = x[i];
        peak = fmaxf(peak, fabsf(xi));
        const double v = step_sample(c, s, (double)xi);
        const double q = v * v;
        if (i < m) p0 = p0 + q; else p1 = p1 + q;
    }
    a.parts[2 * seg] = p0;
    a.parts[2 * seg + 1] = p1;
    a.seg_peak[seg] = peak;
}

inline size_t seg_lds_bytes() { return (size_t)kChunkSegs * kRow * sizeof(float) + (size_t)kChunkSegs * 4 * sizeof(double); }

inline hipError_t launch_local(const SegLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)(a.segs / kChunkSegs), (unsigned)B), block(kChunkSegs);
    return ::iris::launch_kernel(local_kernel, grid, block, seg_lds_bytes(), stream, a);
}

inline hipError_t launch_rerun(const SegLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)(a.segs / kChunkSegs), (unsigned)B), block(kChunkSegs);
    return ::iris::launch_kernel(rerun_kernel, grid, block, seg_lds_bytes(), stream, a);
}

struct GateLaunch {
    const int32_t* lengths;
    int row_scale;
    const double* design;
    const double* parts;        // [B][segs][2]
    const float* seg_peak;      // [B][segs]
    double* hops;               // [B][hop_cap]: S
    double* stats;              // [B][2]: ms_b, g_b
    int L, segs, step, hop_cap;
};

// The sum of the values every thread brings, in the header's order; every thread gets it.  red: 256 doubles of LDS.
__device__ __forceinline__ double fixed_sum(double v, double* red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int block_sum_int(int v, int* red) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(256) gate_kernel(const GateLaunch a) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    __shared__ int redi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const long long step = a.step;
    const int nh = (int)(Lb / step);                                // whole hops
    const int J = nh >= 4 ? nh - 3 : 0;
    const double* __restrict__ parts = a.parts + (size_t)b * a.segs * 2;
    double* S = a.hops + (size_t)b * a.hop_cap;
    for (int h = tid; h < nh; h += 256) {
        const long long k0 = h * step / kSeg, k1 = ((h + 1) * step - 1) / kSeg;
        double s = 0.0;
        for (long long k = k0; k <= k1; ++k) s = s + parts[2 * k + (k * kSeg / step == h ? 0 : 1)];
        S[h] = s;
    }
    // the item's peak: exact, so any order
    const int nseg = (int)(((long long)Lb + kSeg - 1) / kSeg);
    float pk = 0.f;
    for (int k = tid; k < nseg; k += 256) pk = fmaxf(pk, a.seg_peak[(size_t)b * a.segs + k]);
    for (int o = 32; o >= 1; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    __shared__ float redf[4];
    if ((tid & 63) == 0) redf[tid >> 6] = pk;
    __syncthreads();                                                // S is visible to the block, too
    pk = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));

    const double den = (double)(4 * step), abs_thr = a.design[kAbsThr];
    auto z_of = [&](int j) -> double { return (((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) / den; };
    double acc = 0.0;
    int cnt = 0;
    for (int j = tid; j < J; j += 256) {
        const double z = z_of(j);
        if (z > abs_thr) { acc = acc + z; ++cnt; }
    }
    const double sum_abs = fixed_sum(acc, red);
    const int n_abs = block_sum_int(cnt, redi);
    double ms = 0.0;
    if (n_abs > 0) {
        const double rel_thr = 0.1 * (sum_abs / (double)n_abs);
        acc = 0.0; cnt = 0;
        for (int j = tid; j < J; j += 256) {
            const double z = z_of(j);
            if (z > abs_thr && z > rel_thr) { acc = acc + z; ++cnt; }
        }
        const double sum_rel = fixed_sum(acc, red);
        const int n_rel = block_sum_int(cnt, redi);
        if (n_rel > 0) ms = sum_rel / (double)n_rel;
    }
    if (tid == 0) {
        double g = 1.0;
        if (ms > 0.0) {
            g = sqrt(a.design[kTargetMs] / ms);
            g = fmin(g, a.design[kMaxGain]);
            const double ceil_ = a.design[kCeiling];
            if (ceil_ > 0.0 && pk > 0.f) g = fmin(g, ceil_ / (double)pk);
        }
        a.stats[2 * b] = ms;
        a.stats[2 * b + 1] = g;
    }
}

inline hipError_t launch_gate(const GateLaunch& a, int B, hipStream_t stream) {
    return ::iris::launch_kernel(gate_kernel, dim3((unsigned)B), dim3(256), 0, stream, a);
}

struct ApplyLaunch {
    const float* wav;           // [B, L]
    const int32_t* lengths;
    int row_scale;
    const double* stats;        // [B][2]
    float* out;                 // [B, L]
    int B, L;
};

__global__ void __launch_bounds__(256) apply_kernel(const ApplyLaunch a) {
#pragma clang fp contract(off)
    const unsigned total = (unsigned)a.B * (unsigned)a.L, L = (unsigned)a.L;
    const unsigned p_end = blockIdx.x * (unsigned)kApplyRun + kApplyRun;
    const bool vec = (((uintptr_t)a.out | (uintptr_t)a.wav) & 15) == 0;
    auto rows_of = [&](int b) -> unsigned {                         // ragged_rows without its wave-uniform load: b varies by lane
        if (!a.lengths) return L;
        const long long n = (long long)a.lengths[b] * a.row_scale;
        return n <= 0 ? 0u : (n < (long long)L ? (unsigned)n : L);
    };
    for (unsigned p = blockIdx.x * (unsigned)kApplyRun + 4u * threadIdx.x; p < p_end && p < total; p += 1024) {
        const unsigned cnt = total - p < 4u ? total - p : 4u;
        const unsigned b = p / L, n = p - b * L;
        lf32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (n + 3 < L) {                                            // the group lies in one row
            const unsigned Lb = rows_of((int)b);
            if (n < Lb) {
                const float g = (float)a.stats[2 * b + 1];
                if (vec && n + 3 < Lb) {
                    const lf32x4 x = *reinterpret_cast<const lf32x4*>(a.wav + p);
#pragma unroll
                    for (unsigned e = 0; e < 4; ++e) q[e] = x[e] * g;
                } else {
#pragma unroll
                    for (unsigned e = 0; e < 4; ++e) if (n + e < Lb) q[e] = a.wav[p + e] * g;
                }
            }
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e)
                if (e < cnt) {
                    const unsigned be = (p + e) / L, ne = p + e - be * L;
                    if (ne < rows_of((int)be)) q[e] = a.wav[p + e] * (float)a.stats[2 * be + 1];
                }
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<lf32x4*>(a.out + p) = q;
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; ++e) if (e < cnt) a.out[p + e] = q[e];
        }
    }
}

inline hipError_t launch_apply(const ApplyLaunch& a, hipStream_t stream) {
    const long long total = (long long)a.B * a.L;
    const dim3 grid((unsigned)((total + kApplyRun - 1) / kApplyRun)), block(256);
    return ::iris::launch_kernel(apply_kernel, grid, block, 0, stream, a);
}

}  // namespace loudness
}  // namespace iris
