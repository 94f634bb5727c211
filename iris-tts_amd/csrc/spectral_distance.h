// spectral_distance.h -- how far apart two waveforms are, as spectra and as samples, per item of a ragged batch, on the device
// (iris_spectral_distance_*): the sums behind the multi-resolution STFT distance (spectral convergence and log-magnitude L1) and
// behind the SNR.  ref and test [B, L] fp32 share lengths and row_scale; item b owns n_b = min(L, lengths[b] * row_scale) samples
// (ragged_rows; L where lengths is NULL) of both, and nothing behind n_b is read.  The host never reads a length.
//
// Per resolution r = (N, H, win) of at most kMaxRes, K = N / 2 + 1 bins:
//   transform    that of stft_f32.h on both signals: center=True, constant padding, periodic Hann of win centred in N, the same
//                packed table, staging and short chains.  The frame rule is this stage's own: T_b = 1 + n_b / H frames (0 for
//                n_b == 0) and ALL n_b samples are read -- n_b need not be a multiple of H; an item of 3 * 256 samples at H = 512
//                has 2 frames, and its last 256 samples count.  (stft_f32.h's ragged rule, L_b = H (T_b - 1) from a count of
//                frames, cannot say that: Magnitude below brings `samples`, the trait stft_kernel takes an item's bounds from.)
//   magnitudes   A (of ref) and B (of test) = dn::magnitude(re, im) = sqrtf(re re + im im), fp32, stored [B][T][Ks] with
//                T = 1 + L / H; bins 0 and N / 2 are real.  Nothing at t >= T_b or in columns K .. Ks - 1 is written or read.
//   terms        from the two stored fp32 values, in fp64, nothing contracted: a = (double)A, c = (double)B,
//                    d2 += (a - c) (a - c);   a2 += a a;   l1 += |log(fmax(a, 1e-5)) - log(fmax(c, 1e-5))|
//                (1e-5 is the mel front-end's clip; the logarithm is the double one, as mel_frontend.h takes it).
//   order        a tile is kTileFrames frames of the item, counted from its frame 0; its cells are walked as groups of four
//                bins, group i = (t - t0) (Ks / 4) + k / 4 over the tile's own frames.  Thread u of 256 takes the groups
//                i = u, u + 256, ... ascending and in each the bins k ascending (k < K), adding every term to its three sums as
//                it comes; then block_sum: a shuffle tree inside each wave (offsets 32, 16, .., 1, lane l adds lane l + offset),
//                then the four waves in order.  One triple per tile; the item's sums are its tiles' added in tile order
//                (finish_kernel).  No atomics: two runs give the same bits, and an item's sums are those of its batch-of-one call.
//
// In the sample domain, over the item's n_b samples x (ref) and y (test):
//   terms        e2 += ((double)x - (double)y)^2 and x2 += (double)x (double)x in fp64; emax = max |x - y| with the difference
//                in fp32 (exact maximum, any order).
//   order        a chunk is kChunk samples from the item's sample 0; thread u takes n = u, u + 256, ... ascending; block_sum;
//                the chunks in order.
//
// Outputs: spec [B][R][3] = (d2, a2, l1), wave [B][3] = (e2, x2, (double)emax) in fp64, frames [B][R] int32 = T_b.  An item with
// n_b == 0 has frames 0 and every sum 0.  The caller finishes them (iris/metrics.py): sqrt(d2 / a2), l1 / (T_b K), 10 log10(x2 / e2).
//
// Launches: per resolution the transform of ref, the transform of test (both stft_kernel<sd::Magnitude>; the first stores T_b)
// and tile_kernel; then wave_kernel and finish_kernel: 3 R + 2.  Blocks past an item return before their first barrier.
#pragma once
#include "denoiser.h"

namespace iris {
namespace sd {

constexpr int kMaxRes = 4;
constexpr int kThreads = 256;
constexpr int kTileFrames = 8;         // frames of a tile: 125 tiles for 1000 frames, so a batch of one still fills the device
constexpr int kChunk = 4096;           // samples of a chunk
constexpr double kFloor = 1e-5;        // the mel front-end's clip

inline int tiles_of(int T) { return (T + kTileFrames - 1) / kTileFrames; }
inline int chunks_of(int L) { return (int)(((long long)L + kChunk - 1) / kChunk); }

}  // namespace sd
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace sd {

// dn::Magnitude under this stage's frame rule (see "transform" above).  frames: [B][R] + r, or NULL in the launch on `test`.
struct Magnitude : dn::Magnitude {
    const int32_t* lengths;   // [B] (device) or NULL
    int row_scale;
    int* frames;
    int frames_stride;        // R
    static constexpr const char* kName = "sd_stft_kernel<magnitude>";
    __device__ __forceinline__ int samples(int b, int L) const { return ragged_rows(lengths, b, row_scale, L); }
    __device__ __forceinline__ void item(int b, int Tb) const { if (frames) frames[(size_t)b * frames_stride] = Tb; }
};

// The block's sum in thread 0, in the header's order.  red: kThreads / 64 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) s = s + red[w];
    __syncthreads();
    return s;
}

struct TileLaunch {
    const float* A;             // [B][T][Ks]: magnitudes of ref
    const float* Bm;            // [B][T][Ks]: of test
    const int32_t* lengths;
    int row_scale;
    double* part;               // [B][tiles][3]
    int L, T, hop, Ks, bins, tiles;
};

__global__ void __launch_bounds__(kThreads) tile_kernel(const TileLaunch a) {
#pragma clang fp contract(off)
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int nb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const int Tb = nb > 0 ? 1 + nb / a.hop : 0;
    const int t0 = tile * kTileFrames;
    if (t0 >= Tb) return;                                           // block-uniform, before the first barrier
    const int nt = Tb - t0 < kTileFrames ? Tb - t0 : kTileFrames, G4 = a.Ks >> 2;
    const size_t base = ((size_t)b * a.T + t0) * a.Ks;
    double d2 = 0.0, a2 = 0.0, l1 = 0.0;
    for (int i = tid; i < nt * G4; i += kThreads) {
        const int k0 = 4 * (i % G4);                                // rows are Ks floats: group i lies at 4 i
        const f32x4 x = *reinterpret_cast<const f32x4*>(a.A + base + 4 * (size_t)i);
        const f32x4 y = *reinterpret_cast<const f32x4*>(a.Bm + base + 4 * (size_t)i);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < a.bins) {                                  // columns from K on were never written
                const double p = (double)x[e], q = (double)y[e], d = p - q;
                const double dd = d * d, pp = p * p, ll = fabs(log(fmax(p, kFloor)) - log(fmax(q, kFloor)));
                d2 = d2 + dd; a2 = a2 + pp; l1 = l1 + ll;
            }
    }
    d2 = block_sum(d2, red); a2 = block_sum(a2, red); l1 = block_sum(l1, red);
    if (tid == 0) {
        double* out = a.part + ((size_t)b * a.tiles + tile) * 3;
        out[0] = d2; out[1] = a2; out[2] = l1;
    }
}

inline hipError_t launch_tiles(const TileLaunch& a, int B, hipStream_t stream) {
    return launch_kernel_named("sd_tile_kernel", tile_kernel, dim3((unsigned)a.tiles, (unsigned)B), dim3(kThreads), 0, stream, a);
}

struct WaveLaunch {
    const float* ref;           // [B, L]
    const float* test;          // [B, L]
    const int32_t* lengths;
    int row_scale;
    double* part;               // [B][chunks][3]: e2, x2, (double)emax
    int L, chunks;
};

__global__ void __launch_bounds__(kThreads) wave_kernel(const WaveLaunch a) {
#pragma clang fp contract(off)
    __shared__ double red[kThreads / 64];
    __shared__ float redf[kThreads / 64];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y;
    const int nb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    const long long n0 = (long long)chunk * kChunk;
    if (n0 >= nb) return;                                           // block-uniform, before the first barrier
    const int cnt = nb - n0 < kChunk ? (int)(nb - n0) : kChunk;
    const float* __restrict__ x = a.ref + (size_t)b * a.L + n0;
    const float* __restrict__ y = a.test + (size_t)b * a.L + n0;
    double e2 = 0.0, x2 = 0.0;
    float emax = 0.f;
    for (int n = tid; n < cnt; n += kThreads) {
        const float xv = x[n], yv = y[n];
        const double p = (double)xv, d = p - (double)yv;
        const double dd = d * d, pp = p * p;
        e2 = e2 + dd; x2 = x2 + pp;
        emax = fmaxf(emax, fabsf(xv - yv));
    }
    for (int off = 32; off > 0; off >>= 1) emax = fmaxf(emax, __shfl_xor(emax, off, 64));
    if ((tid & 63) == 0) redf[tid >> 6] = emax;
    e2 = block_sum(e2, red); x2 = block_sum(x2, red);               // its barriers publish redf as well
    if (tid == 0) {
        double* out = a.part + ((size_t)b * a.chunks + chunk) * 3;
        out[0] = e2; out[1] = x2;
        out[2] = (double)fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    }
}

inline hipError_t launch_wave(const WaveLaunch& a, int B, hipStream_t stream) {
    return launch_kernel_named("sd_wave_kernel", wave_kernel, dim3((unsigned)a.chunks, (unsigned)B), dim3(kThreads), 0, stream, a);
}

struct FinishLaunch {
    const int32_t* lengths;
    int row_scale;
    const double* spec_part[kMaxRes];   // [B][tiles_r][3]
    const double* wave_part;            // [B][chunks][3]
    double* spec;                       // [B][R][3]
    double* wave;                       // [B][3]
    int hop[kMaxRes], tiles[kMaxRes];
    int L, R, chunks;
};

// One block per item; thread w < 3 adds sum w of each resolution over the item's tiles in order (r is a constant of the unrolled
// loop: the launch's arrays are read where they lie, not copied), threads 3 and 4 add e2 and x2 over its chunks, thread 5 takes
// the largest emax.  No barrier.
__global__ void __launch_bounds__(64) finish_kernel(const FinishLaunch a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, q = threadIdx.x;
    const int nb = ragged_rows(a.lengths, b, a.row_scale, a.L);
    if (q < 3) {
#pragma unroll
        for (int r = 0; r < kMaxRes; ++r) {
            if (r >= a.R) break;
            const int Tb = nb > 0 ? 1 + nb / a.hop[r] : 0, n = (Tb + kTileFrames - 1) / kTileFrames;
            const double* p = a.spec_part[r] + (size_t)b * a.tiles[r] * 3 + q;
            double s = 0.0;
            for (int i = 0; i < n; ++i) s = s + p[3 * (size_t)i];
            a.spec[((size_t)b * a.R + r) * 3 + q] = s;
        }
    } else if (q < 6) {
        const int w = q - 3, n = (int)(((long long)nb + kChunk - 1) / kChunk);
        const double* p = a.wave_part + (size_t)b * a.chunks * 3 + w;
        double s = 0.0;
        for (int i = 0; i < n; ++i) s = w == 2 ? fmax(s, p[3 * (size_t)i]) : s + p[3 * (size_t)i];
        a.wave[(size_t)b * 3 + w] = s;
    }
}

inline hipError_t launch_finish(const FinishLaunch& a, int B, hipStream_t stream) {
    return launch_kernel_named("sd_finish_kernel", finish_kernel, dim3((unsigned)B), dim3(64), 0, stream, a);
}

}  // namespace sd
}  // namespace iris
#endif
