// vae_losses.h -- the two losses a validation pass takes from a reconstruction (TextConditionedVAE.compute_recon_l1 and
// compute_kl, reference src/iris/vae.py:424-446, as scripts/train_vae.py:94-103 calls them), reduced on the device from
// target / recon [B, n_mels, T] (channels-first) and mean / logvar [B, T >> S, latent] with the lengths the ragged forwards
// take:
//   L1 = sum_b sum_{t < len_b} |target - recon|  /  (sum_b len_b * n_mels + 1e-6)
//   KL = sum_b sum_{rows < len_b >> S, all channels} -0.5 (1 + lv - m^2 - e^lv)  /  (sum_b (len_b >> S) + 1e-8)
// (the KL denominator counts rows, not rows x channels: the reference's own), or, without lengths, the plain means over
// all elements.  len_b is item_frames() of vae_decoder.h, and mask[:, ::2^S] of the training script has len_b >> S ones.
//
// Two launches.  vae_loss_partial_kernel: a block reduces one fixed tile of one item -- kLossFrames frames x all n_mels of
// the mel pair (lanes along time: a wave reads 256 consecutive frames of one channel, 16 bytes a lane), or kLossKlElems
// consecutive floats of the item's own [rows x latent] span of mean / logvar -- counted from the item's row 0.  Terms are
// fp32, as keras computes them; every sum is fp64, over a fixed thread -> element map and a fixed tree, and ends as one
// fp64 partial per tile in the workspace.  A tile wholly past its item's length returns without reading; inside a tile
// nothing at or past the length is read.  vae_loss_final_kernel (one block): a thread per item adds the item's partials
// in tile order, then thread 0 adds the items in b order and divides.  No floating-point atomics, no flags: the result is
// the same in every run, and an item's two sums do not depend on the batch around it or on the T it is padded to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_info.h"
#include "vae_decoder.h"

namespace iris {
namespace vae {

constexpr int kLossThreads = 256;
constexpr int kLossFrames = 256;       // frames of an L1 tile: one 16-byte piece per lane of a wave
constexpr int kLossKlElems = 4096;     // floats of a KL tile: four 16-byte pieces per thread

struct LossLaunch {
    const float* target;      // [B, n_mels, T]
    const float* recon;       // [B, n_mels, T]
    const float* mean;        // [B, T >> S, latent]
    const float* logvar;      // [B, T >> S, latent]
    const int32_t* lengths;   // [B] (device), sanitised by item_frames(); nullptr: every item has T frames, plain means
    double* partial;          // [B][n_l1 + n_kl] tile sums; entries of tiles past an item's length are never written or read
    double* item;             // [2][B] item sums: L1, then KL
    float* out;               // [2 + 2B]: L1, KL, item L1 sums, item KL sums
    int B, n_mels, T, latent, S;
    int n_l1, n_kl;           // tiles of an item at the padded shape
    int vec_mel, vec_lat;     // 1: every 16-byte piece of the mel pair / the latent pair is aligned (checked on the host)
};

inline int loss_l1_tiles(int T) { return (T + kLossFrames - 1) / kLossFrames; }
inline int loss_kl_tiles(int T, int S, int latent) {
    return (int)(((int64_t)(T >> S) * latent + kLossKlElems - 1) / kLossKlElems);
}
inline uint64_t loss_workspace_doubles(int B, int T, int S, int latent) {
    return (uint64_t)B * (uint64_t)(loss_l1_tiles(T) + loss_kl_tiles(T, S, latent)) + 2 * (uint64_t)B;
}

// the block's sum in thread 0: a fixed shuffle tree inside each wave, then the waves in order
__device__ __forceinline__ double loss_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kLossThreads / 64; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ float kl_term(float m, float lv) { return -0.5f * (1.f + lv - m * m - expf(lv)); }

__global__ void __launch_bounds__(kLossThreads) vae_loss_partial_kernel(const LossLaunch a) {
    __shared__ double red[kLossThreads / 64];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int len = a.lengths ? item_frames(a.lengths, b, a.T, a.S) : a.T;
    double acc = 0.0;
    if (tile < a.n_l1) {
        const int f0 = tile * kLossFrames;
        if (f0 >= len) return;                             // block-uniform, before the barrier
        // lane -> 4 consecutive frames, wave -> channels wave, wave + 4, ...
        const int t0 = f0 + 4 * (tid & 63);
        for (int c = tid >> 6; c < a.n_mels; c += kLossThreads / 64) {
            const size_t at = ((size_t)b * a.n_mels + c) * a.T + t0;
            if (a.vec_mel && t0 + 4 <= len) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(a.target + at);
                const f32x4 y = *reinterpret_cast<const f32x4*>(a.recon + at);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += (double)fabsf(x[e] - y[e]);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (t0 + e < len) acc += (double)fabsf(a.target[at + e] - a.recon[at + e]);
            }
        }
    } else {
        const int64_t n = (int64_t)(len >> a.S) * a.latent;   // the item's floats: rows [0, len >> S) are one span
        const int64_t e0 = (int64_t)(tile - a.n_l1) * kLossKlElems;
        if (e0 >= n) return;                               // block-uniform, before the barrier
        const size_t item0 = (size_t)b * (size_t)(a.T >> a.S) * a.latent;
        for (int p = 0; p < kLossKlElems / (4 * kLossThreads); ++p) {
            const int64_t i = e0 + 4 * (int64_t)(p * kLossThreads + tid);
            if (a.vec_lat && i + 4 <= n) {
                const f32x4 m = *reinterpret_cast<const f32x4*>(a.mean + item0 + i);
                const f32x4 lv = *reinterpret_cast<const f32x4*>(a.logvar + item0 + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += (double)kl_term(m[e], lv[e]);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (i + e < n) acc += (double)kl_term(a.mean[item0 + i + e], a.logvar[item0 + i + e]);
            }
        }
    }
    const double s = loss_block_sum(acc, red);
    if (tid == 0) a.partial[(size_t)b * (a.n_l1 + a.n_kl) + tile] = s;
}

__global__ void __launch_bounds__(kLossThreads) vae_loss_final_kernel(const LossLaunch a) {
    const int tid = threadIdx.x, nt = a.n_l1 + a.n_kl;
    for (int b = tid; b < a.B; b += kLossThreads) {
        const int len = a.lengths ? item_frames(a.lengths, b, a.T, a.S) : a.T;
        const int n1 = (len + kLossFrames - 1) / kLossFrames;
        const int nk = (int)(((int64_t)(len >> a.S) * a.latent + kLossKlElems - 1) / kLossKlElems);
        const double* p = a.partial + (size_t)b * nt;
        double l1 = 0.0, kl = 0.0;
        for (int t = 0; t < n1; ++t) l1 += p[t];
        for (int t = 0; t < nk; ++t) kl += p[a.n_l1 + t];
        a.item[b] = l1;
        a.item[a.B + b] = kl;
        a.out[2 + b] = (float)l1;
        a.out[2 + a.B + b] = (float)kl;
    }
    __syncthreads();
    if (tid != 0) return;
    double l1 = 0.0, kl = 0.0;
    int64_t frames = 0, rows = 0;
    for (int b = 0; b < a.B; ++b) {
        const int len = a.lengths ? item_frames(a.lengths, b, a.T, a.S) : a.T;
        l1 += a.item[b];
        kl += a.item[a.B + b];
        frames += len;
        rows += len >> a.S;
    }
    if (a.lengths) {
        a.out[0] = (float)(l1 / ((double)frames * a.n_mels + 1e-6));
        a.out[1] = (float)(kl / ((double)rows + 1e-8));
    } else {   // ops.mean over every element (0 / 0 for an empty tensor, as numpy has it)
        a.out[0] = (float)(l1 / ((double)frames * a.n_mels));
        a.out[1] = (float)(kl / ((double)rows * a.latent));
    }
}

#ifndef IRIS_KERNELS_ONLY
// Fills the tile counts and the alignment flags and queues both launches; `ws` holds loss_workspace_doubles() doubles.
inline hipError_t launch_losses(LossLaunch& a, double* ws, hipStream_t stream) {
    a.n_l1 = loss_l1_tiles(a.T);
    a.n_kl = loss_kl_tiles(a.T, a.S, a.latent);
    a.partial = ws;
    a.item = ws + (size_t)a.B * (a.n_l1 + a.n_kl);
    a.vec_mel = !(a.T & 3) && !(((uintptr_t)a.target | (uintptr_t)a.recon) & 15);
    a.vec_lat = !(a.latent & 3) && !(((uintptr_t)a.mean | (uintptr_t)a.logvar) & 15);
    if (a.B > 0 && a.n_l1 + a.n_kl > 0) {
        const hipError_t e = launch_kernel_named("vae_loss_partial_kernel", vae_loss_partial_kernel,
                                                 dim3((unsigned)(a.n_l1 + a.n_kl), (unsigned)a.B), dim3(kLossThreads), 0, stream, a);
        if (e != hipSuccess) return e;
    }
    return launch_kernel_named("vae_loss_final_kernel", vae_loss_final_kernel, dim3(1), dim3(kLossThreads), 0, stream, a);
}
#endif

}  // namespace vae
}  // namespace iris
