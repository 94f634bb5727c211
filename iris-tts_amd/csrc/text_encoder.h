// text_encoder.h -- the text side of the reference's synthesis script for gfx950: the Transformer phoneme encoder
// (PhonemeEncoder, src/iris/encoder.py:115-212), the convolutional duration head (DurationPredictor, :228-315,
// predict_durations, scripts/synthesize.py:41-45) and the length regulator (synthesize.py:48-61, 112-122).  fp32, inference.
//
// txt_embed_kernel     x[b, p, :] = phoneme_embedding[clamp(id)] + position_embedding[p]
// txt_gemm_kernel      channels-last implicit GEMM on v_mfma_f32_32x32x2_f32 over rows [B * P, C_in] with the fragment-ordered
//                      weights of packed_conv_f32.h and the MFMA loop of gemm_tile_f32.h.  C_in is staged in slices of at most 256
//                      channels (the second FFN layer has C_in = 1024: the whole 32 x 1028-float window would leave one block
//                      per CU).  Epilogue: bias, then optionally ReLU, a residual row and LayerNorm (epsilon, gamma, beta,
//                      biased variance, mean first and the squared deviations second).  A LayerNorm launch holds every C_out
//                      tile of its 32 rows in one block (C_out <= 256), so the row statistics are reduced through LDS and the
//                      un-normalised sum never reaches HBM; the other launches walk further C_out tiles with blockIdx.y.
// txt_attention_kernel one wave per (item, head, 32-query tile): S^T = K (Q / sqrt(key_dim))^T on the MFMA, keys walked in
//                      tiles of 32 with a running maximum and sum per query, O^T += V^T P^T on the MFMA.  The scores are laid
//                      out keys x queries, so a query's 32 scores of a tile sit in one lane and its partner (lane ^ 32), and the
//                      registers that hold P are already the B operand of the second product.  [B, H, P, P] never exists.
// txt_layernorm_kernel the encoder's final_norm.
// txt_duration_kernel  duration_output (1x1 to one channel), softplus, frames = clip(rint(exp(pred) - 1), 1, max).
// txt_scan_kernel      exclusive prefix sum of an item's frames: offsets [B, P + 1], totals [B].
// txt_gather_kernel    cond[b, t, :] = enc_out[b, phoneme(t), :] by binary search in offsets; zeros from totals[b] on.
//
// Ragged batches: item b owns lengths[b] positions.  Positions past that read as 0 in every staging loop (so the duration
// head's 'same' padding is the item's own), have weight exactly 0 as keys, and are stored as 0 by every kernel: item b is
// computed bit for bit as a batch of one on its own ids.  Every loop bound is a kernel argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_info.h"
#include "gemm_tile_f32.h"

namespace iris {
namespace txt {

constexpr int kRows = 32;            // rows (positions) of a GEMM block, queries of an attention block, keys of a key tile
constexpr int kMaxWaves = 8;         // C_out tiles of a GEMM block
constexpr int kSlice = 256;          // input channels staged at once
constexpr int kMaxKeyDim = 128;      // attention: four 32-wide output tiles per head at most

// ---------------------------------------------------------------------------------------------
struct EmbedLaunch {
    const int32_t* ids;       // [B, P]
    const int32_t* lengths;   // [B] or nullptr
    const float* tok;         // [vocab, E]
    const float* pos;         // [max_length, E]
    float* x;                 // [B, P, E]
    int B, P, E, vocab;
};

__global__ void __launch_bounds__(256) txt_embed_kernel(const EmbedLaunch a) {
    const int QPR = a.E >> 2;
    const long long total = (long long)a.B * a.P * QPR;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)(idx % QPR);
    const long long row = idx / QPR;
    const int p = (int)(row % a.P), b = (int)(row / a.P);
    int len = a.P;
    if (a.lengths) { len = a.lengths[b]; len = len < 0 ? 0 : (len > a.P ? a.P : len); }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < len) {
        int id = a.ids[row];
        id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);       // never outside the table (the callers reject such ids)
        const f32x4 t = *reinterpret_cast<const f32x4*>(a.tok + (size_t)id * a.E + 4 * q);
        const f32x4 e = *reinterpret_cast<const f32x4*>(a.pos + (size_t)p * a.E + 4 * q);
        v = t + e;
    }
    *reinterpret_cast<f32x4*>(a.x + (size_t)row * a.E + 4 * q) = v;
}

// ---------------------------------------------------------------------------------------------
struct GemmLaunch {
    const float* x;           // [B, P, C_in]
    const f32x4* wp;          // packed weights (pack_conv1d_weights)
    const float* bias;        // [C_out]
    float* y;                 // [B, P, C_out]
    const float* res;         // residual [B, P, C_out] added before the LayerNorm, or nullptr
    const float* gamma;       // LayerNorm scale [C_out], or nullptr: no LayerNorm
    const float* beta;
    const int32_t* lengths;   // [B] or nullptr
    int P, C_in, C_out, ks;   // 'same' padding (ks - 1) / 2, ks odd
    int Gp, n_ct;
    int relu;
    float eps;
};

inline int gemm_slice(int C_in) { const int Cp = (C_in + 7) & ~7; return Cp < kSlice ? Cp : kSlice; }
inline size_t gemm_lds_bytes(int C_in, int ks) {
    return ((size_t)(kRows + ks - 1) * lds_row_floats(gemm_slice(C_in)) + 2 * 64 * kMaxWaves) * sizeof(float);
}

__global__ void __launch_bounds__(64 * kMaxWaves) txt_gemm_kernel(const GemmLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z;
    const int i0 = blockIdx.x * kRows;
    const int ct = blockIdx.y * nw + wave;
    const bool active = ct < a.n_ct;                       // wave-uniform
    const int len = ragged_rows(a.lengths, b, 1, a.P);

    if (i0 >= len) {                                       // block-uniform: a tile past the item's end is zeros
        const int c0 = blockIdx.y * nw * 32;
        const int c1 = c0 + nw * 32 < a.C_out ? c0 + nw * 32 : a.C_out;
        const int QPR = (c1 - c0) >> 2;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int idx = tid; idx < kRows * QPR; idx += nthr) {
            const int r = idx / QPR, q = idx - r * QPR;
            if (i0 + r < a.P) *reinterpret_cast<f32x4*>(a.y + ((size_t)b * a.P + i0 + r) * a.C_out + c0 + 4 * q) = z;
        }
        return;
    }

    const int Cp = (a.C_in + 7) & ~7;
    const int KS = Cp < kSlice ? Cp : kSlice, S = KS + 4;
    const int R = kRows + a.ks - 1;
    const int v0 = i0 - (a.ks - 1) / 2;
    float* red = lds + R * S;                              // [2][nw][64] LayerNorm partial sums

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < Cp; k0 += KS) {
        const int kc = Cp - k0 < KS ? Cp - k0 : KS;        // a multiple of 8
        if (k0) __syncthreads();
        const int QPR = kc >> 2, total = R * QPR;
        for (int idx = tid; idx < total; idx += nthr) {
            const int r = idx / QPR, q = idx - r * QPR;
            const int v = v0 + r, ci = k0 + 4 * q;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (v >= 0 && v < len && ci < a.C_in)
                val = *reinterpret_cast<const f32x4*>(a.x + ((size_t)b * a.P + v) * a.C_in + ci);
            *reinterpret_cast<f32x4*>(lds + r * S + 4 * q) = val;
        }
        __syncthreads();
        if (active)
            mma_loop(acc, lds + lo * S + 4 * hi, S, a.wp + ((size_t)(k0 >> 3) * a.n_ct + ct) * 64 + lane, (size_t)a.n_ct * 64,
                          a.Gp, a.ks, kc >> 3);
    }

    // D[co][t]: lane & 31 = row, registers 4g .. 4g+3 = channels ct*32 + 8g + 4*(lane >> 5) + {0..3}
    const int t = i0 + lo;
    const bool valid = t < len;
    const size_t row = (size_t)b * a.P + (t < a.P ? t : 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = ct * 32 + 8 * g + 4 * hi;
        const bool in = active && co < a.C_out;            // C_out % 4 == 0: a piece of 4 is inside or outside as a whole
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f}, r4 = {0.f, 0.f, 0.f, 0.f};
        if (in) b4 = *reinterpret_cast<const f32x4*>(a.bias + co);
        if (in && a.res && valid) r4 = *reinterpret_cast<const f32x4*>(a.res + row * a.C_out + co);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = in ? acc[4 * g + e] + b4[e] : 0.f;
            if (a.relu) v = fmaxf(v, 0.f);
            acc[4 * g + e] = r4[e] + v;
        }
    }
    if (a.gamma) {
        // nw == n_ct here (the host launches every tile of the rows in this block): both passes see the whole row
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[r];
        red[wave * 64 + lane] = s;
        __syncthreads();
        float tot = 0.f;
        for (int w = 0; w < nw; ++w) tot += red[w * 64 + lo] + red[w * 64 + 32 + lo];
        const float mean = tot / (float)a.C_out;
        float q = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool in = active && ct * 32 + 8 * g + 4 * hi < a.C_out;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = in ? acc[4 * g + e] - mean : 0.f;
                acc[4 * g + e] = d;
                q = fmaf(d, d, q);
            }
        }
        float* red2 = red + 64 * nw;
        red2[wave * 64 + lane] = q;
        __syncthreads();
        float tot2 = 0.f;
        for (int w = 0; w < nw; ++w) tot2 += red2[w * 64 + lo] + red2[w * 64 + 32 + lo];
        const float rstd = 1.f / sqrtf(tot2 / (float)a.C_out + a.eps);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + 8 * g + 4 * hi;
            if (active && co < a.C_out) {
                const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.gamma + co);
                const f32x4 e4 = *reinterpret_cast<const f32x4*>(a.beta + co);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] = fmaf(acc[4 * g + e] * rstd, g4[e], e4[e]);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (active && t < a.P) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + 8 * g + 4 * hi;
            if (co < a.C_out) {
                f32x4 v = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                if (!valid) v = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(a.y + row * a.C_out + co) = v;
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------------------------------------
struct AttnLaunch {
    const float* qkv;         // [B, P, 3E]: q at column h * Dk, k at E + h * Dk, v at 2E + h * Dk
    float* out;               // [B, P, E]
    const int32_t* lengths;   // [B] or nullptr
    int P, E, H, Dk;          // Dk % 8 == 0, Dk <= kMaxKeyDim
    float scale;              // 1 / sqrt(Dk), applied to q = x W + b as a whole
};

inline size_t attn_lds_bytes(int Dk) { return (size_t)3 * kRows * (Dk + 4) * sizeof(float); }

__global__ void __launch_bounds__(64) txt_attention_kernel(const AttnLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, lo = lane & 31, hi = lane >> 5;
    const int i0 = blockIdx.x * kRows, h = blockIdx.y, b = blockIdx.z;
    const int Dk = a.Dk, S = Dk + 4, QPR = Dk >> 2, ld = 3 * a.E;
    const int len = ragged_rows(a.lengths, b, 1, a.P);
    const int nd = (Dk + 31) >> 5;
    float* ql = lds;
    float* kl = ql + kRows * S;
    float* vl = kl + kRows * S;
    const float* base = a.qkv + (size_t)b * a.P * ld + h * Dk;

    f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    if (i0 < len) {                                        // block-uniform; a tile of padded queries is computed from nothing
        for (int idx = lane; idx < kRows * QPR; idx += 64) {
            const int r = idx / QPR, q = idx - r * QPR;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i0 + r < len) v = *reinterpret_cast<const f32x4*>(base + (size_t)(i0 + r) * ld + 4 * q) * a.scale;
            *reinterpret_cast<f32x4*>(ql + r * S + 4 * q) = v;
        }
        for (int j0 = 0; j0 < len; j0 += kRows) {
            __syncthreads();                               // the previous tile's K and V have been read
            for (int idx = lane; idx < kRows * QPR; idx += 64) {
                const int r = idx / QPR, q = idx - r * QPR;
                f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
                if (j0 + r < len) {
                    const float* src = base + (size_t)(j0 + r) * ld + 4 * q;
                    kv = *reinterpret_cast<const f32x4*>(src + a.E);
                    vv = *reinterpret_cast<const f32x4*>(src + 2 * a.E);
                }
                *reinterpret_cast<f32x4*>(kl + r * S + 4 * q) = kv;
                *reinterpret_cast<f32x4*>(vl + r * S + 4 * q) = vv;
            }
            __syncthreads();
            // S^T[key][query]: lane & 31 = query, registers 4g + e = key 8g + 4 (lane >> 5) + e
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            for (int c = 0; c < Dk; c += 8) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(kl + lo * S + c + 4 * hi);
                const f32x4 qf = *reinterpret_cast<const f32x4*>(ql + lo * S + c + 4 * hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[e], s, 0, 0, 0);
            }
            float mt = -INFINITY;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + 8 * g + 4 * hi + e < len) mt = fmaxf(mt, s[4 * g + e]);
            mt = fmaxf(mt, __shfl_xor(mt, 32));            // key j0 is inside the item, so mt is finite
            const float mn = fmaxf(m, mt);
            const float alpha = expf(m - mn);              // 0 at the first tile (m = -inf)
            float ps = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = j0 + 8 * g + 4 * hi + e < len ? expf(s[4 * g + e] - mn) : 0.f;   // a padded key: exactly 0
                    s[4 * g + e] = p;
                    ps += p;
                }
            ps += __shfl_xor(ps, 32);
            l = fmaf(l, alpha, ps);
            m = mn;
            // O^T[d][query] = alpha O^T + V^T P^T: A = V[key 8g + 4 hi + e][d = lane & 31], B = the registers of P
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (d < nd) {                              // wave-uniform
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
                    const int dc = 32 * d + lo;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float vf = dc < Dk ? vl[(8 * g + 4 * hi + e) * S + dc] : 0.f;
                            o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, s[4 * g + e], o[d], 0, 0, 0);
                        }
                }
            }
        }
    }
    const int t = i0 + lo;
    if (t < a.P) {
        const bool valid = t < len;
        float* dst = a.out + ((size_t)b * a.P + t) * a.E + h * Dk;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (d < nd) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dc = 32 * d + 8 * g + 4 * hi;
                    if (dc < Dk) {
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (valid) v = f32x4{o[d][4 * g + 0] / l, o[d][4 * g + 1] / l, o[d][4 * g + 2] / l, o[d][4 * g + 3] / l};
                        *reinterpret_cast<f32x4*>(dst + dc) = v;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One wave per row.  Sums over the wave by xor butterflies: every lane ends with the same bits.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

struct NormLaunch {
    const float* x; const float* gamma; const float* beta; float* y;
    const int32_t* lengths;
    int B, P, C;
    float eps;
};

__global__ void __launch_bounds__(256) txt_layernorm_kernel(const NormLaunch a) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)a.B * a.P) return;               // wave-uniform
    const int b = (int)(row / a.P), p = (int)(row - (long long)b * a.P);
    const int len = ragged_rows(a.lengths, b, 1, a.P);
    const int QPR = a.C >> 2;
    const float* src = a.x + (size_t)row * a.C;
    float* dst = a.y + (size_t)row * a.C;
    if (p >= len) {
        for (int q = lane; q < QPR; q += 64) *reinterpret_cast<f32x4*>(dst + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    float s = 0.f;
    for (int q = lane; q < QPR; q += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_sum(s) / (float)a.C;
    float qq = 0.f;
    for (int q = lane; q < QPR; q += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[e] - mean; qq = fmaf(d, d, qq); }
    }
    const float rstd = 1.f / sqrtf(wave_sum(qq) / (float)a.C + a.eps);
    for (int q = lane; q < QPR; q += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.gamma + 4 * q);
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(a.beta + 4 * q);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaf((v[e] - mean) * rstd, g4[e], e4[e]);
        *reinterpret_cast<f32x4*>(dst + 4 * q) = r;
    }
}

struct DurationLaunch {
    const float* x;           // [B, P, C]
    const float* w;           // duration_output kernel [C], then its bias [1]
    const int32_t* lengths;
    float* pred;              // [B, P] softplus output
    int32_t* frames;          // [B, P]
    int B, P, C, max_frames;
};

__global__ void __launch_bounds__(256) txt_duration_kernel(const DurationLaunch a) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)a.B * a.P) return;
    const int b = (int)(row / a.P), p = (int)(row - (long long)b * a.P);
    const int len = ragged_rows(a.lengths, b, 1, a.P);
    float pred = 0.f;
    int frames = 0;
    if (p < len) {                                         // wave-uniform
        const int QPR = a.C >> 2;
        float s = 0.f;
        for (int q = lane; q < QPR; q += 64) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (size_t)row * a.C + 4 * q);
            const f32x4 w = *reinterpret_cast<const f32x4*>(a.w + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(v[e], w[e], s);
        }
        const float u = wave_sum(s) + a.w[a.C];
        pred = fmaxf(u, 0.f) + log1pf(expf(-fabsf(u)));    // softplus = logaddexp(u, 0)
        float f = rintf(expf(pred) - 1.f);                 // round half to even, as jnp.round
        f = fminf(fmaxf(f, 1.f), (float)a.max_frames);
        frames = (int)f;
    }
    if (lane == 0) { a.pred[row] = pred; a.frames[row] = frames; }
}

// ---------------------------------------------------------------------------------------------
struct ScanLaunch {
    const int32_t* frames;    // [B, P]; negative values count as 0
    const int32_t* lengths;
    int32_t* offsets;         // [B, P + 1]: offsets[b, p] = frames before phoneme p; from lengths[b] on, the total
    int32_t* totals;          // [B]
    int P;
};

__global__ void __launch_bounds__(256) txt_scan_kernel(const ScanLaunch a) {
    __shared__ int part[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int len = ragged_rows(a.lengths, b, 1, a.P);
    const int per = (a.P + 255) / 256;
    const int p0 = tid * per, p1 = p0 + per < a.P ? p0 + per : a.P;
    const int32_t* f = a.frames + (size_t)b * a.P;
    int s = 0;
    for (int p = p0; p < p1; ++p) { const int v = p < len ? f[p] : 0; s += v > 0 ? v : 0; }
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                    // inclusive scan of the 256 partial sums
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    int32_t* o = a.offsets + (size_t)b * (a.P + 1);
    for (int p = p0; p < p1; ++p) {
        o[p] = run;
        const int v = p < len ? f[p] : 0;
        run += v > 0 ? v : 0;
    }
    if (tid == 255) { o[a.P] = part[255]; a.totals[b] = part[255]; }
}

struct GatherLaunch {
    const float* enc;         // [B, P, E]
    const int32_t* offsets;   // [B, P + 1]
    const int32_t* totals;    // [B]
    float* cond;              // [B, T_pad, E]
    int P, E, T_pad;
};

__global__ void __launch_bounds__(256) txt_gather_kernel(const GatherLaunch a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T_pad) return;                              // wave-uniform: one wave per frame
    const int32_t* o = a.offsets + (size_t)b * (a.P + 1);
    int total = a.totals[b];
    total = total < o[a.P] ? total : o[a.P];
    const int QPR = a.E >> 2;
    float* dst = a.cond + ((size_t)b * a.T_pad + t) * a.E;
    if (t >= total) {
        for (int q = lane; q < QPR; q += 64) *reinterpret_cast<f32x4*>(dst + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    int lo = 0, hi = a.P;                                  // the phoneme p with offsets[p] <= t < offsets[p + 1]: lo ends at p + 1
    while (lo < hi) {                                      // first index in [0, P] whose offset is > t
        const int mid = (lo + hi) >> 1;
        if (o[mid] <= (int)t) lo = mid + 1; else hi = mid;
    }
    const int p = lo > 0 ? lo - 1 : 0;                     // offsets[0] = 0 <= t, so lo >= 1; t < offsets[P], so p < P
    const float* src = a.enc + ((size_t)b * a.P + p) * a.E;
    for (int q = lane; q < QPR; q += 64) *reinterpret_cast<f32x4*>(dst + 4 * q) = *reinterpret_cast<const f32x4*>(src + 4 * q);
}

#ifndef IRIS_KERNELS_ONLY
inline hipError_t launch_embed(const EmbedLaunch& a, hipStream_t stream) {
    const long long total = (long long)a.B * a.P * (a.E >> 2);
    return launch_kernel_named("txt_embed_kernel", txt_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
}

// A LayerNorm launch needs every C_out tile in one block (C_out <= 32 * kMaxWaves).
inline hipError_t launch_gemm(GemmLaunch& a, int B, hipStream_t stream) {
    a.Gp = packed_groups(a.C_in);
    a.n_ct = packed_cotiles(a.C_out);
    const int nw = a.n_ct < kMaxWaves ? a.n_ct : kMaxWaves;
    if (a.gamma && a.n_ct > kMaxWaves) return hipErrorInvalidValue;
    dim3 grid((unsigned)((a.P + kRows - 1) / kRows), (unsigned)((a.n_ct + nw - 1) / nw), (unsigned)B);
    return launch_kernel_named(a.gamma ? "txt_gemm_kernel<layernorm>" : "txt_gemm_kernel", txt_gemm_kernel, grid, dim3((unsigned)(64 * nw)),
                               gemm_lds_bytes(a.C_in, a.ks), stream, a);
}

inline hipError_t launch_attention(const AttnLaunch& a, int B, hipStream_t stream) {
    dim3 grid((unsigned)((a.P + kRows - 1) / kRows), (unsigned)a.H, (unsigned)B);
    return launch_kernel_named("txt_attention_kernel", txt_attention_kernel, grid, dim3(64), attn_lds_bytes(a.Dk), stream, a);
}

inline hipError_t launch_layernorm(const NormLaunch& a, hipStream_t stream) {
    const long long rows = (long long)a.B * a.P;
    return launch_kernel_named("txt_layernorm_kernel", txt_layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a);
}

inline hipError_t launch_duration(const DurationLaunch& a, hipStream_t stream) {
    const long long rows = (long long)a.B * a.P;
    return launch_kernel_named("txt_duration_kernel", txt_duration_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a);
}

inline hipError_t launch_scan(const ScanLaunch& a, int B, hipStream_t stream) {
    return launch_kernel_named("txt_scan_kernel", txt_scan_kernel, dim3((unsigned)B), dim3(256), 0, stream, a);
}

inline hipError_t launch_gather(const GatherLaunch& a, int B, hipStream_t stream) {
    dim3 grid((unsigned)((a.T_pad + 3) / 4), (unsigned)B);
    return launch_kernel_named("txt_gather_kernel", txt_gather_kernel, grid, dim3(256), 0, stream, a);
}
#endif

}  // namespace txt
}  // namespace iris
