// vae_decoder.h -- the inference half of the text-conditioned VAE (TextConditionedVAE.generate, reference
// src/iris/vae.py:448-482) for gfx950: frame-level conditioning [B, T, cond_dim] -> mel [B, n_mels, T].
//
// Two kernels carry the whole stage.
//
// vae_gemm_kernel: channels-last implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 with the fragment-ordered weights of
// packed_conv_f32.h (pack_conv1d_weights) and the MFMA loop of gemm_tile_f32.h.  What it adds to conv_mfma_f32.h's formulation:
//   * the input row of output row i, tap kappa is  stride * i - pad_left + kappa * dil  (the stride-2 'same' convs of
//     TemporalDownsample, vae.py:80-105), optionally over the nearest-neighbour x2 repeat of the input, which is folded
//     into the LDS staging (x_up[r] = x[r >> 1], TemporalUpsample vae.py:134-147): the repeated tensor is never written;
//   * a GELU (tanh form) epilogue, and a FiLM epilogue  gamma * h + beta  whose rows come from the conditioning GEMM;
//   * FUSED: the WaveNetResBlock (vae.py:57-67) in one launch -- the FiLM'ed tile stays in LDS and is the A operand of a
//     second GEMM (res_proj, 1x1) whose epilogue adds the block's input;
//   * a channels-first store, [B, C_out, L], for out_proj (the layout PostNet and the vocoder read).
// A block owns 32 output rows and one 32-wide C_out tile per wave (up to 8 waves); all of C_in is staged at once (the
// stage's channel counts are <= 256) and blockIdx.y walks further C_out tiles (the conditioning GEMM has 2C columns per
// decoder block).
//
// vae_flow_kernel: the reverse volume-preserving flow (vae.py:162-243) and latent_dec_proj in plain FMAs -- 8 / 16 / 64
// channels are far below an MFMA tile.  APCoupling never permutes channels, so x1 = z[..., :latent/2] is the SAME tensor
// in every coupling and only x2 changes: t_j depends on x1 and the conditioning alone, and the k3 net_pre therefore needs
// one halo row per side for the whole stack, not one per coupling.  x2 is updated in LDS in the reference's order
// (last coupling first); z never goes to HBM.
//
// The FORWARD instantiation runs the couplings in order with x2 + t instead (TextConditionedVAE.call, vae.py:401): x1 still
// never changes, so the same halo argument holds.  iris_vae_decoder_forward_posterior launches it.
//
// Rows outside an item read 0 and are never stored; every loop bound is a kernel argument.
//
// Ragged form (RAGGED instantiations, iris_vae_decoder_forward_ragged): a device array lengths[B] gives each item's frames
// at the full rate.  item_frames() sanitises it on the device, and an item's rows at a level `sh` halvings below the full
// rate are  item_frames >> sh.  These per-item counts replace L_in / L_out / Tq as BOUNDS only -- what is staged, what
// reads 0, what is stored; row strides and buffer offsets keep coming from the padded shape, so item b lies where the
// dense forward puts it and a block still owns the same 32 rows counted from the item's row 0.  Inside its length an item
// therefore runs the dense form's loads, MFMAs and FMAs in the dense form's order: bit for bit the batch-of-one result.
// A block whose rows all lie past its item's length returns before its first barrier; the two output launches store 0.0f
// there instead (zero_tail).  The dense instantiations contain none of this.
//
// The posterior side is ragged in the same way (iris_vae_posterior_encode_ragged, iris_vae_decoder_forward_posterior_ragged):
// the kGemmMelIn staging loop is bounded by the item's frames, the kGemmSplitOut launch stores mean | logvar rows past the
// item's latent rows as 0.0f (a padded latent row then adds exactly 0 to the KL sum of vae_losses.h), and the FORWARD flow
// takes the RAGGED bound like the reverse one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_info.h"
#include "gemm_tile_f32.h"

namespace iris {
namespace vae {

// keras.ops.gelu default (approximate=True): 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))
__device__ __forceinline__ float gelu_tanh(float x) {
    const float u = 0.7978845608028654f * (x + 0.044715f * (x * x * x));
    return 0.5f * x * (1.f + tanhf(u));
}

struct GemmLaunch {
    const float* x;       // input  [B, L_in, C_in] channels-last
    const f32x4* wp;      // packed weights (pack_conv1d_weights), Gp groups x n_ct C_out tiles per tap
    const float* bias;    // [C_out]
    float* y;             // output [B, L_out, C_out], or [B, C_out, L_out] when y_channels_first
    const float* film;    // FiLM rows [B * L_out, ld_film]: gamma at column gamma_off + co, beta at beta_off + co; or nullptr
    const f32x4* wp2;     // FUSED: packed 1x1 weights C_out -> C_out (same n_ct, Gp2 groups)
    const float* bias2;   // FUSED: [C_out]
    const float* res;     // FUSED: residual [B, L_out, C_out] added after the second GEMM
    int L_in, L_out, C_in, C_out;
    int ks, dil, stride, pad_left;
    int up;               // 1: the conv runs over the x2 nearest-neighbour repeat of x (2 * L_in virtual rows)
    int Gp, n_ct, Gp2;
    int gelu;             // 1: GELU on (acc + bias), before FiLM
    int ld_film, gamma_off, beta_off;
    int y_channels_first;
    // RAGGED only
    const int32_t* lengths;   // [B] frames of each item at the full rate (device), sanitised by item_frames()
    int len_T, len_shift;     // the padded frame count T and down_stages
    int sh_in, sh_out;        // item rows of x: item_frames >> sh_in (before `up`); of y: item_frames >> sh_out
    int zero_tail;            // 1: rows [item rows, L_out) of y are stored as 0.0f (out_proj, residual_proj)
    // kGemmSplitOut only
    float* y2;                // columns [split, C_out) go to y2 [B, L_out, C_out - split]; columns [0, split) to y [B, L_out, split]
    int split;                // a multiple of 4 (checked on the host)
};

// Forms of vae_gemm_kernel beside the plain one (posterior encoder, vae_encoder.h).  The plain form contains none of them.
//   kGemmMelIn:    x is channels-first, [B, C_in, L_in] (the mel as the PostNet and the vocoder hold it): the staging loop
//                  runs lanes along time, so a half-wave reads the block's 32 consecutive frames of one channel (128 bytes)
//                  and writes them down an LDS column.  ks = stride = 1, no `up` (checked on the host).
//   kGemmSplitOut: the output columns are two contiguous tensors, y and y2 (the latent heads: mean | logvar).
constexpr int kGemmPlain = 0, kGemmMelIn = 1, kGemmSplitOut = 2;

// Frames of item b: lengths[b] clamped to [0, T], then rounded down to a multiple of 2^S -- the stride-2 'same' rule (pad 1
// left, 2 right) holds for even lengths only, and a multiple of 2^S is even at every level.
__device__ __forceinline__ int item_frames(const int32_t* __restrict__ lengths, int b, int T, int S) {
    int len = lengths[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    return (len >> S) << S;
}

// zero_tail: row t of item b (t < L_out, past the item's rows) of this wave's C_out tile as 0.0f, in y's layout (FORM ==
// kGemmSplitOut: in the layout of the y | y2 pair)
template <int FORM>
__device__ __forceinline__ void store_zero_row(const GemmLaunch& a, int b, int ct, int t, int hi) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = ct * 32 + 8 * g + 4 * hi;
        if constexpr (FORM == kGemmSplitOut) {
            if (co < a.C_out) {                            // split % 4 == 0: the group lies on one side of it
                const size_t row = (size_t)b * a.L_out + t;
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                float* dst = co < a.split ? a.y + row * a.split + co : a.y2 + row * (a.C_out - a.split) + (co - a.split);
                *reinterpret_cast<f32x4*>(dst) = zero;
            }
        } else if (a.y_channels_first) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (co + e < a.C_out) a.y[((size_t)b * a.C_out + co + e) * a.L_out + t] = 0.f;
        } else if (co < a.C_out) {                         // C_out % 4 == 0 (checked on the host)
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(a.y + ((size_t)b * a.L_out + t) * a.C_out + co) = zero;
        }
    }
}

constexpr int kGemmRows = 32;        // output rows of a block
constexpr int kGemmMaxWaves = 8;     // C_out tiles of a block

inline int gemm_window_rows(int ks, int dil, int stride) { return (kGemmRows - 1) * stride + (ks - 1) * dil + 1; }
inline size_t gemm_lds_bytes(int C_in, int C_out, int ks, int dil, int stride, bool fused) {
    size_t f = (size_t)gemm_window_rows(ks, dil, stride) * lds_row_floats(C_in);
    if (fused) f += (size_t)kGemmRows * lds_row_floats(C_out);
    return f * sizeof(float);
}

template <bool FUSED, bool RAGGED, int FORM = kGemmPlain>
__global__ void __launch_bounds__(64 * kGemmMaxWaves) vae_gemm_kernel(const GemmLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z;
    const int i0 = blockIdx.x * kGemmRows;
    const int ct = blockIdx.y * nw + wave;                 // this wave's 32-wide C_out tile
    const bool active = ct < a.n_ct;                       // wave-uniform
    const int Cp = (a.C_in + 7) & ~7, S = Cp + 4;
    const int R = (kGemmRows - 1) * a.stride + (a.ks - 1) * a.dil + 1;
    const int v0 = i0 * a.stride - a.pad_left;             // first (virtual) input row of the window
    int Lb_in = a.L_in, Lb_out = a.L_out;                  // the item's rows: bounds, never strides
    if constexpr (RAGGED) {
        const int len = item_frames(a.lengths, b, a.len_T, a.len_shift);
        Lb_in = len >> a.sh_in;
        Lb_out = len >> a.sh_out;
        if (i0 >= Lb_out) {                                // block-uniform, before the first barrier
            if (!FUSED && a.zero_tail && active && i0 + lo < a.L_out) store_zero_row<FORM>(a, b, ct, i0 + lo, hi);
            return;
        }
    }
    const int Lv = a.up ? 2 * Lb_in : Lb_in;

    if constexpr (FORM == kGemmMelIn) {
        // stage the window from [B, C_in, L_in]: idx -> (channel, row) with the row fastest, 0 outside [0, Lv) and past C_in
        const int total = R * Cp;
        for (int idx = tid; idx < total; idx += nthr) {
            const int ci = idx / R, r = idx - ci * R;
            const int v = v0 + r;
            float val = 0.f;
            if (v >= 0 && v < Lv && ci < a.C_in) val = a.x[((size_t)b * a.C_in + ci) * a.L_in + v];
            lds[r * S + ci] = val;
        }
    } else {   // stage the window: virtual row v of the item is row v >> up of x, 0 outside [0, Lv)
        const int QPR = Cp >> 2, total = R * QPR;
        for (int idx = tid; idx < total; idx += nthr) {
            const int r = idx / QPR, q = idx - r * QPR;
            const int v = v0 + r, ci = 4 * q;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (v >= 0 && v < Lv && ci < a.C_in) {
                const int src = a.up ? (v >> 1) : v;
                val = *reinterpret_cast<const f32x4*>(a.x + ((size_t)b * a.L_in + src) * a.C_in + ci);
            }
            *reinterpret_cast<f32x4*>(lds + r * S + ci) = val;
        }
    }
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (active)
        mma_loop(acc, lds + lo * a.stride * S + 4 * hi, a.dil * S, a.wp + (size_t)ct * 64 + lane, (size_t)a.n_ct * 64, a.Gp,
                 a.ks, Cp >> 3);

    // Epilogue.  D[co][t]: lane & 31 = time row, registers 4g .. 4g+3 = channels ct*32 + 8g + 4*(lane >> 5) + {0..3}.
    const int t = i0 + lo;
    const bool ok = active && t < Lb_out;
    const size_t row = (size_t)b * a.L_out + (ok ? t : 0);
    if (active) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + 8 * g + 4 * hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.f;
                if (co + e < a.C_out) {
                    v = acc[4 * g + e] + a.bias[co + e];
                    if (a.gelu) v = gelu_tanh(v);
                    if (a.film && ok) {
                        const float* f = a.film + row * a.ld_film + co + e;
                        v = f[a.gamma_off] * v + f[a.beta_off];
                    }
                }
                acc[4 * g + e] = v;
            }
        }
    }

    if constexpr (FUSED) {
        // the FiLM'ed tile h [32, C_out] -> LDS (behind the window), then y = x + res_proj(h)
        const int Cp2 = (a.C_out + 7) & ~7, S2 = Cp2 + 4;
        float* hl = lds + R * S;
        if (active) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct * 32 + 8 * g + 4 * hi;
                if (co < Cp2) {
                    const f32x4 v = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                    *reinterpret_cast<f32x4*>(hl + lo * S2 + co) = v;
                }
            }
        }
        __syncthreads();
        f32x16 acc2;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
        if (active)
            mma_loop(acc2, hl + lo * S2 + 4 * hi, 0, a.wp2 + (size_t)ct * 64 + lane, (size_t)a.n_ct * 64, a.Gp2, 1, Cp2 >> 3);
        if (ok) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct * 32 + 8 * g + 4 * hi;
                if (co < a.C_out) {
                    const f32x4 r4 = *reinterpret_cast<const f32x4*>(a.res + row * a.C_out + co);
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(a.bias2 + co);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc2[4 * g + e] = r4[e] + (acc2[4 * g + e] + b4[e]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ok) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = ct * 32 + 8 * g + 4 * hi;
                if (co < a.C_out) {
                    const f32x4 v = {acc2[4 * g + 0], acc2[4 * g + 1], acc2[4 * g + 2], acc2[4 * g + 3]};
                    *reinterpret_cast<f32x4*>(a.y + row * a.C_out + co) = v;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    } else {
        __builtin_amdgcn_sched_barrier(0);
        if (ok) {
            if constexpr (FORM == kGemmSplitOut) {
                // a group of 4 columns lies on one side of `split` (split % 4 == 0): one 16-byte store into y or y2
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = ct * 32 + 8 * g + 4 * hi;
                    if (co < a.C_out) {
                        const f32x4 v = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                        float* dst = co < a.split ? a.y + row * a.split + co : a.y2 + row * (a.C_out - a.split) + (co - a.split);
                        *reinterpret_cast<f32x4*>(dst) = v;
                    }
                }
            } else if (a.y_channels_first) {
                // [B, C_out, L_out]: the 32 lanes of a half-wave store 32 consecutive frames of one channel
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int co = ct * 32 + 8 * g + 4 * hi + e;
                        if (co < a.C_out) a.y[((size_t)b * a.C_out + co) * a.L_out + t] = acc[4 * g + e];
                    }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = ct * 32 + 8 * g + 4 * hi;
                    if (co < a.C_out) {                    // C_out % 4 == 0 (checked on the host)
                        const f32x4 v = {acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                        *reinterpret_cast<f32x4*>(a.y + row * a.C_out + co) = v;
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RAGGED) {
            if (a.zero_tail && active && t >= Lb_out && t < a.L_out) store_zero_row<FORM>(a, b, ct, t, hi);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Reverse flow + latent_dec_proj.
// Per coupling j the weights lie in Keras layouts, in this order (flow_coupling_floats):
//   net_pre.kernel [3][half][FH], net_pre.bias [FH], net_post.kernel [FH][half], net_post.bias [half],
//   film.proj.kernel [half][2 half], film.proj.bias [2 half]
// cond_proj(lat_cond) of every coupling (before its GELU) is a column block of the conditioning GEMM's output.
struct FlowLaunch {
    const float* z;        // z_prior [B, Tq, latent]
    const float* cond;     // conditioning GEMM output [B * Tq, ld]; coupling j's cond_proj at column ce_off + j * ce_stride
    const float* w;        // couplings, flow_coupling_floats() apart
    const float* wdec;     // latent_dec_proj kernel [latent][C], then bias [C]
    float* y;              // [B, Tq, C]
    int Tq, latent, FH, n_flow, C, ld, ce_off, ce_stride;
    // RAGGED only: item b has item_frames(lengths, b, len_T, len_shift) >> len_shift latent rows
    const int32_t* lengths;
    int len_T, len_shift;
};

constexpr int kFlowRows = 16;
__host__ __device__ inline size_t flow_coupling_floats(int half, int FH) {
    return (size_t)3 * half * FH + FH + (size_t)FH * half + half + (size_t)half * 2 * half + 2 * half;
}
inline size_t flow_lds_bytes(int latent, int FH) {
    const int half = latent / 2;
    return ((size_t)kFlowRows * latent + 2 * (size_t)(kFlowRows + 2) * half + (size_t)kFlowRows * FH) * sizeof(float);
}

template <bool RAGGED, bool FORWARD = false>
__global__ void __launch_bounds__(256) vae_flow_kernel(const FlowLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int TT = kFlowRows;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int b = blockIdx.y, r0 = blockIdx.x * TT;
    const int latent = a.latent, half = latent >> 1, FH = a.FH, Tq = a.Tq;   // Tq: the row stride of an item
    int Tb = Tq;                                                              // the item's rows: the bound
    if constexpr (RAGGED) {
        Tb = item_frames(a.lengths, b, a.len_T, a.len_shift) >> a.len_shift;
        if (r0 >= Tb) return;                                                 // block-uniform, before the first barrier
    }
    float* zt = lds;                              // [TT][latent]      the tile of z (x1 | x2)
    float* ce = zt + TT * latent;                 // [TT + 2][half]    gelu(cond_proj(lat_cond)), rows r0 - 1 ..
    float* hin = ce + (TT + 2) * half;            // [TT + 2][half]    x1 + ce, 0 outside the item ('same' padding)
    float* hid = hin + (TT + 2) * half;           // [TT][FH]          gelu(net_pre(hin))
    const size_t per = flow_coupling_floats(half, FH);

    for (int idx = tid; idx < TT * latent; idx += nthr) {
        const int r = idx / latent, c = idx - r * latent, t = r0 + r;
        zt[idx] = t < Tb ? a.z[((size_t)b * Tq + t) * latent + c] : 0.f;
    }
    // reverse: reversed(layers_list), vae.py:237-239; FORWARD: couplings 0 .. n - 1, vae.py:240-242
    for (int jj = FORWARD ? 0 : a.n_flow - 1; FORWARD ? jj < a.n_flow : jj >= 0; jj += FORWARD ? 1 : -1) {
        const float* wpre = a.w + (size_t)jj * per;
        const float* bpre = wpre + 3 * half * FH;
        const float* wpost = bpre + FH;
        const float* bpost = wpost + FH * half;
        const float* wfilm = bpost + half;
        const float* bfilm = wfilm + half * 2 * half;
        __syncthreads();
        for (int idx = tid; idx < (TT + 2) * half; idx += nthr) {
            const int r = idx / half, c = idx - r * half, t = r0 - 1 + r;
            float cev = 0.f, hv = 0.f;
            if (t >= 0 && t < Tb) {
                const size_t grow = (size_t)b * Tq + t;
                cev = gelu_tanh(a.cond[grow * a.ld + a.ce_off + jj * a.ce_stride + c]);
                hv = a.z[grow * latent + c] + cev;                   // x1 is z_prior's first half in every coupling
            }
            ce[idx] = cev;
            hin[idx] = hv;
        }
        __syncthreads();
        for (int idx = tid; idx < TT * FH; idx += nthr) {
            const int r = idx / FH, f = idx - r * FH;
            float acc = bpre[f];
            for (int kap = 0; kap < 3; ++kap)
                for (int c = 0; c < half; ++c)
                    acc = fmaf(hin[(r + kap) * half + c], wpre[(kap * half + c) * FH + f], acc);
            hid[idx] = gelu_tanh(acc);
        }
        __syncthreads();
        for (int idx = tid; idx < TT * half; idx += nthr) {
            const int r = idx / half, c = idx - r * half;
            float tv = bpost[c];
            for (int f = 0; f < FH; ++f) tv = fmaf(hid[r * FH + f], wpost[f * half + c], tv);
            float gam = bfilm[c], bet = bfilm[half + c];
            for (int k = 0; k < half; ++k) {
                const float cv = ce[(r + 1) * half + k];
                gam = fmaf(cv, wfilm[k * 2 * half + c], gam);
                bet = fmaf(cv, wfilm[k * 2 * half + half + c], bet);
            }
            if constexpr (FORWARD) zt[r * latent + half + c] += gam * tv + bet;   // y2 = x2 + t, vae.py:205-206
            else zt[r * latent + half + c] -= gam * tv + bet;        // y2 = x2 - t (reverse), vae.py:203-204
        }
    }
    __syncthreads();
    const float* bdec = a.wdec + (size_t)latent * a.C;
    for (int idx = tid; idx < TT * a.C; idx += nthr) {
        const int r = idx / a.C, co = idx - r * a.C, t = r0 + r;
        if (t >= Tb) continue;
        float acc = bdec[co];
        for (int l = 0; l < latent; ++l) acc = fmaf(zt[r * latent + l], a.wdec[(size_t)l * a.C + co], acc);
        a.y[((size_t)b * Tq + t) * a.C + co] = acc;
    }
}

#ifndef IRIS_KERNELS_ONLY
// Fills Gp / n_ct and launches.  FUSED launches need every C_out tile in one block (C_out <= 32 * kGemmMaxWaves).
inline hipError_t launch_gemm(GemmLaunch& a, int B, bool fused, hipStream_t stream, int form = kGemmPlain) {
    if (a.C_in < 1 || a.C_out < 1) return hipErrorInvalidValue;   // no C_out tile: no wave, and the grid below divides by the waves
    a.Gp = packed_groups(a.C_in);
    a.n_ct = packed_cotiles(a.C_out);
    a.Gp2 = packed_groups(a.C_out);
    const int nw = a.n_ct < kGemmMaxWaves ? a.n_ct : kGemmMaxWaves;
    if (fused && a.n_ct > kGemmMaxWaves) return hipErrorInvalidValue;
    const size_t lds_bytes = gemm_lds_bytes(a.C_in, a.C_out, a.ks, a.dil, a.stride, fused);
    if (lds_bytes > 160 * 1024) return hipErrorInvalidValue;
    dim3 grid((unsigned)((a.L_out + kGemmRows - 1) / kGemmRows), (unsigned)((a.n_ct + nw - 1) / nw), (unsigned)B);
    dim3 block((unsigned)(64 * nw));
    if (form != kGemmPlain) {                              // unfused forms of the posterior encoder
        if (fused || a.up || a.y_channels_first) return hipErrorInvalidValue;
        if (form == kGemmMelIn) {
            if (a.ks != 1 || a.stride != 1 || a.pad_left != 0) return hipErrorInvalidValue;
            if (a.lengths)
                return launch_kernel_named("vae_gemm_kernel_ragged<mel_in>", vae_gemm_kernel<false, true, kGemmMelIn>, grid, block, lds_bytes, stream, a);
            return launch_kernel_named("vae_gemm_kernel<mel_in>", vae_gemm_kernel<false, false, kGemmMelIn>, grid, block, lds_bytes, stream, a);
        }
        if (form != kGemmSplitOut || !a.y2 || a.split <= 0 || a.split >= a.C_out || (a.split & 3)) return hipErrorInvalidValue;
        if (a.lengths)
            return launch_kernel_named("vae_gemm_kernel_ragged<split_out>", vae_gemm_kernel<false, true, kGemmSplitOut>, grid, block, lds_bytes, stream, a);
        return launch_kernel_named("vae_gemm_kernel<split_out>", vae_gemm_kernel<false, false, kGemmSplitOut>, grid, block, lds_bytes, stream, a);
    }
    if (a.lengths) {
        if (fused) return launch_kernel_named("vae_gemm_kernel_ragged<fused>", vae_gemm_kernel<true, true>, grid, block, lds_bytes, stream, a);
        return launch_kernel_named("vae_gemm_kernel_ragged", vae_gemm_kernel<false, true>, grid, block, lds_bytes, stream, a);
    }
    if (fused) return launch_kernel_named("vae_gemm_kernel<fused>", vae_gemm_kernel<true, false>, grid, block, lds_bytes, stream, a);
    return launch_kernel_named("vae_gemm_kernel", vae_gemm_kernel<false, false>, grid, block, lds_bytes, stream, a);
}

inline hipError_t launch_flow(const FlowLaunch& a, int B, hipStream_t stream, bool forward = false) {
    dim3 grid((unsigned)((a.Tq + kFlowRows - 1) / kFlowRows), (unsigned)B), block(256);
    if (forward) {
        if (a.lengths)
            return launch_kernel_named("vae_flow_kernel_ragged<forward>", vae_flow_kernel<true, true>, grid, block, flow_lds_bytes(a.latent, a.FH), stream, a);
        return launch_kernel_named("vae_flow_kernel<forward>", vae_flow_kernel<false, true>, grid, block, flow_lds_bytes(a.latent, a.FH), stream, a);
    }
    if (a.lengths)
        return launch_kernel_named("vae_flow_kernel_ragged", vae_flow_kernel<true>, grid, block, flow_lds_bytes(a.latent, a.FH), stream, a);
    return launch_kernel_named("vae_flow_kernel", vae_flow_kernel<false>, grid, block, flow_lds_bytes(a.latent, a.FH), stream, a);
}
#endif

}  // namespace vae
}  // namespace iris
