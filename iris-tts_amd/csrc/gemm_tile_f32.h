// gemm_tile_f32.h -- what vae_gemm_kernel (vae_decoder.h) and txt_gemm_kernel (text_encoder.h) have in common: a wave
// multiplies 32 LDS rows by one 32-wide C_out tile of fragment-ordered weights (packed_conv_f32.h) on
// v_mfma_f32_32x32x2_f32.  No kernel lives here: staging loops and epilogues differ and stay with their kernels (so does the
// store of an accumulator row: as a shared function it changed vae_gemm_kernel's generated code).
#pragma once
#include <hip/hip_runtime.h>
#include "packed_conv_f32.h"

namespace iris {

// Floats of an LDS row that holds C channels: C rounded up to a group of 8, plus 4 = 4 * odd, conflict-free 16-byte rows.
inline int lds_row_floats(int C) { return ((C + 7) & ~7) + 4; }

// acc += A (32 rows x K, LDS) * W (K x 32, fragment order).  One group = 8 input channels of one tap = 4 MFMAs; the weight
// fragments run four groups ahead in registers, the LDS fragment one group ahead.
__device__ __forceinline__ void mma_loop(f32x16& acc, const float* abase, int tapstep, const f32x4* __restrict__ wlane,
                                         size_t wstep, int Gp, int ks, int gpc) {
    const int NG = ks * gpc;
    auto a_ptr = [&](int n) { const int kk = n / gpc, g = n - kk * gpc; return abase + kk * tapstep + 8 * g; };
    auto b_ptr = [&](int n) { const int kk = n / gpc, g = n - kk * gpc; return wlane + ((size_t)kk * Gp + g) * wstep; };
    constexpr int D = 4;
    f32x4 bw[D];
#pragma unroll
    for (int d = 0; d < D; ++d) bw[d] = *b_ptr(d < NG ? d : NG - 1);
    f32x4 av = *reinterpret_cast<const f32x4*>(a_ptr(0));
    for (int n0 = 0; n0 < NG; n0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int n = n0 + d;
            if (n < NG) {                                           // wave-uniform
                const f32x4 a_cur = av, b_cur = bw[d];
                av = *reinterpret_cast<const f32x4*>(a_ptr(n + 1 < NG ? n + 1 : n));
                bw[d] = *b_ptr(n + D < NG ? n + D : NG - 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b_cur[e], a_cur[e], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

}  // namespace iris
