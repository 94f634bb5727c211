// packed_conv_f32.h -- what every fp32 MFMA translation unit shares with conv_mfma_f32.h: the register vector types and the
// host-side repacking of a Conv1d weight into v_mfma_f32_32x32x2_f32 B-fragment order.  No kernel and no launch code.
#pragma once
#include <stddef.h>

namespace iris {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// Host side: weight repacking into B-fragment order.
//   packed[((kap*Gp + g)*n_ct + ct)*64 + lane] (an f32x4, component e)
//       = W[co = ct*32 + (lane&31)][ci = 8g + 4*(lane>>5) + e][kap]      (0 outside C_out/C_in)
// Gp = groups padded to a multiple of 8 (64 channels) so that any chunking of C_in stays inside.
inline int packed_groups(int C_in) { return ((C_in + 63) / 64) * 8; }
inline int packed_cotiles(int C_out) { return (C_out + 31) / 32; }
inline size_t packed_conv1d_floats(int C_in, int C_out, int ks) {
    return (size_t)ks * packed_groups(C_in) * packed_cotiles(C_out) * 64 * 4;
}

// w: reference Conv1d layout [C_out][C_in][ks] (hifigan_pretrained.py:50-57).
// Taps [kap0, kap1) only (kap1 < 0: all): the pieces are disjoint in `out`, so iris_hifigan_create packs them on several
// host threads (host_parallel.h).
inline void pack_conv1d_weights(const float* w, int C_in, int C_out, int ks, float* out, int kap0 = 0, int kap1 = -1) {
    const int Gp = packed_groups(C_in), n_ct = packed_cotiles(C_out);
    if (kap1 < 0 || kap1 > ks) kap1 = ks;
    for (int kap = kap0; kap < kap1; ++kap)
        for (int g = 0; g < Gp; ++g)
            for (int ct = 0; ct < n_ct; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int co = ct * 32 + (lane & 31);
                        const int ci = 8 * g + 4 * (lane >> 5) + e;
                        float v = 0.f;
                        if (co < C_out && ci < C_in) v = w[((size_t)co * C_in + ci) * ks + kap];
                        out[((((size_t)kap * Gp + g) * n_ct + ct) * 64 + lane) * 4 + e] = v;
                    }
}

}  // namespace iris
