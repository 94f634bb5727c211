// iris_vae_encoder.hip -- the iris_vae_encoder_* entry points of include/iris_hifigan.h: the posterior encoder of the
// text-conditioned VAE (TextConditionedVAE.call at training=False up to the latent heads, src/iris/vae.py:381-398), built
// from the kernels of csrc/vae_decoder.h.  mel [B, n_mels, T] and frame conditioning [B, T, cond_dim] in, mean and logvar
// [B, T / 2^S, latent_dim] out.  The rest of call() -- forward flow and decoder -- is iris_vae_decoder_forward_posterior.
//
// Launches (N = num_wavenet_blocks, S = down_stages; N + S + 3 in all):
//   1          in_proj, 1x1, reading the channels-first mel (kGemmMelIn: no transposed copy of the mel exists)
//   2          every FiLM Dense(cond) of the encoder at once: N * 2C output columns of a 1x1 problem at the full frame rate
//   3 .. N+2   one fused WaveNet block each (conv -> GELU -> FiLM rows of launch 2 -> LDS -> res_proj -> + h)
//   next S     downsample.blocks[s] on h: k5 stride 2 'same' + GELU -- the weights the conditioning goes through in the decoder
//   last       latent_mean_proj | latent_logvar_proj as one GEMM of 2 * latent_dim columns, stored as two tensors (kGemmSplitOut)
//
// iris_vae_posterior_encode_ragged runs the same launches over the same grids and buffers with the RAGGED instantiations
// ("Ragged form", vae_decoder.h): every launch is bounded by its items' own rows at its level, and the last one stores
// mean | logvar rows past an item's latent rows as 0.0f.
//
// The iris_vae_losses* entry points (csrc/vae_losses.h) are here too: the masked reconstruction L1 and KL of a
// reconstruction, reduced on the device from the tensors the two posterior forwards leave there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "stage_host.h"
#include "vae_decoder.h"
#include "vae_losses.h"

using namespace iris;

struct iris_vae_encoder_handle : StageHandle {
    iris_vae_encoder_config cfg;
    PackedGemm in_proj, film_gemm, heads;
    std::vector<PackedGemm> conv, res, down;
    int film_cols = 0;                               // N * 2C: block i's gamma at 2C i, its beta at 2C i + C
};

namespace {

int enc_validate(const iris_vae_encoder_config* c) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->n_mels < 1 || c->cond_dim < 1 || c->model_channels < 1 || c->latent_dim < 1 || c->num_wavenet_blocks < 0 ||
        c->wavenet_kernel_size < 1 || c->down_stages < 0)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "VAE encoder sizes must be positive");
    if ((c->n_mels & 3) || (c->cond_dim & 3) || (c->model_channels & 3) || (c->latent_dim & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "n_mels %d, cond_dim %d, model_channels %d and latent_dim %d must be multiples of 4 "
                    "(16-byte rows)", c->n_mels, c->cond_dim, c->model_channels, c->latent_dim);
    if (c->model_channels > 32 * vae::kGemmMaxWaves)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "model_channels %d exceeds %d (one block holds a WaveNet block's whole row)",
                    c->model_channels, 32 * vae::kGemmMaxWaves);
    if (!(c->wavenet_kernel_size & 1))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "wavenet_kernel_size %d must be odd (symmetric 'same' padding)", c->wavenet_kernel_size);
    if (c->down_stages > 8 || c->num_wavenet_blocks > 64 || c->latent_dim > 256 || c->n_mels > 1024)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "down_stages <= 8, num_wavenet_blocks <= 64, latent_dim <= 256, n_mels <= 1024");
    const int C = c->model_channels;
    const int dmax = c->num_wavenet_blocks >= 4 ? 8 : (1 << (c->num_wavenet_blocks > 0 ? c->num_wavenet_blocks - 1 : 0));
    const size_t lds_max = 160 * 1024;
    if (vae::gemm_lds_bytes(C, C, c->wavenet_kernel_size, dmax, 1, true) > lds_max || vae::gemm_lds_bytes(C, C, 5, 1, 2, false) > lds_max ||
        vae::gemm_lds_bytes(c->cond_dim, C, 1, 1, 1, false) > lds_max || vae::gemm_lds_bytes(c->n_mels, C, 1, 1, 1, false) > lds_max)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "a tile of this configuration does not fit the 160 KB LDS");
    return IRIS_HIFIGAN_OK;
}

uint64_t enc_weight_count(const iris_vae_encoder_config& c) {
    const uint64_t C = c.model_channels, k = c.wavenet_kernel_size;
    uint64_t n = C * c.n_mels + C;                                              // in_proj
    n += (uint64_t)c.num_wavenet_blocks * ((C * C * k + C) + (2 * C * c.cond_dim + 2 * C) + (C * C + C));
    n += (uint64_t)c.down_stages * (C * C * 5 + C);                             // downsample.blocks
    n += 2 * ((uint64_t)c.latent_dim * C + c.latent_dim);                       // latent_mean_proj, latent_logvar_proj
    return n;
}

struct EncWs { size_t film, h0, ha, hb, d[2], total; };   // float offsets; every buffer starts on 256 bytes

EncWs enc_ws(const iris_vae_encoder_handle* h, int B, int T) {
    const size_t C = h->cfg.model_channels, frames = (size_t)B * T;
    EncWs w;
    WsTaker t;
    w.film = t.take(frames * h->film_cols);
    w.h0 = t.take(frames * C); w.ha = t.take(frames * C); w.hb = t.take(frames * C);
    w.d[0] = t.take((frames >> 1) * C); w.d[1] = t.take((frames >> 2) * C);
    w.total = t.off;
    return w;
}

// where h lies after the last encoder block (h0 -> ha -> hb -> ha ...), and where lat_h = downsample(h) lies
size_t enc_h_out(const iris_vae_encoder_handle* h, const EncWs& w) {
    const int N = h->cfg.num_wavenet_blocks;
    return N == 0 ? w.h0 : (((N - 1) & 1) ? w.hb : w.ha);
}
size_t enc_lat_h(const iris_vae_encoder_handle* h, const EncWs& w) {
    const int S = h->cfg.down_stages;
    return S == 0 ? enc_h_out(h, w) : w.d[(S - 1) & 1];
}

int enc_check_shape(const iris_vae_encoder_handle* h, int32_t B, int32_t T) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (T & ((1 << h->cfg.down_stages) - 1))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "T = %d is not a multiple of 2^down_stages = %d (pad the mel and the conditioning first)",
                    T, 1 << h->cfg.down_stages);
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.z)", B);
    if ((uint64_t)B * T * (uint64_t)h->cfg.model_channels > 0x7fffffffull * 64)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B * T too large");
    return IRIS_HIFIGAN_OK;
}

// Queues the launches of one forward (or, in a dry run, counts them).  `lengths` (device, or nullptr for the dense forward)
// selects the ragged kernels, as in vae_forward (iris_vae_decoder.hip): sh_in / sh_out count the halvings of a launch's input
// and output below the full rate.
int enc_forward(iris_vae_encoder_handle* h, const float* mel, const float* cond, int B, int T, const int32_t* lengths, float* mean,
                float* logvar, float* ws, hipStream_t stream) {
    const iris_vae_encoder_config& c = h->cfg;
    const int C = c.model_channels, S = c.down_stages, Tq = T >> S;
    const EncWs w = enc_ws(h, B, T);
    const float* blob = h->blob;
    auto gemm = [&](const float* x, const PackedGemm& l, float* y, int L_in, int L_out, int sh_in, int sh_out) {
        vae::GemmLaunch a; memset(&a, 0, sizeof(a));
        a.lengths = lengths; a.len_T = T; a.len_shift = S; a.sh_in = sh_in; a.sh_out = sh_out;
        a.x = x; a.wp = (const f32x4*)(blob + l.w_off); a.bias = blob + l.b_off; a.y = y;
        a.L_in = L_in; a.L_out = L_out; a.C_in = l.C_in; a.C_out = l.C_out;
        a.ks = l.k; a.dil = 1; a.stride = 1; a.pad_left = (l.k - 1) / 2;
        return a;
    };
    {   // h = in_proj(mels^T): the transpose is the staging loop's                           vae.py:382-385
        vae::GemmLaunch a = gemm(mel, h->in_proj, ws + w.h0, T, T, 0, 0);
        HIP_TRY(vae::launch_gemm(a, B, false, stream, vae::kGemmMelIn));
    }
    if (c.num_wavenet_blocks > 0) {   // FiLM rows of every block, from the full-rate conditioning         vae.py:21-29
        vae::GemmLaunch a = gemm(cond, h->film_gemm, ws + w.film, T, T, 0, 0);
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    const float* x = ws + w.h0;
    for (int i = 0; i < c.num_wavenet_blocks; ++i) {                                         // vae.py:57-67, 388-389
        float* y = ws + ((i & 1) ? w.hb : w.ha);
        vae::GemmLaunch a = gemm(x, h->conv[i], y, T, T, 0, 0);
        a.dil = 1 << (i % 4); a.pad_left = a.dil * (a.ks - 1) / 2; a.gelu = 1;
        a.film = ws + w.film; a.ld_film = h->film_cols; a.gamma_off = i * 2 * C; a.beta_off = i * 2 * C + C;
        a.wp2 = (const f32x4*)(blob + h->res[i].w_off); a.bias2 = blob + h->res[i].b_off; a.res = x;
        HIP_TRY(vae::launch_gemm(a, B, true, stream));
        x = y;
    }
    for (int s = 0; s < S; ++s) {                                                            // lat_h = downsample(h), vae.py:393
        float* y = ws + w.d[s & 1];
        vae::GemmLaunch a = gemm(x, h->down[s], y, T >> s, T >> (s + 1), s, s + 1);
        a.stride = 2; a.pad_left = 1; a.gelu = 1;
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
        x = y;
    }
    {   // mean | logvar = latent_mean_proj(lat_h) | latent_logvar_proj(lat_h)                vae.py:396-397
        vae::GemmLaunch a = gemm(x, h->heads, mean, Tq, Tq, S, S);
        a.y2 = logvar; a.split = c.latent_dim;
        a.zero_tail = 1;                                                                    // ragged: mean | logvar [b, len_b >> S:] = 0
        HIP_TRY(vae::launch_gemm(a, B, false, stream, vae::kGemmSplitOut));
    }
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_vae_encoder_weight_count(const iris_vae_encoder_config* cfg, uint64_t* count) {
    if (!count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    *count = enc_weight_count(*cfg);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_encoder_create(const iris_vae_encoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                iris_vae_encoder_handle** out) {
    IRIS_ABI_BEGIN
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    const uint64_t expect = enc_weight_count(*cfg);
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, the VAE encoder needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    std::unique_ptr<iris_vae_encoder_handle> h(new (std::nothrow) iris_vae_encoder_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    const iris_vae_encoder_config& c = h->cfg;
    const int C = c.model_channels, N = c.num_wavenet_blocks, L = c.latent_dim;
    h->film_cols = N * 2 * C;
    BlobBuilder bb(weights_host);
    bb.dense(h->in_proj, c.n_mels, C, 1);
    h->conv.resize(N); h->res.resize(N); h->down.resize(c.down_stages);
    // the FiLM GEMM: rows = output columns [film_cols][cond_dim], block i at 2C i
    std::vector<float> fw((size_t)h->film_cols * c.cond_dim, 0.f), fb(h->film_cols, 0.f);
    for (int i = 0; i < N; ++i) {
        bb.dense(h->conv[i], C, C, c.wavenet_kernel_size);
        bb.take(fw.data() + (size_t)i * 2 * C * c.cond_dim, (size_t)2 * C * c.cond_dim);
        bb.take(fb.data() + (size_t)i * 2 * C, 2 * C);
        bb.dense(h->res[i], C, C, 1);
    }
    for (auto& l : h->down) bb.dense(l, C, C, 5);
    // the heads: mean's rows, then logvar's
    std::vector<float> hw((size_t)2 * L * C), hb(2 * L);
    for (int half = 0; half < 2; ++half) {
        bb.take(hw.data() + (size_t)half * L * C, (size_t)L * C);
        bb.take(hb.data() + half * L, L);
    }
    bb.dense(h->film_gemm, fw.data(), fb.data(), c.cond_dim, h->film_cols, 1);
    bb.dense(h->heads, hw.data(), hb.data(), C, 2 * L, 1);
    TRY(upload(bb.host, h.get(), "VAE encoder"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_vae_encoder_destroy(iris_vae_encoder_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_encoder_workspace_bytes(const iris_vae_encoder_handle* h, int32_t B, int32_t T, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_check_shape(h, B, T));
    *bytes = (uint64_t)enc_ws(h, B, T).total * sizeof(float);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_encoder_tap(const iris_vae_encoder_handle* h, int32_t B, int32_t T, int32_t which, uint64_t* byte_offset,
                             uint64_t* floats) {
    if (!byte_offset || !floats) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_check_shape(h, B, T));
    const EncWs w = enc_ws(h, B, T);
    uint64_t rows = (uint64_t)B * T;
    size_t off;
    if (which == IRIS_VAE_ENC_TAP_H_IN) off = w.h0;
    else if (which == IRIS_VAE_ENC_TAP_H_OUT) off = enc_h_out(h, w);
    else if (which == IRIS_VAE_ENC_TAP_LAT_H) { off = enc_lat_h(h, w); rows >>= h->cfg.down_stages; }
    else return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "unknown tap %d", which);
    *byte_offset = (uint64_t)off * sizeof(float);
    *floats = rows * h->cfg.model_channels;
    return IRIS_HIFIGAN_OK;
}

// The dense and the ragged entry point: the same checks in the same order, then the same plan.
static int32_t enc_forward_checked(iris_vae_encoder_handle* h, const float* mel_dev, const float* cond_dev, int32_t B, int32_t T,
                                   bool ragged, const int32_t* lengths_dev, float* mean_out_dev, float* logvar_out_dev,
                                   void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(enc_check_shape(h, B, T));
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (!mel_dev || !cond_dev || !mean_out_dev || !logvar_out_dev || !workspace_dev)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (ragged && !lengths_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "lengths_dev is NULL");
    ForwardScope scope(*h, workspace_bytes, enc_ws(h, B, T).total);
    TRY(scope.rc);
    return enc_forward(h, mel_dev, cond_dev, B, T, ragged ? lengths_dev : nullptr, mean_out_dev, logvar_out_dev,
                       (float*)workspace_dev, (hipStream_t)stream_);
    IRIS_ABI_END
}

int32_t iris_vae_encoder_forward(iris_vae_encoder_handle* h, const float* mel_dev, const float* cond_dev, int32_t B, int32_t T,
                                 float* mean_out_dev, float* logvar_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                 void* stream_) {
    return enc_forward_checked(h, mel_dev, cond_dev, B, T, false, nullptr, mean_out_dev, logvar_out_dev, workspace_dev,
                               workspace_bytes, stream_);
}

int32_t iris_vae_posterior_encode_ragged(iris_vae_encoder_handle* h, const float* mel_dev, const float* cond_dev, int32_t B, int32_t T,
                                        const int32_t* lengths_dev, float* mean_out_dev, float* logvar_out_dev, void* workspace_dev,
                                        uint64_t workspace_bytes, void* stream_) {
    return enc_forward_checked(h, mel_dev, cond_dev, B, T, true, lengths_dev, mean_out_dev, logvar_out_dev, workspace_dev,
                               workspace_bytes, stream_);
}

// ------------------------------------------------------------------------------------------------
// Masked reconstruction L1 and KL of a reconstruction (csrc/vae_losses.h)
// ------------------------------------------------------------------------------------------------
static int losses_check_shape(int32_t B, int32_t n_mels, int32_t T, int32_t latent_dim, int32_t down_stages) {
    if (B < 0 || T < 0 || n_mels < 1 || latent_dim < 1 || down_stages < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "bad loss shape");
    if (down_stages > 8) return fail(IRIS_HIFIGAN_UNSUPPORTED, "down_stages <= 8");
    if (T & ((1 << down_stages) - 1))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "T = %d is not a multiple of 2^down_stages = %d", T, 1 << down_stages);
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.y)", B);
    if ((uint64_t)B * T * (uint64_t)(n_mels > latent_dim ? n_mels : latent_dim) > 0x7fffffffull * 64)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B * T too large");
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_losses_workspace_bytes(int32_t B, int32_t n_mels, int32_t T, int32_t latent_dim, int32_t down_stages, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(losses_check_shape(B, n_mels, T, latent_dim, down_stages));
    *bytes = vae::loss_workspace_doubles(B, T, down_stages, latent_dim) * sizeof(double);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_losses(const float* target_dev, const float* recon_dev, const float* mean_dev, const float* logvar_dev, int32_t B,
                        int32_t n_mels, int32_t T, int32_t latent_dim, int32_t down_stages, const int32_t* lengths_dev,
                        float* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(losses_check_shape(B, n_mels, T, latent_dim, down_stages));
    const uint64_t need = vae::loss_workspace_doubles(B, T, down_stages, latent_dim) * sizeof(double);
    if (!out_dev || (need && !workspace_dev) || (B > 0 && T > 0 && (!target_dev || !recon_dev || !mean_dev || !logvar_dev)))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if ((uintptr_t)workspace_dev & 7) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "workspace_dev must be aligned to 8 bytes");
    TRY(ForwardScope::check_workspace(workspace_bytes, need));
    vae::LossLaunch a; memset(&a, 0, sizeof(a));
    a.target = target_dev; a.recon = recon_dev; a.mean = mean_dev; a.logvar = logvar_dev; a.lengths = lengths_dev; a.out = out_dev;
    a.B = B; a.n_mels = n_mels; a.T = T; a.latent = latent_dim; a.S = down_stages;
    HIP_TRY(vae::launch_losses(a, (double*)workspace_dev, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_vae_encoder_launch_count(const iris_vae_encoder_handle* h, int32_t B, int32_t T, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_check_shape(h, B, T));
    *n = 0;
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    return count_launches([&](float* fake) {
        return enc_forward(const_cast<iris_vae_encoder_handle*>(h), fake, fake, B, T, nullptr, fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

}  // extern "C"
