// iris_vae_decoder.hip -- the iris_vae_decoder_* entry points of include/iris_hifigan.h over csrc/vae_decoder.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "stage_host.h"
#include "vae_decoder.h"

using namespace iris;

// ------------------------------------------------------------------------------------------------
// VAE decoder in front of the PostNet (TextConditionedVAE.generate, src/iris/vae.py:448-482; csrc/vae_decoder.h)
// ------------------------------------------------------------------------------------------------
struct iris_vae_decoder_handle : StageHandle {
    iris_vae_decoder_config cfg;
    PackedGemm cond_proj, out_proj, residual_proj, cond_gemm;
    std::vector<PackedGemm> down, up, dec_conv, dec_res;
    size_t flow_off = 0, dec_proj_off = 0;       // raw (Keras-layout) flow couplings; latent_dec_proj kernel + bias
    int film_cols = 0, ce_off = 0, ce_stride = 0;  // columns of the conditioning GEMM; where the couplings' cond_proj start
};

namespace {

int vae_validate(const iris_vae_decoder_config* c) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->n_mels < 1 || c->cond_dim < 1 || c->model_channels < 1 || c->latent_dim < 1 || c->decoder_blocks < 0 ||
        c->wavenet_kernel_size < 1 || c->down_stages < 0 || c->flow_layers < 0 || c->flow_hidden < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "VAE decoder sizes must be positive");
    if (c->latent_dim & 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "latent_dim %d must be even (vae.py:223)", c->latent_dim);
    if ((c->cond_dim & 3) || (c->model_channels & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "cond_dim %d and model_channels %d must be multiples of 4 (16-byte rows)",
                    c->cond_dim, c->model_channels);
    if (c->model_channels > 32 * vae::kGemmMaxWaves)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "model_channels %d exceeds %d (one block holds a WaveNet block's whole row)",
                    c->model_channels, 32 * vae::kGemmMaxWaves);
    if (!(c->wavenet_kernel_size & 1))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "wavenet_kernel_size %d must be odd (symmetric 'same' padding)", c->wavenet_kernel_size);
    if (c->down_stages > 8 || c->decoder_blocks > 64 || c->flow_layers > 64 || c->latent_dim > 256 || c->flow_hidden > 1024)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "down_stages <= 8, decoder_blocks, flow_layers <= 64, latent_dim <= 256, flow_hidden <= 1024");
    const int C = c->model_channels;
    const int dmax = c->decoder_blocks >= 4 ? 8 : (1 << (c->decoder_blocks > 0 ? c->decoder_blocks - 1 : 0));
    const size_t lds_max = 160 * 1024;
    if (vae::gemm_lds_bytes(C, C, c->wavenet_kernel_size, dmax, 1, true) > lds_max || vae::gemm_lds_bytes(C, C, 5, 1, 2, false) > lds_max ||
        vae::gemm_lds_bytes(c->cond_dim, C, 1, 1, 1, false) > lds_max || vae::flow_lds_bytes(c->latent_dim, c->flow_hidden) > 64 * 1024)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "a tile of this configuration does not fit the 160 KB LDS");
    return IRIS_HIFIGAN_OK;
}

uint64_t vae_weight_count(const iris_vae_decoder_config& c) {
    const uint64_t C = c.model_channels, half = c.latent_dim / 2, FH = c.flow_hidden, k = c.wavenet_kernel_size;
    uint64_t n = C * c.cond_dim + C;                                            // down_cond_proj
    n += (uint64_t)c.down_stages * (C * C * 5 + C);                             // downsample.blocks
    n += (uint64_t)c.flow_layers * (half * C + half + vae::flow_coupling_floats((int)half, (int)FH));
    n += (uint64_t)c.latent_dim * C + C;                                        // latent_dec_proj
    n += (uint64_t)c.decoder_blocks * ((C * C * k + C) + (2 * C * C + 2 * C) + (C * C + C));
    n += (uint64_t)c.down_stages * (C * C * 5 + C);                             // upsample.refine
    n += (uint64_t)c.n_mels * C + c.n_mels;                                     // out_proj
    n += (uint64_t)c.cond_dim * C + c.cond_dim;                                 // residual_proj
    return n;
}

struct VaeWs { size_t p, q, latcond, film, d0, da, db, total; };   // float offsets; every buffer starts on 256 bytes

VaeWs vae_ws(const iris_vae_decoder_handle* h, int B, int T) {
    const size_t C = h->cfg.model_channels, frames = (size_t)B * T, lat = frames >> h->cfg.down_stages;
    VaeWs w;
    WsTaker t;
    w.p = t.take(frames * C); w.q = t.take(frames * C);
    w.latcond = t.take(lat * C); w.film = t.take(lat * h->film_cols);
    w.d0 = t.take(lat * C); w.da = t.take(lat * C); w.db = t.take(lat * C);
    w.total = t.off;
    return w;
}

int vae_check_shape(const iris_vae_decoder_handle* h, int32_t B, int32_t T) {
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    if (B < 0 || T < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative shape");
    if (T & ((1 << h->cfg.down_stages) - 1))
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "T = %d is not a multiple of 2^down_stages = %d (pad the conditioning first)",
                    T, 1 << h->cfg.down_stages);
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.z)", B);
    if ((uint64_t)B * T * (uint64_t)h->cfg.model_channels > 0x7fffffffull * 64)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "B * T too large");
    return IRIS_HIFIGAN_OK;
}

// the decoder block whose output is the last one: d0 -> da -> db -> da ...
float* vae_dec_out(float* ws, const VaeWs& w, int i) { return ws + ((i & 1) ? w.db : w.da); }

// Queues the launches of one forward (or, in a dry run, counts them).  `lengths` (device, or nullptr for the dense forward)
// selects the ragged kernels: the same launches over the same grids and buffers, each bounded by the items' own rows at
// its level -- sh_in / sh_out count the halvings of the launch's input and output below the full rate.
// `posterior`: z is a posterior latent and the flow runs forwards (TextConditionedVAE.call, vae.py:401).
int vae_forward(iris_vae_decoder_handle* h, const float* cond, const float* z, int B, int T, const int32_t* lengths, float* mel,
                float* residual, float* ws, hipStream_t stream, bool posterior = false) {
    const iris_vae_decoder_config& c = h->cfg;
    const int C = c.model_channels, S = c.down_stages, Tq = T >> S;
    const VaeWs w = vae_ws(h, B, T);
    const float* blob = h->blob;
    auto gemm = [&](const float* x, const PackedGemm& l, float* y, int L_in, int L_out, int sh_in, int sh_out) {
        vae::GemmLaunch a; memset(&a, 0, sizeof(a));
        a.lengths = lengths; a.len_T = T; a.len_shift = S; a.sh_in = sh_in; a.sh_out = sh_out;
        a.x = x; a.wp = (const f32x4*)(blob + l.w_off); a.bias = blob + l.b_off; a.y = y;
        a.L_in = L_in; a.L_out = L_out; a.C_in = l.C_in; a.C_out = l.C_out;
        a.ks = l.k; a.dil = 1; a.stride = 1; a.pad_left = (l.k - 1) / 2;
        return a;
    };
    // lat_cond = downsample(down_cond_proj(frame_cond))                                    vae.py:360-364
    float* pq[2] = {ws + w.p, ws + w.q};
    {
        vae::GemmLaunch a = gemm(cond, h->cond_proj, S == 0 ? ws + w.latcond : pq[0], T, T, 0, 0);
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    for (int s = 0; s < S; ++s) {
        // Conv1D(k5, strides 2, 'same') on an even length: pad (1, 2), y[i] = sum_kap x[2i - 1 + kap] W[kap]; then GELU
        vae::GemmLaunch a = gemm(pq[s & 1], h->down[s], s == S - 1 ? ws + w.latcond : pq[(s + 1) & 1], T >> s, T >> (s + 1), s, s + 1);
        a.stride = 2; a.pad_left = 1; a.gelu = 1;
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    // every Dense(lat_cond) of the decoder at once: FiLM rows of each block, cond_proj of each coupling.  No block and no
    // coupling: no column, no launch (the flow reads no `cond` column when n_flow == 0).
    if (h->film_cols > 0) {
        vae::GemmLaunch a = gemm(ws + w.latcond, h->cond_gemm, ws + w.film, Tq, Tq, S, S);
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    {   // z = flow(z_prior, reverse) -- or flow(z, forward) -- ; d = latent_dec_proj(z)     vae.py:466-468, 401-404
        vae::FlowLaunch f; memset(&f, 0, sizeof(f));
        f.z = z; f.cond = ws + w.film; f.w = blob + h->flow_off; f.wdec = blob + h->dec_proj_off; f.y = ws + w.d0;
        f.Tq = Tq; f.latent = c.latent_dim; f.FH = c.flow_hidden; f.n_flow = c.flow_layers; f.C = C;
        f.ld = h->film_cols; f.ce_off = h->ce_off; f.ce_stride = h->ce_stride;
        f.lengths = lengths; f.len_T = T; f.len_shift = S;
        HIP_TRY(vae::launch_flow(f, B, stream, posterior));
    }
    const float* d = ws + w.d0;
    for (int i = 0; i < c.decoder_blocks; ++i) {                                            // vae.py:57-67, 469-470
        float* y = vae_dec_out(ws, w, i);
        vae::GemmLaunch a = gemm(d, h->dec_conv[i], y, Tq, Tq, S, S);
        a.dil = 1 << (i % 4); a.pad_left = a.dil * (a.ks - 1) / 2; a.gelu = 1;
        a.film = ws + w.film; a.ld_film = h->film_cols; a.gamma_off = i * 2 * C; a.beta_off = i * 2 * C + C;
        a.wp2 = (const f32x4*)(blob + h->dec_res[i].w_off); a.bias2 = blob + h->dec_res[i].b_off; a.res = d;
        HIP_TRY(vae::launch_gemm(a, B, true, stream));
        d = y;
    }
    for (int s = 0; s < S; ++s) {                                                           // vae.py:141-147
        vae::GemmLaunch a = gemm(d, h->up[s], pq[s & 1], Tq << s, Tq << (s + 1), S - s, S - s - 1);
        a.up = 1; a.gelu = 1;
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
        d = pq[s & 1];
    }
    {
        vae::GemmLaunch a = gemm(d, h->out_proj, mel, T, T, 0, 0);
        a.zero_tail = 1;                                                                    // ragged: mel[b, :, len_b:T] = 0
        a.y_channels_first = 1;                                                             // recon [B, n_mels, T], vae.py:480
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    if (residual) {
        vae::GemmLaunch a = gemm(d, h->residual_proj, residual, T, T, 0, 0);
        a.zero_tail = 1;                                                                    // ragged: residual[b, len_b:T, :] = 0
        HIP_TRY(vae::launch_gemm(a, B, false, stream));
    }
    return IRIS_HIFIGAN_OK;
}

}  // namespace

extern "C" {

int32_t iris_vae_decoder_weight_count(const iris_vae_decoder_config* cfg, uint64_t* count) {
    if (!count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(vae_validate(cfg));
    *count = vae_weight_count(*cfg);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_decoder_create(const iris_vae_decoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                iris_vae_decoder_handle** out) {
    IRIS_ABI_BEGIN
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(vae_validate(cfg));
    const uint64_t expect = vae_weight_count(*cfg);
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, the VAE decoder needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    std::unique_ptr<iris_vae_decoder_handle> h(new (std::nothrow) iris_vae_decoder_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    const iris_vae_decoder_config& c = h->cfg;
    const int C = c.model_channels, half = c.latent_dim / 2, FH = c.flow_hidden;
    const int hp = (half + 3) & ~3;                            // a coupling's cond_proj columns, padded to a 16-byte piece
    h->film_cols = c.decoder_blocks * 2 * C + c.flow_layers * hp;
    h->ce_off = c.decoder_blocks * 2 * C; h->ce_stride = hp;
    BlobBuilder bb(weights_host);
    bb.dense(h->cond_proj, c.cond_dim, C, 1);
    h->down.resize(c.down_stages); h->up.resize(c.down_stages);
    h->dec_conv.resize(c.decoder_blocks); h->dec_res.resize(c.decoder_blocks);
    for (auto& l : h->down) bb.dense(l, C, C, 5);
    // the conditioning GEMM: rows = output columns [film_cols][C]; dec block i at 2C i, coupling j at ce_off + hp j
    std::vector<float> cw((size_t)h->film_cols * C, 0.f), cb(h->film_cols, 0.f);
    const size_t per = vae::flow_coupling_floats(half, FH);
    h->flow_off = bb.reserve(per * c.flow_layers);
    for (int j = 0; j < c.flow_layers; ++j) {
        bb.take(cw.data() + (size_t)(h->ce_off + j * hp) * C, (size_t)half * C);
        bb.take(cb.data() + h->ce_off + j * hp, half);
        bb.take(bb.host.data() + h->flow_off + j * per, per);
    }
    h->dec_proj_off = bb.raw((size_t)c.latent_dim * C + C);
    for (int i = 0; i < c.decoder_blocks; ++i) {
        bb.dense(h->dec_conv[i], C, C, c.wavenet_kernel_size);
        bb.take(cw.data() + (size_t)i * 2 * C * C, (size_t)2 * C * C);
        bb.take(cb.data() + (size_t)i * 2 * C, 2 * C);
        bb.dense(h->dec_res[i], C, C, 1);
    }
    for (auto& l : h->up) bb.dense(l, C, C, 5);
    bb.dense(h->out_proj, C, c.n_mels, 1);
    bb.dense(h->residual_proj, C, c.cond_dim, 1);
    bb.dense(h->cond_gemm, cw.data(), cb.data(), C, h->film_cols, 1);
    TRY(upload(bb.host, h.get(), "VAE decoder"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_vae_decoder_destroy(iris_vae_decoder_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_decoder_workspace_bytes(const iris_vae_decoder_handle* h, int32_t B, int32_t T, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(vae_check_shape(h, B, T));
    *bytes = (uint64_t)vae_ws(h, B, T).total * sizeof(float);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_vae_decoder_tap(const iris_vae_decoder_handle* h, int32_t B, int32_t T, int32_t which, uint64_t* byte_offset,
                             uint64_t* floats) {
    if (!byte_offset || !floats) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(vae_check_shape(h, B, T));
    const VaeWs w = vae_ws(h, B, T);
    size_t off;
    if (which == IRIS_VAE_TAP_LAT_COND) off = w.latcond;
    else if (which == IRIS_VAE_TAP_DEC_IN) off = w.d0;
    else if (which == IRIS_VAE_TAP_DEC_OUT) off = h->cfg.decoder_blocks == 0 ? w.d0 : (((h->cfg.decoder_blocks - 1) & 1) ? w.db : w.da);
    else return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "unknown tap %d", which);
    *byte_offset = (uint64_t)off * sizeof(float);
    *floats = ((uint64_t)B * T >> h->cfg.down_stages) * h->cfg.model_channels;
    return IRIS_HIFIGAN_OK;
}

// The dense and the ragged entry point: the same checks in the same order, then the same plan.
static int32_t vae_forward_checked(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_prior_dev, int32_t B, int32_t T,
                                   bool ragged, const int32_t* lengths_dev, float* mel_out_dev, float* residual_out_dev,
                                   void* workspace_dev, uint64_t workspace_bytes, void* stream_, bool posterior = false) {
    IRIS_ABI_BEGIN
    TRY(vae_check_shape(h, B, T));
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    if (!cond_dev || !z_prior_dev || !mel_out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    if (ragged && !lengths_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "lengths_dev is NULL");
    ForwardScope scope(*h, workspace_bytes, vae_ws(h, B, T).total);
    TRY(scope.rc);
    return vae_forward(h, cond_dev, z_prior_dev, B, T, ragged ? lengths_dev : nullptr, mel_out_dev, residual_out_dev,
                       (float*)workspace_dev, (hipStream_t)stream_, posterior);
    IRIS_ABI_END
}

int32_t iris_vae_decoder_forward(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_prior_dev, int32_t B, int32_t T,
                                 float* mel_out_dev, float* residual_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                 void* stream_) {
    return vae_forward_checked(h, cond_dev, z_prior_dev, B, T, false, nullptr, mel_out_dev, residual_out_dev, workspace_dev,
                               workspace_bytes, stream_);
}

int32_t iris_vae_decoder_forward_ragged(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_prior_dev, int32_t B,
                                        int32_t T, const int32_t* lengths_dev, float* mel_out_dev, float* residual_out_dev,
                                        void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    return vae_forward_checked(h, cond_dev, z_prior_dev, B, T, true, lengths_dev, mel_out_dev, residual_out_dev, workspace_dev,
                               workspace_bytes, stream_);
}

int32_t iris_vae_decoder_forward_posterior(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_dev, int32_t B, int32_t T,
                                           float* mel_out_dev, float* residual_out_dev, void* workspace_dev,
                                           uint64_t workspace_bytes, void* stream_) {
    return vae_forward_checked(h, cond_dev, z_dev, B, T, false, nullptr, mel_out_dev, residual_out_dev, workspace_dev,
                               workspace_bytes, stream_, true);
}

int32_t iris_vae_decoder_forward_posterior_ragged(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_dev, int32_t B,
                                                  int32_t T, const int32_t* lengths_dev, float* mel_out_dev, float* residual_out_dev,
                                                  void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    return vae_forward_checked(h, cond_dev, z_dev, B, T, true, lengths_dev, mel_out_dev, residual_out_dev, workspace_dev,
                               workspace_bytes, stream_, true);
}

int32_t iris_vae_decoder_launch_count(const iris_vae_decoder_handle* h, int32_t B, int32_t T, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(vae_check_shape(h, B, T));
    *n = 0;
    if (B == 0 || T == 0) return IRIS_HIFIGAN_OK;
    return count_launches([&](float* fake) {
        return vae_forward(const_cast<iris_vae_decoder_handle*>(h), fake, fake, B, T, nullptr, fake, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

}  // extern "C"
