// iris_text_encoder.hip -- the iris_phoneme_encoder_*, iris_duration_predictor_* and iris_length_* entry points of
// include/iris_hifigan.h over csrc/text_encoder.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

#include "stage_host.h"
#include "text_encoder.h"

using namespace iris;

namespace {

struct TxtNorm { size_t g_off = 0, b_off = 0; };
struct TxtBlock { PackedGemm qkv, out, ffn1, ffn2; TxtNorm attn_norm, ffn_norm; };

constexpr float kLayerNormEps = 1e-6f;                     // layers.LayerNormalization(epsilon=1e-6), encoder.py:71,80,184,275

void pack_norm(BlobBuilder& bb, TxtNorm& n, int C) { n.g_off = bb.raw(C); n.b_off = bb.raw(C); }

txt::GemmLaunch gemm_args(const float* blob, const float* x, const PackedGemm& l, float* y, const int32_t* lengths, int P) {
    txt::GemmLaunch a; memset(&a, 0, sizeof(a));
    a.x = x; a.wp = (const f32x4*)(blob + l.w_off); a.bias = blob + l.b_off; a.y = y; a.lengths = lengths;
    a.P = P; a.C_in = l.C_in; a.C_out = l.C_out; a.ks = l.k; a.eps = kLayerNormEps;
    return a;
}

int check_shape(int32_t B, int32_t P) {
    if (B < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "negative batch");
    if (P < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "P = %d: at least one phoneme is required", P);
    if (B > 65535) return fail(IRIS_HIFIGAN_UNSUPPORTED, "batch %d exceeds 65535 (grid.z)", B);
    if ((uint64_t)B * (uint64_t)P > 0x7fffffffull / 4096) return fail(IRIS_HIFIGAN_UNSUPPORTED, "B * P too large");
    return IRIS_HIFIGAN_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Phoneme encoder (PhonemeEncoder, src/iris/encoder.py:115-212)
// ------------------------------------------------------------------------------------------------
struct iris_phoneme_encoder_handle : StageHandle {
    iris_phoneme_encoder_config cfg;
    size_t tok_off = 0, pos_off = 0;
    std::vector<TxtBlock> blocks;
    TxtNorm final_norm;
};

namespace {

int enc_validate(const iris_phoneme_encoder_config* c) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->vocab_size < 1 || c->embed_dim < 1 || c->num_blocks < 0 || c->num_heads < 1 || c->ffn_dim < 1 || c->max_length < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "phoneme encoder sizes must be positive");
    if (c->embed_dim % c->num_heads)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "embed_dim %d is not a multiple of num_heads %d", c->embed_dim, c->num_heads);
    const int Dk = c->embed_dim / c->num_heads;
    if ((Dk & 7) || Dk > txt::kMaxKeyDim)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "key_dim %d must be a multiple of 8 and at most %d", Dk, txt::kMaxKeyDim);
    if ((c->embed_dim & 3) || (c->ffn_dim & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "embed_dim %d and ffn_dim %d must be multiples of 4 (16-byte rows)", c->embed_dim, c->ffn_dim);
    if (c->embed_dim > 32 * txt::kMaxWaves)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "embed_dim %d exceeds %d (one block holds a LayerNorm row)", c->embed_dim, 32 * txt::kMaxWaves);
    if (c->num_blocks > 64 || c->num_heads > 65535 || c->ffn_dim > (1 << 16) || c->max_length > (1 << 20) || c->vocab_size > (1 << 20))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "num_blocks <= 64, ffn_dim <= 65536, max_length and vocab_size <= 2^20");
    return IRIS_HIFIGAN_OK;
}

uint64_t enc_weight_count(const iris_phoneme_encoder_config& c) {
    const uint64_t E = c.embed_dim, F = c.ffn_dim;
    uint64_t n = (uint64_t)c.vocab_size * E + (uint64_t)c.max_length * E;
    n += (uint64_t)c.num_blocks * ((3 * E * E + 3 * E) + (E * E + E) + 2 * E + (F * E + F) + (E * F + E) + 2 * E);
    return n + 2 * E;
}

struct EncWs { size_t x0, x1, t0, qkv, attn, ffn, total; };   // float offsets; every buffer starts on 256 bytes

EncWs enc_ws(const iris_phoneme_encoder_config& c, int B, int P) {
    const size_t rows = (size_t)B * P, E = c.embed_dim;
    EncWs w;
    WsTaker t;
    w.x0 = t.take(rows * E); w.x1 = t.take(rows * E); w.t0 = t.take(rows * E);
    w.qkv = t.take(rows * 3 * E); w.attn = t.take(rows * E); w.ffn = t.take(rows * c.ffn_dim);
    w.total = t.off;
    return w;
}

int enc_check_shape(const iris_phoneme_encoder_config& c, int32_t B, int32_t P) {
    TRY(check_shape(B, P));
    if (P > c.max_length)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "P = %d exceeds max_length = %d (the position table ends there)", P, c.max_length);
    return IRIS_HIFIGAN_OK;
}

// Queues the launches of one forward (or, in a dry run, counts them): 1 + 5 per block + 1.
int enc_forward(const iris_phoneme_encoder_handle* h, const int32_t* ids, const int32_t* lengths, int B, int P, float* enc_out,
                float* ws, hipStream_t stream) {
    const iris_phoneme_encoder_config& c = h->cfg;
    const int E = c.embed_dim, H = c.num_heads, Dk = E / H;
    const EncWs w = enc_ws(c, B, P);
    const float* blob = h->blob;
    {
        txt::EmbedLaunch a{ids, lengths, blob + h->tok_off, blob + h->pos_off, ws + w.x0, B, P, E, c.vocab_size};
        HIP_TRY(txt::launch_embed(a, stream));
    }
    const float* x = ws + w.x0;
    for (int i = 0; i < c.num_blocks; ++i) {                                                // TransformerBlock.call, encoder.py:82-102
        const TxtBlock& k = h->blocks[i];
        float* mid = ws + w.x1;
        float* out = ws + (i == 0 ? w.t0 : w.x0);          // block 0's output keeps a buffer of its own (the tap)
        {
            txt::GemmLaunch a = gemm_args(blob, x, k.qkv, ws + w.qkv, lengths, P);
            HIP_TRY(txt::launch_gemm(a, B, stream));
        }
        {
            txt::AttnLaunch a{ws + w.qkv, ws + w.attn, lengths, P, E, H, Dk, (float)(1.0 / sqrt((double)Dk))};
            HIP_TRY(txt::launch_attention(a, B, stream));
        }
        {
            txt::GemmLaunch a = gemm_args(blob, ws + w.attn, k.out, mid, lengths, P);
            a.res = x; a.gamma = blob + k.attn_norm.g_off; a.beta = blob + k.attn_norm.b_off;
            HIP_TRY(txt::launch_gemm(a, B, stream));
        }
        {
            txt::GemmLaunch a = gemm_args(blob, mid, k.ffn1, ws + w.ffn, lengths, P);
            a.relu = 1;
            HIP_TRY(txt::launch_gemm(a, B, stream));
        }
        {
            txt::GemmLaunch a = gemm_args(blob, ws + w.ffn, k.ffn2, out, lengths, P);
            a.res = mid; a.gamma = blob + k.ffn_norm.g_off; a.beta = blob + k.ffn_norm.b_off;
            HIP_TRY(txt::launch_gemm(a, B, stream));
        }
        x = out;
    }
    {
        txt::NormLaunch a{x, blob + h->final_norm.g_off, blob + h->final_norm.b_off, enc_out, lengths, B, P, E, kLayerNormEps};
        HIP_TRY(txt::launch_layernorm(a, stream));
    }
    return IRIS_HIFIGAN_OK;
}

// the parts of a handle a dry run reads
void enc_layout(iris_phoneme_encoder_handle* h, BlobBuilder* bb) {
    const iris_phoneme_encoder_config& c = h->cfg;
    const int E = c.embed_dim, F = c.ffn_dim;
    h->blocks.resize(c.num_blocks);
    if (!bb) {
        for (auto& k : h->blocks) {
            k.qkv = PackedGemm{E, 3 * E, 1, 0, 0}; k.out = PackedGemm{E, E, 1, 0, 0};
            k.ffn1 = PackedGemm{E, F, 1, 0, 0}; k.ffn2 = PackedGemm{F, E, 1, 0, 0};
        }
        return;
    }
    h->tok_off = bb->raw((size_t)c.vocab_size * E);
    h->pos_off = bb->raw((size_t)c.max_length * E);
    for (auto& k : h->blocks) {
        bb->dense(k.qkv, E, 3 * E, 1);
        bb->dense(k.out, E, E, 1);
        pack_norm(*bb, k.attn_norm, E);
        bb->dense(k.ffn1, E, F, 1);
        bb->dense(k.ffn2, F, E, 1);
        pack_norm(*bb, k.ffn_norm, E);
    }
    pack_norm(*bb, h->final_norm, E);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Duration head (DurationPredictor, encoder.py:228-315; predict_durations, scripts/synthesize.py:41-45)
// ------------------------------------------------------------------------------------------------
struct iris_duration_predictor_handle : StageHandle {
    iris_duration_predictor_config cfg;
    std::vector<PackedGemm> conv;
    std::vector<TxtNorm> norm;
    size_t out_off = 0;                                    // duration_output kernel [C], then its bias
};

namespace {

int dur_validate(const iris_duration_predictor_config* c) {
    if (!c) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "config is NULL");
    if (c->in_dim < 1 || c->hidden_dim < 1 || c->num_layers < 0 || c->kernel_size < 1 || c->max_frames_per_phoneme < 1)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "duration predictor sizes must be positive");
    if ((c->in_dim & 3) || (c->hidden_dim & 3))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "in_dim %d and hidden_dim %d must be multiples of 4 (16-byte rows)", c->in_dim, c->hidden_dim);
    if (!(c->kernel_size & 1))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "kernel_size %d must be odd (symmetric 'same' padding)", c->kernel_size);
    if (c->hidden_dim > 32 * txt::kMaxWaves)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "hidden_dim %d exceeds %d (one block holds a LayerNorm row)", c->hidden_dim, 32 * txt::kMaxWaves);
    if (c->num_layers > 64 || c->kernel_size > 63 || c->in_dim > (1 << 16))
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "num_layers <= 64, kernel_size <= 63, in_dim <= 65536");
    return IRIS_HIFIGAN_OK;
}

int dur_out_channels(const iris_duration_predictor_config& c) { return c.num_layers ? c.hidden_dim : c.in_dim; }

uint64_t dur_weight_count(const iris_duration_predictor_config& c) {
    const uint64_t Hd = c.hidden_dim, k = c.kernel_size;
    uint64_t n = 0;
    for (int i = 0; i < c.num_layers; ++i) n += Hd * (i == 0 ? (uint64_t)c.in_dim : Hd) * k + Hd + 2 * Hd;
    return n + dur_out_channels(c) + 1;
}

struct DurWs { size_t d[3]; size_t total; };

DurWs dur_ws(const iris_duration_predictor_config& c, int B, int P) {
    DurWs w;
    WsTaker t;
    for (int i = 0; i < 3; ++i) w.d[i] = t.take((size_t)B * P * c.hidden_dim);
    w.total = t.off;
    return w;
}

int dur_check_shape(const iris_duration_predictor_config& c, int32_t B, int32_t P) {
    TRY(check_shape(B, P));
    if ((uint64_t)P * (uint64_t)c.max_frames_per_phoneme > 0x7fffffffull)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "P = %d phonemes of up to %d frames overflow the int32 offsets", P, c.max_frames_per_phoneme);
    return IRIS_HIFIGAN_OK;
}

// layer i writes buffer 0 (i = 0: the tap) or alternates between 1 and 2
int dur_buffer(int i) { return i == 0 ? 0 : 1 + (i & 1); }

// num_layers + 2 launches
int dur_forward(const iris_duration_predictor_handle* h, const float* enc, const int32_t* lengths, int B, int P, float* pred,
                int32_t* frames, int32_t* offsets, int32_t* totals, float* ws, hipStream_t stream) {
    const iris_duration_predictor_config& c = h->cfg;
    const DurWs w = dur_ws(c, B, P);
    const float* blob = h->blob;
    const float* x = enc;
    for (int i = 0; i < c.num_layers; ++i) {               // Conv1D('same', relu) -> LayerNorm, encoder.py:302-305
        float* y = ws + w.d[dur_buffer(i)];
        txt::GemmLaunch a = gemm_args(blob, x, h->conv[i], y, lengths, P);
        a.relu = 1; a.gamma = blob + h->norm[i].g_off; a.beta = blob + h->norm[i].b_off;
        HIP_TRY(txt::launch_gemm(a, B, stream));
        x = y;
    }
    {
        txt::DurationLaunch a{x, blob + h->out_off, lengths, pred, frames, B, P, dur_out_channels(c), c.max_frames_per_phoneme};
        HIP_TRY(txt::launch_duration(a, stream));
    }
    {
        txt::ScanLaunch a{frames, lengths, offsets, totals, P};
        HIP_TRY(txt::launch_scan(a, B, stream));
    }
    return IRIS_HIFIGAN_OK;
}

void dur_layout(iris_duration_predictor_handle* h, BlobBuilder* bb) {
    const iris_duration_predictor_config& c = h->cfg;
    h->conv.resize(c.num_layers); h->norm.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        const int C_in = i == 0 ? c.in_dim : c.hidden_dim;
        if (!bb) { h->conv[i] = PackedGemm{C_in, c.hidden_dim, c.kernel_size, 0, 0}; continue; }
        bb->dense(h->conv[i], C_in, c.hidden_dim, c.kernel_size);
        pack_norm(*bb, h->norm[i], c.hidden_dim);
    }
    if (bb) h->out_off = bb->raw((size_t)dur_out_channels(c) + 1);
}

}  // namespace

extern "C" {

int32_t iris_phoneme_encoder_weight_count(const iris_phoneme_encoder_config* cfg, uint64_t* count) {
    if (!count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    *count = enc_weight_count(*cfg);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_phoneme_encoder_create(const iris_phoneme_encoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                    iris_phoneme_encoder_handle** out) {
    IRIS_ABI_BEGIN
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    const uint64_t expect = enc_weight_count(*cfg);
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, the phoneme encoder needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    std::unique_ptr<iris_phoneme_encoder_handle> h(new (std::nothrow) iris_phoneme_encoder_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    BlobBuilder bb(weights_host);
    enc_layout(h.get(), &bb);
    TRY(upload(bb.host, h.get(), "phoneme encoder"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_phoneme_encoder_destroy(iris_phoneme_encoder_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_phoneme_encoder_workspace_bytes(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    TRY(enc_check_shape(*cfg, B, P));
    *bytes = (uint64_t)enc_ws(*cfg, B, P).total * sizeof(float);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_phoneme_encoder_tap(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, uint64_t* byte_offset, uint64_t* floats) {
    if (!byte_offset || !floats) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    TRY(enc_check_shape(*cfg, B, P));
    const EncWs w = enc_ws(*cfg, B, P);
    *byte_offset = (uint64_t)(cfg->num_blocks ? w.t0 : w.x0) * sizeof(float);
    *floats = (uint64_t)B * P * cfg->embed_dim;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_phoneme_encoder_forward(iris_phoneme_encoder_handle* h, const int32_t* ids_dev, const int32_t* lengths_dev, int32_t B,
                                     int32_t P, float* enc_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(enc_check_shape(h->cfg, B, P));
    if (B == 0) return IRIS_HIFIGAN_OK;
    if (!ids_dev || !enc_out_dev || !workspace_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardScope scope(*h, workspace_bytes, enc_ws(h->cfg, B, P).total);
    TRY(scope.rc);
    return enc_forward(h, ids_dev, lengths_dev, B, P, enc_out_dev, (float*)workspace_dev, (hipStream_t)stream_);
    IRIS_ABI_END
}

int32_t iris_phoneme_encoder_launch_count(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(enc_validate(cfg));
    TRY(enc_check_shape(*cfg, B, P));
    *n = 0;
    if (B == 0) return IRIS_HIFIGAN_OK;
    iris_phoneme_encoder_handle h;                         // the forward's own code in a dry run over a handle without weights
    h.cfg = *cfg;
    enc_layout(&h, nullptr);
    return count_launches([&](float* fake) {
        return enc_forward(&h, reinterpret_cast<const int32_t*>(fake), nullptr, B, P, fake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_duration_predictor_weight_count(const iris_duration_predictor_config* cfg, uint64_t* count) {
    if (!count) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(dur_validate(cfg));
    *count = dur_weight_count(*cfg);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_duration_predictor_create(const iris_duration_predictor_config* cfg, const float* weights_host, uint64_t n_weights,
                                       iris_duration_predictor_handle** out) {
    IRIS_ABI_BEGIN
    if (!weights_host || !out) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(dur_validate(cfg));
    const uint64_t expect = dur_weight_count(*cfg);
    if (n_weights != expect)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "weight blob has %llu values, the duration predictor needs %llu",
                    (unsigned long long)n_weights, (unsigned long long)expect);
    std::unique_ptr<iris_duration_predictor_handle> h(new (std::nothrow) iris_duration_predictor_handle);
    if (!h) return fail(IRIS_HIFIGAN_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    BlobBuilder bb(weights_host);
    dur_layout(h.get(), &bb);
    TRY(upload(bb.host, h.get(), "duration predictor"));
    *out = h.release();
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_duration_predictor_destroy(iris_duration_predictor_handle* h) {
    delete h;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_duration_predictor_workspace_bytes(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, uint64_t* bytes) {
    if (!bytes) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(dur_validate(cfg));
    TRY(dur_check_shape(*cfg, B, P));
    *bytes = (uint64_t)dur_ws(*cfg, B, P).total * sizeof(float);
    return IRIS_HIFIGAN_OK;
}

int32_t iris_duration_predictor_tap(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, uint64_t* byte_offset,
                                    uint64_t* floats) {
    if (!byte_offset || !floats) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(dur_validate(cfg));
    TRY(dur_check_shape(*cfg, B, P));
    if (cfg->num_layers < 1) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "a head without conv layers has no tap");
    *byte_offset = (uint64_t)dur_ws(*cfg, B, P).d[0] * sizeof(float);
    *floats = (uint64_t)B * P * cfg->hidden_dim;
    return IRIS_HIFIGAN_OK;
}

int32_t iris_duration_predictor_forward(iris_duration_predictor_handle* h, const float* enc_out_dev, const int32_t* lengths_dev,
                                        int32_t B, int32_t P, float* pred_dev, int32_t* frames_dev, int32_t* offsets_dev,
                                        int32_t* totals_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream_) {
    IRIS_ABI_BEGIN
    if (!h) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL handle");
    TRY(dur_check_shape(h->cfg, B, P));
    if (B == 0) return IRIS_HIFIGAN_OK;
    if (!enc_out_dev || !pred_dev || !frames_dev || !offsets_dev || !totals_dev || !workspace_dev)
        return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    ForwardScope scope(*h, workspace_bytes, dur_ws(h->cfg, B, P).total);
    TRY(scope.rc);
    return dur_forward(h, enc_out_dev, lengths_dev, B, P, pred_dev, frames_dev, offsets_dev, totals_dev, (float*)workspace_dev,
                       (hipStream_t)stream_);
    IRIS_ABI_END
}

int32_t iris_duration_predictor_launch_count(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, int32_t* n) {
    IRIS_ABI_BEGIN
    if (!n) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL argument");
    TRY(dur_validate(cfg));
    TRY(dur_check_shape(*cfg, B, P));
    *n = 0;
    if (B == 0) return IRIS_HIFIGAN_OK;
    iris_duration_predictor_handle h;
    h.cfg = *cfg;
    dur_layout(&h, nullptr);
    return count_launches([&](float* fake) {
        int32_t* const ifake = reinterpret_cast<int32_t*>(fake);
        return dur_forward(&h, fake, nullptr, B, P, fake, ifake, ifake, ifake, fake, nullptr); }, n);
    IRIS_ABI_END
}

int32_t iris_length_scan(const int32_t* frames_dev, const int32_t* lengths_dev, int32_t B, int32_t P, int32_t* offsets_dev,
                         int32_t* totals_dev, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_shape(B, P));
    if (B == 0) return IRIS_HIFIGAN_OK;
    if (!frames_dev || !offsets_dev || !totals_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    txt::ScanLaunch a{frames_dev, lengths_dev, offsets_dev, totals_dev, P};
    HIP_TRY(txt::launch_scan(a, B, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

int32_t iris_length_regulate(const float* enc_out_dev, const int32_t* offsets_dev, const int32_t* totals_dev, int32_t B, int32_t P,
                             int32_t E, int32_t T_pad, float* cond_dev, void* stream_) {
    IRIS_ABI_BEGIN
    TRY(check_shape(B, P));
    if (E < 1 || T_pad < 0) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "E = %d, T_pad = %d", E, T_pad);
    if (E & 3) return fail(IRIS_HIFIGAN_UNSUPPORTED, "E = %d must be a multiple of 4 (16-byte rows)", E);
    if (B == 0 || T_pad == 0) return IRIS_HIFIGAN_OK;
    if (!enc_out_dev || !offsets_dev || !totals_dev || !cond_dev) return fail(IRIS_HIFIGAN_INVALID_ARGUMENT, "NULL device pointer");
    txt::GatherLaunch a{enc_out_dev, offsets_dev, totals_dev, cond_dev, P, E, T_pad};
    HIP_TRY(txt::launch_gather(a, B, (hipStream_t)stream_));
    return IRIS_HIFIGAN_OK;
    IRIS_ABI_END
}

}  // extern "C"
