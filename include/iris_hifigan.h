/*
 * iris_hifigan.h -- C-ABI of the MI355X (gfx950) HiFiGAN generator path.
 *
 * The reference (ZECTBynmo/iris-tts) is pure Python and has no FFI for this path
 * (SURVEY.md section 8b): its boundary is two Python call surfaces,
 *   iris.hifigan_pretrained.HiFiGANGenerator.__call__   (src/iris/hifigan_pretrained.py:208-242)
 *   iris.vocoder.HiFiGANVocoder.infer                   (src/iris/vocoder.py:177-209)
 * both of which end in one call of the generator forward
 *   HiFiGANModel.forward                                (src/iris/hifigan_pretrained.py:123-143)
 *   HiFiGANGenerator.call                               (src/iris/vocoder.py:103-130).
 * The entry points below are what a binding for that forward has to provide; the
 * drop-in Python modules in iris-tts_amd/iris/ bind them with ctypes.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer named *_dev is a HIP device pointer
 *     owned by the caller (e.g. a PyTorch-ROCm tensor's data_ptr()), *_host is host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); forward is
 *     asynchronous on it and performs no allocation and no synchronisation -- with ONE exception: the first forward of
 *     IRIS_HIFIGAN_BF16 / IRIS_HIFIGAN_F32_SPLIT on a handle that was not prepared for that dtype
 *     (iris_hifigan_prepare) builds the dtype's weight packing first (host repack, hipMalloc, synchronous upload).
 *     Forwards of IRIS_HIFIGAN_F32 never do (create uploads everything fp32 needs).  Inside a stream capture that
 *     lazy build is refused with IRIS_HIFIGAN_NOT_PREPARED instead of invalidating the capture;
 *   - every function returns an iris_hifigan_status; on failure the calling thread's
 *     message is available from iris_hifigan_last_error(); no exception crosses the ABI;
 *   - a handle may be used by one thread at a time, with ONE forward in flight: a handle owns per-forward
 *     device state (the next-tile counters of the persistent MRF kernel, the profiling events) and every
 *     forward of a handle writes the same caller-provided workspace, so a second forward of the same handle
 *     (another stream, or a hipGraph replay that captured it) must be ordered after the first one -- put them
 *     on one stream or give each stream its own handle and workspace;
 *   - a handle belongs to the HIP device that was current in iris_hifigan_create; forward selects that device
 *     for its launches and restores the caller's, so `stream` and all *_dev pointers must belong to it;
 *   - the library reads no environment variable (A/B switches are compile-time macros).
 *
 * Activations inside the library are channels-last [B, L, C], fp32 (bf16 with dtype
 * IRIS_HIFIGAN_BF16); the mel comes in as the
 * reference hands it over, channels-first [B, n_mels, T] (hifigan_pretrained.py:228), and the
 * waveform goes out as [B, prod(upsample_rates) * T] (hifigan_pretrained.py:235-236) -- fp32, or 16-bit PCM
 * (iris_hifigan_forward_pcm16).
 */
#ifndef IRIS_HIFIGAN_H
#define IRIS_HIFIGAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRIS_HIFIGAN_ABI_VERSION 4
#define IRIS_HIFIGAN_MAX_STAGES 8    /* upsample stages            */
#define IRIS_HIFIGAN_MAX_KERNELS 8   /* MRF branches per stage     */
#define IRIS_HIFIGAN_MAX_DILATIONS 8 /* conv pairs per ResBlock    */

typedef enum iris_hifigan_status {
    IRIS_HIFIGAN_OK = 0,
    IRIS_HIFIGAN_INVALID_ARGUMENT = 1,
    IRIS_HIFIGAN_HIP_ERROR = 2,
    IRIS_HIFIGAN_OUT_OF_MEMORY = 3,
    IRIS_HIFIGAN_UNSUPPORTED = 4,
    IRIS_HIFIGAN_WORKSPACE_TOO_SMALL = 5,
    IRIS_HIFIGAN_NOT_PREPARED = 6 /* a forward needs a weight packing that cannot be built now: the stream is being captured
                                    (call iris_hifigan_prepare first), or the host weights were released before the dtype's
                                    first use */
} iris_hifigan_status;

typedef enum iris_hifigan_dtype {
    IRIS_HIFIGAN_F32 = 0, /* fp32 storage, fp32 MFMA (exact fmaf chains): the parity path (<= 1e-4 vs reference) */
    IRIS_HIFIGAN_BF16 = 1, /* bf16 storage of activations and weights, fp32 accumulation (bf16 MFMA); mel in and
                             waveform out stay fp32.  BASELINE.json configs[2].  The reference has no bf16 path:
                             its error against the fp32 generator (~1e-2 max-abs) is documented, not pinned. */
    IRIS_HIFIGAN_F32_SPLIT = 2 /* fp32 storage everywhere, fp32 accumulation; the ResBlock convolutions form each product
                             from two bf16 terms per operand (hi*hi + hi*mid + mid*hi on the bf16 MFMA).  Within
                             north_star's 1e-4 of the fp32 generator (measured ~2e-5) but not the exact fp32 arithmetic
                             of IRIS_HIFIGAN_F32: opt-in, never the headline.  Same workspace as IRIS_HIFIGAN_F32. */
} iris_hifigan_dtype;

/* Generator hyper-parameters: the constructor arguments of HiFiGANModel
 * (hifigan_pretrained.py:77-85) == HiFiGANGenerator (vocoder.py:59-67). */
typedef struct iris_hifigan_config {
    int32_t in_channels;              /* 80  */
    int32_t upsample_initial_channel; /* 512 */
    int32_t num_upsamples;            /* 4   */
    int32_t upsample_rates[IRIS_HIFIGAN_MAX_STAGES];        /* 8,8,2,2   */
    int32_t upsample_kernel_sizes[IRIS_HIFIGAN_MAX_STAGES]; /* 16,16,4,4 */
    int32_t num_kernels;              /* 3   */
    int32_t resblock_kernel_sizes[IRIS_HIFIGAN_MAX_KERNELS]; /* 3,7,11 */
    int32_t num_dilations[IRIS_HIFIGAN_MAX_KERNELS];         /* 3,3,3  */
    int32_t resblock_dilations[IRIS_HIFIGAN_MAX_KERNELS][IRIS_HIFIGAN_MAX_DILATIONS]; /* 1,3,5 each */
    int32_t pre_kernel_size;          /* 7 (hifigan_pretrained.py:93)  */
    int32_t post_kernel_size;         /* 7 (hifigan_pretrained.py:120) */
    float lrelu_slope;                /* 0.1 everywhere (hifigan_pretrained.py:66,68,127,139) */
} iris_hifigan_config;

typedef struct iris_hifigan_handle iris_hifigan_handle;

/* Per-launch record filled when profiling is enabled (bench.py's roofline leg). */
typedef struct iris_hifigan_launch_record {
    int32_t kind;      /* 0 conv_pre, 1 upsample (ConvTranspose1d), 2 MRF ResBlock conv group, 3 conv_post */
    int32_t stage;     /* upsample stage index, -1 for conv_pre / conv_post */
    int32_t step;      /* 0..2*num_dilations-1 inside a stage's MRF, else 0 (grouped record: that of its first launch) */
    int32_t launches;  /* kernel launches this record covers: 1, or in grouped mode the MRF launches of a stage */
    double flops;      /* algorithmic FLOP of this launch (2*MAC, zero padding counted)   */
    double bytes;      /* algorithmic bytes of this launch, accounting L of SURVEY.md 8d  */
    float ms;          /* hipEventElapsedTime of this launch on the forward's stream      */
    float reserved2;
} iris_hifigan_launch_record;

int32_t iris_hifigan_abi_version(void);
const char* iris_hifigan_last_error(void);

/* Number of fp32 values iris_hifigan_create expects in `weights_host`: the folded
 * (weight-norm already applied) tensors of the reference state-dict, concatenated in
 * this order, each in the reference's own layout:
 *   conv_pre.weight [C0,in,kpre], conv_pre.bias [C0],
 *   for i in stages:  ups.i.weight [Cin,Cout,k] (ConvTranspose1d layout), ups.i.bias [Cout],
 *                     for j in kernels: for m in dilations: convs1.m.weight [C,C,k], convs1.m.bias [C]
 *                                       for m in dilations: convs2.m.weight [C,C,k], convs2.m.bias [C]
 *   conv_post.weight [1,Clast,kpost], conv_post.bias [1].                                         */
int32_t iris_hifigan_weight_count(const iris_hifigan_config* cfg, uint64_t* count);

/* Builds a generator: validates cfg, repacks the weights into MFMA fragment order and
 * uploads them to the current HIP device. Replaces HiFiGANModel() + load_state_dict
 * (hifigan_pretrained.py:186-190). */
int32_t iris_hifigan_create(const iris_hifigan_config* cfg, const float* weights_host,
                            uint64_t n_weights, iris_hifigan_handle** out);
int32_t iris_hifigan_destroy(iris_hifigan_handle* h);

/* create uploads what IRIS_HIFIGAN_F32 needs (the 32x32 MFMA fragments and the 16x16 fragments of the short-input kernel;
 * the repacking runs on up to 16 host threads).  The packings of the other arithmetic (bf16 fragments for IRIS_HIFIGAN_BF16,
 * hi/mid bf16 planes for IRIS_HIFIGAN_F32_SPLIT) are built on the first use of that dtype: by this call, or by the first
 * forward of the dtype (which is then synchronous and allocates once; refused with IRIS_HIFIGAN_NOT_PREPARED inside a stream
 * capture).  A failed build (out of memory) is reported and retried by the next call; it does not disable the dtype.
 * Call prepare before capturing forwards of a dtype into a hipGraph. */
int32_t iris_hifigan_prepare(iris_hifigan_handle* h, int32_t dtype);
/* Until both of those packings exist the handle keeps the reference-layout weights on the host (55.7 MB for V1, per handle)
 * to build them from.  A caller that has prepared every dtype it will use drops that copy here; a later first use of
 * another dtype then fails with IRIS_HIFIGAN_NOT_PREPARED. */
int32_t iris_hifigan_release_host_weights(iris_hifigan_handle* h);

/* Activation workspace needed by one forward of [B, in_channels, T].  Batch items are independent: a batch of more than
 * 65,536 mel frames in all runs as consecutive passes over sub-batches that share the workspace, so the figure is bounded
 * (fp32: 229 KB per frame of ONE pass, at most ~15 GB; bf16 half of that) instead of growing with the batch; one item
 * longer than that still needs its own length (split long utterances along time with iris.streaming). */
int32_t iris_hifigan_workspace_bytes(const iris_hifigan_handle* h, int32_t B, int32_t T,
                                     int32_t dtype, uint64_t* bytes);

/* mel_dev [B, in_channels, T] fp32 -> wav_dev [B, hop*T] fp32, hop = prod(upsample_rates).
 * Replaces `self.model(mel_tensor)` (hifigan_pretrained.py:231-232; vocoder.py:200). */
int32_t iris_hifigan_forward(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                             void* wav_dev, void* workspace_dev, uint64_t workspace_bytes,
                             int32_t dtype, void* stream);

/* Ragged batch: items of different lengths in one forward.
 * mel_dev [B, in_channels, T] fp32, lengths_dev [B] int32 on the device (caller-owned, like mel_dev).
 * Item b is computed exactly as iris_hifigan_forward of mel[b, :, :lengths[b]] alone would compute it,
 * bit for bit. Mel frames >= lengths[b] are never read, so they may hold anything, NaN included.
 * wav[b, hop*lengths[b] : hop*T] is written as 0.0f. lengths are clamped to [0, T] on the device.
 * Workspace as iris_hifigan_workspace_bytes(B, T). Same stream, allocation and capture rules as forward.
 * The host never reads the lengths: the launch plan is the one of iris_hifigan_forward(B, T), and tiles past an
 * item's length return at once on the device. Profiling records still count the work of B*T frames.
 * dtype: IRIS_HIFIGAN_F32 only; others return IRIS_HIFIGAN_UNSUPPORTED. lengths_dev == NULL (B, T > 0) returns
 * IRIS_HIFIGAN_INVALID_ARGUMENT. */
int32_t iris_hifigan_forward_ragged(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                    const int32_t* lengths_dev, void* wav_dev, void* workspace_dev,
                                    uint64_t workspace_bytes, int32_t dtype, void* stream);

/* The forward with the output stage on the device: 16-bit PCM, optionally peak-normalised per item.  What a caller of the
 * reference does with the fp32 waveform on the host (scripts/synthesize.py writes a 16-bit WAV; demo_vocoder.py first
 * scales to 0.95 / (max|w| + 1e-8)) happens in the forward's last launch instead, so half the bytes cross to the host.
 *   normalize == 0:  pcm[b, i] = (int16) rintf(clamp(w, -1, 1) * 32767), w the sample iris_hifigan_forward would store
 *                    -- bit for bit numpy's round(clip(w, -1, 1) * 32767) (half to even); conv_post stores it in place of
 *                    the waveform.  wav_dev, peak_dev and peak_target are ignored (may be NULL).
 *   normalize != 0:  q = (w / (peak[b] + 1e-8f)) * peak_target, pcm = (int16) rintf(clamp(q, -1, 1) * 32767), every
 *                    operation its own fp32 rounding, the division correctly rounded; peak[b] = max |w| over the item's
 *                    own samples.  Afterwards wav_dev [B, hop*T] holds the fp32 waveform, bit for bit
 *                    iris_hifigan_forward's (iris_hifigan_forward_ragged's with lengths), and peak_dev [B] the per-item
 *                    peaks (0 for an empty or silent item, whose PCM is 0).  conv_post reduces the peaks beside its store
 *                    (one vector atomic max per block; deterministic) and a second kernel converts.  NULL wav_dev or
 *                    peak_dev, or peak_target outside (0, 1], returns IRIS_HIFIGAN_INVALID_ARGUMENT.
 * lengths_dev: NULL = a plain batch (every dtype); else [B] int32 on the device as in iris_hifigan_forward_ragged --
 * IRIS_HIFIGAN_F32 only (others return IRIS_HIFIGAN_UNSUPPORTED); pcm[b, hop*lengths[b]:] is 0 and the item's peak covers
 * its own samples only.  B == 0 or T == 0 returns IRIS_HIFIGAN_OK.
 * Workspace as iris_hifigan_workspace_bytes(B, T, dtype); same stream, allocation, synchronisation and capture rules as
 * iris_hifigan_forward (a normalising call also queues one memset of its peaks per pass).  Batches above 65,536 frames run
 * as passes; every buffer advances per pass. */
int32_t iris_hifigan_forward_pcm16(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                   const int32_t* lengths_dev /* NULL = plain batch */,
                                   int16_t* pcm_dev           /* [B, hop*T] */,
                                   float* wav_dev             /* [B, hop*T]; required iff normalize, else may be NULL */,
                                   float* peak_dev            /* [B]; required iff normalize, else may be NULL */,
                                   int32_t normalize, float peak_target,
                                   void* workspace_dev, uint64_t workspace_bytes, int32_t dtype, void* stream);

/* ---- intermediates (parity tests of the layers inside a forward; not needed by a caller) ----
 * forward_until queues the same launches as forward up to and including MRF step `stop_step`
 * (0 .. 2*num_dilations-1: even = convs1[m], odd = convs2[m] + residual, hifigan_pretrained.py:64-71) of
 * upsample stage `stop_stage` and returns; no waveform is produced.  The intermediates are then in the
 * workspace at the offsets workspace_layout reports, channels-last [B, L_stage, C_stage]:
 *   pre  conv_pre output [B, T, C0];  up  the stage's ConvTranspose1d output;
 *   y[j] running x of ResBlock j (after an odd step);  xt[j] output of convs1 of ResBlock j (after an even step).
 * *flags (may be NULL) receives
 *   IRIS_HIFIGAN_UNTIL_MEAN_IN_Y0  stop_step is the last step of the stage and the kernel already stored
 *                                  (y[0]+y[1]+y[2])/num_kernels (hifigan_pretrained.py:131-137) in y[0] instead of the
 *                                  branch outputs;
 *   IRIS_HIFIGAN_UNTIL_X_IN_XT     the roles of the y and xt buffers are swapped at this point (the fused conv-pair
 *                                  kernel of the bf16 path cannot work in place and alternates between them). */
#define IRIS_HIFIGAN_UNTIL_MEAN_IN_Y0 1
#define IRIS_HIFIGAN_UNTIL_X_IN_XT 2
typedef struct iris_hifigan_workspace_map {
    uint64_t pre_offset, up_offset;                 /* byte offsets into the workspace */
    uint64_t y_offset[IRIS_HIFIGAN_MAX_KERNELS];
    uint64_t xt_offset[IRIS_HIFIGAN_MAX_KERNELS];
    uint64_t total_bytes;                           /* == iris_hifigan_workspace_bytes */
    int32_t element_bytes;                          /* 4 (fp32 storage) or 2 (bf16 storage) */
    int32_t reserved;
} iris_hifigan_workspace_map;
int32_t iris_hifigan_workspace_layout(const iris_hifigan_handle* h, int32_t B, int32_t T, int32_t dtype,
                                      iris_hifigan_workspace_map* out);
int32_t iris_hifigan_forward_until(iris_hifigan_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                   void* workspace_dev, uint64_t workspace_bytes, int32_t dtype,
                                   int32_t stop_stage, int32_t stop_step, int32_t* flags, void* stream);

/* Samples of waveform per mel frame (256 for the V1 config). */
int32_t iris_hifigan_hop_length(const iris_hifigan_handle* h, int32_t* hop);

/* Profiling: enabled = 1 brackets every launch of forward by hipEvents on `stream`; enabled = 2 does the same but
 * gives the MRF launches of a stage ONE record (flops/bytes summed, `launches` counted): 11 events per forward
 * instead of 31 -- an event costs about 3 us of stream time, which is 10 % of a 100-frame forward.
 * Records accumulate over successive forwards until set_profiling is called again (which resets
 * them).  After the stream has been synchronised, read_profile copies up to `capacity` records and
 * returns how many launches were recorded. */
int32_t iris_hifigan_set_profiling(iris_hifigan_handle* h, int32_t enabled);
int32_t iris_hifigan_read_profile(iris_hifigan_handle* h, iris_hifigan_launch_record* out,
                                  int32_t capacity, int32_t* n_launches);
/* paused != 0: forwards record nothing until resumed; the records collected so far are kept (set_profiling would
 * reset them).  For forwards that are captured into a hipGraph (no events inside a capture). */
int32_t iris_hifigan_pause_profiling(iris_hifigan_handle* h, int32_t paused);

/* ---- launch plan of one forward, computed on the host alone (no device, nothing launched) ----
 * Runs the forward's own argument checks, workspace layout and launch planning for [B, in_channels, T] in `dtype` on a
 * chip of `cu_count` compute units (0 = 256, MI355X) and reports every launch it would issue, in order.  Used by the CPU
 * tests (address/undefined-behaviour sanitizer sweeps over the index arithmetic of the plans) and for inspection. */
#define IRIS_HIFIGAN_MAX_PLAN_LAUNCHES 96
typedef struct iris_hifigan_plan_launch {
    char kernel[80];        /* kernel (template) name as the launch site spells it */
    uint32_t grid[3];
    uint32_t block;
    uint64_t lds_bytes;     /* dynamic LDS per block */
} iris_hifigan_plan_launch;
typedef struct iris_hifigan_plan {
    uint64_t workspace_bytes;
    int32_t n_launches;     /* over all passes; may exceed IRIS_HIFIGAN_MAX_PLAN_LAUNCHES: only that many are described */
    int32_t cu_count;
    int32_t passes;         /* sub-batch passes the forward runs as (1 unless B * T exceeds 65,536 frames) */
    int32_t reserved;
    iris_hifigan_plan_launch launches[IRIS_HIFIGAN_MAX_PLAN_LAUNCHES];
} iris_hifigan_plan;
int32_t iris_hifigan_describe_plan(const iris_hifigan_config* cfg, int32_t B, int32_t T, int32_t dtype, int32_t cu_count,
                                   iris_hifigan_plan* out);

/* ---- single-layer entry points (bring-up and parity tests; synchronous, they allocate) ----
 * x_dev/y_dev/res_dev are channels-last [B, L, C]; weights/bias are HOST arrays in the
 * reference's layout. in_act: 0 none, 1 LeakyReLU(slope) applied to the input. */
int32_t iris_hifigan_op_conv1d(const float* x_dev, const float* w_host, const float* bias_host,
                               const float* res_dev, float* y_dev, int32_t B, int32_t L,
                               int32_t C_in, int32_t C_out, int32_t k, int32_t dilation,
                               int32_t in_act, float slope, int32_t x_channels_first, void* stream);
/* ConvTranspose1d(C_in->C_out, k, stride=u, padding=(k-u)/2), weight [C_in, C_out, k]; y is [B, u*L, C_out]. */
int32_t iris_hifigan_op_conv_transpose1d(const float* x_dev, const float* w_host,
                                         const float* bias_host, float* y_dev, int32_t B, int32_t L,
                                         int32_t C_in, int32_t C_out, int32_t k, int32_t u,
                                         int32_t in_act, float slope, void* stream);
/* tanh(Conv1d(C_in->1, k, pad=(k-1)/2)(LeakyReLU((x0+x1+x2)/n_in))): x1/x2 may be NULL (n_in = 1). */
int32_t iris_hifigan_op_conv_post(const float* x0_dev, const float* x1_dev, const float* x2_dev,
                                  const float* w_host, const float* bias_host, float* y_dev,
                                  int32_t B, int32_t L, int32_t C_in, int32_t k, float slope,
                                  void* stream);

/* The stand-alone half of the output stage on its own (csrc/pcm_out.h): fp32 wav_dev [B, L] -> int16 pcm_dev [B, L] by the
 * formulas of iris_hifigan_forward_pcm16.  normalize != 0 first reduces peak_dev [B] (written; may be NULL otherwise) from
 * wav_dev.  lengths_dev (may be NULL) and row_scale >= 1: item b has min(L, lengths[b] * row_scale) samples; the rest of
 * its PCM is 0 and does not count towards its peak.  Items need no alignment (odd L is fine). */
int32_t iris_hifigan_op_pcm16(const float* wav_dev, const int32_t* lengths_dev, int32_t row_scale,
                              int16_t* pcm_dev, float* peak_dev, int32_t B, int32_t L,
                              int32_t normalize, float peak_target, void* stream);

/* fp32 wav_dev [B, L] -> G.711 bytes out_u8_dev [B, L] on a waveform that exists (csrc/pcm_out.h: g711_kernel, 16-byte loads and
 * 4-byte stores with a scalar head and tail, so items need no alignment).  law: IRIS_OUT_ULAW or IRIS_OUT_ALAW, the rules stated
 * at iris_resampler_forward_g711.  lengths_dev and row_scale as in iris_hifigan_op_pcm16; the rest of an item's row holds the
 * law's code for 0.  Synchronises `stream`, as iris_hifigan_op_pcm16 does. */
int32_t iris_hifigan_op_g711(const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev, int32_t row_scale,
                             int32_t law, uint8_t* out_u8_dev, void* stream);

/* One grouped MRF step of the fp32 path -- the hot kernel -- on its own: the three ResBlock branches
 * (kernel sizes k[j] = 3, 7, 11; hifigan_pretrained.py:64-71,130-136) each run
 *     y_j = Conv1d_{k[j], dil[j]}(LeakyReLU(x_j)) (+ res_j)
 * on fp32 channels-last tensors [B, L, C].  mean_dev != NULL makes it the last step of a stage: only
 * ((y_0 + y_1) + y_2) / 3 is stored, into mean_dev (y_dev is then unused).
 * plan: 0 = the library's own choice, 1 = persistent blocks with full-height tiles, 2 = with half-height tiles,
 * 3 = one branch per block, 4 = the small-problem kernel (16 x 16 jobs on v_mfma_f32_16x16x4_f32), 5 / 6 = snake-ordered
 * (tile, branch) jobs at half / full tile height (C >= 128); all of them produce identical bits.  mean_dev is
 * available in plans 0-2.  Returns IRIS_HIFIGAN_UNSUPPORTED when the shape cannot take
 * the requested kernel. */
int32_t iris_hifigan_op_mrf_step(const float* const* x_dev, const float* const* w_host, const float* const* bias_host,
                                 const float* const* res_dev, float* const* y_dev, float* mean_dev,
                                 int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                 float slope, int32_t plan, void* stream);

/* One ResBlock conv PAIR of the three branches in one launch, exact fp32 (csrc/mrf_pair_f32.h, mrf_pair_f32_pf.h; C = 32
 * or 64, k[j] in {3, 7, 11}): y_j = Conv1d_{k[j], 1}(LeakyReLU(Conv1d_{k[j], dil[j]}(LeakyReLU(x_j)))) + x_j
 * (hifigan_pretrained.py:64-71), bit for bit what two iris_hifigan_op_mrf_step calls produce.
 * mode: 0 = one block per (tile, branch) job; 1 = persistent blocks that prefetch the next job's window and draw their
 * jobs from a device counter; 2 = the same with a fixed job stride.
 * mean_dev != NULL (modes 1, 2) makes it the LAST pair of a stage: only ((y_0 + y_1) + y_2) / 3 is stored, into mean_dev
 * (hifigan_pretrained.py:131-137; y_dev is then unused).  No y_dev[i] / mean_dev may alias an x_dev[j].
 * The library carries modes 1 / 2 in the summing form only (as plain pairs they measured slower than mode 0 at every
 * size): modes 1 / 2 without mean_dev return IRIS_HIFIGAN_UNSUPPORTED, as do other shapes. */
int32_t iris_hifigan_op_mrf_pair(const float* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                 const float* const* w2_host, const float* const* b2_host, float* const* y_dev,
                                 float* mean_dev, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                 float slope, int32_t mode, void* stream);

/* bf16 variants of the two layers above (dtype IRIS_HIFIGAN_BF16): x_dev / res_dev / y_dev are bf16
 * channels-last [B, L, C] (C_in % 8 == 0, C_out % 4 == 0); host weights are fp32 in the reference layout and are
 * rounded to bf16 (nearest even); bias stays fp32; accumulation is fp32, one rounding to bf16 at the store.
 * Same reference layers: hifigan_pretrained.py:50-57,64-71 (Conv1d) and :100-108,127-128 (ConvTranspose1d). */
int32_t iris_hifigan_op_conv1d_bf16(const void* x_dev, const float* w_host, const float* bias_host,
                                    const void* res_dev, void* y_dev, int32_t B, int32_t L, int32_t C_in,
                                    int32_t C_out, int32_t k, int32_t dilation, int32_t in_act, float slope,
                                    void* stream);
int32_t iris_hifigan_op_conv_transpose1d_bf16(const void* x_dev, const float* w_host, const float* bias_host,
                                              void* y_dev, int32_t B, int32_t L, int32_t C_in, int32_t C_out,
                                              int32_t k, int32_t u, int32_t in_act, float slope, void* stream);
/* One fused ResBlock conv pair of `n_branches` MRF branches in bf16 storage (hifigan_pretrained.py:64-71, one
 * iteration of the loop):  y_j = Conv1d_{k_j, 1}(LeakyReLU(Conv1d_{k_j, dil_j}(LeakyReLU(x_j)))) + x_j  on bf16
 * channels-last tensors [B, L, C], C = 32, 64 or 128 (the stages where the bf16 path is HBM-bound or at the ridge); the intermediate never
 * leaves the CU.  Same rounding points as the two separate bf16 layers (so: bit-identical to them).  NOT in place: no
 * y_dev[i] may be an x_dev[j] (a block's input window overlaps the rows its neighbours write).
 * Returns IRIS_HIFIGAN_UNSUPPORTED for other channel counts. */
int32_t iris_hifigan_op_mrf_pair_bf16(const void* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                      const float* const* w2_host, const float* const* b2_host, void* const* y_dev,
                                      int32_t n_branches, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                      float slope, void* stream);
/* The LAST conv pair of a stage's three ResBlocks in bf16 storage, summed (hifigan_pretrained.py:64-71 and 131-137): one block
 * runs the pair of all three branches on its rows, rounds each y_j to bf16 as the kernel above stores it, and writes ONE tensor
 * [B, L, C]:  mean_f32 == 0: bf16(LeakyReLU(((y_0 + y_1) + y_2) * fp32(1/3))) -- bit for bit the operand the next
 * ConvTranspose1d builds from the three tensors, which then reads one tensor and applies no activation;  mean_f32 != 0: the
 * fp32 mean itself (conv_post's input after the last stage).  C = 32 or 64 (csrc/mrf_pair_bf16.h); mean_dev must not be an
 * input.  Returns IRIS_HIFIGAN_UNSUPPORTED for other shapes. */
int32_t iris_hifigan_op_mrf_pair_mean_bf16(const void* const* x_dev, const float* const* w1_host, const float* const* b1_host,
                                           const float* const* w2_host, const float* const* b2_host, void* mean_dev,
                                           int32_t mean_f32, int32_t B, int32_t L, int32_t C, const int32_t* k, const int32_t* dil,
                                           float slope, void* stream);
/* the ResBlock Conv1d (C -> C, LeakyReLU on the input, optional residual) with fp32 tensors and split-bf16 products
 * (dtype IRIS_HIFIGAN_F32_SPLIT; C % 32 == 0): hifigan_pretrained.py:50-57,64-71. */
int32_t iris_hifigan_op_conv1d_f32s(const float* x_dev, const float* w_host, const float* bias_host, const float* res_dev,
                                    float* y_dev, int32_t B, int32_t L, int32_t C, int32_t k, int32_t dilation, float slope,
                                    void* stream);
/* LeakyReLU + ConvTranspose1d(C_in -> C_out, k, stride u, padding (k-u)/2) on fp32 tensors with split-bf16 products
 * (the upsamplers in dtype IRIS_HIFIGAN_F32_SPLIT): hifigan_pretrained.py:100-108,127-128. */
int32_t iris_hifigan_op_conv_transpose1d_f32s(const float* x_dev, const float* w_host, const float* bias_host, float* y_dev,
                                              int32_t B, int32_t L, int32_t C_in, int32_t C_out, int32_t k, int32_t u,
                                              float slope, void* stream);

/* ---- PostNet, the layer in front of the vocoder --------------------------
 * Replaces `postnet(mel_bt_f, training=False)` (scripts/synthesize.py:148-166; model src/iris/postnet.py:48-67):
 * num_layers Conv1D(kernel_size, 'same') layers over time, the first num_layers-1 with `channels`
 * filters + BatchNorm + tanh, the last back to n_mels + BatchNorm; output = mel + residual.
 * `weights_host`: per layer, weight [C_out, C_in, k] then bias [C_out], with the inference BatchNorm
 * already folded in (w' = w*g/sqrt(var+eps), b' = (b-mean)*g/sqrt(var+eps)+beta).                     */
typedef struct iris_postnet_handle iris_postnet_handle;
int32_t iris_postnet_create(int32_t n_mels, int32_t num_layers, int32_t channels, int32_t kernel_size,
                            const float* weights_host, uint64_t n_weights, iris_postnet_handle** out);
int32_t iris_postnet_destroy(iris_postnet_handle* h);
int32_t iris_postnet_workspace_bytes(const iris_postnet_handle* h, int32_t B, int32_t T, uint64_t* bytes);
/* mel_dev, out_dev: [B, n_mels, T] fp32 (channels-first, like the reference); asynchronous on `stream`. */
int32_t iris_postnet_forward(iris_postnet_handle* h, const void* mel_dev, int32_t B, int32_t T,
                             void* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* Ragged batch: mels of different lengths refined in one call (the PostNet half of iris_hifigan_forward_ragged).
 * mel_dev, out_dev [B, n_mels, T] fp32 channels-first, lengths_dev [B] int32 on the device (caller-owned, like mel_dev);
 * lengths are clamped to [0, T] on the device.
 * Item b is computed exactly as iris_postnet_forward of mel[b, :, :lengths[b]] alone would compute it, bit for bit: every
 * layer's 'same' padding ends at the item's own length. Mel frames >= lengths[b] are never read, so they may hold
 * anything, NaN included. out[b, :, lengths[b]:T] is written as 0.0f.
 * The host never reads the lengths: the launch plan is the one of iris_postnet_forward(B, T), and tiles past an item's
 * length return at once on the device. Workspace as iris_postnet_workspace_bytes(B, T).
 * Asynchronous on `stream`, allocates nothing, safe inside a stream capture.
 * lengths_dev == NULL (B, T > 0) returns IRIS_HIFIGAN_INVALID_ARGUMENT; B > 65535 returns IRIS_HIFIGAN_UNSUPPORTED, as
 * iris_postnet_forward does. */
int32_t iris_postnet_forward_ragged(iris_postnet_handle* h, const void* mel_dev, int32_t B, int32_t T,
                                    const int32_t* lengths_dev, void* out_dev,
                                    void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- sample-rate conversion behind conv_post (csrc/resample.h) ---------------------------------------
 * The generator produces 22 050 Hz; the reference never resamples (it only labels the WAV with --sample_rate), so there
 * is no reference for this stage: the contract is the filter below and its exact host restatement
 * (iris.resample.resample_host), which the device matches bit for bit.
 *   g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, s = min(1, up / down), fc = rolloff * s,
 *   Hw = ceil(zeros / s) (half_width), taps = 2 * Hw
 *   bank[p][j] = fc * sinc(fc * t) * I0(beta * sqrt(1 - (t / Hw)^2)) / I0(beta),  t = (j - Hw + 1) - p / up,
 *                sinc(x) = sin(pi x) / (pi x), 0 where |t| > Hw; evaluated in double, rounded once to fp32
 *   out[n]     = the chain over j = 0 .. taps - 1, ascending, of acc = fmaf(x[i0 - Hw + 1 + j], bank[p][j], acc) from
 *                acc = 0.0f, with i0 = floor(n * down / up) and p = (n * down) mod up
 * n and the index of x are utterance-global: a call passes `origin` >= 0, the global index of wav[:, 0], and its L
 * samples produce exactly the outputs n with origin <= n * down / up < origin + L, i.e.
 * n_lo = ceil(origin * up / down) .. ceil((origin + L) * up / down) - 1 (with origin 0: ceil(L * up / down) of them), so
 * consecutive windows partition the output, and a window that carries Hw samples of context on each side reproduces the
 * one-shot samples of its interior.  x outside the item's own samples reads as 0.
 * zeros, beta, rolloff: 0 takes the default (16, 9.0, 0.945); negative values, rolloff > 1, rates < 1 and
 * rate_out == rate_in return IRIS_HIFIGAN_INVALID_ARGUMENT.  Configurations outside 4000 <= rate_out <= 192000,
 * up <= 640, taps <= 256 (or whose input span of 1024 outputs exceeds 64 KB) return IRIS_HIFIGAN_UNSUPPORTED; from
 * 22 050 Hz that admits 8000, 11 025, 16 000, 24 000, 32 000, 44 100 and 48 000. */
typedef struct iris_resampler_handle iris_resampler_handle;

/* Host only (no device): the sizes, and with bank_host != NULL (capacity >= up * taps floats) the bank [up][taps]. */
int32_t iris_resampler_design(int32_t rate_in, int32_t rate_out, int32_t zeros, double beta, double rolloff,
                              int32_t* up, int32_t* down, int32_t* taps, float* bank_host, uint64_t capacity);
/* Designs the bank by the same function and uploads it to the current HIP device. */
int32_t iris_resampler_create(int32_t rate_in, int32_t rate_out, int32_t zeros, double beta, double rolloff,
                              iris_resampler_handle** out);
int32_t iris_resampler_destroy(iris_resampler_handle* h);
int32_t iris_resampler_info(const iris_resampler_handle* h, int32_t* up, int32_t* down, int32_t* taps, int32_t* half_width);
/* Host only: the first global output and the number of outputs of a window of L samples at `origin` (both in [0, 2^40]). */
int32_t iris_resampler_out_range(const iris_resampler_handle* h, int64_t origin, int64_t L, int64_t* n_lo, int64_t* n_count);
/* wav_dev [B, L] fp32 -> [B, n_count] (iris_resampler_out_range(origin, L)), in ONE of three forms:
 *   normalize == 0, out_f32_dev:  the fp32 samples;
 *   normalize == 0, out_pcm_dev:  int16, (int16) rintf(clamp(out, -1, 1) * 32767) -- the output stage's plain formula;
 *   normalize != 0:               out_f32_dev receives the fp32 samples, peak_dev [B] the items' max |out| over their own
 *                                 outputs (0 for an empty item) and out_pcm_dev the output stage's normalised formula
 *                                 applied to them, q = (out / (peak[b] + 1e-8f)) * peak_target; all three are required and
 *                                 peak_target must lie in (0, 1].  The kernel reduces the peaks beside its store and the
 *                                 output stage's second kernel converts.
 * Giving neither or both outputs without normalize, or NULL wav_dev (B, L > 0), returns IRIS_HIFIGAN_INVALID_ARGUMENT.
 * lengths_dev (may be NULL) and row_scale >= 1 as in iris_hifigan_op_pcm16: item b owns min(L, lengths[b] * row_scale)
 * input samples; samples past that are never read (they may hold NaN), the item is computed bit for bit as a call on its
 * own samples alone, and its outputs past its own count ceil((origin + own) * up / down) - n_lo are 0.
 * Asynchronous on `stream`, allocates nothing, safe inside a stream capture (a normalising call queues one memset of its
 * peaks).  B == 0 or L == 0 returns IRIS_HIFIGAN_OK; B > 65535, L > 2^30 or more than 2^31 - 1 outputs per item return
 * IRIS_HIFIGAN_UNSUPPORTED.  The handle belongs to the device that was current in iris_resampler_create. */
int32_t iris_resampler_forward(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t L,
                               const int32_t* lengths_dev /* NULL = plain batch */, int32_t row_scale, int64_t origin,
                               float* out_f32_dev, int16_t* out_pcm_dev, float* peak_dev,
                               int32_t normalize, float peak_target, void* stream);

/* Output forms of the entry points below.  G.711 (telephony: one byte per sample) is an integer function of the 16-bit sample
 * s = (int16) rintf(clamp(out, -1, 1) * 32767), restated in numpy by iris.synthesis_output.ulaw_from_pcm16 / alaw_from_pcm16:
 *   mu-law  sign = s < 0;  m = min(|s|, 32635) + 132 (|s| in 32 bits);  e = floor(log2 m) - 7;  mant = (m >> (e + 3)) & 15;
 *           byte = ~(sign << 7 | e << 4 | mant) & 0xFF
 *   A-law   a = s >> 3 (arithmetic);  a < 0: a = ~a, mask = 0x55, else mask = 0xD5;  seg = a < 32 ? 0 : floor(log2 a) - 4;
 *           mant = seg < 2 ? (a >> 1) & 15 : (a >> seg) & 15;  byte = (seg << 4 | mant) ^ mask
 * Sample 0 has the code 0xFF (mu-law) / 0xD5 (A-law), and that -- never byte 0, which decodes to -32 124 -- is what fills a
 * ragged item's row behind its own samples.  The A-law rule is the common table-free encoder (CPython's audioop.lin2alaw on all
 * 65 536 inputs); the mu-law rule is the G.711 one on the 16-bit magnitude and differs from audioop.lin2ulaw at 381 inputs. */
enum {
    IRIS_OUT_F32 = 0,
    IRIS_OUT_PCM16 = 1,
    IRIS_OUT_ULAW = 3,
    IRIS_OUT_ALAW = 4
};

/* iris_resampler_forward in a fourth form, G.711 bytes: wav_dev [B, L] -> out_u8_dev [B, n_count], `law`
 * IRIS_OUT_ULAW or IRIS_OUT_ALAW, everything else -- origin, lengths_dev, row_scale, the limits, the one launch -- as there.
 * Bit for bit the law of the int16 form's samples; an item's row behind its own outputs holds the law's code for 0. */
int32_t iris_resampler_forward_g711(iris_resampler_handle* h, const float* wav_dev, int32_t B, int32_t L,
                                    const int32_t* lengths_dev /* NULL = plain batch */, int32_t row_scale, int64_t origin,
                                    int32_t law, uint8_t* out_u8_dev, void* stream);

/* Windows: the resampler on samples [origin, origin + Lw) of B utterances of one length, for a caller that receives the
 * waveform piece by piece (iris.resample.ResamplerSession).  With Hw = half_width and i0(n) = floor(n * down / up), output n
 * reads x[i0(n) - Hw + 1 .. i0(n) + Hw] and nothing else.  n_next is the first output not yet emitted; `final` (0 or not) says
 * that origin + Lw is the utterance's end.  The rule (csrc/resample.h: struct Window):
 *     n_hi = ceil((origin + Lw) * up / down) if final, else ceil(max(0, origin + Lw - Hw) * up / down)
 *            -- the outputs whose last tap lies inside the window;
 *     the window emits [n_next, n_hi): max(0, n_hi - n_next) outputs;
 *     keep_from = max(0, i0(n_hi) - Hw + 1): the first sample the next window must still hold.
 * Precondition: origin == 0, or i0(n_next) - Hw + 1 >= origin -- the first tap of the first output is held; otherwise, or with
 * origin, Lw outside [0, 2^40] or n_next outside [0, ceil((origin + Lw) * up / down)], IRIS_HIFIGAN_INVALID_ARGUMENT.  The window
 * forms no sample in front of sample 0 and, when final, none past the end: those read as 0 exactly as the whole call reads them,
 * so the concatenation of an utterance's windows is iris_resampler_forward of the whole, bit for bit, in every form.
 * window_plan is host only.  forward_window: wav_dev [B, Lw] -> out_dev [B, n_hi - n_next], packed rows of fp32, int16 or
 * bytes by out_form (IRIS_OUT_F32, _PCM16, _ULAW, _ALAW; there is no normalised form: the peak belongs to the whole item).  ONE
 * launch of the whole call's kernel -- iris_resampler_forward is the case final, n_next = ceil(origin * up / down) of the same
 * launch builder, without the precondition -- no workspace, nothing allocated, asynchronous on `stream`, safe inside a stream
 * capture.  B == 0, Lw == 0 or a count of 0 launch nothing and return IRIS_HIFIGAN_OK; B > 65535 and Lw > 2^30 return
 * IRIS_HIFIGAN_UNSUPPORTED; a NULL pointer or out_dev off its type's bytes IRIS_HIFIGAN_INVALID_ARGUMENT. */
int32_t iris_resampler_window_plan(const iris_resampler_handle* h, int64_t origin, int64_t Lw, int64_t n_next, int32_t final,
                                   int64_t* n_hi, int64_t* keep_from);
int32_t iris_resampler_forward_window(iris_resampler_handle* h, const float* wav_dev /* [B, Lw] */, int32_t B, int32_t Lw,
                                      int64_t origin, int64_t n_next, int32_t final, void* out_dev, int32_t out_form, void* stream);

/* ---- VAE decoder in front of the PostNet (csrc/vae_decoder.h) ------------------------------------------
 * The inference half of the reference's TextConditionedVAE (src/iris/vae.py:448-482, generate()): frame-level text
 * conditioning [B, T, cond_dim] and a latent prior sample [B, T / 2^down_stages, latent_dim] in, the mel [B, n_mels, T]
 * (channels-first: what iris_postnet_forward and iris_hifigan_forward read) and optionally the frame residual
 * [B, T, cond_dim] out.  fp32 throughout.
 * weights_host, in this order, every tensor followed by its bias (Dense and Conv1D kernels transposed to
 * [C_out][C_in][k] unless stated; iris.vae.TextConditionedVAE.blob() writes it, iris_vae_decoder_weight_count sizes it):
 *   down_cond_proj; downsample.blocks[s] (k = 5) for each stage;
 *   per coupling j: cond_proj [latent/2][C]; then in the Keras layouts net_pre [3][latent/2][flow_hidden],
 *                   net_post [flow_hidden][latent/2], film.proj [latent/2][latent];
 *   latent_dec_proj in the Keras layout [latent][C];
 *   per decoder block: conv (k = wavenet_kernel_size, dilation 2^(i % 4)); film.proj [2C][C]; res_proj;
 *   upsample.refine[s] (k = 5) for each stage; out_proj; residual_proj.
 * Configurations the kernels cannot take -- cond_dim or model_channels not a multiple of 4, model_channels > 256, an even
 * wavenet_kernel_size, a tile beyond the 160 KB LDS -- return IRIS_HIFIGAN_UNSUPPORTED; an odd latent_dim, a wrong blob size
 * and a T that is not a multiple of 2^down_stages return IRIS_HIFIGAN_INVALID_ARGUMENT (the caller pads, as
 * scripts/synthesize.py:117-122 does); a short workspace returns IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches. */
typedef struct iris_vae_decoder_config {
    int32_t n_mels, cond_dim, model_channels, latent_dim, decoder_blocks, wavenet_kernel_size, down_stages, flow_layers,
            flow_hidden;
} iris_vae_decoder_config;
typedef struct iris_vae_decoder_handle iris_vae_decoder_handle;

/* Host only. */
int32_t iris_vae_decoder_weight_count(const iris_vae_decoder_config* cfg, uint64_t* count);
int32_t iris_vae_decoder_create(const iris_vae_decoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                iris_vae_decoder_handle** out);
int32_t iris_vae_decoder_destroy(iris_vae_decoder_handle* h);
int32_t iris_vae_decoder_workspace_bytes(const iris_vae_decoder_handle* h, int32_t B, int32_t T, uint64_t* bytes);
/* Asynchronous on `stream`, allocates nothing.  residual_out_dev may be NULL: residual_proj is then not launched and the
 * mel is bit for bit the same. */
int32_t iris_vae_decoder_forward(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_prior_dev, int32_t B, int32_t T,
                                 float* mel_out_dev, float* residual_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                 void* stream);

/* Ragged batch: utterances of different lengths decoded in one call (the VAE half of iris_postnet_forward_ragged).
 * cond_dev [B, T, cond_dim], z_prior_dev [B, T / 2^down_stages, latent_dim], mel_out_dev [B, n_mels, T], residual_out_dev
 * [B, T, cond_dim] (may be NULL) as in iris_vae_decoder_forward; lengths_dev [B] int32 on the device (caller-owned, like
 * cond_dev): item b's frames at the full rate.  Lengths are sanitised on the device: clamped to [0, T], then rounded down
 * to a multiple of 2^down_stages (the stride-2 'same' padding is defined for even lengths, and the caller pads an
 * utterance to that multiple as for the dense call), giving len_b.
 * Item b is computed exactly as iris_vae_decoder_forward of cond[b, :len_b] and z_prior[b, :len_b >> down_stages] alone
 * would compute it, bit for bit: at every level of the stack -- conditioning and mel rows, the rows after each stride-2
 * stage and each x2 upsample, the latent rows -- the 'same' padding ends at the item's own length.  cond[b, len_b:, :]
 * and z_prior[b, len_b >> down_stages:, :] are never read, so they may hold anything, NaN included.
 * mel[b, :, len_b:T] and residual[b, len_b:T, :] are written as 0.0f.
 * The host never reads the lengths: launch plan, launch count and workspace are those of iris_vae_decoder_forward(B, T)
 * (iris_vae_decoder_launch_count, iris_vae_decoder_workspace_bytes), and blocks past an item's length return at once on
 * the device.  Workspace rows past an item's length are neither written nor read.
 * Asynchronous on `stream`, allocates nothing, safe inside a stream capture.
 * lengths_dev == NULL (B, T > 0) returns IRIS_HIFIGAN_INVALID_ARGUMENT; shape and workspace errors are those of
 * iris_vae_decoder_forward.  No failing call launches. */
int32_t iris_vae_decoder_forward_ragged(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_prior_dev, int32_t B,
                                        int32_t T, const int32_t* lengths_dev, float* mel_out_dev, float* residual_out_dev,
                                        void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* The decoder half of TextConditionedVAE.call(training=False) (vae.py:401-422): z_dev [B, T / 2^down_stages, latent_dim] is a
 * posterior latent (the mean that iris_vae_encoder_forward writes) and the flow runs FORWARDS -- couplings 0 .. n - 1,
 * y2 = x2 + t -- where iris_vae_decoder_forward runs it in reverse.  Everything else is iris_vae_decoder_forward: the same
 * plan, launches (iris_vae_decoder_launch_count), workspace, outputs, checks and errors. */
int32_t iris_vae_decoder_forward_posterior(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_dev, int32_t B, int32_t T,
                                           float* mel_out_dev, float* residual_out_dev, void* workspace_dev,
                                           uint64_t workspace_bytes, void* stream);
/* iris_vae_decoder_forward_posterior over a ragged batch: lengths_dev, its sanitising, what is read, what is written as 0.0f,
 * the plan, the checks and the errors are those of iris_vae_decoder_forward_ragged; the flow runs forwards.  Item b is bit
 * for bit iris_vae_decoder_forward_posterior of cond[b, :len_b] and z[b, :len_b >> down_stages] alone. */
int32_t iris_vae_decoder_forward_posterior_ragged(iris_vae_decoder_handle* h, const float* cond_dev, const float* z_dev, int32_t B,
                                                  int32_t T, const int32_t* lengths_dev, float* mel_out_dev, float* residual_out_dev,
                                                  void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* Host only: kernel launches of one forward that asks for the residual (one fewer without it):
 * 3 + 2 * down_stages + decoder_blocks + 2. */
int32_t iris_vae_decoder_launch_count(const iris_vae_decoder_handle* h, int32_t B, int32_t T, int32_t* n);
/* Host only, for tests: where a forward of (B, T) leaves an intermediate [B, T / 2^down_stages, model_channels] in its
 * workspace (valid until the next forward on that workspace).  After iris_vae_decoder_forward_ragged the rows of item b
 * from len_b >> down_stages on are undefined: the ragged call neither writes nor reads them. */
#define IRIS_VAE_TAP_LAT_COND 0   /* downsample(down_cond_proj(cond)) */
#define IRIS_VAE_TAP_DEC_IN 1     /* latent_dec_proj(flow(z_prior, reverse)) */
#define IRIS_VAE_TAP_DEC_OUT 2    /* after the last decoder block */
int32_t iris_vae_decoder_tap(const iris_vae_decoder_handle* h, int32_t B, int32_t T, int32_t which, uint64_t* byte_offset,
                             uint64_t* floats);

/* ---- VAE posterior encoder (csrc/iris_vae_encoder.hip over csrc/vae_decoder.h) ------------------------------------
 * The encoder half of TextConditionedVAE.call(training=False) (src/iris/vae.py:381-398): a mel [B, n_mels, T] (channels-first,
 * as the PostNet and the vocoder hold it; it is never transposed in memory) and its frame conditioning [B, T, cond_dim] in,
 * the posterior statistics mean and logvar, [B, T / 2^down_stages, latent_dim] each, out.  z = mean at inference, so
 * iris_vae_decoder_forward_posterior(cond, mean) completes call(): reconstruction and residual.  fp32, inference only.
 * weights_host, in this order, every tensor followed by its bias (Dense and Conv1D kernels transposed to [C_out][C_in][k]):
 *   in_proj [C][n_mels][1];
 *   per encoder block i: conv (k = wavenet_kernel_size, dilation 2^(i % 4)); film.proj [2C][cond_dim]; res_proj;
 *   downsample.blocks[s] (k = 5) for each stage -- the tensors the decoder's blob holds too: the reference has one set;
 *   latent_mean_proj [latent_dim][C]; latent_logvar_proj [latent_dim][C].
 * num_wavenet_blocks + down_stages + 3 launches (one fewer with no block: there is no FiLM GEMM then).
 * Configurations the kernels cannot take -- n_mels, cond_dim, model_channels or latent_dim not a multiple of 4,
 * model_channels > 256, an even wavenet_kernel_size, a tile beyond the 160 KB LDS -- return IRIS_HIFIGAN_UNSUPPORTED; a wrong
 * blob size and a T that is not a multiple of 2^down_stages return IRIS_HIFIGAN_INVALID_ARGUMENT; a short workspace returns
 * IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches. */
typedef struct iris_vae_encoder_config {
    int32_t n_mels, cond_dim, model_channels, latent_dim, num_wavenet_blocks, wavenet_kernel_size, down_stages;
} iris_vae_encoder_config;
typedef struct iris_vae_encoder_handle iris_vae_encoder_handle;

/* Host only. */
int32_t iris_vae_encoder_weight_count(const iris_vae_encoder_config* cfg, uint64_t* count);
int32_t iris_vae_encoder_create(const iris_vae_encoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                iris_vae_encoder_handle** out);
int32_t iris_vae_encoder_destroy(iris_vae_encoder_handle* h);
int32_t iris_vae_encoder_workspace_bytes(const iris_vae_encoder_handle* h, int32_t B, int32_t T, uint64_t* bytes);
/* Asynchronous on `stream`, allocates nothing.  mel_dev and cond_dev are only read. */
int32_t iris_vae_encoder_forward(iris_vae_encoder_handle* h, const float* mel_dev, const float* cond_dev, int32_t B, int32_t T,
                                 float* mean_out_dev, float* logvar_out_dev, void* workspace_dev, uint64_t workspace_bytes,
                                 void* stream);
/* Ragged batch: recorded utterances of different lengths encoded in one call (the posterior half of
 * iris_vae_decoder_forward_ragged, and with the same semantics).  mel_dev [B, n_mels, T], cond_dev [B, T, cond_dim] and the
 * outputs [B, T / 2^down_stages, latent_dim] as in the dense call; lengths_dev [B] int32 on the device (caller-owned): item
 * b's frames at the full rate, sanitised on the device -- clamped to [0, T], then rounded down to a multiple of
 * 2^down_stages -- giving len_b.
 * Item b is computed exactly as the dense call on mel[b, :, :len_b] and cond[b, :len_b] alone would compute it, bit for
 * bit: at every level the 'same' padding ends at the item's own length.  mel[b, :, len_b:] and cond[b, len_b:, :] are
 * never read, so they may hold anything, NaN included; workspace rows past an item's length are neither written nor read
 * (the taps below are undefined there).  mean[b, len_b >> down_stages:, :] and logvar[b, len_b >> down_stages:, :] are
 * written as 0.0f: such a row adds exactly 0 to the KL sum of iris_vae_losses.
 * The host never reads the lengths: launches, grids and workspace are the dense call's for (B, T), and the launch count
 * and workspace queries above and below hold for both calls.  Asynchronous on `stream`, allocates nothing, safe inside a
 * stream capture.  lengths_dev == NULL (B, T > 0) returns IRIS_HIFIGAN_INVALID_ARGUMENT; shape and workspace errors are the
 * dense call's.  No failing call launches.  (Named outside the iris_vae_encoder_ family, whose seven functions are the
 * dense stage; it takes that stage's handle.) */
int32_t iris_vae_posterior_encode_ragged(iris_vae_encoder_handle* h, const float* mel_dev, const float* cond_dev, int32_t B, int32_t T,
                                        const int32_t* lengths_dev, float* mean_out_dev, float* logvar_out_dev,
                                        void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* Host only: kernel launches of one forward (a dry run of the forward's own code). */
int32_t iris_vae_encoder_launch_count(const iris_vae_encoder_handle* h, int32_t B, int32_t T, int32_t* n);
/* Host only, for tests: where a forward of (B, T) leaves an intermediate in its workspace (valid until the next forward on
 * that workspace): [B, T, model_channels], or [B, T / 2^down_stages, model_channels] for LAT_H. */
#define IRIS_VAE_ENC_TAP_H_IN 0    /* in_proj(mel^T) */
#define IRIS_VAE_ENC_TAP_H_OUT 1   /* after the last encoder block */
#define IRIS_VAE_ENC_TAP_LAT_H 2   /* downsample(h) */
int32_t iris_vae_encoder_tap(const iris_vae_encoder_handle* h, int32_t B, int32_t T, int32_t which, uint64_t* byte_offset,
                             uint64_t* floats);

/* ---- Masked VAE losses of a reconstruction (csrc/vae_losses.h) -----------------------------------------------------
 * TextConditionedVAE.compute_recon_l1 and compute_kl (src/iris/vae.py:424-446) as scripts/train_vae.py:94-103 calls them,
 * reduced on the device: target_dev and recon_dev [B, n_mels, T] (channels-first), mean_dev and logvar_dev
 * [B, T / 2^down_stages, latent_dim], lengths_dev [B] int32 on the device or NULL.  out_dev holds 2 + 2B floats:
 *   out[0]          the reconstruction L1,  sum_b sum_{t < len_b} |target - recon|  /  (sum_b len_b * n_mels + 1e-6)
 *   out[1]          the KL,  sum_b sum -0.5 (1 + logvar - mean^2 - exp(logvar)) over latent rows < len_b >> down_stages and
 *                   every channel  /  (sum_b (len_b >> down_stages) + 1e-8)  -- rows, not rows x channels: the reference's own
 *   out[2 + b]      item b's L1 sum (the numerator's part);  out[2 + B + b]  item b's KL sum.
 * len_b is lengths_dev[b] sanitised as the ragged forwards sanitise it (clamped to [0, T], rounded down to a multiple of
 * 2^down_stages); nothing at or past an item's length is read, in any of the four tensors.  lengths_dev == NULL: both are
 * the plain means over all elements (ops.mean), and the item sums cover whole items.
 * Terms are computed in fp32 and added in fp64 in a fixed order (fixed tiles counted from each item's row 0, a fixed tree
 * inside a tile, tiles in order, items in order; no floating-point atomics): two calls give the same bits, and item b's
 * two sums are bit for bit those of the call on its own rows alone, whatever T it is padded to.  An all-empty batch gives
 * 0 / (0 + eps) = 0.  Two launches (one when B == 0 or T == 0), asynchronous on `stream`, on the current device; allocates
 * nothing.  workspace_dev: iris_vae_losses_workspace_bytes bytes, aligned to 8.
 * A NULL pointer, a negative size and a T that is not a multiple of 2^down_stages return IRIS_HIFIGAN_INVALID_ARGUMENT,
 * B > 65535 and down_stages > 8 IRIS_HIFIGAN_UNSUPPORTED, a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call
 * launches. */
int32_t iris_vae_losses_workspace_bytes(int32_t B, int32_t n_mels, int32_t T, int32_t latent_dim, int32_t down_stages, uint64_t* bytes);
int32_t iris_vae_losses(const float* target_dev, const float* recon_dev, const float* mean_dev, const float* logvar_dev, int32_t B,
                        int32_t n_mels, int32_t T, int32_t latent_dim, int32_t down_stages, const int32_t* lengths_dev /* or NULL */,
                        float* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Phoneme encoder, duration head and length regulator in front of the VAE decoder (csrc/text_encoder.h) ----
 * The text side of the reference's scripts/synthesize.py:93-122: phoneme ids [B, P] -> encoder output [B, P, embed_dim]
 * (PhonemeEncoder, src/iris/encoder.py:115-212) -> softplus duration output [B, P] and integer frames
 * clip(rint(exp(pred) - 1), 1, max_frames_per_phoneme) (DurationPredictor, :228-315; predict_durations,
 * synthesize.py:41-45) -> frame conditioning [B, T_pad, embed_dim] (length regulator, synthesize.py:48-61, 112-122),
 * which iris_vae_decoder_forward reads.  fp32, inference only (dropout is the identity).
 * lengths_dev (int32 [B], may be NULL = every item has P phonemes): item b owns its first lengths[b] positions.  Keys past
 * them have attention weight exactly 0, the duration head's 'same' padding starts at them, and every output row past them
 * is 0 (frames included): item b is bit for bit what a batch of one computes from its own ids.
 * Encoder weights_host, in this order (iris.encoder.PhonemeEncoder.blob() writes it): phoneme_embedding [vocab][E];
 * position_embedding [max_length][E]; per block: query|key|value kernels as one [3E][E] matrix (row = output column
 * h * key_dim + d of q, then of k, then of v) and its bias [3E]; attention output [E][H * key_dim] + bias; attention_norm
 * gamma, beta; ffn.0 [F][E] + bias; ffn.2 [E][F] + bias; ffn_norm gamma, beta; then encoder_output_norm gamma, beta.
 * Duration weights_host (iris.encoder.DurationPredictor.blob()): per layer duration_conv [hidden][C_in][k] + bias and
 * duration_norm gamma, beta; then duration_output [C] + bias [1].
 * Configurations the kernels cannot take -- embed_dim not a multiple of num_heads, key_dim not a multiple of 8 or above 128,
 * a channel count that is not a multiple of 4, embed_dim or hidden_dim above 256, an even kernel_size -- return
 * IRIS_HIFIGAN_UNSUPPORTED; P < 1, P > max_length, a wrong blob size and a NULL pointer return
 * IRIS_HIFIGAN_INVALID_ARGUMENT; a short workspace returns IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches.
 * The ids must lie in [0, vocab_size): the kernel clamps, so a bad id reads a wrong row but never outside the table. */
typedef struct iris_phoneme_encoder_config {
    int32_t vocab_size, embed_dim, num_blocks, num_heads, ffn_dim, max_length;
} iris_phoneme_encoder_config;
typedef struct iris_duration_predictor_config {
    int32_t in_dim, hidden_dim, num_layers, kernel_size, max_frames_per_phoneme;
} iris_duration_predictor_config;
typedef struct iris_phoneme_encoder_handle iris_phoneme_encoder_handle;
typedef struct iris_duration_predictor_handle iris_duration_predictor_handle;

/* Host only (no device is needed): sizes, and the kernel launches of one forward -- 5 * num_blocks + 2 for the encoder,
 * num_layers + 2 for the duration head (its scan included). */
int32_t iris_phoneme_encoder_weight_count(const iris_phoneme_encoder_config* cfg, uint64_t* count);
int32_t iris_phoneme_encoder_workspace_bytes(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, uint64_t* bytes);
int32_t iris_phoneme_encoder_launch_count(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, int32_t* n);
int32_t iris_phoneme_encoder_create(const iris_phoneme_encoder_config* cfg, const float* weights_host, uint64_t n_weights,
                                    iris_phoneme_encoder_handle** out);
int32_t iris_phoneme_encoder_destroy(iris_phoneme_encoder_handle* h);
/* Asynchronous on `stream`, allocates nothing. */
int32_t iris_phoneme_encoder_forward(iris_phoneme_encoder_handle* h, const int32_t* ids_dev, const int32_t* lengths_dev, int32_t B,
                                     int32_t P, float* enc_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* Host only, for tests: where a forward of (B, P) leaves the output of block 0, [B, P, embed_dim], in its workspace. */
int32_t iris_phoneme_encoder_tap(const iris_phoneme_encoder_config* cfg, int32_t B, int32_t P, uint64_t* byte_offset, uint64_t* floats);

int32_t iris_duration_predictor_weight_count(const iris_duration_predictor_config* cfg, uint64_t* count);
int32_t iris_duration_predictor_workspace_bytes(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, uint64_t* bytes);
int32_t iris_duration_predictor_launch_count(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, int32_t* n);
int32_t iris_duration_predictor_create(const iris_duration_predictor_config* cfg, const float* weights_host, uint64_t n_weights,
                                       iris_duration_predictor_handle** out);
int32_t iris_duration_predictor_destroy(iris_duration_predictor_handle* h);
/* enc_out [B, P, in_dim] -> pred float [B, P], frames int32 [B, P], offsets int32 [B, P + 1] (the exclusive prefix sum of
 * the item's frames; entries from lengths[b] on hold the total) and totals int32 [B].  P * max_frames_per_phoneme must fit
 * int32 (IRIS_HIFIGAN_INVALID_ARGUMENT otherwise).  Asynchronous on `stream`, allocates nothing. */
int32_t iris_duration_predictor_forward(iris_duration_predictor_handle* h, const float* enc_out_dev, const int32_t* lengths_dev,
                                        int32_t B, int32_t P, float* pred_dev, int32_t* frames_dev, int32_t* offsets_dev,
                                        int32_t* totals_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* Host only, for tests: where a forward of (B, P) leaves the output of the first layer, [B, P, hidden_dim]. */
int32_t iris_duration_predictor_tap(const iris_duration_predictor_config* cfg, int32_t B, int32_t P, uint64_t* byte_offset,
                                    uint64_t* floats);

/* Stateless.  iris_length_scan: the head's scan alone, for frames that come from elsewhere (an aligner): negative entries
 * count as 0 and the caller keeps each item's sum within int32.  iris_length_regulate: cond[b, t, :] = enc_out[b, p, :]
 * for offsets[b, p] <= t < offsets[b, p + 1], and 0 for totals[b] <= t < T_pad; E must be a multiple of 4.  The caller
 * chooses T_pad (ceil(max(totals) / 2^down_stages) * 2^down_stages for the VAE decoder), which takes the one read-back
 * of the stage: totals. */
int32_t iris_length_scan(const int32_t* frames_dev, const int32_t* lengths_dev, int32_t B, int32_t P, int32_t* offsets_dev,
                         int32_t* totals_dev, void* stream);
int32_t iris_length_regulate(const float* enc_out_dev, const int32_t* offsets_dev, const int32_t* totals_dev, int32_t B, int32_t P,
                             int32_t E, int32_t T_pad, float* cond_dev, void* stream);

/* ---- Mel front-end: waveform to log-mel in front of the posterior encoder (csrc/mel_frontend.h) --------------------
 * The reference's compute_mel_spectrogram (src/iris/data.py:25-67): librosa 0.11's melspectrogram(power=1.0) and
 * log(max(mel, 1e-5)).  audio [B, L] -> mel [B, n_mels, T], T = 1 + L / hop_length, channels-first as every consumer reads it.
 *   frame t covers samples [t * hop - n_fft / 2, t * hop + n_fft / 2) of its item, 0 outside the item (center=True,
 *   pad_mode="constant"); periodic Hann of win_length centred in n_fft; magnitudes of bins 0 .. n_fft / 2; Slaney mel scale
 *   and area normalisation (htk=False, norm="slaney"); fmax <= 0 means sample_rate / 2.
 * Samples are fp32, or int16 taken as x * (1.0f / 32768) (what a 16-bit WAV reads as): bit for bit the fp32 call on those.
 * One launch; magnitudes stay in LDS.  hop_length that does not divide n_fft or is no multiple of 4, win_length > n_fft,
 * n_fft > 4096, and a config whose sample window and magnitude tile exceed 160 KB of LDS return IRIS_HIFIGAN_UNSUPPORTED
 * (from every function below that takes the config; create reports it before it touches the device); a NULL pointer, a
 * negative shape and an unknown sample format IRIS_HIFIGAN_INVALID_ARGUMENT; a short workspace
 * IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches.  audio_dev may be NULL when L == 0 (every item is one frame
 * of zeros). */
typedef struct iris_mel_frontend_config {
    int32_t sample_rate, n_fft, hop_length, win_length, n_mels, reserved;
    double fmin, fmax;
} iris_mel_frontend_config;
typedef struct iris_mel_frontend_handle iris_mel_frontend_handle;
#define IRIS_MEL_SAMPLES_F32 0
#define IRIS_MEL_SAMPLES_I16 1

/* Host only (no device is needed).  design: *n_bins = n_fft / 2 + 1 and, where the pointers are not NULL, the fp32 tables
 * the handle uploads -- dft_host [2][n_bins][n_fft]: w[n] cos(2 pi k n / n_fft), then w[n] sin(2 pi k n / n_fft), evaluated in
 * double with the angle reduced by (k n) mod n_fft and rounded once; fb_host [n_mels][n_bins].  launch_count: a dry run of the
 * forward's own code. */
int32_t iris_mel_frontend_design(const iris_mel_frontend_config* cfg, int32_t* n_bins, float* dft_host, uint64_t dft_floats,
                                 float* fb_host, uint64_t fb_floats);
int32_t iris_mel_frontend_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, uint64_t* bytes);
int32_t iris_mel_frontend_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, int32_t* n);
/* create: on the current device, which becomes the handle's.  The forwards are asynchronous on `stream`, allocate and copy
 * nothing, and are safe inside a stream capture. */
int32_t iris_mel_frontend_create(const iris_mel_frontend_config* cfg, iris_mel_frontend_handle** out);
int32_t iris_mel_frontend_destroy(iris_mel_frontend_handle* h);
int32_t iris_mel_frontend_forward(iris_mel_frontend_handle* h, const void* audio_dev, int32_t sample_format, int32_t B, int32_t L,
                                  float* mel_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* Ragged: n_samples_dev [B] int32 on the device, clamped to [0, L] and never read by the host; samples at or past an item's
 * count read as 0 and are not fetched.  max_frames_dev [B] (or NULL) caps an item's frames: item b has
 * min(1 + n_b / hop_length, max(max_frames[b], 0)) frames, counted from its own sample 0, which go to frames_out_dev [B];
 * mel[b, :, frames_b:] is stored as 0.0f.  Item b is bit for bit its batch-of-one dense call. */
int32_t iris_mel_frontend_forward_ragged(iris_mel_frontend_handle* h, const void* audio_dev, int32_t sample_format, int32_t B, int32_t L,
                                         const int32_t* n_samples_dev, const int32_t* max_frames_dev /* or NULL */, float* mel_out_dev,
                                         int32_t* frames_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Griffin-Lim vocoder: log-mel to waveform without trained weights (csrc/griffin_lim.h) -------------------------
 * The reference's --use_griffin_lim path (scripts/synthesize.py:174-194): m = exp(clip(logmel, -11.513, 2.0)), librosa 0.11's
 * mel_to_stft(power=1.0) and griffinlim(n_iter, hop_length, win_length), in fp32.  logmel [B, n_mels, T] -> waveform
 * [B, hop_length * (T - 1)].  Window, frames and filterbank fb [n_mels][n_bins] are the mel front-end's, and so are the config
 * rules (the first eight fields are its fields).
 *   inversion  x0 = max(P m, 0) with P = pinv(fb) [n_bins][n_mels] from the caller (float64, rounded once), then nnls_iters
 *              projected-gradient steps x <- max(x - nnls_step * fb^T (fb x - m), 0); nnls_step = 1 / lambda_max(fb fb^T) keeps
 *              ||fb x - m|| from growing.  S = x.
 *   phase      c = S * (cos phi0, sin phi0); n_iter times: y = istft(c), r = stft(y), a = r - momentum / (1 + momentum) * r_prev
 *              (r_prev = 0 in the first pass), c = S * a / (|a| + FLT_MIN); then out = istft(c).
 *   stft       frame t covers samples [t * hop - n_fft / 2, t * hop + n_fft / 2) of y, 0 outside (the front-end's frames).
 *   istft      w[n] * irfft(c[:, t])[n] overlap-added, divided by the window-sum-square where that exceeds FLT_MIN, n_fft / 2
 *              samples trimmed at each end; the imaginary parts of bins 0 and n_fft / 2 are ignored.
 * phase0_dev: fp32 [B][T][n_bins][2], frame-major -- cos(phi0[b, k, t]) then sin(phi0[b, k, t]) at ((b * T + t) * n_bins + k) * 2;
 * 8-byte aligned.  2 * n_iter + 2 launches, no atomics: two runs agree bit for bit, and item b is its batch-of-one call.
 * After a forward the workspace starts with S as fp32 [B][T][Ks], Ks = n_bins rounded up to a multiple of 4.
 * The front-end's unsupported configs, an n_fft that is no multiple of 32, and an inversion tile (32 frames of n_mels and n_bins
 * floats) or a frame window of the transforms (31 + n_fft / hop_length frames of 260 floats: n_fft / hop_length >= 128) above
 * 160 KB of LDS return
 * IRIS_HIFIGAN_UNSUPPORTED (from every function below that takes the config; create reports it before it touches the device);
 * T < 2, a NULL pointer, a negative count, momentum outside [0, 1), a non-positive nnls_step and a wrong pinv size
 * IRIS_HIFIGAN_INVALID_ARGUMENT; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches. */
typedef struct iris_griffin_lim_config {
    int32_t sample_rate, n_fft, hop_length, win_length, n_mels, n_iter;
    double fmin, fmax;
    int32_t nnls_iters, reserved;
    double momentum, nnls_step;
} iris_griffin_lim_config;
typedef struct iris_griffin_lim_handle iris_griffin_lim_handle;

/* Host only (no device is needed).  design: *n_bins and, where the pointers are not NULL, the fp32 tables the handle uploads --
 * dft_host as iris_mel_frontend_design gives it; idft_host [2][n_bins][n_fft]: w[n] f_k cos(2 pi k n / n_fft) / n_fft, then
 * -w[n] f_k sin(2 pi k n / n_fft) / n_fft (f_k = 1 for k = 0 and n_fft / 2, else 2; those two bins' sine rows are 0), in double
 * with the angle reduced by (k n) mod n_fft, rounded once; fb_host [n_mels][n_bins]; wsq_host [n_fft]: w[n]^2.
 * launch_count: a dry run of the forward's own code. */
int32_t iris_griffin_lim_design(const iris_griffin_lim_config* cfg, int32_t* n_bins, float* dft_host, uint64_t dft_floats,
                                float* idft_host, uint64_t idft_floats, float* fb_host, uint64_t fb_floats, float* wsq_host,
                                uint64_t wsq_floats);
int32_t iris_griffin_lim_workspace_bytes(const iris_griffin_lim_config* cfg, int32_t B, int32_t T, uint64_t* bytes);
int32_t iris_griffin_lim_launch_count(const iris_griffin_lim_config* cfg, int32_t B, int32_t T, int32_t* n);
/* create: on the current device, which becomes the handle's; pinv_host [n_bins][n_mels].  The forward is asynchronous on
 * `stream`, allocates and copies nothing, and is safe inside a stream capture. */
int32_t iris_griffin_lim_create(const iris_griffin_lim_config* cfg, const float* pinv_host, uint64_t n_pinv, iris_griffin_lim_handle** out);
int32_t iris_griffin_lim_destroy(iris_griffin_lim_handle* h);
int32_t iris_griffin_lim_forward(iris_griffin_lim_handle* h, const float* logmel_dev, const float* phase0_dev, int32_t B, int32_t T,
                                 float* wav_out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);
/* The ragged forward: lengths_dev [B] (device, or NULL: every item has T frames) holds the items' frame counts.  Item b has
 * T_b = min(max(lengths[b], 0), T) frames, 0 if that is below 2 (an empty item); its samples wav[b, :hop_length * (T_b - 1)] are
 * bit for bit its batch-of-one dense call on logmel[b, :, :T_b] and its phase rows, and wav[b, hop_length * (T_b - 1):] is stored
 * as 0.0f.  Nothing of logmel, phase0 or the workspace at frames t >= T_b is read or written.  The lengths are never read by the
 * host: a captured graph follows new contents of lengths_dev.  Strides, the workspace and the launch count are the dense call's.
 * phase0_dev may be NULL: the start phase is then drawn on the device -- Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 * and counter (k >> 2, t, item0 + b, 0), output word k & 3 for bin k of frame t of item b; u = (x >> 8) * 2^-24, angle =
 * 6.2831855f * u in fp32, phase = (cosf, sinf) of it -- and depends on no batch position but item0 + b (item0 >= 0).  seed and
 * item0 are ignored otherwise.  draw_phase stores the same draw as the packed phase_out_dev [B][T][n_bins][2] (one launch).
 * Status rules as for iris_griffin_lim_forward, checked before anything is launched. */
int32_t iris_griffin_lim_forward_ragged(iris_griffin_lim_handle* h, const float* logmel_dev, const float* phase0_dev, uint64_t seed,
                                        int32_t item0, int32_t B, int32_t T, const int32_t* lengths_dev, float* wav_out_dev,
                                        void* workspace_dev, uint64_t workspace_bytes, void* stream);
int32_t iris_griffin_lim_draw_phase(iris_griffin_lim_handle* h, uint64_t seed, int32_t item0, int32_t B, int32_t T, float* phase_out_dev,
                                    void* stream);

/* ---- Bias denoiser: spectral bias subtraction on the vocoder's waveform (csrc/denoiser.h) -----------------------------
 * What HiFiGAN users run behind the vocoder: the magnitude spectrum of the vocoder's output for a silent mel (its constant
 * hum, the "bias") is subtracted, times `strength`, from the magnitudes of an utterance; the phase is kept.  fp32, on the
 * Griffin-Lim stage's transforms above (stft, istft: the mel front-end's window, frames and tables; sample_rate, n_mels,
 * fmin and fmax of the config are checked by the front-end's rules and otherwise unused).  wav [B, L] -> out [B, L], L a
 * multiple of hop_length (M = L / hop_length mel frames, T = M + 1 frames).  Per frame t and bin k of a = stft(wav):
 *     mag = sqrtf(re re + im im);  g = fmaxf(fmaf(-strength, bias[k], mag), 0);  scale = mag > 0 ? g / mag : 0;
 *     c = (scale re, scale im);  out = istft(c)
 * Bins 0 and n_fft / 2 are real.  strength = 0 leaves c = stft(wav); a strength at or above max(mag / bias) gives out == 0.
 * bias [n_bins] is finite and not negative (create checks bias_host; NULL: zeros).  set_bias copies n_bins floats from the
 * device into the handle, asynchronously on `stream`: an estimate never visits the host.
 * estimate_bias: wav [1, L] -> bias_out_dev [n_bins], the mean of mag[t, k] over the frames whose window lies wholly inside the
 * signal, e <= t < T - e with e = ceil(n_fft / 2 / hop_length); fp32 terms summed in fp64 in ascending t, rounded once: the
 * same bits on every run.  Its workspace is that of a forward of shape (1, L).
 * forward: 2 launches (the STFT with the subtraction as its epilogue, the inverse STFT); estimate_bias: 2 launches (the STFT
 * storing magnitudes, the mean).  No atomics: two runs agree bit for bit.  lengths_dev [B] (device, or NULL: dense) holds the
 * items' MEL frames: item b has M_b = min(max(lengths[b], 0), M) frames; out[b, :hop_length * M_b] is bit for bit the
 * batch-of-one dense call on wav[b, :hop_length * M_b], out[b, hop_length * M_b:] is stored as 0.0f, and nothing of wav at or
 * past hop_length * M_b is read.  The lengths are never read by the host: a captured graph follows new contents.
 * After a forward the workspace starts with c as fp32 [B][T][Qp] (column 2 k Re, 2 k + 1 Im of bin k; Qp = n_fft + 2 rounded
 * up to 8; rows t > M_b and columns from n_fft + 2 on are not written), followed by the items' frame counts.
 * L that is no multiple of hop_length, a negative shape, a negative or non-finite strength, a NULL pointer, out_dev
 * overlapping wav_dev, and (estimate_bias) an L without an interior frame return IRIS_HIFIGAN_INVALID_ARGUMENT; the front-end's
 * and the Griffin-Lim stage's unsupported configs and B > 65535 IRIS_HIFIGAN_UNSUPPORTED (from every function that takes the
 * config; create reports it before it touches the device); a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing
 * call launches.  B == 0 or L == 0: nothing to do, IRIS_HIFIGAN_OK. */
typedef struct iris_denoiser_handle iris_denoiser_handle;
/* Host only (no device is needed); the launch counts are dry runs of the forward's and the estimator's own code. */
int32_t iris_denoiser_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, uint64_t* bytes);
int32_t iris_denoiser_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, int32_t* n);
int32_t iris_denoiser_estimate_launch_count(const iris_mel_frontend_config* cfg, int32_t L, int32_t* n);
/* create: on the current device, which becomes the handle's.  The calls below it are asynchronous on `stream`, allocate
 * nothing, and are safe inside a stream capture. */
int32_t iris_denoiser_create(const iris_mel_frontend_config* cfg, const float* bias_host /* [n_bins] or NULL */, iris_denoiser_handle** out);
int32_t iris_denoiser_destroy(iris_denoiser_handle* h);
int32_t iris_denoiser_set_bias(iris_denoiser_handle* h, const float* bias_dev, void* stream);
int32_t iris_denoiser_estimate_bias(iris_denoiser_handle* h, const float* wav_dev, int32_t L, float* bias_out_dev, void* workspace_dev,
                                    uint64_t workspace_bytes, void* stream);
int32_t iris_denoiser_forward(iris_denoiser_handle* h, const float* wav_dev, int32_t B, int32_t L, const int32_t* lengths_dev /* or NULL */,
                              float strength, float* out_dev, void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* Windows: the forward on samples [origin, origin + Lw) of an utterance, for a caller that receives the waveform piece by piece.
 * origin = hop_length m0 and Lw = hop_length Mw; `final` (0 or not) says that origin + Lw is the utterance's end.  Frame t covers
 * samples [t hop_length - n_fft / 2, t hop_length + n_fft / 2) and exists when t >= 0 and, only if final, t <= m0 + Mw.  A frame
 * is computable in the window when every sample of its span that lies inside the utterance lies inside the window; sample s,
 * the sum over the n_fft / hop_length frames that end at floor((s + n_fft / 2) / hop_length), is final in the window when each
 * of those frames is computable or does not exist.  The final samples of a window are one range:
 *     window_range -> out_lo (an index into the utterance) and out_count (0: none; out_lo is then origin).
 * An interior window loses (n_fft / hop_length - 1) hop_length samples on either side: 768 at 1024 / 256, 128 at 256 / 128.
 * forward_window: wav_dev [B, Lw] -> out_dev [B, out_count], each sample bit for bit that of iris_denoiser_forward on the whole
 * utterance: a frame's sums depend on its own n_fft samples and a sample's on its own frames, in a fixed order, whichever
 * window they are computed in.  Dense only; stateless; 2 launches, none when B == 0 or out_count == 0 (IRIS_HIFIGAN_OK).  The
 * workspace is that of a forward of shape (B, Lw).  An origin or Lw that is negative or no multiple of hop_length returns
 * IRIS_HIFIGAN_INVALID_ARGUMENT, an origin above 2^60 IRIS_HIFIGAN_UNSUPPORTED; the other refusals are the forward's. */
int32_t iris_denoiser_window_range(const iris_mel_frontend_config* cfg, int64_t origin, int32_t Lw, int32_t final, int64_t* out_lo,
                                   int64_t* out_count);
int32_t iris_denoiser_window_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, uint64_t* bytes);
int32_t iris_denoiser_window_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, int64_t origin, int32_t final,
                                          int32_t* n);
int32_t iris_denoiser_forward_window(iris_denoiser_handle* h, const float* wav_dev /* [B, Lw] */, int32_t B, int32_t Lw, int64_t origin,
                                     int32_t final, float strength, float* out_dev /* [B, out_count] */, void* workspace_dev,
                                     uint64_t workspace_bytes, void* stream);

/* ---- Time stretch: a phase vocoder between the two transforms above (csrc/time_stretch.h) -------------------------------
 * Tempo without pitch: librosa.effects.time_stretch(y, rate=, n_fft=, hop_length=, win_length=) on the stage's own frame rules
 * (center=True, zero padding, periodic Hann centred in n_fft), fp32.  Only n_fft, hop_length and win_length of the config are
 * read: n_fft <= 4096, hop_length divides n_fft and is a multiple of 4, win_length <= n_fft, and the Griffin-Lim stage's
 * limits on the transforms (2048 / 512, librosa's defaults for this effect, is inside them).  wav [B, L], L a multiple of
 * hop_length, has T = L / hop_length + 1 frames c = stft(wav); rate is an argument of the forward, in [0.25, 4]:
 *     T_out = ceil(T / rate);  step_t = t rate;  i = floor(step_t);  alpha = (float)(step_t - i)        (double; a column >= T is 0)
 *     mag[t,k] = fmaf(alpha, |c[i+1,k]|, (1 - alpha) |c[i,k]|)
 *     dphi = turns(c[i+1,k]) - turns(c[i,k]) - adv_k;  dphi -= rintf(dphi);  adv_k = ((k hop_length) mod n_fft) / n_fft
 *     acc[0,k] = turns(c[0,k]);  acc[t+1,k] = acc[t,k] + adv_k + dphi;  out_c[t,k] = mag[t,k] (cos, sin)(2 pi acc[t,k])
 *     n_out = rint(L / rate) (double, half to even);  out = istft(out_c, length = n_out)
 * acc is a uint32 of 2^-32 turns: it wraps where an fp32 sum of radians would lose the phase, and its sum is associative, so
 * two runs agree bit for bit whatever order the scan takes.  istft(length=): samples below min(n_out, hop_length (T_out - 1) +
 * n_fft / 2) are the overlap-add value over the window-sum-square of the frames that exist, the rest are 0.0f.
 * out_samples: T_out and n_out of one item of L samples, on the host, by the lines the device runs.
 * forward: wav_dev [B, L] -> out_dev [B, n_out], 4 launches (the STFT, the vocoder's step, its scan, the inverse STFT).
 * forward_ragged: lengths_dev [B] (device, or NULL: dense) holds the items' MEL frames as for the denoiser: M_b =
 * min(max(lengths[b], 0), L / hop_length), L_b = hop_length M_b, T_b = M_b + 1 (an item with M_b == 0 is empty).  Item b's
 * n_out_b = rint(L_b / rate) samples are bit for bit its batch-of-one call on wav[b, :L_b], out[b, n_out_b:] is stored as 0.0f,
 * nothing of wav past L_b is read, and counts_out_dev [B] (or NULL) receives n_out_b: the next stage's lengths.  Row strides
 * are n_out of the whole L.  The host never reads the lengths.
 * After a forward the workspace holds, each starting on 256 bytes: c [B][T][Qp], mag [B][T_out][Ks] (fp32), inc and acc
 * [B][T_out][Ks] (uint32), out_c [B][T_out][Qp], then T_b, T_out_b and n_out_b [B] (int32).  Ks = n_fft / 2 + 1 rounded up to 4,
 * Qp = n_fft + 2 rounded up to 8.
 * A rate outside [0.25, 4] or not finite, L no multiple of hop_length, a negative shape, a NULL pointer and out_dev overlapping
 * wav_dev return IRIS_HIFIGAN_INVALID_ARGUMENT; an unsupported config, B > 65535 and a shape whose buffers pass 2^31 elements
 * IRIS_HIFIGAN_UNSUPPORTED; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches.  B == 0 or L == 0:
 * nothing to do, IRIS_HIFIGAN_OK. */
typedef struct iris_time_stretch_handle iris_time_stretch_handle;
/* Host only (no device is needed); the launch count is a dry run of the forward's own code. */
int32_t iris_time_stretch_out_samples(const iris_mel_frontend_config* cfg, int32_t L, double rate, int32_t* frames_out, int32_t* samples_out);
int32_t iris_time_stretch_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, double rate, uint64_t* bytes);
int32_t iris_time_stretch_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t L, double rate, int32_t* n);
/* create: on the current device, which becomes the handle's.  The forwards are asynchronous on `stream`, allocate nothing,
 * and are safe inside a stream capture. */
int32_t iris_time_stretch_create(const iris_mel_frontend_config* cfg, iris_time_stretch_handle** out);
int32_t iris_time_stretch_destroy(iris_time_stretch_handle* h);
int32_t iris_time_stretch_forward(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t L, double rate, float* out_dev,
                                  void* workspace_dev, uint64_t workspace_bytes, void* stream);
int32_t iris_time_stretch_forward_ragged(iris_time_stretch_handle* h, const float* wav_dev, int32_t B, int32_t L,
                                         const int32_t* lengths_dev /* or NULL */, double rate, float* out_dev,
                                         int32_t* counts_out_dev /* [B] or NULL */, void* workspace_dev, uint64_t workspace_bytes,
                                         void* stream);

/* Windows: the stretch on samples [origin, origin + Lw) of an utterance, for a caller that receives the waveform piece by piece.
 * N = n_fft, H = hop_length, taps = N / H (>= 2 here), e = ceil(N / 2 / H).  origin = H m0, Lw = H Mw; `final` (0 or not) says that
 * origin + Lw is the utterance's end -- only then are T, T_out and n_out known.  Input rows [f_lo, f_hi) are computable as for the
 * denoiser's windows: f_lo = m0 ? m0 + e : 0, f_hi = final ? m0 + Mw + 1 : m0 + Mw - e + 1.  The caller carries one integer u, the
 * next output frame (0 at the start), and the state.  Output frame t reads rows i and i + 1, i = floor((double)t * rate):
 *     not final: t is computable iff i >= f_lo and i + 1 < f_hi;   final: iff t < T_out and i >= f_lo (rows >= T read as 0).
 * The window computes frames [u, u_hi), the longest such run; floor(u rate) < f_lo is refused (samples were dropped too early).
 * keep_from = H max(0, floor(u_hi rate) - e) is the first sample the next window must still hold.  Sample s lies in row
 * j = floor((s + N / 2) / H) and is emitted by this window when each of frames j - taps + 1 .. j lies in [max(0, u - taps + 1),
 * u_hi) or does not exist (negative, or -- only if final -- >= T_out), no earlier window emitted it (j >= u), and s < n_out
 * (final; samples from min(n_out, H (T_out - 1) + N / 2) on are stored as 0.0f, the forward's tail rule) or s < rint((origin +
 * Lw) / rate) (not final: the least n_out a continuation can have).  The emitted samples are one range, contiguous with the
 * previous window's:
 *     window_plan -> u_hi, out_lo (an index into the stretched utterance), out_count, keep_from.
 * State (state_bytes; caller-owned, read and written in place by the scan's launch, never copied): acc [B][Ks] uint32, the phase
 * at frame u_hi, then -- on the next 256 bytes -- tail [B][taps - 1][Qp], row q holding out_c of frame u_hi - (taps - 1) + q.
 * Rows of negative frames, columns of acc from n_fft / 2 + 1 on and columns of tail from n_fft + 2 on are never read or
 * written.  A state need not be initialised for u == 0; state_dev may be NULL only for a final window with u == 0.
 * forward_window: wav_dev [B, Lw] -> out_dev [B, out_count], each sample bit for bit that of iris_time_stretch_forward on the whole
 * utterance: the phase is an exact integer sum, a row's chain depends on its own n_fft samples and a sample's on its own taps
 * frames, in a fixed order, whichever window they are computed in.  Dense only, one rate per utterance.  The forward's 4
 * launches; 3 where frames advance but no sample is emitted yet; 2 (scan and inverse STFT) where a final window has samples
 * left but no frame; none, and IRIS_HIFIGAN_OK, when B == 0 or u_hi == u and out_count == 0.  No copies, nothing allocated,
 * asynchronous, safe in a stream capture.  After a window the workspace holds, in the window's own coordinates and each
 * starting on 256 bytes at an offset that depends on (B, Lw, rate) alone: c [B][f_hi - f_lo][Qp], mag, inc, acc
 * [B][u_hi - u][Ks] and out_c [B][n_tail + u_hi - u][Qp], n_tail = min(taps - 1, u), the carried rows first.
 * Refusals are the forward's, and: origin or Lw negative or no multiple of hop_length, u < 0, u > 0 or a window that is not
 * final without a state, floor(u rate) < f_lo -> IRIS_HIFIGAN_INVALID_ARGUMENT; origin above 2^60, u hop_length above 2^61,
 * hop_length == n_fft -> IRIS_HIFIGAN_UNSUPPORTED.  No failing call launches. */
int32_t iris_time_stretch_state_bytes(const iris_mel_frontend_config* cfg, int32_t B, uint64_t* bytes);
int32_t iris_time_stretch_window_plan(const iris_mel_frontend_config* cfg, double rate, int64_t origin, int32_t Lw, int32_t final, int64_t u,
                                      int64_t* u_hi, int64_t* out_lo, int64_t* out_count, int64_t* keep_from);
int32_t iris_time_stretch_window_workspace_bytes(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, double rate, uint64_t* bytes);
int32_t iris_time_stretch_window_launch_count(const iris_mel_frontend_config* cfg, int32_t B, int32_t Lw, double rate, int64_t origin,
                                              int32_t final, int64_t u, int32_t* n);
int32_t iris_time_stretch_forward_window(iris_time_stretch_handle* h, const float* wav_dev /* [B, Lw] */, int32_t B, int32_t Lw, int64_t origin,
                                         int32_t final, double rate, int64_t u, void* state_dev, float* out_dev /* [B, out_count] */,
                                         void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Assemble: silence trim and sentence join, a ragged batch becomes one waveform (csrc/assemble.h) ----------------------
 * Per item the decision of librosa.effects.trim(y, top_db=, ref=np.max, frame_length=F, hop_length=H), then one launch lays the
 * trimmed items end to end with a pause between them and a short fade at every cut.  fp32; the host never reads a length.
 * lengths_dev (may be NULL) and row_scale >= 1 as in iris_resampler_forward: item b owns L_b = min(L, lengths[b] * row_scale)
 * samples; samples past that are never read (they may hold NaN).  csrc/assemble.h states every rule; in short:
 *     T_b = L_b / H + 1 frames; frame t covers samples [t H - F / 2, t H + F / 2) (0 outside the item); mse[t] = sum(y^2) / F,
 *         summed in a fixed fp32 order that depends on the item's own sample indices alone;
 *     ref_b = max_t mse[t], or ref * ref where cfg.ref > 0;  frame t is non-silent iff
 *         fmaxf(mse[t], 1e-10f) > fmaxf(ref_b, 1e-10f) * (float)pow(10, -top_db / 10)      (strict; an item of digital silence
 *         keeps every frame with ref == 0, as in librosa);
 *     t0 / t1 the first / last non-silent frame: start = t0 H, end = min(L_b, (t1 + 1) H) (none: 0, 0);
 *         start' = max(0, start - pad), end' = min(L_b, end + pad), len_b = end' - start';
 *     off_b = sum over a < b of (len_a + (len_a > 0 ? pause : 0)); total = off_B less the last pause; an empty item adds
 *         neither samples nor a pause;
 *     out[off_b + n] = (wav[b, start' + n] * a) * b2, a = n < fade ? ramp[n] : 1, b2 = len_b - 1 - n < fade ? ramp[len_b - 1 - n]
 *         : 1, ramp[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade) (double, rounded once); pauses and [total, cap) are stored as 0.0f.
 * forward: wav_dev [B, L] -> out_dev [cap], cap = B L + pause (B - 1) (out_capacity); every element of out_dev is stored exactly
 * once, without atomics, and two runs give the same bits.  spans_out_dev [B][2] (or NULL) receives start', end';
 * offsets_out_dev [B + 1] receives off_0 .. off_(B-1) and, last, total -- offsets_out_dev + B is the lengths pointer of a
 * following iris_resampler_forward / iris_hifigan_op_pcm16 on out_dev as ONE row of cap samples (row_scale 1).  Item b's span
 * and samples are those of its batch-of-one call.  Chaining: behind the vocoder with lengths in mel frames and row_scale =
 * hop; behind iris_time_stretch_forward_ragged with its counts and row_scale = 1.
 * trim_ragged: the same bounds with each item stored in its own row, out_dev [B, L], 0.0f behind len_b, and counts_out_dev [B] =
 * len_b as the next stage's lengths (the same launches; the gather runs with one row per item and no pause).
 * After a call the workspace holds, each starting on 256 bytes: mse [B][L / H + 1] fp32, of which row b is stored up to T_b,
 * and spans [B][2] int32; nothing else is written.  3 launches, asynchronous on `stream`, nothing allocated, safe in a stream
 * capture.
 * frame_length odd or below 2, hop_length not dividing frame_length / 2, top_db <= 0 or not finite, ref < 0 or not finite, a
 * negative pad / fade / pause, row_scale < 1, a negative shape, a NULL pointer and out_dev overlapping wav_dev return
 * IRIS_HIFIGAN_INVALID_ARGUMENT; frame_length > 8192, fade > 65536, B > 4096 (the join stages the B + 1 offsets in LDS), and
 * cap or B L above 2^31 - 1 IRIS_HIFIGAN_UNSUPPORTED; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call
 * launches.  B == 0 or L == 0: nothing to do, IRIS_HIFIGAN_OK. */
typedef struct iris_assemble_config {
    int32_t frame_length, hop_length;
    float top_db;
    float ref;                  /* absolute reference amplitude; 0: the item's own maximum */
    int32_t pad_samples, fade_samples, pause_samples;
} iris_assemble_config;
typedef struct iris_assemble_handle iris_assemble_handle;
/* Host only (no device is needed); the launch count is a dry run of the forward's own code. */
int32_t iris_assemble_out_capacity(const iris_assemble_config* cfg, int32_t B, int32_t L, int64_t* cap);
int32_t iris_assemble_workspace_bytes(const iris_assemble_config* cfg, int32_t B, int32_t L, uint64_t* bytes);
int32_t iris_assemble_launch_count(const iris_assemble_config* cfg, int32_t B, int32_t L, int32_t* n);
/* create: on the current device, which becomes the handle's; it uploads the ramp. */
int32_t iris_assemble_create(const iris_assemble_config* cfg, iris_assemble_handle** out);
int32_t iris_assemble_destroy(iris_assemble_handle* h);
int32_t iris_assemble_forward(iris_assemble_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                              const int32_t* lengths_dev /* or NULL */, int32_t row_scale, float* out_dev /* [cap] */,
                              int32_t* spans_out_dev /* [B][2] or NULL */, int32_t* offsets_out_dev /* [B + 1] */,
                              void* workspace_dev, uint64_t workspace_bytes, void* stream);
int32_t iris_assemble_trim_ragged(iris_assemble_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                                  const int32_t* lengths_dev /* or NULL */, int32_t row_scale, float* out_dev /* [B, L] */,
                                  int32_t* spans_out_dev /* [B][2] or NULL */, int32_t* counts_out_dev /* [B] */,
                                  void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Loudness: ITU-R BS.1770-4 integrated loudness per item of a ragged batch, and the gain to a target (csrc/loudness.h) ----
 * Mono fp32.  lengths_dev (may be NULL) and row_scale >= 1 as in iris_resampler_forward: item b owns L_b = min(L, lengths[b] *
 * row_scale) samples; samples past that are never read (they may hold NaN).  The host never reads a length.  csrc/loudness.h
 * states every rule and every order of summation; in short, all of it in fp64 with nothing contracted:
 *     K-weighting: a high shelf and a high pass, derived for sample_rate on the host in double with K = tan(pi f0 / fs), as
 *         libebur128 and pyloudnorm derive them (at 48000 the standard's table); state 0 at sample 0 of every item;
 *     step = sample_rate / 10; block j covers filtered samples [j step, j step + 4 step); J_b = L_b >= 4 step ? (L_b - 4 step) /
 *         step + 1 : 0; z_j = the block's mean square;
 *     absolute gate z_j > 10^((-70 + 0.691) / 10); relative gate z_j > 0.1 * mean(z over the absolutely gated); ms_b = mean of
 *         z_j over the blocks passing both (strict), 0 if none; integrated loudness = -0.691 + 10 log10(ms_b), the caller's to form;
 *     g_b = sqrt(10^((target_lufs + 0.691) / 10) / ms_b), at most 10^(max_gain_db / 20) and, with peak_ceiling > 0, at most
 *         peak_ceiling / max|y_b|; ms_b == 0 (too short, or nothing above the absolute gate): g_b = 1;
 *     out[b, n] = wav[b, n] * (float)g_b for n < L_b, 0.0f behind L_b.
 * normalize_ragged: wav_dev [B, L] -> out_dev [B, L], every element stored exactly once, without atomics; stats_out_dev [B][2]
 * doubles = (ms_b, g_b).  4 launches.  measure_ragged: stats_out_dev only, no sample is stored; the first 3 of them.  Item b's
 * results are those of its batch-of-one call, and two runs give the same bits.  Chaining: lengths and row_scale of the stage in
 * front are those of the stage behind (iris_assemble_forward, iris_resampler_forward, iris_hifigan_op_pcm16).
 * The recurrence is serial in time, so an item is cut into segments of 64 samples that run in parallel from state 0; their end
 * states are scanned with powers of the 4 x 4 transition matrix, and every segment runs again from its true start state.
 * After a call the workspace holds, each starting on 256 bytes: the segments' scanned end states [B][segs][4], their partial sums
 * of squares [B][segs][2], the 100 ms sums [B][L / step + 1] (doubles) and the segments' peaks [B][segs] (fp32), segs = 128 *
 * ceil(L / 8192); only what belongs to an item's own samples is written.  Asynchronous on `stream`, nothing allocated, safe in a
 * stream capture.
 * design: the handle's table of 144 doubles -- shelf (b0, b1, b2, a1, a2), high pass (b0, b1, b2, a1, a2), the absolute
 * threshold, target_ms, the gain cap, peak_ceiling, two zeros, then A^(64 * 2^k) for k = 0 .. 7, row-major.  Host only.
 * sample_rate outside 8000 .. 48000 or no multiple of 10, target_lufs outside -70 .. 0, max_gain_db outside 0 .. 120,
 * peak_ceiling outside 0 .. 1, anything not finite, row_scale < 1, a negative shape, a NULL pointer, stats_out_dev or
 * workspace_dev off 8 bytes and out_dev overlapping wav_dev return IRIS_HIFIGAN_INVALID_ARGUMENT; B > 65535 (grid.y) and B L
 * above 2^31 - 1 IRIS_HIFIGAN_UNSUPPORTED; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches.
 * B == 0 or L == 0: nothing to do, IRIS_HIFIGAN_OK. */
typedef struct iris_loudness_config {
    int32_t sample_rate;
    float target_lufs;
    float max_gain_db;          /* a cap on the boost */
    float peak_ceiling;         /* amplitude in (0, 1]; 0: none */
} iris_loudness_config;
typedef struct iris_loudness_handle iris_loudness_handle;
/* Host only (no device is needed); the launch count is a dry run of the call's own code (measure_only != 0: measure_ragged). */
int32_t iris_loudness_design(const iris_loudness_config* cfg, double* out /* [n] */, uint64_t n /* 144 */);
int32_t iris_loudness_workspace_bytes(const iris_loudness_config* cfg, int32_t B, int32_t L, uint64_t* bytes);
int32_t iris_loudness_launch_count(const iris_loudness_config* cfg, int32_t B, int32_t L, int32_t measure_only, int32_t* n);
/* create: on the current device, which becomes the handle's; it uploads the design table. */
int32_t iris_loudness_create(const iris_loudness_config* cfg, iris_loudness_handle** out);
int32_t iris_loudness_destroy(iris_loudness_handle* h);
int32_t iris_loudness_normalize_ragged(iris_loudness_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                                       const int32_t* lengths_dev /* or NULL */, int32_t row_scale, float* out_dev /* [B, L] */,
                                       double* stats_out_dev /* [B][2] */, void* workspace_dev, uint64_t workspace_bytes, void* stream);
int32_t iris_loudness_measure_ragged(iris_loudness_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                                     const int32_t* lengths_dev /* or NULL */, int32_t row_scale, double* stats_out_dev /* [B][2] */,
                                     void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Limiter: a look-ahead true-peak ceiling per item of a ragged batch, without turning the item down (csrc/limiter.h) ----
 * Mono fp32.  lengths_dev (may be NULL) and row_scale >= 1 as in iris_loudness_normalize_ragged: item b owns L_b = min(L,
 * lengths[b] * row_scale) samples; samples past that are never read (they may hold NaN); x[n] = 0 outside [0, L_b).  The host
 * never reads a length.  csrc/limiter.h states every rule; in short, with ceiling c and lookahead A, all of it in fp32 with
 * nothing contracted except the fmaf named here, and the one division in fp64:
 *     u[n, q], q = 1, 2, 3 = the chain over j = 0 .. 11 ascending of acc = fmaf(x[n - 5 + j], bank[q][j], acc), acc = 0.0f, with
 *         bank the Kaiser-windowed sinc of iris_resampler_* for 1 : 4 with 6 zeros and its default beta and rolloff: the three
 *         points between sample n and n + 1;
 *     p[n] = max(|x[n]|, |u[n-1, 1..3]|, |u[n, 1..3]|); tp_b = max p[n] over n < L_b, 0 for an empty item;
 *     r[n] = p[n] > c ? (float)((double)c / (double)p[n]) : 1.0f inside [0, L_b), 1.0f outside;
 *     m[n] = min r[n + k] over |k| <= A; d[n] = 1.0f - m[n];
 *     s[n] = the chain over j = -A .. A ascending of acc = fmaf(d[n + j], w[j], acc), acc = 0.0f, w a Hann shape 0.5 (1 + cos(pi
 *         j / (A + 1))) normalised to sum 1 in double and rounded to fp32 upward, so that the table's sum is never under 1 and
 *         g[n] <= r[n] in exact arithmetic; g[n] = 1.0f - s[n], exactly 1 where nothing within 2A samples exceeds c;
 *     out[b, n] = fminf(fmaxf(x[n] * g[n], -c), c) for n < L_b, 0.0f behind L_b: |out| <= c always.
 * forward_ragged: wav_dev [B, L] -> out_dev [B, L], every element stored exactly once, without atomics; stats_out_dev [B][2]
 * floats = (tp_b, min g[n] over n < L_b), (0, 1) for an empty item.  2 launches: one fused kernel over tiles of 2048 samples
 * that stages x with a halo of 2A + 7 per side in LDS, and the reduction of the tiles' (max p, min g) per item.  measure_ragged:
 * the same two, the same stats, and no sample is stored.  Item b's results are those of its batch-of-one call, and two runs give
 * the same bits.  Chaining: lengths and row_scale of the stage in front are those of the stage behind.
 * After a call the workspace holds the tiles' partials [B][ceil(L / 2048)][2] (fp32); only an item's own tiles, the first
 * ceil(L_b / 2048), are written.  Asynchronous on `stream`, nothing allocated, safe in a stream capture.
 * design: the handle's table of 36 + 2A + 1 floats -- bank[1..3][0..11], then w[-A .. A].  Host only.
 * ceiling outside (0, 1] or not finite, lookahead outside 1 .. 256, row_scale < 1, a negative shape, a NULL pointer,
 * stats_out_dev off 4 bytes, workspace_dev off 8 bytes and out_dev overlapping wav_dev return IRIS_HIFIGAN_INVALID_ARGUMENT;
 * B > 65535 (grid.y) and B L above 2^31 - 1 IRIS_HIFIGAN_UNSUPPORTED; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No
 * failing call launches.  B == 0 or L == 0: nothing to do, IRIS_HIFIGAN_OK. */
typedef struct iris_limiter_config {
    float ceiling;              /* amplitude in (0, 1] */
    int32_t lookahead;          /* samples, 1 .. 256 */
} iris_limiter_config;
typedef struct iris_limiter_handle iris_limiter_handle;
/* Host only (no device is needed); the launch count is a dry run of the call's own code (measure_only != 0: measure_ragged). */
int32_t iris_limiter_design(const iris_limiter_config* cfg, float* out /* [n] */, uint64_t n /* 36 + 2 * lookahead + 1 */);
int32_t iris_limiter_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t L, uint64_t* bytes);
int32_t iris_limiter_launch_count(const iris_limiter_config* cfg, int32_t B, int32_t L, int32_t measure_only, int32_t* n);
/* create: on the current device, which becomes the handle's; it uploads the design table. */
int32_t iris_limiter_create(const iris_limiter_config* cfg, iris_limiter_handle** out);
int32_t iris_limiter_destroy(iris_limiter_handle* h);
int32_t iris_limiter_forward_ragged(iris_limiter_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                                    const int32_t* lengths_dev /* or NULL */, int32_t row_scale, float* out_dev /* [B, L] */,
                                    float* stats_out_dev /* [B][2] */, void* workspace_dev, uint64_t workspace_bytes, void* stream);
int32_t iris_limiter_measure_ragged(iris_limiter_handle* h, const float* wav_dev /* [B, L] */, int32_t B, int32_t L,
                                    const int32_t* lengths_dev /* or NULL */, int32_t row_scale, float* stats_out_dev /* [B][2] */,
                                    void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* Windows: the limiter on samples [origin, origin + Lw) of B utterances of one length, for a caller that receives the waveform
 * piece by piece.  Any origin >= 0 and any Lw >= 0; `final` (0 or not) says that origin + Lw is the utterance's end, and the
 * window starts its utterance when origin == 0.  out[n] reads x[n - R .. n + R] and nothing else, R = 2 * lookahead + 7, so a
 * window settles the samples for which all of that lies inside the window or outside the utterance (where the whole-item call
 * also uses x = 0 and r = 1):
 *     window_range -> out_lo = origin + (origin > 0 ? R : 0) and out_count = max(0, origin + Lw - (final ? 0 : R) - out_lo).
 * An interior window loses R samples on either side: 73 at the default 1.5 ms and 22.05 kHz, 519 at lookahead 256.
 * forward_window: wav_dev [B, Lw] -> out_dev [B, out_count], packed rows, each sample bit for bit that of
 * iris_limiter_forward_ragged on the whole utterance; with out_is_pcm16 != 0 out_dev is int16 and holds (int16) rintf(clamp(out,
 * -1, 1) * 32767) of the same samples, the output stage's formula (the ceiling is at most 1, so the clamp never acts).
 * stats_out_dev [B][2] = (max p, min g) over the window's settled samples: the running (max, min) over an utterance's windows is
 * the whole-item call's stats.  Dense only; stateless; the same 2 launches with tiles over the settled samples, none when B == 0
 * or out_count == 0 (IRIS_HIFIGAN_OK, nothing is looked at).  The workspace is that of a call of shape (B, Lw); afterwards it
 * holds the partials [B][ceil(out_count / 2048)][2].  A negative origin or shape, a NULL pointer, out_dev off its type's
 * bytes or overlapping wav_dev return IRIS_HIFIGAN_INVALID_ARGUMENT; origin + Lw beyond int64, B > 65535 and B Lw above 2^31 - 1
 * IRIS_HIFIGAN_UNSUPPORTED; a short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches; nothing synchronises.
 * The first three are host only; window_launch_count is a dry run. */
int32_t iris_limiter_window_range(const iris_limiter_config* cfg, int64_t origin, int32_t Lw, int32_t final, int64_t* out_lo,
                                  int64_t* out_count);
int32_t iris_limiter_window_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t Lw, uint64_t* bytes);
int32_t iris_limiter_window_launch_count(const iris_limiter_config* cfg, int32_t B, int32_t Lw, int64_t origin, int32_t final,
                                         int32_t* n);
int32_t iris_limiter_forward_window(iris_limiter_handle* h, const float* wav_dev /* [B, Lw] */, int32_t B, int32_t Lw, int64_t origin,
                                    int32_t final, void* out_dev /* [B, out_count] fp32 or int16 */, int32_t out_is_pcm16,
                                    float* stats_out_dev /* [B][2] */, void* workspace_dev, uint64_t workspace_bytes, void* stream);

/* ---- Groups of windows: many streaming sessions in one call (iris.stream_group) -------------------------------------------
 * forward_window takes one origin and one `final` for its whole batch; a group call takes them per row, so the windows of B
 * DIFFERENT utterances -- each at its own position -- cost the launches of one.  Row b of wav_dev [B, in_stride] holds samples
 * [origin_b, origin_b + Lw_b) of its own utterance in its first Lw_b slots (Lw_b <= in_stride; the rest of the row is never
 * read).  What a row settles is the existing rule applied to its own item -- iris_limiter_window_range(origin_b, Lw_b, final_b),
 * iris_resampler_window_plan(origin_b, Lw_b, n_next_b, final_b) -- and goes to the first count_b slots of row b of out_dev
 * [B, out_stride]; the slots behind count_b hold the value of sample 0: 0.0f, int16 0, 0xFF as mu-law, 0xD5 as A-law.  Every
 * slot of out_dev is stored exactly once.  out_stride below any count_b is IRIS_HIFIGAN_INVALID_ARGUMENT.
 * Row b's count_b values -- and the limiter's stats -- are bit for bit those of the B = 1 forward_window call of the same item,
 * in every output form.
 * The descriptors are host arrays and travel BY VALUE in the kernel argument, indexed by the block's row: there is no device
 * descriptor buffer, no copy and nothing allocated, so the calls are asynchronous on `stream` and safe inside a stream capture,
 * as forward_window is -- and a call takes at most IRIS_WINDOW_GROUP_MAX rows (a kernel argument has 4 KB); B above it returns
 * IRIS_HIFIGAN_UNSUPPORTED and the caller splits.
 * Limiter: 2 launches, the tile kernel over grid.x = the largest tile count of the rows and the stats reduction over each row's
 * own tiles.  A row with count_b == 0 is legal: its output row is all padding and its stats are (0, 1).  When EVERY count is 0
 * nothing is launched and neither out_dev nor stats_out_dev is written, as forward_window leaves them for an empty window.  The
 * workspace is that of a call of shape (B, in_stride): windows_workspace_bytes.  windows_launch_count is a dry run: 2, or 0.
 * Resampler: ONE launch, no workspace; every row must meet window_plan's precondition, and one that does not fails the whole
 * call.  When every count is 0 nothing is launched.
 * Errors as the window entry points: a negative shape, origin or Lw_b, Lw_b > in_stride, a NULL pointer, out_dev off its type's
 * bytes, the limiter's out_dev overlapping wav_dev, the resampler's origin, Lw or n_next outside its bounds return
 * IRIS_HIFIGAN_INVALID_ARGUMENT; B in_stride or B out_stride above 2^31 - 1 IRIS_HIFIGAN_UNSUPPORTED; a short workspace
 * IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches. */
#define IRIS_WINDOW_GROUP_MAX 64
typedef struct iris_limiter_window_item { int64_t origin; int32_t Lw; int32_t final; } iris_limiter_window_item;
typedef struct iris_resampler_window_item { int64_t origin; int64_t n_next; int32_t Lw; int32_t final; } iris_resampler_window_item;
int32_t iris_limiter_windows_workspace_bytes(const iris_limiter_config* cfg, int32_t B, int32_t in_stride, uint64_t* bytes);
int32_t iris_limiter_windows_launch_count(const iris_limiter_config* cfg, int32_t B, const iris_limiter_window_item* items_host /* [B] */,
                                          int32_t* n);
int32_t iris_limiter_forward_windows(iris_limiter_handle* h, const float* wav_dev /* [B, in_stride] */, int32_t B, int32_t in_stride,
                                     const iris_limiter_window_item* items_host /* [B] */, void* out_dev /* [B, out_stride] fp32 or int16 */,
                                     int32_t out_stride, int32_t out_is_pcm16, float* stats_out_dev /* [B][2] */, void* workspace_dev,
                                     uint64_t workspace_bytes, void* stream);
int32_t iris_resampler_forward_windows(iris_resampler_handle* h, const float* wav_dev /* [B, in_stride] */, int32_t B, int32_t in_stride,
                                       const iris_resampler_window_item* items_host /* [B] */, void* out_dev /* [B, out_stride] */,
                                       int32_t out_stride, int32_t out_form, void* stream);

/* ---- Spectral distance: the sums behind the multi-resolution STFT distance and the SNR of two waveforms (csrc/spectral_distance.h) ----
 * ref_dev and test_dev [B, L], mono fp32, share lengths_dev (may be NULL) and row_scale >= 1 as in iris_loudness_normalize_ragged:
 * item b owns n_b = min(L, lengths[b] * row_scale) samples of both; samples past that are never read (they may hold NaN).  The
 * host never reads a length.  resolutions [n_res][3] = (n_fft, hop, win), 1 .. 4 of them, is a host array.  Per resolution, with
 * N = n_fft, H = hop, K = N / 2 + 1:
 *     the transform of csrc/stft_f32.h on both signals (center=True, constant padding, periodic Hann of win centred in N); item b
 *         has T_b = 1 + n_b / H frames (0 for n_b == 0) and ALL of its n_b samples are read -- n_b need not be a multiple of H;
 *     A (of ref) and B (of test) = sqrtf(re re + im im), fp32, bins 0 .. N / 2;
 *     over the item's T_b K cells, each term in fp64 from the two fp32 values:  d2 = sum (A - B)^2;  a2 = sum A^2;
 *         l1 = sum |log(max(A, 1e-5)) - log(max(B, 1e-5))| (the mel front-end's clip, the logarithm in double).
 * Over the item's n_b samples x (ref), y (test):  e2 = sum (x - y)^2 and x2 = sum x^2 in fp64; emax = max |x - y| in fp32.
 * spec_out_dev [B][n_res][3] = (d2, a2, l1) and wave_out_dev [B][3] = (e2, x2, (double)emax), doubles; frames_out_dev [B][n_res] =
 * T_b.  An item with n_b == 0 has frames 0 and every sum 0.  The caller finishes them: spectral convergence sqrt(d2 / a2), log-STFT
 * L1 l1 / (T_b K), SNR 10 log10(x2 / e2) dB.  csrc/spectral_distance.h states the order of every sum: fixed tiles of 8 frames and
 * chunks of 4096 samples counted from the item's own start, a fixed thread map and tree, no atomics -- item b's results are those
 * of its batch-of-one call on its own n_b samples, and two runs give the same bits.
 * 3 n_res + 2 launches: per resolution the transform of ref, of test, and the tile sums; the chunk sums; the sums of an item's
 * partials.  After a call the workspace holds, each starting on 256 bytes: the two magnitude buffers [B][1 + L / H][Ks] of the
 * LAST resolution (fp32, Ks = K rounded up to 4, sized for the largest), every resolution's tile sums [B][ceil((1 + L / H) / 8)][3]
 * and the chunk sums [B][ceil(L / 4096)][3] (doubles); only what belongs to an item's own frames and samples is written.
 * test_dev may be ref_dev.  Asynchronous on `stream`, nothing allocated, safe in a stream capture.
 * The handle owns one packed windowed DFT per resolution and no inverse table.
 * n_res outside 1 .. 4, a size below 1, win > n_fft, hop not dividing n_fft, row_scale < 1, a negative shape, a NULL pointer,
 * spec_out_dev, wave_out_dev or workspace_dev off 8 bytes return IRIS_HIFIGAN_INVALID_ARGUMENT; n_fft above 4096 or no multiple
 * of 32, hop no multiple of 4, a frame window beyond the LDS, B > 65535 (grid.y) and B L above 2^31 - 1 IRIS_HIFIGAN_UNSUPPORTED; a
 * short workspace IRIS_HIFIGAN_WORKSPACE_TOO_SMALL.  No failing call launches.  B == 0 or L == 0: nothing to do, nothing is
 * written, IRIS_HIFIGAN_OK. */
typedef struct iris_spectral_distance_handle iris_spectral_distance_handle;
/* Host only (no device is needed); the launch count is a dry run of the forward's own code. */
int32_t iris_spectral_distance_workspace_bytes(const int32_t* resolutions /* [n_res][3] */, int32_t n_res, int32_t B, int32_t L,
                                               uint64_t* bytes);
int32_t iris_spectral_distance_launch_count(const int32_t* resolutions /* [n_res][3] */, int32_t n_res, int32_t B, int32_t L, int32_t* n);
/* create: on the current device, which becomes the handle's; it packs and uploads the tables. */
int32_t iris_spectral_distance_create(const int32_t* resolutions /* [n_res][3] */, int32_t n_res, iris_spectral_distance_handle** out);
int32_t iris_spectral_distance_destroy(iris_spectral_distance_handle* h);
int32_t iris_spectral_distance_forward(iris_spectral_distance_handle* h, const float* ref_dev /* [B, L] */, const float* test_dev /* [B, L] */,
                                       int32_t B, int32_t L, const int32_t* lengths_dev /* or NULL */, int32_t row_scale,
                                       double* spec_out_dev /* [B][n_res][3] */, double* wave_out_dev /* [B][3] */,
                                       int32_t* frames_out_dev /* [B][n_res] */, void* workspace_dev, uint64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IRIS_HIFIGAN_H */
