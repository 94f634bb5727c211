// stft_f32.h -- the two fp32 transforms the DSP stages share, with everything that belongs to a transform and to no one stage:
// the windowed forward DFT of the mel front-end (mel_frontend.h), the spectral distance (spectral_distance.h), Griffin-Lim
// (griffin_lim.h) and the bias denoiser (denoiser.h), and the windowed inverse STFT of the last two.  N = n_fft, H = hop,
// K = N / 2 + 1 bins, T frames.
//
//   frames   center=True, pad_mode="constant": frame t covers samples [t H - N / 2, t H + N / 2) of the item, 0 outside its own
//            [0, n); an item of n samples has 1 + n / H frames
//   window   periodic Hann of win_length, (N - win_length) / 2 zeros in front of it and the rest behind
//   stft     sum_n x[n] w[n] e^(-2 pi i k n / N), k = 0 .. N / 2
//   istft    w[n] irfft(c[:, t])[n] overlap-added, divided by the window-sum-square where that exceeds FLT_MIN, N / 2
//            samples trimmed at each end; Im of bins 0 and N / 2 is ignored
//
// Tables (host only): the windowed DFT  w[n] cos(2 pi k n / N), w[n] sin(2 pi k n / N)  and the windowed inverse DFT are
// evaluated in double with the angle reduced by (k n) mod N first (one table of N cosines and sines serves every entry), w^2
// in double; all are rounded once to fp32.  These are the bits the kernels multiply by.  pack_tables puts them into a stage's
// blob in fragment order (packed_conv_f32.h).
//
// Forward transform as a GEMM: view an item's samples as rows of H floats; the windowed DFT of frame t is a k = N / H tap,
// C_in = H implicit-GEMM convolution over rows t .. t + k - 1 of the window that starts N / 2 samples before frame t's centre
// -- the formulation of vae_gemm_kernel, on the MFMA loop of gemm_tile_f32.h.  A block owns 32 frames and stages their 31 + k
// rows once (stage_window; rows padded to hop8 + 4 floats: conflict-free 16-byte reads).  Output columns come in 32-wide tiles
// that pair Re and Im of the same 16 bins in one lane:
//     column j of tile ct:  bin = 16 ct + 8 ((j >> 3) & 1) + (j & 7),  Re for j < 16, the sine sum (= -Im) for j >= 16
// Im of bin 0 is identically 0, so that column carries Re of bin N / 2 instead (whose Im is 0 as well): N / 2 bin pairs,
// ceil(N / 32) tiles.  decode_bins is the one place that reads an accumulator tile by this rule.
//
// Buffers of stft_kernel and gl_istft_kernel (fp32, frame-major so that a block stages 32 frames as 32 LDS rows):
//   S, mag, bias [..][Ks]  Ks = K rounded up to 4
//   c, r [B][T][Qp] interleaved complex: column 2 k is Re, 2 k + 1 is Im of bin k; Q = N + 2 columns, Qp = Q rounded up to 8
//                  (columns from Q on are never written and read as 0)
//   y [B][L]
//
// stft_kernel<Policy>: the forward transform with a stage's arithmetic as its epilogue (dn::Subtract, dn::Magnitude; what a
// policy is stands beside the kernel).  grid.z counts groups of 8 column tiles, so a wave runs one tile.  gl_stft_update_kernel
// (griffin_lim.h) is this kernel written out with the phase update in it: as a policy it ran 0.3 % slower per forward.
//
// gl_istft_kernel: gather form, no atomics.  View the zero-padded signal as rows of H samples: row j is the sum over taps
// kap < N / H of frame j - kap's samples [kap H, (kap + 1) H) -- an N / H tap, C_in = Q implicit-GEMM convolution over frames
// against the windowed inverse-DFT table [Q][N], with the taps in reverse order.  A block owns 32 rows and a wave one 32-wide
// tile of a row's H columns (grid.z counts groups of 8 tiles); the Q columns are staged in slices of 256 (the text stage's
// precedent), 31 + N / H frames at a time.  The epilogue sums w^2 over the frames that exist (at most N / H terms, ascending
// tap), divides and stores the samples that survive the trim.  launch_istft_slice stores samples [s_org, s_org + Ly) only
// ("Windows" in denoiser.h).  Internal linkage: each translation unit that launches it carries its own copy.
//
// Summation: the MFMA adds a chain's terms one after the other, and a chain of N / H * (N + 2) = 4104 terms (the inverse STFT
// at the defaults) loses more than the blocked sums of a host BLAS.  Both kernels here therefore run short chains and add the
// partial sums: one per tap and 64 columns (inverse) or 64 samples (forward).  mel_kernel deliberately does not: its DFT is
// one long chain (mel_frontend.h).
//
// Ragged batches: each kernel takes `lengths` (a device pointer to [B] counts, or NULL: every item has T frames).  A block
// reads T_b = item_frames(lengths, b, T, extra): lengths[b] clamped to [0, T - extra], plus extra, 0 if that is below 2.
// extra = 0: the counts are frames (Griffin-Lim, the inverse kernel); extra = 1: they are mel frames M_b of a waveform of
// H M_b samples, which has M_b + 1 frames (the denoiser).  L_b = H (T_b - 1) bounds the loads, the window-sum-square terms and
// the stores; strides stay T and L, and the tiling (i0 = 32 blockIdx.x, j0 = first_row + 32 blockIdx.x) does not depend on T,
// so every chain of item b has the terms and the order of its batch-of-one call at T = T_b.  A block past its item returns
// before its first barrier.  Nothing at t >= T_b is read or written, except that an inverse transform with zero_tail set
// stores 0.f to y[b, L_b:].  The time stretch (time_stretch.h) sets IstftLaunch::sample_counts beside `lengths`: item b then owns
// sample_counts[b] samples instead of H (T_b - 1) and lengths[b] frames as they stand (one frame is an item), which is
// istft(c, length=); samples past H (T_b - 1) + N / 2 have no frame and come out as 0.  NULL in every other launch.
#pragma once
#include <float.h>
#include <math.h>

#include "stage_host.h"

namespace iris {
namespace stft {

constexpr int kRows = 32;            // frames (forward) or output rows (inverse) of a block: the MFMA's rows
constexpr int kWaves = 8;
constexpr int kSlice = 256;          // columns of c staged at a time by the inverse transform
constexpr size_t kMaxLdsBytes = 160 * 1024;

// What the transforms derive from (n_fft, hop); win only shapes the window.
struct Sizes {
    int n_fft = 0, hop = 0, win = 0;
    int taps() const { return n_fft / hop; }
    int bins() const { return n_fft / 2 + 1; }
    int dft_tiles() const { return (n_fft / 2 + 15) / 16; }
    int hop_tiles() const { return (hop + 31) / 32; }
    int hop8() const { return (hop + 7) & ~7; }
    int ks() const { return (bins() + 3) & ~3; }
    int q() const { return n_fft + 2; }
    int qp() const { return (q() + 7) & ~7; }
    int first_row() const { return (n_fft / 2) / hop; }                      // the padded row that holds output sample 0
    int window_rows() const { return kRows - 1 + taps(); }
    size_t stft_lds_bytes() const { return (size_t)window_rows() * (hop8() + 4) * sizeof(float); }
    size_t istft_lds_bytes() const { return (size_t)window_rows() * (kSlice + 4) * sizeof(float); }
};

// periodic Hann of `win`, centred in n_fft (librosa pad_center)
inline void fill_window(const Sizes& d, std::vector<double>& w) {
    const double two_pi = 6.283185307179586476925286766559;
    w.assign(d.n_fft, 0.0);
    const int lpad = (d.n_fft - d.win) / 2;
    for (int n = 0; n < d.win; ++n) w[lpad + n] = 0.5 - 0.5 * cos(two_pi * n / d.win);
}

// dft [2][bins][n_fft]: w[n] cos(2 pi k n / n_fft), then w[n] sin(2 pi k n / n_fft)
inline void fill_dft(const Sizes& d, float* dft) {
    const double two_pi = 6.283185307179586476925286766559;
    const int N = d.n_fft, nb = d.bins();
    std::vector<double> w, c(N), s(N);
    fill_window(d, w);
    for (int j = 0; j < N; ++j) { c[j] = cos(two_pi * j / N); s[j] = sin(two_pi * j / N); }
    s[0] = 0.0;
    if (!(N & 1)) s[N / 2] = 0.0;                       // sin(pi): exactly 0, not 1.2e-16
    for (int k = 0; k < nb; ++k)
        for (int n = 0; n < N; ++n) {
            const int j = (int)(((long long)k * n) % N);
            dft[(size_t)k * N + n] = (float)(w[n] * c[j]);
            dft[((size_t)nb + k) * N + n] = (float)(w[n] * s[j]);
        }
}

// idft [2][bins][n_fft]: w[n] f_k cos(2 pi k n / N) / N, then -w[n] f_k sin(2 pi k n / N) / N, with f_k = 1 for k = 0 and
// N / 2 and 2 otherwise -- w[n] irfft(c)[n] = sum_k Re c_k idft[0][k][n] + Im c_k idft[1][k][n].  In double, angle reduced
// by (k n) mod N, rounded once.
inline void fill_idft(const Sizes& d, float* idft) {
    const double two_pi = 6.283185307179586476925286766559;
    const int N = d.n_fft, nb = d.bins();
    std::vector<double> w, c(N), s(N);
    fill_window(d, w);
    for (int j = 0; j < N; ++j) { c[j] = cos(two_pi * j / N); s[j] = sin(two_pi * j / N); }
    s[0] = 0.0;
    if (!(N & 1)) s[N / 2] = 0.0;
    for (int k = 0; k < nb; ++k) {
        const bool edge = k == 0 || 2 * k == N;
        const double f = (edge ? 1.0 : 2.0) / N;
        for (int n = 0; n < N; ++n) {
            const int j = (int)(((long long)k * n) % N);
            idft[(size_t)k * N + n] = (float)(w[n] * f * c[j]);
            idft[((size_t)nb + k) * N + n] = edge ? 0.f : (float)(-(w[n] * f * s[j]));
        }
    }
}

// wsq [n_fft]: w[n]^2 in double, rounded once
inline void fill_wsq(const Sizes& d, float* wsq) {
    std::vector<double> w;
    fill_window(d, w);
    for (int n = 0; n < d.n_fft; ++n) wsq[n] = (float)(w[n] * w[n]);
}

// The DFT table as the [C_out][C_in = hop][k] Conv1d weight the forward transform's column order asks for (see the head of
// the file).
inline void conv_weight_from_dft(const Sizes& d, const float* dft, std::vector<float>& w) {
    const int N = d.n_fft, H = d.hop, K = d.taps(), nb = d.bins(), half = N / 2, C_out = 32 * d.dft_tiles();
    w.assign((size_t)C_out * H * K, 0.f);
    for (int co = 0; co < C_out; ++co) {
        const int j = co & 31, bin = 16 * (co >> 5) + 8 * ((j >> 3) & 1) + (j & 7), im = j >> 4;
        if (bin >= half) continue;
        const float* row = (bin == 0 && im) ? dft + (size_t)half * N : dft + ((size_t)(im ? nb : 0) + bin) * N;
        for (int ci = 0; ci < H; ++ci)
            for (int kap = 0; kap < K; ++kap) w[((size_t)co * H + ci) * K + kap] = row[kap * H + ci];
    }
}

// The inverse table as the [C_out = 32 * hop_tiles][C_in = Q][k = taps] Conv1d weight of the gather: tap kk multiplies frame
// j - (taps - 1 - kk), whose samples [(taps - 1 - kk) H, ...) land in row j.
inline void conv_weight_from_idft(const Sizes& d, const float* idft, std::vector<float>& w) {
    const int N = d.n_fft, H = d.hop, K = d.taps(), nb = d.bins(), Q = d.q(), C_out = 32 * d.hop_tiles();
    w.assign((size_t)C_out * Q * K, 0.f);
    for (int co = 0; co < H; ++co)
        for (int q = 0; q < Q; ++q) {
            const float* row = idft + ((size_t)(q & 1 ? nb : 0) + (q >> 1)) * N;
            for (int kk = 0; kk < K; ++kk) w[((size_t)co * Q + q) * K + kk] = row[(K - 1 - kk) * H + co];
        }
}

// Where a stage's blob holds the packed transforms.
struct Tables { PackedGemm dft, idft; size_t wsq_off = 0; };

// Fills the windowed DFT and packs it into the blob; with `inverse`, the windowed inverse DFT and w^2 behind it.
inline void pack_tables(BlobBuilder& bb, const Sizes& d, bool inverse, Tables& t) {
    const int nb = d.bins(), N = d.n_fft;
    const std::vector<float> no_bias(32 * (d.dft_tiles() > d.hop_tiles() ? d.dft_tiles() : d.hop_tiles()), 0.f);   // neither GEMM has one
    std::vector<float> table((size_t)2 * nb * N), w;
    fill_dft(d, table.data());
    conv_weight_from_dft(d, table.data(), w);
    bb.dense(t.dft, w.data(), no_bias.data(), d.hop, 32 * d.dft_tiles(), d.taps());
    if (!inverse) return;
    fill_idft(d, table.data());
    conv_weight_from_idft(d, table.data(), w);
    bb.dense(t.idft, w.data(), no_bias.data(), d.q(), 32 * d.hop_tiles(), d.taps());
    t.wsq_off = bb.reserve(N);
    fill_wsq(d, bb.host.data() + t.wsq_off);
}

// What stft_kernel and gl_istft_kernel ask of a config that the front-end's rules (mel_validate) leave open: two rules, so that
// a stage with a rule of its own between them (Griffin-Lim's inversion) keeps its order of error texts.
inline int validate_bin_tiles(const Sizes& d) {
    if (d.n_fft % 32) return fail(IRIS_HIFIGAN_UNSUPPORTED, "n_fft %d is not a multiple of 32 (bins come in tiles of 16)", d.n_fft);
    return IRIS_HIFIGAN_OK;
}
inline int validate_frame_window(const Sizes& d) {
    const size_t transform = d.istft_lds_bytes() > d.stft_lds_bytes() ? d.istft_lds_bytes() : d.stft_lds_bytes();
    if (transform > kMaxLdsBytes)
        return fail(IRIS_HIFIGAN_UNSUPPORTED, "the frame window of n_fft %d, hop_length %d (31 + %d frames) needs %llu bytes of LDS, more than "
                    "%llu: no form that slices the frames is built", d.n_fft, d.hop, d.taps(), (unsigned long long)transform,
                    (unsigned long long)kMaxLdsBytes);
    return IRIS_HIFIGAN_OK;
}
inline int transform_validate(const Sizes& d) {
    TRY(validate_bin_tiles(d));
    return validate_frame_window(d);
}

// frames on either side whose window leaves the signal
inline int edge_frames(const Sizes& d) { return (d.n_fft / 2 + d.hop - 1) / d.hop; }

// The finality rule of "Windows" in denoiser.h for the window [H m0, H (m0 + Mw)): frames [f_lo, f_hi) are computable (f_lo is
// clamped to f_hi when there is none) and samples [out_lo, out_lo + out_count) are final.  Frames before f_lo exist unless
// m0 == 0, frames from f_hi on exist unless `final`, so a row j = floor((s + n_fft / 2) / H) is final when
// j - taps + 1 >= f_lo (or m0 == 0) and j < f_hi (or final).
struct Window {
    long long f_lo, f_hi, out_lo, out_count;
    Window(const Sizes& d, long long m0, long long Mw, bool final) {
        const long long H = d.hop, half = d.n_fft / 2, e = edge_frames(d), o = H * m0, end = o + H * Mw;
        f_lo = m0 ? m0 + e : 0;
        f_hi = final ? m0 + Mw + 1 : m0 + Mw - e + 1;
        if (f_hi < f_lo) f_hi = f_lo;
        long long lo = o, hi = end;
        if (m0 && (f_lo + d.taps() - 1) * H - half > lo) lo = (f_lo + d.taps() - 1) * H - half;
        if (!final && f_hi * H - half < hi) hi = f_hi * H - half;
        out_count = f_hi > f_lo && hi > lo ? hi - lo : 0;
        out_lo = out_count ? lo : o;
    }
};

}  // namespace stft
}  // namespace iris

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <type_traits>
#include "device_info.h"
#include "gemm_tile_f32.h"

namespace iris {
namespace stft {

// T_b of item b ("Ragged batches" above); lengths == NULL: T.  The clamp comes before the increment, so INT_MAX cannot overflow.
__device__ __forceinline__ int item_frames(const int* lengths, int b, int T, int extra) {
    if (!lengths) return T;
    int n = lengths[b];
    n = (n < 0 ? 0 : (n > T - extra ? T - extra : n)) + extra;
    return n < 2 ? 0 : n;
}

__device__ __forceinline__ float load_sample(const float* x, size_t i) { return x[i]; }
__device__ __forceinline__ float load_sample(const int16_t* x, size_t i) { return (float)x[i] * (1.0f / 32768); }

// Stages a block's window of 31 + taps rows: row r, column c is sample s0 + r * hop + c of `item`; 0 outside [0, n) and in
// the columns from hop up to hop8.
template <class Sample>
__device__ __forceinline__ void stage_window(float* lds, const Sample* item, long long s0, int n, int hop, int taps) {
    const int Cp = (hop + 7) & ~7, S = Cp + 4, total = (kRows - 1 + taps) * Cp;
    for (int idx = threadIdx.x; idx < total; idx += 64 * kWaves) {
        const int r = idx / Cp, c = idx - r * Cp;
        const long long s = s0 + (long long)r * hop + c;
        lds[r * S + c] = (c < hop && s >= 0 && s < n) ? load_sample(item, (size_t)s) : 0.f;
    }
}

// Reads a lane's 16 accumulators of column tile ct by the rule at the head of the file.  D[col][frame]: lane & 31 = frame,
// registers 4g .. 4g + 3 = columns 8g + 4 (lane >> 5) + {0..3}; g < 2 Re, g >= 2 the sine sum.  bins4(bin0, re, im, nyq) gets each
// group of four bins that starts below n_fft / 2, with im = -sine (the table holds +sin) and Im of bin 0 as 0.f.  Where
// bin0 == 0 -- one lane of tile 0 -- nyq is Re of bin n_fft / 2; it comes with that group so that an epilogue can have the
// group's loads in flight before it turns to the Nyquist bin.
template <class Bins4>
__device__ __forceinline__ void decode_bins(const f32x16& acc, int ct, int hi, int half, Bins4 bins4) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int bin0 = 16 * ct + 8 * g + 4 * hi;
        if (bin0 >= half) continue;
        float re[4], im[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { re[e] = acc[4 * g + e]; im[e] = -acc[4 * (g + 2) + e]; }
        if (bin0 == 0) im[0] = 0.f;
        bins4(bin0, re, im, acc[4 * (g + 2)]);
    }
}

struct StftLaunch {
    const float* y;           // [B, L]; frame 0 is centred on sample y_org
    const f32x4* wdft;        // the packed windowed DFT
    const int* lengths;       // [B] counts (Policy::kExtraFrames says of what), or NULL
    int L, T, hop, taps, n_fft, Ks, Qp, Gp, n_ct;
    int y_org;                // a window: H f_lo - o ("Windows" in denoiser.h); 0 for a whole utterance, where L = H (T - 1)
};

// The kernel owns the block and wave indices, the item's bounds, the staging, the chain loop and the decode.  A Policy is a
// stage's launch arguments and its arithmetic:
//   kName, kExtraFrames                        the launch's name in dry runs and profiles; the `extra` of item_frames
//   void item(int b, int Tb) const             once per item, from one thread (dn::Subtract stores T_b)
//   void bins4(a, row, bin0, re, im, nyq) const   four bins of frame `row` = b T + t: 8 consecutive floats of an interleaved
//                                              row; where bin0 == 0, nyq is bin n_fft / 2 of that frame (decode_bins)
//   int samples(int b, int L) const            optional (sd::Magnitude): the item owns that many samples n_b, ALL of them read,
//                                              and T_b = 1 + n_b / H frames (0 for n_b == 0) -- n_b need not be a multiple of H;
//                                              a.lengths and kExtraFrames are then not looked at.  A policy without it compiles
//                                              to the frame rule of "Ragged batches" above, as before the trait existed.
template <class Policy, class = void> struct owns_samples : std::false_type {};
template <class Policy> struct owns_samples<Policy, std::void_t<decltype(&Policy::samples)>> : std::true_type {};

template <class Policy>
__global__ void __launch_bounds__(64 * kWaves) stft_kernel(const StftLaunch a, const Policy p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * kRows;
    const int ct = blockIdx.z * kWaves + wave;               // wave-uniform
    const int H = a.hop, Cp = (H + 7) & ~7, S = Cp + 4, half = a.n_fft >> 1;
    int Tb, Lb = 0;
    if constexpr (owns_samples<Policy>::value) {
        Lb = p.samples(b, a.L);
        Tb = Lb > 0 ? 1 + Lb / H : 0;
    } else {
        Tb = item_frames(a.lengths, b, a.T, Policy::kExtraFrames);
    }
    if (blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) p.item(b, Tb);
    if (i0 >= Tb) return;                                    // block-uniform: all 32 frames lie past the item
    if constexpr (!owns_samples<Policy>::value) Lb = a.lengths ? H * (Tb - 1) : a.L;     // H (T - 1) of a dense whole utterance as well

    stage_window(lds, a.y + (size_t)b * a.L, (long long)a.y_org + (long long)i0 * H - half, Lb, H, a.taps);
    __syncthreads();
    const int t = i0 + lo;
    if (ct >= a.n_ct) return;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kk = 0; kk < a.taps; ++kk)                      // one chain per tap and 64 samples (see "Summation" above)
        for (int g0 = 0; g0 < Cp >> 3; g0 += 8) {
            f32x16 part;
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.f;
            mma_loop(part, lds + (lo + kk) * S + 4 * hi + 8 * g0, 0, a.wdft + ((size_t)kk * a.Gp + g0) * a.n_ct * 64 + (size_t)ct * 64 + lane,
                     (size_t)a.n_ct * 64, a.Gp, 1, (Cp >> 3) - g0 < 8 ? (Cp >> 3) - g0 : 8);
            acc += part;
        }
    if (t >= Tb) return;

    const size_t row = (size_t)b * a.T + t;
    decode_bins(acc, ct, hi, half, [&](int bin0, const float (&re)[4], const float (&im)[4], float nyq) { p.bins4(a, row, bin0, re, im, nyq); });
}

// The caller sets y, lengths, L, T and y_org (a whole utterance: L = hop * (T - 1), y_org = 0).
template <class Policy>
inline hipError_t launch_stft(StftLaunch& a, const Policy& p, const Sizes& d, int B, hipStream_t stream) {
    a.hop = d.hop; a.taps = d.taps(); a.n_fft = d.n_fft; a.Ks = d.ks(); a.Qp = d.qp();
    a.Gp = packed_groups(d.hop); a.n_ct = d.dft_tiles();
    const dim3 grid((unsigned)((a.T + kRows - 1) / kRows), (unsigned)B, (unsigned)((a.n_ct + kWaves - 1) / kWaves)), block(64 * kWaves);
    return launch_kernel_named(Policy::kName, stft_kernel<Policy>, grid, block, d.stft_lds_bytes(), stream, a, p);
}

#ifndef IRIS_STFT_NO_INVERSE             // a translation unit that launches no inverse transform carries no copy of it
struct IstftLaunch {
    const float* c;           // [B, T, Qp]
    const f32x4* widft;       // packed inverse table: `taps` taps, Gp groups, n_ct column tiles
    const float* wsq;         // [n_fft]
    float* y;                 // [B, Ly]: samples [s_org, s_org + Ly)
    const int* lengths;       // [B] frame counts, or NULL
    const int* sample_counts; // [B] or NULL (every launch but the time stretch's): item b owns samples [0, sample_counts[b]) and
                              // lengths[b] frames, one frame included -- istft(c, length=) on a ragged batch (time_stretch.h)
    int T, Ly, hop, taps, n_fft, Q, Qp, Gp, n_ct, first_row;
    int zero_tail;            // the last transform of a ragged forward: y[b, Ly_b:] = 0
    int s_org;                // 0, and Ly = hop * (T - 1), unless a slice of the samples is stored (launch_istft_slice)
};

static __global__ void __launch_bounds__(64 * kWaves) gl_istft_kernel(const IstftLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nthr = 64 * kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = a.first_row + blockIdx.x * kRows;         // the block's first padded row
    const int ct = blockIdx.z * kWaves + wave;               // wave-uniform
    const int R = kRows - 1 + a.taps, S = kSlice + 4;
    const int t0 = j0 - (a.taps - 1);                        // LDS row r holds frame t0 + r
    int Tb, Lyb;
    if (a.sample_counts) {
        Tb = a.lengths[b] < 0 ? 0 : (a.lengths[b] > a.T ? a.T : a.lengths[b]);
        Lyb = a.sample_counts[b] < 0 ? 0 : (a.sample_counts[b] > a.s_org + a.Ly ? a.s_org + a.Ly : a.sample_counts[b]);
    } else {
        Tb = item_frames(a.lengths, b, a.T, 0);
        Lyb = a.lengths ? (Tb ? a.hop * (Tb - 1) : 0) : a.s_org + a.Ly;                  // dense: the end of what is stored, hop * (T - 1)
    }
    const long long s_first = (long long)j0 * a.hop - (a.n_fft >> 1);     // the block's first sample; negative ones are trimmed
    if (Lyb <= (s_first > 0 ? s_first : 0)) {                // block-uniform: every row lies past the item
        if (a.zero_tail && ct < a.n_ct) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = ct * 32 + 8 * g + 4 * hi + e;
                    const long long s = s_first + (long long)lo * a.hop + col - a.s_org;
                    if (col < a.hop && s >= 0 && s < a.Ly) a.y[(size_t)b * a.Ly + (size_t)s] = 0.f;
                }
        }
        return;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int q0 = 0; q0 < a.Qp; q0 += kSlice) {
        const int width = a.Qp - q0 < kSlice ? a.Qp - q0 : kSlice;          // a multiple of 8
        for (int idx = tid; idx < R * (kSlice / 4); idx += nthr) {
            const int r = idx / (kSlice / 4), q = q0 + 4 * (idx - r * (kSlice / 4)), t = t0 + r;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t >= 0 && t < Tb && q < a.Qp) {
                v = *reinterpret_cast<const f32x4*>(a.c + ((size_t)b * a.T + t) * a.Qp + q);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = q + e < a.Q ? v[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(lds + r * S + (q - q0)) = v;
        }
        __syncthreads();
        if (ct < a.n_ct)
            for (int kk = 0; kk < a.taps; ++kk)              // one chain per tap and 64 columns (see "Summation" above)
                for (int g0 = 0; g0 < width >> 3; g0 += 8) {
                    f32x16 part;
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[r] = 0.f;
                    mma_loop(part, lds + (lo + kk) * S + 4 * hi + 8 * g0, 0,
                             a.widft + ((size_t)kk * a.Gp + (q0 >> 3) + g0) * a.n_ct * 64 + (size_t)ct * 64 + lane, (size_t)a.n_ct * 64, a.Gp, 1,
                             (width >> 3) - g0 < 8 ? (width >> 3) - g0 : 8);
                    acc += part;
                }
        __syncthreads();
    }
    if (ct >= a.n_ct) return;

    // D[col][row]: lane & 31 = row, registers 4g .. 4g + 3 = columns 8g + 4 (lane >> 5) + {0..3}
    const int j = j0 + lo, half = a.n_fft >> 1;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = ct * 32 + 8 * g + 4 * hi + e;
            const long long s = (long long)j * a.hop + col - half, so = s - a.s_org;
            if (col >= a.hop || so < 0 || so >= a.Ly) continue;
            if (s >= Lyb) {
                if (a.zero_tail) a.y[(size_t)b * a.Ly + (size_t)so] = 0.f;
                continue;
            }
            float wss = 0.f;
            for (int kap = 0; kap < a.taps; ++kap) {
                const int t = j - kap;
                if (t >= 0 && t < Tb) wss += a.wsq[kap * a.hop + col];
            }
            const float v = acc[4 * g + e];
            a.y[(size_t)b * a.Ly + (size_t)so] = wss > FLT_MIN ? v / wss : v;
        }
}

// Stores samples [s_org, s_org + Ly) of istft(c [B, T, Qp]) into y [B, Ly]; the caller has set both (Ly > 0, s_org >= 0).
inline hipError_t launch_istft_slice(IstftLaunch& a, const Sizes& d, int B, hipStream_t stream) {
    a.hop = d.hop; a.taps = d.taps(); a.n_fft = d.n_fft; a.Q = d.q(); a.Qp = d.qp();
    a.Gp = packed_groups(d.q()); a.n_ct = d.hop_tiles();
    a.first_row = (int)(((long long)d.n_fft / 2 + a.s_org) / d.hop);                     // the padded row of the first sample
    const long long last = ((long long)d.n_fft / 2 + a.s_org + a.Ly - 1) / d.hop;       // and of the last
    const int rows = (int)(last - a.first_row + 1);
    const dim3 grid((unsigned)((rows + kRows - 1) / kRows), (unsigned)B, (unsigned)((a.n_ct + kWaves - 1) / kWaves)), block(64 * kWaves);
    return launch_kernel_named("gl_istft_kernel", gl_istft_kernel, grid, block, d.istft_lds_bytes(), stream, a);
}

inline hipError_t launch_istft(IstftLaunch& a, const Sizes& d, int B, hipStream_t stream) {
    a.Ly = d.hop * (a.T - 1); a.s_org = 0;                                               // first_row = d.first_row()
    return launch_istft_slice(a, d, B, stream);
}

#endif

}  // namespace stft
}  // namespace iris
#endif
