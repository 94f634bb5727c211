// time_stretch.h -- the phase vocoder between the two transforms of stft_f32.h (iris_time_stretch_*): tempo without pitch,
// librosa.effects.time_stretch(y, rate=, n_fft=, hop_length=, win_length=) under that file's frame rules, fp32.
// N = n_fft, H = hop, K = N / 2 + 1 bins.  A waveform of L = H M samples has T = M + 1 frames c[t, k] = stft(y).
//
//   T_out     = ceil(T / rate) in double                    (len(np.arange(0, T, rate)))
//   step_t    = t * rate in double;  i = floor(step_t);  alpha = (float)(step_t - i);  a column >= T reads as 0
//   mag[t,k]  = fmaf(alpha, |c[i+1,k]|, (1 - alpha) |c[i,k]|)          |c| = sqrtf(re re + im im)
//   dphi      = turns(c[i+1,k]) - turns(c[i,k]) - adv_k;  dphi -= rintf(dphi)
//   acc[0,k]  = fixed(turns(c[0,k]));  acc[t+1,k] = acc[t,k] + inc[t,k],  inc = adv_fixed_k + fixed(dphi)
//   out_c[t,k]= mag[t,k] (cos, sin)(2 pi acc[t,k] / 2^32)
//   n_out     = rint(L / rate) in double (half to even)
//   y_out     = istft(out_c, length = n_out): samples below min(n_out, H (T_out - 1) + N / 2) are the overlap-add value over the
//               window-sum-square of the frames that exist, the rest are 0
//
// Phase is accumulated in 32-bit fixed-point turns, 2^32 = one turn: the advance of the top bin is pi H radians a frame, and
// an fp32 sum of radians would stand near 8e5 after 1000 frames at hop 256, where one ulp is 0.06 rad.  A uint32 sum wraps
// for free and is associative, so the scan along t may run in any order and every run gives the same bits.  The
// conversions, written down here once:
//   turns(c)      atan2f(im, re) * (1 / (2 pi)) in fp32: [-0.5, 0.5]
//   wrap          x - rintf(x): the nearest representative of x turns, [-0.5, 0.5]
//   fixed(x)      (uint32)(int64)llrintf(x * 4294967296.f): half a turn is 2^31 either way round
//   adv_k         r = (k H) mod N;  adv_fixed_k = (uint32)(((uint64)r << 32) / N);  in fp32 turns (float)r / (float)N
//   unfixed(a)    (float)(int32)a * 2^-32: [-0.5, 0.5)
//
// Four launches: stft_kernel<ts::Spectrum> (the plain interleaved spectrum c [B, T, Qp] and the items' counts), ts_step_kernel
// (mag and inc [B, T_out, Ks]), ts_scan_kernel (the exclusive scan of inc along t, acc [B, T_out, Ks], and the phasor
// out_c [B, T_out, Qp]) and gl_istft_kernel bounded by the items' sample counts (IstftLaunch::sample_counts).
//
// ts_scan_kernel is two-level: a block owns kScanBins bins of one item and splits the item's T_out_b frames into kScanRuns
// runs of ceil(T_out_b / kScanRuns) frames; a thread sums its run of one bin, the run sums go to LDS, a thread adds those
// in front of its own, and walks its run again.  Integer sums: no order matters, no atomics.
//
// Ragged batches: `lengths` (device [B], or NULL) holds MEL frames M_b as in denoiser.h: T_b = M_b + 1 (0 if M_b == 0),
// L_b = H M_b.  Spectrum::item computes T_out_b = ceil(T_b / rate) and n_out_b = rint(L_b / rate) on the device, in double, and
// stores them with T_b; every later launch bounds item b by them.  Strides are those of the dense call (T, T_out, n_out of
// the whole L), a thread's work depends on its own (b, t, k) alone, and so item b is bit for bit its batch-of-one call.
// out_samples() is the same arithmetic on the host.
//
// Windows (iris_time_stretch_forward_window): a dense call on samples [o, o + Lw) of an utterance, o = H m0, Lw = H Mw, `final`
// when o + Lw is the utterance's end -- only then are M = m0 + Mw, T = M + 1, T_out and n_out known.  taps = N / H >= 2,
// e = stft::edge_frames.  Input rows [f_lo, f_hi) are computable as for the denoiser (stft::Window).  The caller carries one
// integer u, the next output frame (0 at the start), and the state below.  With i(t) = floor((double)t * rate):
//   frames    not final: t is computable iff i(t) >= f_lo and i(t) + 1 < f_hi (whether a row from f_hi on exists is unknown, so
//             "a column >= T reads as 0" may not be assumed);  final: iff t < T_out and i(t) >= f_lo (rows >= T read as 0).
//             The window computes [u, u_hi), the longest such run; i(u) < f_lo means the caller dropped samples too early.
//             keep_from = H max(0, i(u_hi) - e) is the first sample the next window must still hold.
//   samples   s lies in row j = floor((s + N / 2) / H).  The window emits it when each of frames j - taps + 1 .. j lies in
//             [max(0, u - taps + 1), u_hi) or does not exist (negative; or, only if final, >= T_out), when no earlier window
//             emitted it (j >= u: implied by the first condition once u >= taps), and when s < n_out (final) or
//             s < rint((o + Lw) / rate) (not final: the smallest n_out a continuation can have, rint being monotone).
//             In closed form: rows [u, u_hi) -- every row from u on when final and u_hi >= T_out -- clipped to [0, cap).
//             One range [out_lo, out_lo + out_count), contiguous with the previous window's.  WindowPlan is the one place
//             this is written down.
//   state     acc [B, Ks] uint32: the phase at frame u_hi (columns from K on are never read or written), then tail
//             [B, taps - 1, Qp]: row q holds out_c of frame u_hi - (taps - 1) + q; rows of negative frames and columns from
//             2 K on are never read or written.  A block of ts_scan_kernel owns its 32 bins of an item over every frame, so
//             it reads its columns of the state before its first barrier and writes them behind its last one: in place.
// The launches: the STFT of rows [f_lo, f_hi) (StftLaunch::y_org, as the denoiser's windows) into c [B, f_hi - f_lo, Qp];
// the step with the global frame origin u (step = (double)(u + t) * rate: the one-shot's alpha) and the row origin f_lo; the
// scan seeded from the state's acc, which copies the tail into rows [0, n_tail) of out_c [B, n_tail + n_new, Qp], n_tail =
// min(taps - 1, u), and stores the new rows behind them; the inverse transform, which sees that as a whole utterance's c in
// coordinates that start at frame u - n_tail and stores the samples from s_org = out_lo - H (u - n_tail) on.  Counts are
// host-known (windows are dense): frames and frames_out are NULL and T, T_out hold.  With the new fields zero or NULL the
// launches are the whole-utterance ones.
#pragma once
#include <math.h>
#include <stdint.h>

#include "stft_f32.h"

namespace iris {
namespace ts {

constexpr double kMinRate = 0.25, kMaxRate = 4.0;
constexpr int kStepThreads = 256;
constexpr int kScanBins = 32, kScanRuns = 32;            // a block of ts_scan_kernel: 32 runs of 32 consecutive bins

// T_out and n_out of an item of T frames and L samples (T == 0: an empty item).  Host and device run these same lines.
__host__ __device__ inline int frames_out(int T, double rate) { return T > 0 ? (int)ceil((double)T / rate) : 0; }
__host__ __device__ inline long long samples_out(long long L, double rate) { return (long long)rint((double)L / rate); }
// T_out of a window's utterance, whose frames may pass 2^31, and i(t), the input row under output frame t
__host__ __device__ inline long long frames_out_ll(long long T, double rate) { return T > 0 ? (long long)ceil((double)T / rate) : 0; }
__host__ __device__ inline long long source_row(long long t, double rate) { return (long long)floor((double)t * rate); }

// adv_k in fixed-point turns and in fp32 turns
__host__ __device__ inline uint32_t advance_fixed(int k, int hop, int n_fft) {
    const uint64_t r = (uint64_t)(((long long)k * hop) % n_fft);
    return (uint32_t)((r << 32) / (uint64_t)n_fft);
}
__host__ __device__ inline float advance_turns(int k, int hop, int n_fft) {
    return (float)(((long long)k * hop) % n_fft) / (float)n_fft;
}

// "Windows" above in closed form, for the window [H m0, H (m0 + Mw)) and the caller's next frame u.  Host only.
struct WindowPlan {
    long long f_lo = 0, f_hi = 0;         // the input rows the window can compute (stft::Window)
    long long u_hi = 0;                   // it computes output frames [u, u_hi)
    long long out_lo = 0, out_count = 0;  // and emits these samples (out_count == 0: out_lo is where the next one goes)
    long long keep_from = 0;              // the first sample the next window must still hold
    long long n_tail = 0, n_keep = 0;     // rows of the state's tail that exist before and after: min(taps - 1, u), min(taps - 1, u_hi)
    bool dropped = false;                 // i(u) < f_lo: row i(u) is no longer in the window; nothing is planned
    WindowPlan() {}
    WindowPlan(const stft::Sizes& d, double rate, long long m0, long long Mw, bool final, long long u) {
        const stft::Window w(d, m0, Mw, final);
        const long long H = d.hop, half = d.n_fft / 2, e = stft::edge_frames(d), end = H * (m0 + Mw);
        f_lo = w.f_lo; f_hi = w.f_hi;
        dropped = source_row(u, rate) < f_lo;
        const long long T_out = final && m0 + Mw > 0 ? frames_out_ll(m0 + Mw + 1, rate) : 0;
        long long hi = T_out;
        if (!final) {                                            // the first t with i(t) >= f_hi - 1; i is monotone
            const long long row = f_hi - 1;
            hi = row > 0 ? (long long)ceil((double)row / rate) : 0;
            while (hi > 0 && source_row(hi - 1, rate) >= row) --hi;
            while (source_row(hi, rate) < row) ++hi;
        }
        u_hi = dropped || hi < u ? u : hi;
        const long long keep = source_row(u_hi, rate) - e;
        keep_from = H * (keep > 0 ? keep : 0);
        const long long cap = samples_out(end, rate);           // final: n_out; otherwise the least n_out of any continuation
        long long lo = u * H - half, up = final && u_hi >= T_out ? cap : u_hi * H - half;
        lo = lo < 0 ? 0 : (lo > cap ? cap : lo);
        up = up < lo ? lo : (up > cap ? cap : up);
        out_lo = lo; out_count = dropped ? 0 : up - lo;
        n_tail = u < d.taps() - 1 ? u : d.taps() - 1;
        n_keep = u_hi < d.taps() - 1 ? u_hi : d.taps() - 1;
    }
};

}  // namespace ts
}  // namespace iris

#ifdef __HIPCC__
namespace iris {
namespace ts {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// every product and sum below is a rounding of its own: nothing is contracted into an fma that the text does not name
#pragma clang fp contract(off)
__device__ __forceinline__ float magnitude(float re, float im) { return sqrtf(re * re + im * im); }
__device__ __forceinline__ float turns(float re, float im) { return atan2f(im, re) * 0.15915494309189535f; }
__device__ __forceinline__ float wrap(float x) { return x - rintf(x); }
__device__ __forceinline__ uint32_t fixed(float x) { return (uint32_t)(long long)llrintf(x * 4294967296.f); }
__device__ __forceinline__ float unfixed(uint32_t a) { return (float)(int32_t)a * 2.3283064365386963e-10f; }

// The epilogue of launch 1 (a stft::stft_kernel policy): the plain spectrum, and per item T_b, T_out_b and n_out_b.
struct Spectrum {
    float* c;                 // [B, T, Qp] out
    int* frames;              // [B] out: T_b
    int* frames_out;          // [B] out: T_out_b
    int* counts;              // [B] out: n_out_b
    int* counts_user;         // [B] out, or NULL: the same, for the caller's next stage
    double rate;
    int hop;                  // item() gets no launch arguments
    static constexpr const char* kName = "stft_kernel<ts::Spectrum>";
    static constexpr int kExtraFrames = 1;
    __device__ __forceinline__ void item(int b, int Tb) const {
        const int n = (int)samples_out(Tb ? (long long)hop * (Tb - 1) : 0, rate);
        frames[b] = Tb;
        frames_out[b] = ts::frames_out(Tb, rate);
        counts[b] = n;
        if (counts_user) counts_user[b] = n;
    }
    __device__ __forceinline__ void bins4(const stft::StftLaunch& a, size_t row, int bin0, const float (&re)[4], const float (&im)[4], float nyq) const {
        float* crow = c + row * a.Qp + 2 * bin0;             // 4 bins, 8 consecutive floats of c
        if (bin0 == 0) {
            float* nrow = c + row * a.Qp + a.n_fft;           // column 2 (n_fft / 2)
            nrow[0] = nyq; nrow[1] = 0.f;
        }
        *reinterpret_cast<f32x4*>(crow) = f32x4{re[0], im[0], re[1], im[1]};
        *reinterpret_cast<f32x4*>(crow + 4) = f32x4{re[2], im[2], re[3], im[3]};
    }
};

// The same spectrum for a window: the counts are the host's (StepLaunch, ScanLaunch), so nothing is stored per item.
struct WindowSpectrum : Spectrum {
    static constexpr const char* kName = "stft_kernel<ts::WindowSpectrum>";
    __device__ __forceinline__ void item(int, int) const {}
};

struct StepLaunch {
    const float* c;           // [B, T, Qp]
    const int* frames;        // [B] T_b, or NULL (a window): T
    const int* frames_out;    // [B] T_out_b, or NULL (a window): T_out
    float* mag;               // [B, T_out, Ks] out
    uint32_t* inc;            // [B, T_out, Ks] out
    double rate;
    int T, T_out, Ks, Qp, bins, hop, n_fft;
    long long t_org, f_lo;    // a window: thread t is output frame t_org + t, and row 0 of c is input row f_lo; 0 and 0 otherwise
};

// Launch 2.  A thread owns 4 consecutive bins of one output frame: 8 consecutive floats of source rows i and i + 1 (two 16-byte
// loads each), 4 magnitudes and 4 increments (one 16-byte store each).  Consecutive lanes are consecutive groups of bins.
// Columns of c from 2 K on were never written: they are loaded with their group and replaced by 0.
__global__ void __launch_bounds__(kStepThreads) ts_step_kernel(const StepLaunch a) {
    const int b = blockIdx.y, G = a.Ks >> 2;
    const int Tb = a.frames ? a.frames[b] : a.T, To = a.frames_out ? a.frames_out[b] : a.T_out;
    const long long idx = (long long)blockIdx.x * kStepThreads + threadIdx.x;
    const int t = (int)(idx / G), g = (int)(idx - (long long)t * G);
    if (t >= To) return;
    const double step = (double)(a.t_org + t) * a.rate;       // the global product: the one-shot's alpha in every window
    const double fl = floor(step);
    const int i = (int)((long long)fl - a.f_lo);
    const float alpha = (float)(step - fl);
    const int bin0 = 4 * g;
    float v0[8], v1[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
        if (i < Tb) x0 = *reinterpret_cast<const f32x4*>(a.c + ((size_t)b * a.T + i) * a.Qp + 2 * bin0 + 4 * h);
        if (i + 1 < Tb) x1 = *reinterpret_cast<const f32x4*>(a.c + ((size_t)b * a.T + i + 1) * a.Qp + 2 * bin0 + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v0[4 * h + e] = x0[e]; v1[4 * h + e] = x1[e]; }
    }
    f32x4 mv;
    u32x4 iv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = bin0 + e;
        const bool live = k < a.bins;
        const float re0 = live ? v0[2 * e] : 0.f, im0 = live ? v0[2 * e + 1] : 0.f;
        const float re1 = live ? v1[2 * e] : 0.f, im1 = live ? v1[2 * e + 1] : 0.f;
        mv[e] = fmaf(alpha, magnitude(re1, im1), (1.f - alpha) * magnitude(re0, im0));
        const float dphi = wrap(turns(re1, im1) - turns(re0, im0) - advance_turns(k, a.hop, a.n_fft));
        iv[e] = live ? advance_fixed(k, a.hop, a.n_fft) + fixed(dphi) : 0u;
    }
    const size_t o = ((size_t)b * a.T_out + t) * a.Ks + bin0;
    *reinterpret_cast<f32x4*>(a.mag + o) = mv;
    *reinterpret_cast<u32x4*>(a.inc + o) = iv;
}

inline hipError_t launch_step(const StepLaunch& a, int B, hipStream_t stream) {
    const long long work = (long long)a.T_out * (a.Ks >> 2);
    const dim3 grid((unsigned)((work + kStepThreads - 1) / kStepThreads), (unsigned)B), block(kStepThreads);
    return launch_kernel_named("ts_step_kernel", ts_step_kernel, grid, block, 0, stream, a);
}

struct ScanLaunch {
    const float* c;           // [B, T, Qp]: row 0 gives the start phase
    const float* mag;         // [B, T_out, Ks]
    const uint32_t* inc;      // [B, T_out, Ks]
    const int* frames_out;    // [B] T_out_b, or NULL (a window): T_out
    uint32_t* acc;            // [B, T_out, Ks] out
    float* out_c;             // [B, row_off + T_out, Qp] out: frame t is row row_off + t
    int T, T_out, Ks, Qp, bins;
    // a window ("Windows" above); NULL and 0 in a whole-utterance launch
    const uint32_t* acc_in;   // [B, Ks] the phase at frame 0 of this launch; NULL: row 0 of c seeds it (legal only when u == 0)
    uint32_t* acc_out;        // [B, Ks] out, or NULL: the phase behind the last frame (may be acc_in)
    const float* tail_in;     // [B, tail_rows, Qp]: its last row_off rows become rows [0, row_off) of out_c
    float* tail_out;          // [B, tail_rows, Qp] out, or NULL: the last tail_keep rows of out_c, into its last rows (may be tail_in)
    int row_off, tail_rows, tail_keep;
};

// Launch 3.  Thread (run r = threadIdx.x / kScanBins, bin k = kScanBins blockIdx.x + threadIdx.x % kScanBins) of item b: frames
// [r len, (r + 1) len) with len = ceil(T_out_b / kScanRuns).  2 Ks == Qp, so the bins of a row fill every column of out_c.
__global__ void __launch_bounds__(kScanBins * kScanRuns) ts_scan_kernel(const ScanLaunch a) {
    __shared__ uint32_t sums[kScanRuns][kScanBins];
    const int b = blockIdx.y, lane = threadIdx.x % kScanBins, r = threadIdx.x / kScanBins;
    const int k = blockIdx.x * kScanBins + lane;
    const int To = a.frames_out ? a.frames_out[b] : a.T_out, rows = a.row_off + a.T_out;
    // a window: the block's columns of the state are read here, before the first barrier, and written behind the last one
    for (int q = r; q < a.row_off; q += kScanRuns)
        if (k < a.Ks) {
            float2 v = {0.f, 0.f};
            if (k < a.bins) v = *reinterpret_cast<const float2*>(a.tail_in + ((size_t)b * a.tail_rows + a.tail_rows - a.row_off + q) * a.Qp + 2 * k);
            *reinterpret_cast<float2*>(a.out_c + ((size_t)b * rows + q) * a.Qp + 2 * k) = v;
        }
    const uint32_t seed = a.acc_in && k < a.bins ? a.acc_in[(size_t)b * a.Ks + k] : 0u;
    if (To <= 0) return;                                     // block-uniform
    const int len = (To + kScanRuns - 1) / kScanRuns;
    const int t0 = r * len < To ? r * len : To, t1 = t0 + len < To ? t0 + len : To;
    const bool live = k < a.Ks;
    const size_t base = (size_t)b * a.T_out * a.Ks + k;
    uint32_t sum = 0;
    if (live)
        for (int t = t0; t < t1; ++t) sum += a.inc[base + (size_t)t * a.Ks];
    sums[r][lane] = sum;
    __syncthreads();
    if (live) {
        uint32_t acc = seed;
        if (!a.acc_in && k < a.bins) {
            const float* c0 = a.c + (size_t)b * a.T * a.Qp + 2 * k;
            acc = fixed(turns(c0[0], c0[1]));
        }
        if (a.acc_out && r == 0 && k < a.bins) {
            uint32_t last = acc;
            for (int q = 0; q < kScanRuns; ++q) last += sums[q][lane];
            a.acc_out[(size_t)b * a.Ks + k] = last;
        }
        for (int q = 0; q < r; ++q) acc += sums[q][lane];
        for (int t = t0; t < t1; ++t) {
            const size_t o = base + (size_t)t * a.Ks;
            const float m = a.mag[o], x = 2.f * unfixed(acc);
            float s, co;
            sincospif(x, &s, &co);
            a.acc[o] = acc;
            *reinterpret_cast<float2*>(a.out_c + ((size_t)b * rows + a.row_off + t) * a.Qp + 2 * k) = float2{m * co, m * s};
            acc += a.inc[o];
        }
    }
    if (!a.tail_out) return;                                 // launch-uniform
    __syncthreads();                                         // the block's own stores to out_c, its tail rows included
    for (int q = r; q < a.tail_keep; q += kScanRuns)
        if (k < a.bins)
            *reinterpret_cast<float2*>(a.tail_out + ((size_t)b * a.tail_rows + a.tail_rows - a.tail_keep + q) * a.Qp + 2 * k) =
                *reinterpret_cast<const float2*>(a.out_c + ((size_t)b * rows + rows - a.tail_keep + q) * a.Qp + 2 * k);
}

inline hipError_t launch_scan(const ScanLaunch& a, int B, hipStream_t stream) {
    const dim3 grid((unsigned)((a.Ks + kScanBins - 1) / kScanBins), (unsigned)B), block(kScanBins * kScanRuns);
    return launch_kernel_named("ts_scan_kernel", ts_scan_kernel, grid, block, 0, stream, a);
}

}  // namespace ts
}  // namespace iris
#endif
