// limiter.h -- a look-ahead true-peak limiter per item of a ragged batch of waveforms, on the device (iris_limiter_*): the stage
// behind the loudness stage that holds a ceiling without turning the whole sentence down.  It has no recursion: a short
// interpolation FIR, a sliding minimum and a smoothing FIR, each with one stated order of operations, so the contract is the
// rules below and their numpy restatement with the same operations (tests/limiter_restatement.py: device_f32), bit for bit.
// Item b of wav [B, L] fp32 owns L_b = min(L, lengths[b] * row_scale) samples (ragged_rows); mono.  Samples behind L_b are never
// read and may hold NaN; x[n] = 0 outside [0, L_b); the item's own samples are taken to be finite.  The host never reads a length.
//
// Config: ceiling c, an amplitude in (0, 1], and lookahead A in samples, 1 .. 256.  Every operation is fp32 with NOTHING
// contracted except the fmaf named below, and the one division is done in fp64.
//
//   points       bank[q][j], q = 1, 2, 3, j = 0 .. 11: the Kaiser-windowed sinc of resample.h for up = 4, s = 1, Hw = 6 with that
//              file's default beta and rolloff (its own plan() and fill_bank() for 1000 -> 4000 Hz with 6 zeros; row 0, the
//              samples themselves, is not kept), computed on the host in double and rounded to fp32.
//              u[n, q] = the chain over j = 0 .. 11 ascending of acc = fmaf(x[n - 5 + j], bank[q][j], acc), acc = 0.0f: the point
//              q / 4 of the way from sample n to n + 1.
//   envelope     p[n] = max(|x[n]|, |u[n-1, 1..3]|, |u[n, 1..3]|) (a maximum is exact: any order);  tp_b = max p[n] over n < L_b,
//              0 for an empty item.
//   gain         r[n] = p[n] > c ? (float)((double)c / (double)p[n]) : 1.0f for n in [0, L_b), and 1.0f outside.
//   hold         m[n] = min r[n + k] over |k| <= A (a minimum is exact: any algorithm gives these bits).
//   smoothing    d[n] = 1.0f - m[n];  s[n] = the chain over j = -A .. A ascending of acc = fmaf(d[n + j], w[j], acc), acc = 0.0f;
//              w[j] = 0.5 (1 + cos(pi j / (A + 1))) divided by the sum of these 2A + 1 values (summed j ascending), all in double,
//              rounded to fp32 UPWARD (the least fp32 not under the double);  g[n] = 1.0f - s[n].  Where nothing within 2A
//              samples exceeds c, every d in the chain is +0 and g[n] is exactly 1.  Every m[n + j] of the chain covers sample n,
//              so in exact arithmetic with this table g[n] <= 1 - (1 - r[n]) sum(w) <= r[n]: that needs sum(w) >= 1, which
//              rounding to nearest does not give (the nearest table sums to 1 - 3.8e-9 at A = 33, and the gain at an isolated
//              peak then passes r by that share of 1 - r) and rounding upward does (1 + 3.7e-8 at A = 33; exactly 1 at A = 1).
//   output       out[b, n] = fminf(fmaxf(x[n] * g[n], -c), c) for n < L_b and 0.0f behind: the clamp only absorbs the rounding of
//              the smoothing and makes |out| <= c unconditional.  Every element of out [B, L] is stored exactly once, by one
//              thread, without atomics: two runs give the same bits.
//   stats        stats[b] = (tp_b, min g[n] over n < L_b) in fp32; an empty item gives (0, 1).
//   Everything above depends on the item's own sample indices alone, not on B, addresses or the item's neighbours.
//
// Two launches.  tile: grid (ceil(L / kTile), B), 256 threads; a block owns kTile = 2048 output samples of one item.  g on the
// tile needs m within A of it, r within 2A, u within 2A + 1 and x within 2A + 7: the block stages x with a halo of 2A + 7 per side
// in LDS (4-byte loads, bounded by L_b) and runs every step out of LDS:
//     v[k] = max_q |u[k, q]| over the tile and 2A + 1 (left) / 2A (right) around it, then r over the tile and 2A per side;
//     the minimum by log-step doubling between two buffers, M_0 = r, M_(k+1)[i] = min(M_k[i], M_k[i + 2^k]), K = floor(log2(2A
//     + 1)) passes, then m = min(M_K[i], M_K[i + 2A + 1 - 2^K]): K + 1 <= 10 pairs of reads per sample, whatever A is;
//     d is stored with one word of padding after every 8 (index i + i / 8), so that lane l, which owns outputs 8 l .. 8 l + 7
//     and reads at a stride of 9 words, meets no bank twice; it holds 8 values of d in registers, and a step of the chain is 8
//     fmaf for one LDS read of d and one broadcast read of w;
//     g goes back into LDS and the tile is stored lane-contiguously, 16 bytes at a time where the tile's first output address
//     lies on 16 bytes (whole groups inside the row), by scalars otherwise.
// A tile in which r = 1 everywhere within 2A (the block votes) has d = +0 and g = 1.0f exactly, so it skips the minimum and the
// smoothing: an utterance under the ceiling costs a staged copy.  A tile that starts behind L_b stores its zeros and returns.
// The block writes (max p, min g) over its own samples to the workspace, parts [B][tiles][2] fp32; tiles behind L_b write nothing.
// stats: one wave per item takes the maximum and the minimum over the item's own ceil(L_b / kTile) tiles.
//
// The tile and the block.  The LDS of a block is x (kTile + 4A + 14 words), two buffers of max(kTile + 4A + 1, 9 (kTile + 2A) /
// 8 + 1) words -- v, then the doubling's two sides, then the padded d and g -- and w: 39 KB at A = 256, 28 KB at A = 33.  The CU
// has 160 KB, so 4 to 5 blocks of 256 threads (16 to 20 of its 32 waves) are resident at any A, which is what hides the
// barriers between the passes; a tile of 4096 would halve the halo's share (25 % of the work at A = 256, 3 % at A = 33) but
// leave 2 blocks per CU at A = 256, and 1024 doubles the halo's share for nothing: the LDS is not the limit at 2048.  256
// threads x 8 consecutive outputs is exactly one tile, which the register window of the smoothing needs.
//
// Windows (iris_limiter_*_window*): the same two launches on a piece of an utterance, for a caller that receives it piece by piece.
// A window is wav [B, Lw], the samples [origin, origin + Lw) of B utterances of one length; it starts its utterance when origin
// == 0 and ends it when `final` is set.  By the rules above out[n] reads x[n - R .. n + R] and nothing else, R = halo(A) = 2A + 7
// (g reads m within A, m reads r within A, r reads u[n - 1] and u[n], u reads x[n - 5 .. n + 6]; R is the tile's halo, which has
// one sample to spare on either side).  A sample is *settled* by a window when all of that lies inside the window or outside
// the utterance, where the one-shot call also uses x = 0 and r = 1.  That is the finality rule, and struct Window below is the
// one place it is written down:
//     out_lo = origin + (origin > 0 ? R : 0);  out_hi = origin + Lw - (final ? 0 : R);  count = max(0, out_hi - out_lo)
// so the last R samples of a window that is not final are held back for the next one, which must begin at or before
// (first sample not yet settled) - R.
// One kernel body serves both.  A launch names the input row (in_len readable samples, in_stride apart), the row's sample that
// is output 0 (`offset`: 0 for a whole item, out_lo - origin for a window) and the outputs (n_out per row, out_stride apart:
// a window's rows are packed, [B, count]).  Tile i owns outputs [i kTile, (i + 1) kTile) of the n_out, so a window's tiles cover
// settled samples only, and a tile stages its halo from the window's own context instead of recomputing a tile that would be
// thrown away.  forward_ragged / measure_ragged are the case offset = 0, in_len = in_stride = n_out = out_stride = L with
// `lengths` as before: every index and every operation is then what it was, and so is every bit.
// Two kinds of edge meet the staging (`lo`, `hi`: the slots that are samples of the row).  Beyond an end of the utterance --
// slots in front of sample 0 of a window with origin == 0, slots behind L_b, or behind the last sample of a final window --
// x = 0 and r = 1, as the rules say.  Beyond an end of a window that is not an end of the utterance lie real samples that the
// kernel does not have; it stages 0 and r = 1 there too, and that is harmless only because of the finality rule: no settled
// output reads such a slot, nor any r, m or d computed from one.  The tile's (max p, min g) are taken over its settled outputs
// alone (`own`), never over the held-back samples that share the tile.
// The tile seams of a window fall on other samples than those of the one-shot call.  The bits do not move: every rule is per
// sample, a maximum and a minimum are exact, and every chain (u, s) has its one stated order whatever tile it is computed in.
// The shortcut "no r < 1 within 2A of the tile -> g = 1.0f" holds too: where it does not fire in one tiling and fires in the
// other, the chain it skips is fmaf(+0, w, +0) throughout and 1.0f - 0 = 1.0f.
// The store is 16 bytes at a time where the OUTPUT ROW's own address at the tile's first output lies on 16 bytes -- out_lo is in
// general no multiple of 4 and packed rows of `count` samples start anywhere -- and scalars otherwise.  tile_kernel<true> is the
// same body with a 16-bit store: pcm::pcm16_of(out) of pcm_out.h, (int16) rintf(clamp(out, -1, 1) * 32767), 8 bytes at a time on
// the same condition at 8 bytes.  |out| <= c <= 1, so that clamp never acts, and the result is the output stage's on the fp32
// samples, bit for bit.  Window statistics are stats [B, 2] = (max p, min g) over the window's settled samples: the reduction
// runs over the window's own ceil(count / kTile) tiles.  A window that settles nothing launches nothing.
// Nothing about the speed of a window has been measured on a GPU.
//
// Groups of windows (iris_limiter_forward_windows): the rows of one call are windows of DIFFERENT utterances, each with its own
// origin, length and `final`.  The same body again, tile_kernel<PCM, true>: what the launch names once for every row above --
// `offset`, n_out, in_len, and the row's tile count -- it names per row, in TileItem item[kGroupMax] that travels by value in the
// kernel argument behind the TileLaunch and is indexed by blockIdx.y (uniform: scalar loads from the kernarg segment, no
// descriptor buffer, no copy, capture-safe; 64 items are 1 KB of the 4 KB a kernel argument may have, hence the cap).  The host
// fills an item from limiter::Window and nothing else.  Rows are in_stride / out_stride apart, grid.x is the largest tile count
// of the group, and parts are [B][grid.x][2].  A block at or past its row's own tile count stores zeros and returns, writing no
// partials; every block stores zeros behind its row's n_out within its tile, and the blocks of the LAST column go on to
// out_stride, so every slot of out [B, out_stride] is stored exactly once.  Whether a store is 16 bytes or scalars is decided
// from the row's own address, as it always was.  The stats reduction runs over each row's own tiles; a row that settles nothing
// gets (0, 1).  Registers, LDS and the private segment of the group forms: DESIGN.md, "Concurrent streams".
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "device_info.h"
#include "pcm_out.h"
#include "resample.h"

namespace iris {
namespace limiter {

constexpr int kTile = 2048, kThreads = 256, kPerLane = 8;
constexpr int kMaxLookahead = 256;
constexpr int kBankPhases = 3, kBankTaps = 12, kBank = kBankPhases * kBankTaps;      // the design table: bank, then 2A + 1 weights
static_assert(kTile == kThreads * kPerLane, "a lane owns kPerLane consecutive outputs of the tile");

typedef float mf32x4 __attribute__((ext_vector_type(4)));

inline int design_floats(int A) { return kBank + 2 * A + 1; }

// out [kBank + 2A + 1]: bank[1..3][0..11], then w[-A .. A].  false: resample.h no longer admits 4 : 1 with 6 zeros.
inline bool fill_design(int A, float* out) {
    resample::Design d;
    if (resample::plan(1000, 4000, 6, 0.0, 0.0, &d) != 0 || d.up != 4 || d.down != 1 || d.taps != kBankTaps) return false;
    float bank[4 * kBankTaps];
    resample::fill_bank(d, bank);
    for (int i = 0; i < kBank; ++i) out[i] = bank[kBankTaps + i];
    const double pi = 3.14159265358979323846;
    double sum = 0.0;
    for (int j = -A; j <= A; ++j) sum += 0.5 * (1.0 + cos(pi * (double)j / (double)(A + 1)));
    for (int j = -A; j <= A; ++j) {
        const double v = 0.5 * (1.0 + cos(pi * (double)j / (double)(A + 1))) / sum;
        float f = (float)v;
        if ((double)f < v) f = nextafterf(f, INFINITY);             // rounded UP: the table's sum is never under 1
        out[kBank + j + A] = f;
    }
    return true;
}

__host__ __device__ inline int halo(int A) { return 2 * A + 7; }
__host__ __device__ inline int x_floats(int A) { return (kTile + 2 * halo(A) + 3) & ~3; }
__host__ __device__ inline int pad8(int i) { return i + (i >> 3); }
// one of the two work buffers: v [kTile + 4A + 1], or the padded d [pad8(kTile + 2A) + 1] (the window's last, unused read)
__host__ __device__ inline int buf_floats(int A) {
    const int a = kTile + 4 * A + 1, b = pad8(kTile + 2 * A) + 1;
    return ((a > b ? a : b) + 3) & ~3;
}
__host__ __device__ inline int w_floats(int A) { return (2 * A + 1 + 3) & ~3; }
inline size_t lds_bytes(int A) { return (size_t)(x_floats(A) + 2 * buf_floats(A) + w_floats(A)) * sizeof(float); }

// The samples of an utterance that a window [origin, origin + Lw) settles: the finality rule, written down here once.
struct Window {
    long long out_lo, out_count;    // an index into the utterance; a count that may be 0
    int offset;                     // out_lo - origin: where the first settled sample lies in the window's row
    Window(int A, long long origin, int Lw, bool final) {
        const long long R = halo(A);
        out_lo = origin + (origin > 0 ? R : 0);
        const long long out_hi = origin + Lw - (final ? 0 : R);
        out_count = out_hi > out_lo ? out_hi - out_lo : 0;
        offset = (int)(out_lo - origin);
    }
};

constexpr int kGroupMax = 64;    // IRIS_WINDOW_GROUP_MAX: the items of a group call, by value in the kernel argument

// What a group call names per row where a TileLaunch names it once.
struct TileItem {
    int offset, n_out, in_len;  // as in TileLaunch, of this row
    int tiles;                  // ceil(n_out / kTile): the blocks of the row that compute
};

struct TileLaunch {
    const float* wav;           // [B] rows of in_stride fp32, of which [0, in_len) may be read
    const int32_t* lengths;     // ragged: rows of each item [B] (device), or nullptr
    int row_scale;
    const float* table;         // [kBank + 2A + 1]: the design table
    void* out;                  // [B] rows of out_stride fp32 (or int16: tile_kernel<true>), or nullptr: measure only
    float* parts;               // [B][tiles][2]: max p, min g of the tile's own samples
    int in_len, in_stride;      // a whole item: L, L;  a window: Lw, Lw
    int offset;                 // the row's sample that is output 0: 0, or Window::offset
    int n_out, out_stride;      // outputs of a row and the row's stride: L, L, or the window's count twice (rows are packed)
    int tiles, A;               // tiles = ceil(n_out / kTile); a group: the largest of its rows', the stride of parts
    float ceiling;
};

struct TileGroupLaunch {
    TileLaunch a;               // in_stride, out_stride, tiles and what the rows share; in_len, offset and n_out are the items'
    TileItem item[kGroupMax];
};
template <bool GROUP> struct TileArg { typedef TileLaunch type; };
template <> struct TileArg<true> { typedef TileGroupLaunch type; };

// The largest (MAX) or smallest value the block's threads bring; every thread gets it.  red: 4 words of LDS.
template <bool MAX>
__device__ __forceinline__ float block_extreme(float v, float* red) {
    for (int o = 32; o >= 1; o >>= 1) {
        const float t = __shfl_xor(v, o, 64);
        v = MAX ? fmaxf(v, t) : fminf(v, t);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    __syncthreads();
    return r;
}

typedef short mi16x4 __attribute__((ext_vector_type(4)));

// Four consecutive outputs, of which the first n (1 .. 4) exist: one store of 16 bytes (8 as PCM) where `vec` says that the
// row's own address allows it and all four exist, scalars otherwise.
template <bool PCM>
__device__ __forceinline__ void store4(void* row, int q, const mf32x4& y, int n, bool vec) {
    if constexpr (PCM) {
        int16_t* o = static_cast<int16_t*>(row) + q;
        if (vec && n >= 4) {
            *reinterpret_cast<mi16x4*>(o) = mi16x4{pcm::pcm16_of(y[0]), pcm::pcm16_of(y[1]), pcm::pcm16_of(y[2]), pcm::pcm16_of(y[3])};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) o[e] = pcm::pcm16_of(y[e]);
        }
    } else {
        float* o = static_cast<float*>(row) + q;
        if (vec && n >= 4) {
            *reinterpret_cast<mf32x4*>(o) = y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) o[e] = y[e];
        }
    }
}

template <bool GROUP> __device__ __forceinline__ const TileLaunch& shared_of(const typename TileArg<GROUP>::type& arg) {
    if constexpr (GROUP) return arg.a;
    else                 return arg;
}

template <bool PCM, bool GROUP>
__global__ void __launch_bounds__(kThreads) tile_kernel(const typename TileArg<GROUP>::type arg) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float red[4];
    const TileLaunch& a = shared_of<GROUP>(arg);
    const int b = blockIdx.y, tid = threadIdx.x, A = a.A, H = halo(A);
    int offset = a.offset, n_out = a.n_out, in_len = a.in_len, tiles = a.tiles;
    if constexpr (GROUP) { const TileItem it = arg.item[b]; offset = it.offset; n_out = it.n_out; in_len = it.in_len; tiles = it.tiles; }
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, in_len);      // the row's samples [0, Lb) are the ones that exist here
    const long long t0 = (long long)blockIdx.x * kTile;                // the tile's first output
    const long long s0 = t0 + offset;                                  // ... and the row's sample it is
    const int in_row = n_out - t0 < kTile ? (int)(n_out - t0) : kTile;            // outputs of this tile that exist (>= 1; a group: maybe none)
    // the slots of the output row this block stores: its tile's outputs, and in a group also the zeros behind the row's own
    // outputs -- within the tile, and from the last column on to the end of the row
    int slots = in_row;
    if constexpr (GROUP) slots = (blockIdx.x + 1 == gridDim.x || a.out_stride - t0 < kTile) ? (int)(a.out_stride - t0) : kTile;
    constexpr size_t kOutBytes = PCM ? sizeof(int16_t) : sizeof(float);
    char* orow = a.out ? static_cast<char*>(a.out) + ((size_t)b * a.out_stride + t0) * kOutBytes : nullptr;
    const bool vec = orow && ((uintptr_t)orow & (4 * kOutBytes - 1)) == 0;        // the output row's own address

    if (s0 >= Lb || (GROUP && (int)blockIdx.x >= tiles)) {          // behind the item, or the row's own tiles: zeros, no partials
        if (!orow) return;
        for (int q = 4 * tid; q < slots; q += 4 * kThreads) store4<PCM>(orow, q, mf32x4{0.f, 0.f, 0.f, 0.f}, slots - q, vec);
        return;
    }
    const int own = Lb - s0 < in_row ? (int)(Lb - s0) : in_row;     // the tile's outputs that are the item's own samples (>= 1)

    float* xs = lds;                                                // slot i: the row's sample s0 - H + i
    float* P = xs + x_floats(A);
    float* Q = P + buf_floats(A);
    float* wl = Q + buf_floats(A);
    const int nx = kTile + 2 * H;
    const int lo = s0 >= H ? 0 : (int)(H - s0);                     // slots [lo, hi) are samples of the row that exist: the rest
    const int hi = Lb - s0 + H < nx ? (int)(Lb - s0 + H) : nx;      // is 0 and r = 1, as beyond an end of the utterance
    {
        const float* __restrict__ x = a.wav + (size_t)b * a.in_stride;
        for (int i = tid; i < nx; i += kThreads) xs[i] = (i >= lo && i < hi) ? x[s0 - H + i] : 0.f;
        for (int j = tid; j <= 2 * A; j += kThreads) wl[j] = a.table[kBank + j];
    }
    __syncthreads();

    // v[k] = max_q |u[s0 - 2A - 1 + k, q]|, k <= kTile + 4A: the chain reads slots k + 1 .. k + 12
    {
        float c1[kBankTaps], c2[kBankTaps], c3[kBankTaps];
#pragma unroll
        for (int j = 0; j < kBankTaps; ++j) { c1[j] = a.table[j]; c2[j] = a.table[kBankTaps + j]; c3[j] = a.table[2 * kBankTaps + j]; }
        for (int k = tid; k <= kTile + 4 * A; k += kThreads) {
            float u1 = 0.f, u2 = 0.f, u3 = 0.f;
#pragma unroll
            for (int j = 0; j < kBankTaps; ++j) {
                const float xv = xs[k + 1 + j];
                u1 = __builtin_fmaf(xv, c1[j], u1);
                u2 = __builtin_fmaf(xv, c2[j], u2);
                u3 = __builtin_fmaf(xv, c3[j], u3);
            }
            Q[k] = fmaxf(fmaxf(fabsf(u1), fabsf(u2)), fabsf(u3));
        }
    }
    __syncthreads();

    // r[k] for sample s0 - 2A + k, k < kTile + 4A: its x is slot k + 7, its two v are k and k + 1
    const float c = a.ceiling;
    const int nr = kTile + 4 * A;
    float pmax = 0.f;
    int over = 0;
    for (int k = tid; k < nr; k += kThreads) {
        float r = 1.0f;
        if (k + 7 >= lo && k + 7 < hi) {
            const float p = fmaxf(fabsf(xs[k + 7]), fmaxf(Q[k], Q[k + 1]));
            if (p > c) { r = (float)((double)c / (double)p); over = 1; }
            if (k >= 2 * A && k < 2 * A + own) pmax = fmaxf(pmax, p);            // the tile's own outputs
        }
        P[k] = r;
    }
    over = __syncthreads_or(over);
    pmax = block_extreme<true>(pmax, red);

    float* G = nullptr;                                             // g of the tile's outputs, where it is not 1 throughout
    if (over) {
        const int W = 2 * A + 1;
        float* cur = P;
        float* oth = Q;
        int step = 1;
        for (; 2 * step <= W; step *= 2) {                          // cur = M_k, step = 2^k
            for (int i = tid; i < nr; i += kThreads) oth[i] = i + step < nr ? fminf(cur[i], cur[i + step]) : cur[i];
            __syncthreads();
            float* t = cur; cur = oth; oth = t;
        }
        // d for sample s0 - A + i, i < kTile + 2A: the minimum of r over slots i .. i + 2A
        for (int i = tid; i < kTile + 2 * A; i += kThreads) oth[pad8(i)] = 1.0f - fminf(cur[i], cur[i + W - step]);
        __syncthreads();
        // s for the outputs 8 tid .. 8 tid + 7: the chain over d slots o .. o + 2A, a window of 8 in registers
        const float* __restrict__ D = oth;
        const int o0 = kPerLane * tid;
        float win[kPerLane], acc[kPerLane];
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) { win[i] = D[pad8(o0 + i)]; acc[i] = 0.f; }
        int j = 0;
        for (; j + kPerLane <= W; j += kPerLane) {
#pragma unroll
            for (int u = 0; u < kPerLane; ++u) {                    // win[(u + i) % 8] holds d slot o0 + i + j + u
                const float wj = wl[j + u];
#pragma unroll
                for (int i = 0; i < kPerLane; ++i) acc[i] = __builtin_fmaf(win[(u + i) & (kPerLane - 1)], wj, acc[i]);
                win[u] = D[pad8(o0 + j + u + kPerLane)];
            }
        }
        for (; j < W; ++j) {                                        // at most 7 steps: the window moves by copies
            const float wj = wl[j];
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) acc[i] = __builtin_fmaf(win[i], wj, acc[i]);
#pragma unroll
            for (int i = 0; i + 1 < kPerLane; ++i) win[i] = win[i + 1];
            win[kPerLane - 1] = D[pad8(o0 + j + kPerLane)];         // the last one is the buffer's spare word, unused
        }
        G = cur;                                                    // M_K is read; every thread is behind the barrier above
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) G[o0 + i] = 1.0f - acc[i];
        __syncthreads();
    }

    float gmin = 1.0f;
    for (int q = 4 * tid; q < slots; q += 4 * kThreads) {
        mf32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = 0.f;
            if (q + e < own) {
                const float g = G ? G[q + e] : 1.0f;
                gmin = fminf(gmin, g);
                y[e] = fminf(fmaxf(xs[q + e + H] * g, -c), c);
            }
        }
        if (orow) store4<PCM>(orow, q, y, slots - q, vec);
    }
    gmin = block_extreme<false>(gmin, red);
    if (tid == 0) {
        float* part = a.parts + ((size_t)b * a.tiles + blockIdx.x) * 2;
        part[0] = pmax;
        part[1] = gmin;
    }
}

// items: nullptr, or the B <= kGroupMax rows of a group, whose in_len, offset and n_out replace a's.
inline hipError_t launch_tile(const TileLaunch& a, const TileItem* items, int B, bool pcm16, hipStream_t stream) {
    const dim3 grid((unsigned)a.tiles, (unsigned)B), block(kThreads);
    if (items) {
        if (B > kGroupMax) return hipErrorInvalidValue;
        TileGroupLaunch g; memset(&g, 0, sizeof(g));
        g.a = a;
        for (int b = 0; b < B; ++b) g.item[b] = items[b];
        if (pcm16) return ::iris::launch_kernel_named("tile_kernel", tile_kernel<true, true>, grid, block, lds_bytes(a.A), stream, g);
        return ::iris::launch_kernel_named("tile_kernel", tile_kernel<false, true>, grid, block, lds_bytes(a.A), stream, g);
    }
    if (pcm16) return ::iris::launch_kernel_named("tile_kernel", tile_kernel<true, false>, grid, block, lds_bytes(a.A), stream, a);
    return ::iris::launch_kernel_named("tile_kernel", tile_kernel<false, false>, grid, block, lds_bytes(a.A), stream, a);
}

struct StatsLaunch {
    const int32_t* lengths;
    int row_scale;
    const float* parts;         // [B][tiles][2]
    float* stats;               // [B][2]: tp_b, min g
    int in_len, offset, n_out;  // as in TileLaunch
    int tiles;
};

struct StatsGroupLaunch {
    StatsLaunch a;              // parts, stats and the stride `tiles`; in_len, offset and n_out are the items'
    TileItem item[kGroupMax];
};
template <bool GROUP> struct StatsArg { typedef StatsLaunch type; };
template <> struct StatsArg<true> { typedef StatsGroupLaunch type; };

template <bool GROUP>
__global__ void __launch_bounds__(64) stats_kernel(const typename StatsArg<GROUP>::type arg) {
    const StatsLaunch& a = [&]() -> const StatsLaunch& { if constexpr (GROUP) return arg.a; else return arg; }();
    const int b = blockIdx.x, tid = threadIdx.x;
    int offset = a.offset, n_out = a.n_out, in_len = a.in_len;
    if constexpr (GROUP) { const TileItem it = arg.item[b]; offset = it.offset; n_out = it.n_out; in_len = it.in_len; }
    const int Lb = ragged_rows(a.lengths, b, a.row_scale, in_len);
    const int n = Lb - offset < n_out ? (Lb > offset ? Lb - offset : 0) : n_out;    // the row's outputs that are its own samples
    const int own = (int)(((long long)n + kTile - 1) / kTile);      // the tiles that hold one
    const float* __restrict__ parts = a.parts + (size_t)b * a.tiles * 2;
    float tp = 0.f, g = 1.0f;
    for (int t = tid; t < own; t += 64) { tp = fmaxf(tp, parts[2 * t]); g = fminf(g, parts[2 * t + 1]); }
    for (int o = 32; o >= 1; o >>= 1) { tp = fmaxf(tp, __shfl_xor(tp, o, 64)); g = fminf(g, __shfl_xor(g, o, 64)); }
    if (tid == 0) { a.stats[2 * b] = tp; a.stats[2 * b + 1] = g; }
}

inline hipError_t launch_stats(const StatsLaunch& a, const TileItem* items, int B, hipStream_t stream) {
    if (items) {
        if (B > kGroupMax) return hipErrorInvalidValue;
        StatsGroupLaunch g; memset(&g, 0, sizeof(g));
        g.a = a;
        for (int b = 0; b < B; ++b) g.item[b] = items[b];
        return ::iris::launch_kernel_named("stats_kernel", stats_kernel<true>, dim3((unsigned)B), dim3(64), 0, stream, g);
    }
    return ::iris::launch_kernel_named("stats_kernel", stats_kernel<false>, dim3((unsigned)B), dim3(64), 0, stream, a);
}

}  // namespace limiter
}  // namespace iris
