/* chain_oracle.c -- the fp32 fmaf chain of every output element of the fp32 path, on the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * The fp32 kernels (csrc/conv_mfma_f32.h, convt_mfma_f32.h, mrf_conv_mfma_f32.h, mrf_small_f32.h, mrf_pair_f32*.h) promise
 * that an output element is ONE chain of fused multiply-adds whatever the launch plan is:
 *     acc = 0
 *     for each chunk of `chunk` input channels (the kernel's CIC), ascending
 *       for each tap, ascending
 *         for each group of 8 channels of the chunk, ascending
 *           for the channels 0, 4, 1, 5, 2, 6, 3, 7 of the group
 *             acc = fmaf(x[row of the tap][channel], w[co][channel][tap], acc)
 *     y = (acc + bias) (+ residual)
 * and conv_post (csrc/conv_post.h):  acc = bias;  taps ascending, channels ascending;  the caller takes tanh.
 * Rows outside the tensor and channels past C_in are zeros in the kernels: fmaf(0, w, acc) == acc by value, so they are
 * skipped here (compare by value: +0 == -0).
 *
 * Every multiply-add is an explicit fmaf() (glibc's is correctly rounded with or without an FMA unit); compile with
 * -ffp-contract=off and without -march=native / -mfma (see the two forms of the hot loop below).  Threads split the output rows, never a chain; at most 16.
 *
 * Layouts (the Python binding transposes): x [B][L][C_in], w [taps][C_in][C_out padded to a multiple of 16 with zeros],
 * res / out [B][rows][C_out].
 * `variant` selects a WRONG restatement (tests/test_oracle_chain.py shows each is visible); 0 is the chain. */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <unistd.h>

enum {
    CHAIN_ASCENDING = 1,      /* channels 0 .. 7 ascending inside a group */
    CHAIN_TAP_MAJOR = 2,      /* taps outside chunks */
    CHAIN_BIAS_FIRST = 4,     /* acc starts at the bias */
    CHAIN_RES_FIRST = 8       /* (acc + res) + bias */
};

static const int kOrder[8] = {0, 4, 1, 5, 2, 6, 3, 7};

typedef struct {
    const float *x, *w, *b, *res;
    float *out;
    int B, L, Ci, Co, k, dil, pad, chunk, variant;
    int u, taps, p;                 /* transpose only (u > 0) */
    const int32_t *rows;            /* the output rows restated, per batch item */
    int n_rows;
    long long begin, end;           /* this thread's part of the B * n_rows output rows */
} Job;

/* Portable speed: the hot loop is compiled twice, for any CPU (fmaf() is glibc's) and for CPUs with an FMA unit (fmaf() is
 * the instruction -- correctly rounded as well); run_conv picks one on the host it runs on.  No build flag depends on the
 * build host.  chain_set_portable(1) forces the first form, so that a test can hold BOTH to exact arithmetic on one host. */
#if defined(__x86_64__) && defined(__GNUC__)
#define CHAIN_HAVE_FMA_FORM 1
#else
#define CHAIN_HAVE_FMA_FORM 0
#endif
static int g_portable = 0;
void chain_set_portable(int on) { g_portable = on; }
/* 1 when the next call runs fmaf() as the hardware instruction, 0 when it calls glibc's */
int chain_uses_fma_unit(void) {
#if CHAIN_HAVE_FMA_FORM
    return !g_portable && __builtin_cpu_supports("fma");
#else
    return 0;
#endif
}
#define CB 16     /* output channels whose (independent) chains advance together; w is padded to a multiple of it */

/* one (chunk, tap) of CB chains: x row `xr`, weights `wr` [Ci][Cop] at this tap and channel block, channels [c0, c1) */
static inline __attribute__((always_inline)) void chain_piece(float *restrict acc, const float *restrict xr,
                                                              const float *restrict wr, int Cop, int c0,
                                                              int c1, int ascending) {
    for (int g = c0; g < c1; g += 8)
        for (int e = 0; e < 8; ++e) {
            const int ci = g + (ascending ? e : kOrder[e]);
            if (ci < c1) {
                const float xv = xr[ci];
                const float *restrict wv = wr + (size_t)ci * Cop;
#pragma GCC unroll 16
                for (int c = 0; c < CB; ++c) acc[c] = fmaf(xv, wv[c], acc[c]);     /* CB independent chains: in registers */
            }
        }
}

static inline __attribute__((always_inline)) void conv_body(void *arg) {
    const Job *j = (const Job *)arg;
    const int asc = j->variant & CHAIN_ASCENDING;
    const int Cop = (j->Co + CB - 1) / CB * CB;
    for (long long n = j->begin; n < j->end; ++n) {
        const int b = (int)(n / j->n_rows), ri = (int)(n - (long long)b * j->n_rows);
        const int o = j->rows[ri];
        /* tap kap reads input row row0 + kap * dil and weight slice wk0 + kap * wks (transpose: one phase's taps) */
        int row0, n_taps, wk0, wks;
        if (j->u > 0) {
            const int q = o + j->p, ph = q % j->u, i = q / j->u;
            row0 = i - (j->taps - 1); n_taps = j->taps; wk0 = ph + (j->taps - 1) * j->u; wks = -j->u;
        } else {
            row0 = o - j->pad; n_taps = j->k; wk0 = 0; wks = 1;
        }
        const float *xb = j->x + (size_t)b * j->L * j->Ci;
        for (int co0 = 0; co0 < j->Co; co0 += CB) {
            float acc[CB];
            for (int c = 0; c < CB; ++c) acc[c] = ((j->variant & CHAIN_BIAS_FIRST) && co0 + c < j->Co) ? j->b[co0 + c] : 0.0f;
            if (j->variant & CHAIN_TAP_MAJOR) {
                for (int kap = 0; kap < n_taps; ++kap) {
                    const int row = row0 + kap * j->dil, kk = wk0 + kap * wks;
                    if (row < 0 || row >= j->L || kk < 0 || kk >= j->k) continue;
                    for (int c0 = 0; c0 < j->Ci; c0 += j->chunk)
                        chain_piece(acc, xb + (size_t)row * j->Ci, j->w + (size_t)kk * j->Ci * Cop + co0, Cop, c0,
                                    c0 + j->chunk < j->Ci ? c0 + j->chunk : j->Ci, asc);
                }
            } else {
                for (int c0 = 0; c0 < j->Ci; c0 += j->chunk)
                    for (int kap = 0; kap < n_taps; ++kap) {
                        const int row = row0 + kap * j->dil, kk = wk0 + kap * wks;
                        if (row < 0 || row >= j->L || kk < 0 || kk >= j->k) continue;
                        chain_piece(acc, xb + (size_t)row * j->Ci, j->w + (size_t)kk * j->Ci * Cop + co0, Cop, c0,
                                    c0 + j->chunk < j->Ci ? c0 + j->chunk : j->Ci, asc);
                    }
            }
            for (int c = 0; c < CB && co0 + c < j->Co; ++c) {
                const int co = co0 + c;
                const size_t oi = ((size_t)b * j->n_rows + ri) * j->Co + co;
                float y;
                if (j->variant & CHAIN_BIAS_FIRST)     y = j->res ? acc[c] + j->res[oi] : acc[c];
                else if (j->variant & CHAIN_RES_FIRST) y = j->res ? (acc[c] + j->res[oi]) + j->b[co] : acc[c] + j->b[co];
                else                                   y = j->res ? (acc[c] + j->b[co]) + j->res[oi] : acc[c] + j->b[co];
                j->out[oi] = y;
            }
        }
    }
}

static void *run_conv_portable(void *arg) { conv_body(arg); return NULL; }
#if CHAIN_HAVE_FMA_FORM
__attribute__((target("fma"))) static void *run_conv_fma(void *arg) { conv_body(arg); return NULL; }
#endif
static void *run_conv(void *arg) {
#if CHAIN_HAVE_FMA_FORM
    if (chain_uses_fma_unit()) return run_conv_fma(arg);
#endif
    return run_conv_portable(arg);
}

static void *run_post(void *arg) {
    const Job *j = (const Job *)arg;
    for (long long n = j->begin; n < j->end; ++n) {
        const int b = (int)(n / j->n_rows), ri = (int)(n - (long long)b * j->n_rows);
        const int o = j->rows[ri];
        const float *xb = j->x + (size_t)b * j->L * j->Ci;
        float acc = j->b[0];
        for (int kap = 0; kap < j->k; ++kap) {
            const int row = o - j->pad + kap;
            if (row < 0 || row >= j->L) continue;
            for (int ci = 0; ci < j->Ci; ++ci) acc = fmaf(xb[(size_t)row * j->Ci + ci], j->w[(size_t)kap * j->Ci + ci], acc);
        }
        j->out[(size_t)b * j->n_rows + ri] = acc;
    }
    return NULL;
}

static int n_threads(long long work) {
    long n = sysconf(_SC_NPROCESSORS_ONLN);
    if (n > 16) n = 16;
    if (n < 1) n = 1;
    if (work < n) n = work > 0 ? (long)work : 1;
    return (int)n;
}

static int run(Job *proto, void *(*fn)(void *)) {
    const long long total = (long long)proto->B * proto->n_rows;
    if (total <= 0) return 0;
    const int nt = n_threads(total);
    pthread_t tid[16];
    Job jobs[16];
    int started = 0, rc = 0;
    for (int t = 0; t < nt; ++t) {
        jobs[t] = *proto;
        jobs[t].begin = total * t / nt;
        jobs[t].end = total * (t + 1) / nt;
        if (t == nt - 1 || pthread_create(&tid[started], NULL, fn, &jobs[t]) != 0) fn(&jobs[t]);   /* (falls back to this thread) */
        else ++started;
    }
    for (int t = 0; t < started; ++t) if (pthread_join(tid[t], NULL) != 0) rc = 1;
    return rc;
}

static int bad_rows(const int32_t *rows, int n_rows, int limit) {
    for (int i = 0; i < n_rows; ++i) if (rows[i] < 0 || rows[i] >= limit) return 1;
    return 0;
}

/* Conv1d, 'same' zero padding dil * (k - 1) / 2.  x [B][L][Ci] is the ACTIVATED input; res / out [B][n_rows][Co]. */
int chain_conv1d(const float *x, const float *w, const float *b, const float *res, float *out, int B, int L, int Ci, int Co,
                 int k, int dil, int chunk, const int32_t *rows, int n_rows, int variant) {
    if (chunk < 8 || (chunk & 7) || k < 1 || dil < 1 || bad_rows(rows, n_rows, L)) return 2;
    Job j = {x, w, b, res, out, B, L, Ci, Co, k, dil, dil * (k - 1) / 2, chunk, variant, 0, 0, 0, rows, n_rows, 0, 0};
    return run(&j, run_conv);
}

/* ConvTranspose1d(k, stride u, padding (k - u) / 2) as u phases of ceil(k / u) taps: output row o, q = o + p, phase q % u,
 * row index i = q / u, tap kap reads x[i - (taps - 1) + kap] and w[:, :, phase + (taps - 1 - kap) * u].  w [k][Ci][Co padded]. */
int chain_conv_transpose1d(const float *x, const float *w, const float *b, float *out, int B, int L, int Ci, int Co, int k, int u,
                           int chunk, const int32_t *rows, int n_rows, int variant) {
    if (chunk < 8 || (chunk & 7) || k < 1 || u < 1 || k < u || bad_rows(rows, n_rows, L * u)) return 2;
    Job j = {x, w, b, NULL, out, B, L, Ci, Co, k, 1, 0, chunk, variant, u, (k + u - 1) / u, (k - u) / 2, rows, n_rows, 0, 0};
    return run(&j, run_conv);
}

/* out[i] = fmaf(a[i], b[i], c[i]): one correctly rounded multiply-add per element, for the restatement of an epilogue whose
 * source leaves a * b + c open to contraction (oracle/dsp_chain_cases.py tries the fused and the plain form). */
void chain_fmaf(const float *a, const float *b, const float *c, float *out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = fmaf(a[i], b[i], c[i]);
}

/* conv_post before tanh: bias first, taps ascending, channels ascending.  w [k][Ci]; out [B][n_rows]. */
int chain_conv_post_preact(const float *x, const float *w, const float *b, float *out, int B, int L, int Ci, int k,
                           const int32_t *rows, int n_rows) {
    if (k < 1 || bad_rows(rows, n_rows, L)) return 2;
    Job j = {x, w, b, NULL, out, B, L, Ci, 1, k, 1, (k - 1) / 2, 8, 0, 0, 0, 0, rows, n_rows, 0, 0};
    return run(&j, run_post);
}
