"""The mel front-end (csrc/mel_frontend.h) and the Griffin-Lim vocoder (csrc/griffin_lim.h), launch by launch, each on its
OWN input.  TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

Both stages run ``mma_loop`` of csrc/gemm_tile_f32.h: taps ascending, groups of 8 channels ascending, the channels 0, 4, 1, 5,
2, 6, 3, 7 of a group -- ``chain_oracle.chain_conv1d`` with ONE chunk.  The transforms are valid convolutions with an even
number of taps, so ``chain`` below hands the oracle a k = 1 convolution over the taps laid side by side (each padded to a
multiple of 8 channels with zero samples AND zero weights: ``fmaf(0, 0, acc) == acc`` by value), which walks the same terms in
the same order.  Conv weights are built here from ``design()``'s ``dft`` / ``idft`` tables exactly as ``conv_weight_from_dft``
/ ``conv_weight_from_idft`` build them; nothing is read back from the device.  Comparisons are ``np.array_equal``: -0 == +0.

Restatements, per item (the caller loops over the batch), every one taking the launch's own input:

    ``mel_launch``     mel_kernel, all four forms: stage (0 outside [0, n_b), int16 times 1.0f / 32768), one chain of
                       taps * hop8 terms per column, |re| for bin 0, |Im column of bin 0| for bin n_fft / 2, sqrtf(re re + im im)
                       otherwise, the filterbank chain over bins8 columns, (float) log((double) max(acc, 1e-5f)); frames past
                       the item's count are 0.0f.
    ``invert_launch``  gl_invert_kernel: m = (float) exp(clip(l)) in double, x0 = max(chain(P, m), 0), nnls_iters times
                       res = chain(fb, x) - m and x = max(x - step chain(fb^T, res), 0); S = x, c0 = (S cos, S sin).
    ``istft_launch``   gl_istft_kernel: for each 256-column slice of c (columns from Q on read as 0), each tap ascending, each run
                       of 64 columns a partial chain from 0, ``acc = acc + part`` in that nesting; wss = the sum of
                       wsq[kap hop + col] over taps ascending whose frame exists; v / wss where wss > FLT_MIN; the trim; with
                       ``zero_tail`` exact zeros from Ly_b to Ly.
    ``update_launch``  gl_stft_update_kernel: the front-end's window of y bounded by Ly_b, a partial chain per tap and run of 64
                       samples added as above, Re = acc, Im = -acc of the sine column, bins 0 and n_fft / 2 real (the Nyquist
                       value from the Im column of bin 0 with its own r_prev at 2 half), ``phase_update`` as written.

What survives a forward (``gl_forward`` in csrc/iris_griffin_lim.hip): S, the last c, the last r, the last in-loop y and the
output.  r_prev is overwritten in place and c by every update.  So the same inputs run at ``n_iter`` = 0, 1 and 2, and what
one forward destroyed is taken from the forward before it (reruns are bit-equal: test_determinism_and_batch_independence, and
the chain shows it too -- the r1 judged in run 1 is the r_prev that reproduces run 2):

    run 0   invert (logmel, phase -> S, c0);  final istft (c0 -> out0)
    run 1   in-loop istft (c0 of run 0 -> y0);  update, first (y0, S -> r1, c1);  final istft (c1 -> out1)
    run 2   in-loop istft (c1 of run 1 -> y1);  update, momentum (y1, S, r1 of run 1 -> r2, c2);  final istft (c2 -> out2)

and once more for ``n_iter`` = 31 and 32 on ``small``: a late-loop state.  (The in-loop transform of run 2's FIRST pass is
overwritten by its second, so the in-loop form is judged twice per two-pass forward, not three times.)

Claims -- derived, none measured against the device:

* Bit for bit wherever the source fixes every rounding: the chains and the additions of the partial sums, fmaxf, acc - m, wss,
  the products s ph, (s ar) / den, sqrtf, the stored zeros.  fp32 division and sqrtf are IEEE-rounded under the project's
  flags (csrc/Makefile passes no fast-math option and hipcc keeps both correctly rounded by default).
* Four sites where the source leaves FMA contraction open: ``re re + im im`` (mel_kernel), ``x - step acc`` (NNLS),
  ``re - alpha pr`` and ``ar ar + ai ai`` (phase_update).  A restatement takes the rounding of each as a parameter -- 0 plain,
  1 fused on the first product, 2 fused on the second where there are two -- and the claim is that ONE assignment per kernel
  reproduces every element of every case, seed and form of a session (``Session.judge`` keeps the assignments that survive
  and fails when none is left).
* exp / log in double, rounded once: the device's libm and numpy's may differ by a double ulp.  An element is *decided* when
  numpy's float64 result lies further than 2^-40 (relative) from the nearest fp32 rounding midpoint; then both round alike.  A
  frame with an undecided element leaves the exact claim of its launch and is held to 1 fp32 ulp at the exp / log and to
  4 e32 downstream (S of the inversion; e32 as tests/griffin_lim_cases.py measures it).  At most 1 % of a case's frames may;
  tests/test_oracle_dsp_chain.py shows that the inputs here leave out none.  An exact-zero frame gives (float) log(1e-5f).
* c0 of a ``phase0="device"`` forward is S times what ``draw_phase`` stores for the same seed and stream, bit for bit.

The bias denoiser (csrc/denoiser.h, ``iris_denoiser_*``) runs the same two transforms, so its launches are judged with the same
parts and these beside them:

    ``window_acc``        the transform of stft_kernel for a dense call whose frame 0 is centred on sample y_org of its input
                          (StftLaunch::y_org); at y_org = 0 it is ``update_acc``.
    ``subtract_launch``   Subtract::bins4 / nyquist: im = -sine with Im of bin 0 as 0.f, mag = sqrtf(re re + im im),
                          g = fmaxf(fmaf(-strength, bias, mag), 0), scale = g / mag where mag > 0 and 0 otherwise,
                          c = (scale re, scale im); the Nyquist bin from the sine column of bin 0, with bias[n_fft / 2] and
                          magnitude(nyq, 0), and 0.f behind it.
    ``magnitude_launch``  Magnitude::bins4 / nyquist: the same magnitudes, stored.
    ``bias_reduce``       dn_bias_reduce_kernel: float64 sum in ascending t, float64 quotient, one rounding.
    ``dn_window``         dn::Window.  The window's inverse transform is ``window_slice``: a slice of ``istft_launch``.

Claims: ``fmaf(-strength, bias, mag)`` is written as an FMA, ``g / mag``, sqrtf and the products scale re, scale im are
IEEE-rounded, and ``re re + im im`` is the one open contraction site -- of each of the two instantiations of dn_stft_kernel on
its own (``DN_SITES``; they are judged separately).  The exact claim covers every stored element, subnormal squares included;
a device test may leave out only elements whose float64 re^2 + im^2 is below ``DN_TINY`` = 2^-125, only where the device
disagrees, at most ``DN_TINY_SHARE`` of a call's stored elements and none of a silence case
(tests/test_oracle_denoiser_chain.py bounds their share on the CPU).

The time stretch (csrc/time_stretch.h, ``iris_time_stretch_*``) is four launches, judged with these:

    ``ts_counts``         Spectrum::item: T_b = item_frames at extra = 1, T_out_b = ceil(T_b / rate) and n_out_b = rint(hop (T_b - 1)
                          / rate) of float64 quotients (half to even); T_b = 0 gives 0, 0.
    ``spectrum_launch``   Spectrum::bins4: ``window_acc`` at y_org = 0 stored as it is -- Re and Im = -sine interleaved, Im of bin 0
                          as 0.f, column n_fft the Nyquist value from the sine column of bin 0 with 0.f behind it.  Exact.
    ``step_launch``       ts_step_kernel.  alpha = (float)(t rate - floor(t rate)) with the product in double; a row i >= T_b and a
                          row i + 1 >= T_b read as 0; mag = fmaf(alpha, sqrtf(re1 re1 + im1 im1), (1 - alpha) sqrtf(re0 re0 + im0 im0))
                          with every product and sum rounded on its own (``#pragma clang fp contract(off)``): EXACT, with no
                          contraction search -- the fused forms are mutations.  Padding bins hold +0 and 0u.  inc: see below.
    ``scan_launch``       ts_scan_kernel.  acc is the exclusive scan of the launch's own inc from its own acc[0], modulo 2^32, in
                          the block's two-level form (``time_stretch_restatement.scan_fixed``): exact.  out_c on the launch's own
                          mag and acc: x = 2 (float)(int32) acc 2^-32 is exact, so the wanted value is mag (cospi x, sinpi x) in
                          float64; columns 2 K .. Qp hold the padding bins' 0 (1, 0).
    ``istft_launch``      with ``sample_count``: the ``sample_counts`` branch of gl_istft_kernel -- T_b = lengths[b] clamped to
                          [0, T] with no item_frames rule, Ly_b = sample_count clamped to [0, Ly], samples at or past Ly_b stored
                          as 0.f, wss over the frames that exist; samples past hop (T_b - 1) + n_fft / 2 have no frame: their
                          chains and wss are 0 and so are they.  Exact.

Derived bars of the time stretch (u32(v) = the distance from fp32(|v|) to the next fp32 value, 0 at v = 0; every term from the
float64 values, none from the device's; first order):

* ``TS_ATAN2_ULP`` = 4: HIP's table of math-function errors is not at hand where this was written, so atan2f is allowed the
  4 ulp that tests/test_gpu_time_stretch.py already grants it.  ``TS_SINCOSPI_ULP`` = 2: twice one ulp, the allowance
  oracle/text_chain_cases.py makes for expf and log1pf (HIP documents one ulp for those; the same is assumed of sincospif).
* turns(c) = atan2f(im, re) * fl32(1 / (2 pi)): with theta = atan2(im, re) in float64 and c32 the fp32 constant,
      e_turn(theta) = TS_ATAN2_ULP u32(theta) / (2 pi) + |theta| |c32 - 1 / (2 pi)| + u32(theta c32) / 2       [turns]
  -- the function's error, the constant's own, the product's rounding.
* inc, in units of 2^-32 turn, compared as a wrapped signed difference modulo 2^32.  Wanted: adv_fixed_k + 2^32 (tau1 - tau0 -
  adv32_k) in float64, tau = theta / (2 pi), adv32 = the fp32 quotient (float) r / (float) n_fft the header names.  Bar:
      2^32 (e_turn(theta1) + e_turn(theta0) + u32(tau1 - tau0) / 2 + u32(tau1 - tau0 - adv32) / 2) + 1 / 2
  -- two angles, the two fp32 subtractions, llrintf.  ``wrap`` adds nothing: x - rintf(x) is exact for |x| <= 2 (the result is
  a multiple of ulp(x) no larger than 1 / 2), the product by 2^32 is exact, and fixed(x) == fixed(wrap(x)) modulo 2^32, so the
  comparison is continuous across the rintf and a restatement without ``wrap`` is the SAME restatement (shown on the CPU; it is
  not a mutation).  Where both angles are exactly 0 (atan2f(0, x >= 0) = 0: digital silence, bins 0 and n_fft / 2 with Re > 0)
  nothing rounds -- 0 - 0, 0 - adv32 and 2^32 adv32 (adv32 >= 2^-9 or 0) are exact -- and the bar is 0.  That is where a one-unit
  error of advance_fixed shows; it can only at a config whose n_fft / hop is no power of two (``three_tap``): (k hop mod n_fft)
  / n_fft = (k mod taps) / taps is dyadic otherwise, at odd_hop too, and both of the header's forms of the advance are exact.
* acc[0]: wanted 2^32 tau(c[0, k]), bar 2^32 e_turn(theta) + 1 / 2, 0 where theta is 0; padding bins hold 0u.
* out_c: |got - mag trig| <= TS_SINCOSPI_ULP |mag| u32(trig) + u32(mag trig) / 2 + 2^-126 per element, trig = cospi x or sinpi x.
  For digital silence (mag == 0) that is 2^-126 against a wanted 0: 0 by value.
tests/test_oracle_time_stretch_chain.py asserts that the largest inc / acc[0] bar stays below 2^19 units -- half the smallest
nonzero difference between two bins' advances, 2^32 / n_fft with n_fft <= 4096 -- and the out_c bar below
(TS_SINCOSPI_ULP + 1) 2^-23 |mag| + 2^-126.  The exact claim on mag covers subnormal squares; a device test may leave out only
elements whose float64 re^2 + im^2 of either source row is below ``DN_TINY``, by the denoiser's rule.

``MUTATIONS`` are wrong restatements; tests/test_oracle_dsp_chain.py, tests/test_oracle_denoiser_chain.py and
tests/test_oracle_time_stretch_chain.py show that each fails against the right one.
"""
import numpy as np

from oracle import chain_oracle as co

FLT_MIN = np.float32(np.finfo(np.float32).tiny)
LOG_LO, LOG_HI = -11.513, 2.0
CLIP = np.float32(1e-5)
LOG_CLIP = np.float32(np.log(np.float64(CLIP)))
K_ROWS, K_SLICE, K_WAVES, RUN = 32, 256, 8, 64
DECIDED = 2.0 ** -40
MOMENTUM, NNLS_ITERS = 0.99, 32

# ---- cases ---------------------------------------------------------------------------------------------------------------------
# default   five 256-column slices, the last 8 wide; grid.z = 4 in the update; B 2, T 33 crosses a block
# small     win < n_fft; 9 groups = 8 + 1 in one slice; T 3 (fewer frames than taps) and T 70
# two_tap   two taps
# odd_hop   hop % 8 != 0 (Cp = 16 > H), n_mels < 8 (Mp padding), Ks = 52 != 49 bins
# wide_hop  16 column tiles: blockIdx.z = 1 in gl_istft_kernel
GL_CONFIGS = {
    "default": dict(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=80, fmin=0.0, fmax=8000.0),
    "small": dict(sample_rate=8000, n_fft=64, hop_length=16, win_length=48, n_mels=12, fmin=0.0, fmax=None),
    "two_tap": dict(sample_rate=16000, n_fft=256, hop_length=128, win_length=256, n_mels=20, fmin=0.0, fmax=None),
    "odd_hop": dict(sample_rate=8000, n_fft=96, hop_length=12, win_length=80, n_mels=6, fmin=0.0, fmax=None),
    "wide_hop": dict(sample_rate=22050, n_fft=1024, hop_length=512, win_length=1024, n_mels=12, fmin=0.0, fmax=8000.0),
}
GL_CASES = (("default", 2, 33), ("small", 1, 3), ("small", 1, 70), ("two_tap", 1, 34), ("odd_hop", 1, 3), ("odd_hop", 1, 35),
            ("wide_hop", 1, 3), ("wide_hop", 1, 34))
GL_SEEDS = (1337, 7)                              # start-phase seeds of a dense case
GL_LATE = ("small", 1, 70)                        # the case of the n_iter = 31 / 32 pair
# (config, T, lengths): the full T, 0, 1 (sanitised to 0), inside a block, on a block edge
GL_RAGGED = (("small", 70, (70, 0, 1, 33, 64)), ("odd_hop", 35, (35, 0, 1, 20, 32)))
MEL_CONFIGS = {
    "default": GL_CONFIGS["default"],
    "small": dict(sample_rate=16000, n_fft=256, hop_length=64, win_length=192, n_mels=20, fmin=50.0, fmax=None),
    "odd_hop": GL_CONFIGS["odd_hop"],
}
# (config, B, L): 33 frames (two blocks); odd_hop at 3 and 35 frames
MEL_CASES = (("default", 2, 8229), ("small", 1, 2085), ("odd_hop", 1, 31), ("odd_hop", 1, 413))
MEL_SEEDS = (0, 1)
# (config, L, n_samples): frames 33, 1, 1, 17, 32 (default) and 35, 1, 1, 17, 32 (odd_hop)
MEL_RAGGED = (("default", 8229, (8229, 0, 1, 4096, 31 * 256 + 5)), ("odd_hop", 413, (413, 0, 1, 200, 31 * 12)))

MUTATIONS = ("taps_descending", "istft_one_chain", "stft_one_chain", "mel_partial_sums", "istft_taps_outside_slices", "ascending",
             "mel_no_nyquist", "idft_nyquist_2", "window_uncentred", "frames_shifted", "wss_past_end", "trim_short",
             "alpha_momentum", "first_uses_rprev", "im_sign", "exp_f32", "log_f32", "clip_after_exp", "residual_sign",
             # the bias denoiser
             "dn_fma_unfused", "dn_scale_unguarded", "dn_divide_last", "dn_im_sign", "dn_nyquist_bias0", "dn_nyquist_im_kept",
             "dn_bias_sum_f32", "dn_bias_pairwise", "dn_interior_wide", "dn_mean_over_all_frames", "dn_frames_extra0",
             "dn_window_origin_shift",
             # the time stretch
             "ts_alpha_f32", "ts_lerp_fma_swapped", "ts_mag_fma_re", "ts_mag_fma_im", "ts_adv_no_modulo", "ts_adv_fixed_rounded",
             "ts_fixed_truncated", "ts_scan_inclusive", "ts_start_phase_0", "ts_unfixed_u32", "ts_sin_cos_swapped", "ts_row_past_end_kept",
             "ts_nyquist_im_kept", "ts_n_out_truncated", "ts_n_out_half_up", "ts_tail_dropped", "ts_istft_item_rule", "ts_sample_count_ignored")

# ---- the bias denoiser's cases (csrc/denoiser.h) ------------------------------------------------------------------------------------
# (config, B, M): M mel frames, L = hop M samples, T = M + 1 frames
# default   33 frames: two 32-frame blocks, grid.z = 4 in the forward transform, five inverse slices
# small     fewer frames than taps (M 2); three blocks (M 69)
# odd_hop   Cp = 16 > hop, Ks = 52 against 49 bins: the f32x4 bias load and the magnitude rows of Ks
# wide_hop  two taps, 16 column tiles: blockIdx.z = 1 in the inverse kernel
DN_CASES = (("default", 2, 32), ("small", 1, 2), ("small", 1, 69), ("two_tap", 1, 33), ("odd_hop", 1, 2), ("odd_hop", 1, 34),
            ("wide_hop", 1, 2), ("wide_hop", 1, 33))
# (config, M, lengths in mel frames): the full M, 0, 1, inside a block, T_b on a block edge, one past it
DN_RAGGED = (("small", 69, (69, 0, 1, 31, 32, 33)), ("odd_hop", 34, (34, 0, 1, 20, 31)))
# (config, M, m0, Mw, final), each at B = 2: a first, an interior and a last window, and the window that is the whole utterance
DN_WINDOWS = (("default", 39, 0, 20, False), ("default", 39, 5, 20, False), ("default", 39, 19, 20, True), ("default", 39, 0, 39, True),
              ("odd_hop", 34, 6, 20, False), ("odd_hop", 34, 14, 20, True), ("two_tap", 33, 4, 20, False), ("two_tap", 33, 13, 20, True))
DN_STRENGTH = 1.0                                 # with denoiser_cases.bias: both branches of the clamp live
DN_STRENGTHS = (DN_STRENGTH, 0.1, 0.0)            # 0.1 is the library's default
DN_TINY = 2.0 ** -125                             # float64 re^2 + im^2 below this: the only elements a device test may leave out
DN_TINY_SHARE = 1e-3                              # and at most this share of a case's stored elements

# ---- the time stretch's cases (csrc/time_stretch.h) ----------------------------------------------------------------------------------
# (config, B, M, rate): T = M + 1 frames, T_out = ceil(T / rate).  ts_step_kernel's 256-thread blocks hold 256 / G frames, G = Ks / 4
# (9 at small, 13 at odd_hop, 33 at two_tap, 129 at default and wide_hop) -- never a whole number, so a block straddles a frame
# boundary as soon as there is more than one; every config's last scan block has fewer than 32 live lanes (Ks % 32 is 4 or 20).
# three_tap  n_fft / hop = 3 is no power of two: the advance (k mod 3) / 3 is an inexact fp32 quotient and advance_fixed a truncation.
#            (odd_hop's n_fft is no power of two either, but its advance (k mod 8) / 8 is dyadic: both forms are exact there.)
TS_CONFIGS = {**GL_CONFIGS, "three_tap": dict(sample_rate=8000, n_fft=96, hop_length=32, win_length=80, n_mels=6, fmin=0.0, fmax=None)}
TS_SEMITONE_DOWN = 2.0 ** (-1.0 / 12.0)
TS_CASES = (
    ("default", 2, 32, 0.8),                # T_out 42: runs of 2 with empty trailing runs; n_out < hop (T_out - 1): the crop is live
    ("default", 2, 39, 1.25),               # T_out exactly 32: 32 runs of 1; n_out > hop (T_out - 1): the zero tail is live
    ("default", 1, 32, 1.0),                # T_out 33: runs of 2, the last of 1; rate 1
    ("small", 1, 1, 4.0),                   # T 2, T_out 1: one frame is an item; 31 empty runs
    ("small", 1, 69, TS_SEMITONE_DOWN),     # T_out 75: runs of 3 (several frames a run), a non-dyadic rate
    ("small", 1, 16, 0.25),                 # the slow end: T_out 68; alpha in {0, 1/4, 1/2, 3/4}
    ("small", 1, 69, 4.0),                  # the fast end: T_out 18, runs of 1 with empty trailing runs; alpha in {0, 1/2}
    ("two_tap", 1, 33, 1.25),               # two taps; T_out 28
    ("odd_hop", 1, 2, 1.0),                 # n_fft 96 is no power of two; fewer frames than taps
    ("odd_hop", 1, 34, 0.8),                # T_out 44: hop % 8 != 0, Ks 52 against 49 bins: a group that straddles `bins`
    ("odd_hop", 1, 34, 1.25),               # T_out 28
    ("three_tap", 1, 34, 0.8),              # T_out 44: an inexact advance_turns, a truncated advance_fixed
    ("three_tap", 1, 34, 1.25),             # T_out 28
    ("wide_hop", 1, 2, 4.0),                # T_out 1 at two taps
    ("wide_hop", 1, 33, TS_SEMITONE_DOWN),  # r in {0, 512}; blockIdx.z = 1 in the inverse; T_out 37
)
# (config, M, lengths in mel frames, rates): the full M, 0, 1, inside a block, T_b on a 32-frame block edge, one past it; NaN past
# each item's samples; a rate below 1 and a rate above 1
TS_RAGGED = (("small", 69, (69, 0, 1, 20, 31, 32), (0.8, 1.25)), ("odd_hop", 34, (34, 0, 1, 20, 31, 32), (0.8, 1.25)))
# (config, rate): ``ts_silence`` at the config's largest M
TS_SILENCE = (("default", 0.8), ("small", TS_SEMITONE_DOWN), ("two_tap", 1.25), ("odd_hop", 0.8), ("three_tap", 0.8), ("three_tap", 1.25),
              ("wide_hop", 1.0))
# (config, M, rate): ``ts_small_angles`` -- start phases of a few 1e-5 rad, where the bar of acc[0] is llrintf's own half unit and
# 2^32 x is no whole number: the only place a truncating ``fixed`` can show
TS_SMALL_ANGLES = ("small", 8, 1.0)
# fl(L / rate) is exactly 4.5 (L = 16, rate = fl(32 / 9)): rint's half-to-even decides n_out = 4; T_out 1
TS_HALF = ("small", 1, 1, 32.0 / 9.0)
TS_ATAN2_ULP = 4.0                                # allowed of atan2f (the module docstring says where both figures come from)
TS_SINCOSPI_ULP = 2.0                             # allowed of sincospif
TS_UNIT = 4294967296.0                            # 2^32 units are one turn
TS_INV_2PI32 = np.float32(0.15915494309189535)    # the constant of ts::turns
TS_FLOOR = 2.0 ** -126


def case_id(case) -> str:
    return f"{case[0]}-B{case[1]}-T{case[2]}"


class Design:
    """``mel::Design`` and ``gl::Design`` restated, with what the launch code derives from them."""

    def __init__(self, cfg):
        self.n_fft, self.hop, self.win, self.n_mels = cfg["n_fft"], cfg["hop_length"], cfg["win_length"], cfg["n_mels"]
        N, H = self.n_fft, self.hop
        self.taps, self.bins, self.half = N // H, N // 2 + 1, N // 2
        self.cp, self.bins8, self.mp = (H + 7) & ~7, (self.bins + 7) & ~7, (self.n_mels + 7) & ~7
        self.dft_tiles, self.hop_tiles = (self.half + 15) // 16, (H + 31) // 32
        self.ks, self.q = (self.bins + 3) & ~3, N + 2
        self.qp = (self.q + 7) & ~7
        self.first_row = self.half // H
        self.slices = [(q0, min(K_SLICE, self.qp - q0)) for q0 in range(0, self.qp, K_SLICE)]
        self.istft_grid_z = (self.hop_tiles + K_WAVES - 1) // K_WAVES
        self.update_grid_z = (self.dft_tiles + K_WAVES - 1) // K_WAVES

    def dft_col(self, bins, im):
        """The output column of ``conv_weight_from_dft`` that holds Re (im = 0) or the sine sum (im = 1) of ``bins``."""
        bins = np.asarray(bins)
        return 32 * (bins // 16) + 16 * im + bins % 16


def tables_np(cfg, centred=True, nyquist_factor=1.0):
    """``fill_dft``, ``fill_idft`` and ``fill_wsq`` in numpy's float64, for the mutations that change a table (the right
    tables are ``design()``'s)."""
    N, win = cfg["n_fft"], cfg["win_length"]
    w = np.zeros(N)
    lpad = (N - win) // 2 if centred else 0
    w[lpad:lpad + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    k, n = np.arange(N // 2 + 1)[:, None], np.arange(N)[None, :]
    j = (k * n) % N
    c, s = np.cos(2.0 * np.pi * j / N), np.where(2 * j % N == 0, 0.0, np.sin(2.0 * np.pi * j / N))
    edge = (k == 0) | (2 * k == N)
    f = np.where(edge, 1.0, 2.0) / N
    f[-1] *= nyquist_factor
    return {"dft": np.stack([w * c, w * s]).astype(np.float32),
            "idft": np.stack([w * f * c, np.where(edge, 0.0, -(w * f * s))]).astype(np.float32), "wsq": (w * w).astype(np.float32)}


def mutate_tables(tab, cfg, mut):
    if mut == "window_uncentred":
        return {**tab, **tables_np(cfg, centred=False)}
    if mut == "idft_nyquist_2":
        idft = tab["idft"].copy()
        idft[0, -1] *= np.float32(2.0)
        return {**tab, "idft": idft}
    return tab


# ---- inputs (tests/ is on sys.path in every test that comes here) -----------------------------------------------------------------
_cache: dict = {}


def gl_model(name, **kw):
    from iris.griffin_lim import GriffinLim
    return GriffinLim(**TS_CONFIGS[name], momentum=MOMENTUM, nnls_iters=NNLS_ITERS, **kw)


def gl_tables(name):
    """``design()``'s fp32 tables with ``P`` and ``step`` (host only), fetched once."""
    if ("tab", name) not in _cache:
        gl = gl_model(name)
        t = gl.design()
        t["P"], t["step"] = gl.inversion_tables()
        _cache[("tab", name)] = t
    return _cache[("tab", name)]


def gl_logmel(case):
    """``[B, n_mels, T]`` float32: ``griffin_lim_cases.logmel``'s recipe on this module's configs."""
    if ("lm", case) not in _cache:
        import griffin_lim_cases as GC
        import mel_restatement as M
        name, B, T = case
        cfg = GL_CONFIGS[name]
        _cache[("lm", case)] = np.stack([M.mel_np(GC.waveform(cfg["hop_length"] * (T - 1), cfg, seed=b), **cfg)
                                         for b in range(B)]).astype(np.float32)
    return _cache[("lm", case)]


def gl_phase(case, seed):
    """``phi0 [B, bins, T]`` float64, the draw of ``griffin_lim_cases.phase``."""
    name, B, T = case
    return 2.0 * np.pi * np.random.default_rng(seed).random((B, GL_CONFIGS[name]["n_fft"] // 2 + 1, T))


def mel_tables(name):
    if ("mtab", name) not in _cache:
        from iris.mel import MelFrontend
        dft, fb = MelFrontend(**MEL_CONFIGS[name]).design()
        _cache[("mtab", name)] = {"dft": dft, "fb": fb}
    return _cache[("mtab", name)]


def mel_audio(name, B, L, seed):
    """``[B, L]`` float32 of ``mel_cases.waveform`` (item b: seed + 10 b)."""
    import mel_cases as MC
    return np.stack([MC.waveform(L, MEL_CONFIGS[name], seed=seed + 10 * b) for b in range(B)])


def to_int16(audio):
    return np.round(np.asarray(audio, dtype=np.float64) * 32767.0).astype(np.int16)


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def chain(x, w, mut=None):
    """``x [n, C]``, ``w [C_out, C]``, C a multiple of 8 -> ``[n, C_out]``: per element ONE fmaf chain from 0 over the groups of 8
    ascending, channels 0, 4, 1, 5, 2, 6, 3, 7 inside a group."""
    n, C = x.shape
    assert w.shape[1] == C and C % 8 == 0 and x.dtype == np.float32 and w.dtype == np.float32
    if n == 0:
        return np.zeros((0, w.shape[0]), np.float32)
    y = co.chain_conv1d(x.T[None], w[:, :, None], np.zeros(w.shape[0], np.float32), 1, C, [(0, n)],
                        variant=co.ASCENDING if mut == "ascending" else 0)
    return np.ascontiguousarray(y[0].T)


def pad_cols(a, C):
    out = np.zeros(a.shape[:-1] + (C,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def dft_conv_weight(d, dft):
    """``conv_weight_from_dft``: ``[32 dft_tiles, hop, taps]``."""
    w = np.zeros((32 * d.dft_tiles, d.hop, d.taps), np.float32)
    for c in range(w.shape[0]):
        j = c & 31
        b, im = 16 * (c >> 5) + 8 * ((j >> 3) & 1) + (j & 7), j >> 4
        if b >= d.half:
            continue
        row = dft[0, d.half] if (b == 0 and im) else dft[im, b]
        w[c] = row.reshape(d.taps, d.hop).T
    return w


def idft_conv_weight(d, idft):
    """``conv_weight_from_idft``: ``[32 hop_tiles, Q, taps]``; tap kk multiplies frame j - (taps - 1 - kk)."""
    rows = np.empty((d.q, d.n_fft), np.float32)
    rows[0::2], rows[1::2] = idft[0], idft[1]
    w = np.zeros((32 * d.hop_tiles, d.q, d.taps), np.float32)
    w[:d.hop] = rows.reshape(d.q, d.taps, d.hop)[:, ::-1, :].transpose(2, 0, 1)
    return w


def tap_weights(w, C):
    """``[C_out, C_in, taps]`` -> ``[taps, C_out, C]`` with the channels padded to C by zeros."""
    return np.ascontiguousarray(pad_cols(w.transpose(2, 0, 1), C))


def stage_rows(x, n_b, d, T, mut=None, org=0):
    """``[T, taps, hop8]``: row t, tap kk, column c is sample org + t hop - n_fft / 2 + kk hop + c; 0 for c >= hop and outside
    [0, n_b).  ``org``: StftLaunch::y_org, 0 for a whole utterance."""
    t, kk, c = np.arange(T)[:, None, None], np.arange(d.taps)[None, :, None], np.arange(d.cp)[None, None, :]
    s = (t + kk + (1 if mut == "frames_shifted" else 0)) * d.hop + c - d.half + int(org)
    ok = (c < d.hop) & (s >= 0) & (s < n_b)
    x = np.asarray(x, dtype=np.float32)
    if x.size == 0:
        x = np.zeros(1, np.float32)
    return np.where(ok, x[np.clip(s, 0, x.size - 1)], np.float32(0))


def transform_acc(rows, wt, partial, mut=None):
    """The forward DFT of staged ``rows [T, taps, hop8]`` against ``wt [taps, C_out, hop8]``: ONE chain of taps * hop8 terms
    (mel_kernel), or a partial chain per tap and run of 64 samples, added in that order (gl_stft_update_kernel)."""
    T, K, Cp = rows.shape
    order = range(K - 1, -1, -1) if mut == "taps_descending" else range(K)
    if not partial:
        return chain(np.concatenate([rows[:, kk] for kk in order], axis=1), np.concatenate([wt[kk] for kk in order], axis=1), mut)
    acc = np.zeros((T, wt.shape[1]), np.float32)
    for kk in order:
        for g in range(0, Cp, RUN):
            acc = acc + chain(np.ascontiguousarray(rows[:, kk, g:g + RUN]), np.ascontiguousarray(wt[kk][:, g:g + RUN]), mut)
    return acc


def sum_sq(a, b, mode):
    """a a + b b: 0 both products rounded, 1 fmaf(a, a, fl(b b)), 2 fmaf(b, b, fl(a a))."""
    if mode == 0:
        return a * a + b * b
    return co.fmaf32(a, a, b * b) if mode == 1 else co.fmaf32(b, b, a * a)


def sub_prod(x, s, a, mode):
    """x - s a: 0 the product rounded, 1 fmaf(-s, a, x)."""
    return x - s * a if mode == 0 else co.fmaf32(-s, a, x)


def decided(v64):
    """Where the float64 value lies further than 2^-40 (relative) from the fp32 rounding midpoints around it."""
    v64 = np.asarray(v64, dtype=np.float64)
    f = v64.astype(np.float32)
    out = np.ones(v64.shape, bool)
    for side in (-np.inf, np.inf):
        mid = 0.5 * (f.astype(np.float64) + np.nextafter(f, np.float32(side)).astype(np.float64))
        out &= np.abs(v64 - mid) > DECIDED * np.abs(v64)
    return out


# ---- mel_kernel --------------------------------------------------------------------------------------------------------------------
MEL_SITES = {"mag": 3}
INVERT_SITES = {"nnls": 2}
UPDATE_SITES = {"alpha": 2, "den": 3}
DN_SITES = {"mag": 3}                             # per instantiation of dn_stft_kernel: the compiler may contract each its own way


def assignments(sites):
    out = [{}]
    for name, n in sites.items():
        out = [{**a, name: v} for a in out for v in range(n)]
    return out


def mel_samples(audio):
    """What the staging loads: fp32 as it is, int16 times ``1.0f / 32768``."""
    audio = np.asarray(audio)
    if audio.dtype == np.int16:
        return audio.astype(np.float32) * (np.float32(1.0) / np.float32(32768))
    assert audio.dtype == np.float32
    return audio


def mel_launch(audio, n_b, cap, cfg, tab, fma, mut=None):
    """One item of mel_kernel: ``audio [L]`` fp32 or int16, ``n_b`` its own samples (L of a dense call), ``cap`` its
    max_frames or None -> ``(mel [n_mels, T], frames, ok [T])``: ``ok`` marks the frames whose logarithms are all decided."""
    d = Design(cfg)
    tab = mutate_tables(tab, cfg, mut)
    L = len(audio)
    T = 1 + L // d.hop
    n_b = min(max(int(n_b), 0), L)
    Tb = 1 + n_b // d.hop
    if cap is not None:
        Tb = min(Tb, max(int(cap), 0))
    out, ok = np.zeros((d.n_mels, T), np.float32), np.ones(T, bool)
    if Tb == 0:
        return out, Tb, ok
    rows = stage_rows(mel_samples(audio), n_b, d, Tb, mut)
    acc = transform_acc(rows, tap_weights(dft_conv_weight(d, tab["dft"]), d.cp), mut == "mel_partial_sums", mut)
    b = np.arange(1, d.half)
    mag = np.zeros((Tb, d.bins8), np.float32)
    mag[:, 0] = np.abs(acc[:, d.dft_col(0, 0)])
    mag[:, d.half] = 0 if mut == "mel_no_nyquist" else np.abs(acc[:, d.dft_col(0, 1)])
    mag[:, 1:d.half] = np.sqrt(sum_sq(acc[:, d.dft_col(b, 0)], acc[:, d.dft_col(b, 1)], fma["mag"]))
    m = np.maximum(chain(mag, pad_cols(tab["fb"], d.bins8), mut), CLIP)
    lg = np.log(m) if mut == "log_f32" else np.log(m.astype(np.float64))
    out[:, :Tb] = lg.astype(np.float32).T
    ok[:Tb] = decided(lg).all(axis=1)
    return out, Tb, ok


# ---- gl_invert_kernel ------------------------------------------------------------------------------------------------------------
def item_frames(n, T):
    """``stft::item_frames`` of csrc/stft_f32.h at ``extra`` = 0 (n None: a dense call)."""
    if n is None:
        return T
    n = min(max(int(n), 0), T)
    return 0 if n < 2 else n


def invert_launch(logmel, phase, Tb, cfg, tab, nnls_iters, fma, mut=None):
    """``logmel [n_mels, T]``, ``phase [T, bins, 2]`` (the packed cos / sin the launch was given, or what ``draw_phase``
    stores) -> ``(S [Tb, bins], c0 [Tb, Q], ok [Tb], m [Tb, n_mels])``."""
    d = Design(cfg)
    lm = np.asarray(logmel, dtype=np.float32)[:, :Tb].T
    if mut == "exp_f32":
        e = np.exp(np.clip(lm, np.float32(LOG_LO), np.float32(LOG_HI)))
    elif mut == "clip_after_exp":
        e = np.clip(np.exp(lm.astype(np.float64)), LOG_LO, LOG_HI)
    else:
        e = np.exp(np.clip(lm.astype(np.float64), LOG_LO, LOG_HI))
    ok = decided(e).all(axis=1)
    m = pad_cols(e.astype(np.float32), d.mp)
    P, fb, fbt = pad_cols(tab["P"], d.mp), pad_cols(tab["fb"], d.bins8), pad_cols(np.ascontiguousarray(tab["fb"].T), d.mp)
    step, zero = np.float32(tab["step"]), np.float32(0)
    x = np.maximum(chain(m, P, mut), zero)
    for _ in range(nnls_iters):
        acc = chain(pad_cols(x, d.bins8), fb, mut)
        res = pad_cols(m[:, :d.n_mels] - acc if mut == "residual_sign" else acc - m[:, :d.n_mels], d.mp)
        x = np.maximum(sub_prod(x, step, chain(res, fbt, mut), fma["nnls"]), zero)
    c0 = np.empty((Tb, d.q), np.float32)
    ph = np.asarray(phase, dtype=np.float32)[:Tb]
    c0[:, 0::2], c0[:, 1::2] = x * ph[:, :, 0], x * ph[:, :, 1]
    return x, c0, ok, m[:, :d.n_mels]


# ---- gl_istft_kernel -------------------------------------------------------------------------------------------------------------
def istft_launch(c, Tb, T, cfg, tab, zero_tail, mut=None, sample_count=None, Ly=None):
    """``c [T, Qp]`` (or ``[.., Q]``; rows from Tb on are never read) -> ``(y [Ly], written [Ly])``: what the launch stores and
    where.  ``sample_count`` (the time stretch's IstftLaunch::sample_counts): the item owns that many samples of the ``Ly`` the
    launch stores (default hop (T - 1)) and ``Tb`` frames as they stand, one frame included."""
    d = Design(cfg)
    tab = mutate_tables(tab, cfg, mut)
    H, K = d.hop, d.taps
    if sample_count is None:
        assert Ly is None
        Ly, Lyb = H * (T - 1), (H * (Tb - 1) if Tb else 0)
    else:
        Tb = min(max(int(Tb), 0), T)
        if mut == "ts_istft_item_rule" and Tb < 2:
            Tb = 0
        Ly = H * (T - 1) if Ly is None else int(Ly)
        by_frames = H * (Tb - 1) if Tb else 0
        Lyb = min(max(int(sample_count), 0), Ly)
        if mut == "ts_sample_count_ignored":
            Lyb = min(by_frames, Ly)
        elif mut == "ts_tail_dropped":
            Lyb = min(Lyb, by_frames)
    y, written = np.zeros(Ly, np.float32), np.zeros(Ly, bool)
    if zero_tail:
        written[Lyb:] = True
    if Lyb == 0:
        return y, written
    if Tb == 0:                                                  # no frame exists: every chain and every wss is 0
        written[:Lyb] = True
        return y, written
    trim = d.half - H if mut == "trim_short" else d.half
    j = np.arange(trim // H, (trim + Lyb - 1) // H + 1)                            # padded rows that hold a surviving sample
    cz = np.zeros((Tb, d.qp), np.float32)
    cz[:, :d.q] = np.asarray(c, dtype=np.float32)[:Tb, :d.q]
    wt = tap_weights(idft_conv_weight(d, tab["idft"]), d.qp)[:, :H]               # [taps, hop, Qp]
    shift = 1 if mut == "frames_shifted" else 0

    def frames_of(kk):
        t = j - (K - 1 - kk) + shift
        ok = (t >= 0) & (t < Tb)
        return np.where(ok[:, None], cz[np.clip(t, 0, Tb - 1)], np.float32(0))

    taps = list(range(K - 1, -1, -1) if mut == "taps_descending" else range(K))
    runs = [(q0 + g, min(RUN, q0 + width - (q0 + g))) for q0, width in d.slices for g in range(0, width, RUN)]
    if mut == "istft_one_chain":
        order = [(kk, q0, width) for q0, width in d.slices for kk in taps]
        acc = chain(np.concatenate([frames_of(kk)[:, q0:q0 + n] for kk, q0, n in order], axis=1),
                    np.concatenate([wt[kk][:, q0:q0 + n] for kk, q0, n in order], axis=1), mut)
    else:
        if mut == "istft_taps_outside_slices":
            order = [(kk, q, n) for kk in taps for q, n in runs]
        else:
            order = [(kk, q, n) for q0, width in d.slices for kk in taps for q, n in runs if q0 <= q < q0 + width]
        xs = {kk: frames_of(kk) for kk in taps}
        acc = np.zeros((len(j), H), np.float32)
        for kk, q, n in order:
            acc = acc + chain(np.ascontiguousarray(xs[kk][:, q:q + n]), np.ascontiguousarray(wt[kk][:, q:q + n]), mut)
    wss = np.zeros((len(j), H), np.float32)
    for kap in range(K):
        t = j - kap
        ok = (t >= 0) if mut == "wss_past_end" else (t >= 0) & (t < Tb)
        wss = wss + np.where(ok[:, None], tab["wsq"][kap * H:(kap + 1) * H][None, :], np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(wss > FLT_MIN, acc / wss, acc)
    s = j[:, None] * H + np.arange(H)[None, :] - trim
    keep = (s >= 0) & (s < Lyb)
    y[s[keep]] = v[keep]
    written[s[keep]] = True
    return y, written


# ---- gl_stft_update_kernel -------------------------------------------------------------------------------------------------------
def phase_update(re, im, pr, pi, alpha, s, fma):
    ar, ai = sub_prod(re, alpha, pr, fma["alpha"]), sub_prod(im, alpha, pi, fma["alpha"])
    den = np.sqrt(sum_sq(ar, ai, fma["den"])) + FLT_MIN
    return s * ar / den, s * ai / den


def update_acc(y, Tb, cfg, tab, mut=None):
    """The transform of gl_stft_update_kernel alone (it does not depend on the contraction sites): ``[Tb, 32 dft_tiles]``."""
    d = Design(cfg)
    tab = mutate_tables(tab, cfg, mut)
    rows = stage_rows(y, d.hop * (Tb - 1), d, Tb, mut)
    return transform_acc(rows, tap_weights(dft_conv_weight(d, tab["dft"]), d.cp), mut != "stft_one_chain", mut)


def update_launch(acc, S, r_prev, cfg, first, fma, mut=None, momentum=MOMENTUM):
    """``acc`` of ``update_acc``, ``S [.., Ks]``, ``r_prev [.., Qp]`` (read unless ``first``) -> ``(r [Tb, Q], c [Tb, Q])``."""
    d = Design(cfg)
    Tb, half = acc.shape[0], d.half
    alpha = np.float32(momentum if mut == "alpha_momentum" else momentum / (1.0 + momentum))
    b = np.arange(half)
    re, sine = acc[:, d.dft_col(b, 0)], acc[:, d.dft_col(b, 1)]
    im = sine.copy() if mut == "im_sign" else -sine
    im[:, 0] = 0
    nyq = sine[:, 0]
    if first and mut != "first_uses_rprev":
        pr, pi, pn = np.zeros_like(re), np.zeros_like(re), np.zeros_like(nyq)
    else:
        rp = np.asarray(r_prev, dtype=np.float32)[:Tb]
        pr, pi, pn = rp[:, 0:2 * half:2].copy(), rp[:, 1:2 * half:2].copy(), rp[:, 2 * half].copy()
        pi[:, 0] = 0
    S = np.asarray(S, dtype=np.float32)[:Tb]
    r, c = np.zeros((Tb, d.q), np.float32), np.zeros((Tb, d.q), np.float32)
    r[:, 0:2 * half:2], r[:, 1:2 * half:2], r[:, 2 * half] = re, im, nyq
    with np.errstate(divide="ignore", invalid="ignore"):
        c[:, 0:2 * half:2], c[:, 1:2 * half:2] = phase_update(re, im, pr, pi, alpha, S[:, :half], fma)
        c[:, 2 * half] = phase_update(nyq, np.zeros_like(nyq), pn, np.zeros_like(nyq), alpha, S[:, half], fma)[0]
    return r, c


# ---- the bias denoiser: dn_stft_kernel<subtract | magnitude>, dn_bias_reduce_kernel, dn::Window ------------------------------------
def dn_waveform_item(n, cfg, seed):
    """``[n]`` float32, the seeded waveform of a denoiser case (tests/denoiser_cases.py describes it): two tones at 1 % and 9 %
    of the sample rate, amplitudes 0.7 and 0.1, white noise at 1e-3."""
    rng = np.random.default_rng(4700 + 13 * n + seed)
    t = np.arange(n, dtype=np.float64) / cfg["sample_rate"]
    x = 1e-3 * rng.standard_normal(n)
    for f, a in ((0.01 * cfg["sample_rate"], 0.7), (0.09 * cfg["sample_rate"], 0.1)):
        x += a * np.sin(2.0 * np.pi * f * t + rng.uniform(0.0, 2.0 * np.pi))
    return x.astype(np.float32)


def dn_wave(name, B, M, seed=0):
    """``[B, hop M]`` float32, the caller's own copy: item b is ``dn_waveform_item(hop M, cfg, seed + b)``."""
    if ("dnwav", name, B, M, seed) not in _cache:
        cfg = TS_CONFIGS[name]
        _cache[("dnwav", name, B, M, seed)] = np.stack([dn_waveform_item(cfg["hop_length"] * M, cfg, seed + b) for b in range(B)])
    return _cache[("dnwav", name, B, M, seed)].copy()


def dn_case_m(name):
    """The largest M of a config in ``DN_CASES``: the shape of its silence case."""
    return max(M for n, _, M in DN_CASES if n == name)


def dn_silence(name, M=None):
    """``[2, hop M]`` (M: that of the config's largest denoiser case): item 0 is digital silence; item 1 has its middle 2 n_fft
    samples at 0.0f -- whole frames with mag == 0 beside live ones, and frames that are partly silent."""
    cfg = TS_CONFIGS[name]
    w = dn_wave(name, 2, dn_case_m(name) if M is None else M, seed=20)
    w[0] = 0
    mid = w.shape[1] // 2
    w[1, mid - cfg["n_fft"]:mid + cfg["n_fft"]] = 0
    return w


def dn_forced_bias(bias):
    """``bias`` with every fourth entry from 0 forced to exactly 0.0 (scale == 1; bins 0 and n_fft / 2 are among them) and
    every fourth from 2 to 1e30 (scale == 0), the odd ones left as they are."""
    out = np.array(bias, dtype=np.float32)
    out[0::4], out[2::4] = 0.0, 1e30
    return out


def dn_item_frames(m, T, mut=None):
    """``stft::item_frames`` at ``extra`` = 1 -- ``m`` is an item's MEL frames (None: a dense call) -> its T_b."""
    if m is None:
        return T
    extra = 0 if mut == "dn_frames_extra0" else 1
    n = min(max(int(m), 0), T - extra) + extra
    return 0 if n < 2 else n


def window_acc(y, y_org, frames, cfg, tab, mut=None):
    """The transform of ``stft_kernel`` for a dense call whose frame 0 is centred on sample ``y_org`` of ``y [Lw]``:
    ``[frames, 32 dft_tiles]``.  Samples outside [0, Lw) read as 0.  With ``y_org`` = 0 and Lw = hop (frames - 1) it is
    ``update_acc``; a ragged item is the dense call on its own ``y[:L_b]``."""
    d = Design(cfg)
    tab = mutate_tables(tab, cfg, mut)
    y = np.asarray(y, dtype=np.float32)
    org = int(y_org) + (d.hop if mut == "dn_window_origin_shift" else 0)
    rows = stage_rows(y, len(y), d, frames, mut, org)
    return transform_acc(rows, tap_weights(dft_conv_weight(d, tab["dft"]), d.cp), True, mut)


def dn_parts(acc, d, mut=None):
    """``(re, im, nyq)`` as ``decode_bins`` hands them to a policy: im = -sine, Im of bin 0 as 0.f, nyq from the sine column of bin 0."""
    b = np.arange(d.half)
    re, sine = acc[:, d.dft_col(b, 0)], acc[:, d.dft_col(b, 1)]
    im = sine.copy() if mut == "dn_im_sign" else -sine
    im[:, 0] = 0
    return re, im, sine[:, 0].copy()


def subtract_scale(re, im, bias, strength, fma, mut=None):
    """``(scale, g, mag)`` of ``dn::subtract_scale(dn::magnitude(re, im), bias, strength)``."""
    zero, s = np.float32(0), np.float32(strength)
    mag = np.sqrt(sum_sq(re, im, fma["mag"]))
    g = np.maximum(mag - s * bias if mut == "dn_fma_unfused" else co.fmaf32(-s, bias, mag), zero)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = g / mag if mut == "dn_scale_unguarded" else np.where(mag > 0, g / mag, zero)
    return scale.astype(np.float32), g, mag


def subtract_launch(acc, bias, strength, cfg, fma, mut=None):
    """``acc`` of ``window_acc`` -> ``c [Tb, Q]`` exactly as ``Subtract::bins4`` and ``Subtract::nyquist`` write it."""
    d = Design(cfg)
    half = d.half
    bias = np.asarray(bias, dtype=np.float32)
    assert bias.shape == (d.bins,)
    re, im, nyq = dn_parts(acc, d, mut)
    c = np.zeros((acc.shape[0], d.q), np.float32)
    scale, g, mag = subtract_scale(re, im, bias[None, :half], strength, fma, mut)
    if mut == "dn_divide_last":
        with np.errstate(divide="ignore", invalid="ignore"):
            c[:, 0:2 * half:2], c[:, 1:2 * half:2] = np.where(mag > 0, g * re / mag, 0), np.where(mag > 0, g * im / mag, 0)
    else:
        c[:, 0:2 * half:2], c[:, 1:2 * half:2] = scale * re, scale * im
    c[:, 2 * half] = subtract_scale(nyq, np.zeros_like(nyq), bias[0 if mut == "dn_nyquist_bias0" else half], strength, fma, mut)[0] * nyq
    if mut == "dn_nyquist_im_kept":                              # the sine column that carried the value, scaled like an Im
        c[:, 2 * half + 1] = -c[:, 2 * half]
    return c


def magnitude_launch(acc, cfg, fma):
    """``acc`` of ``window_acc`` -> ``mag [Tb, bins]`` as ``Magnitude::bins4`` and ``Magnitude::nyquist`` write it."""
    d = Design(cfg)
    re, im, nyq = dn_parts(acc, d)
    mag = np.empty((acc.shape[0], d.bins), np.float32)
    mag[:, :d.half] = np.sqrt(sum_sq(re, im, fma["mag"]))
    mag[:, d.half] = np.sqrt(sum_sq(nyq, np.zeros_like(nyq), fma["mag"]))
    return mag


def dn_tiny(acc, cfg):
    """``[Tb, Q]`` bool: the elements of c whose float64 re^2 + im^2 lies below ``DN_TINY`` -- where fp32 squares go subnormal."""
    d = Design(cfg)
    re, im, nyq = (v.astype(np.float64) for v in dn_parts(acc, d))
    tiny = np.zeros((acc.shape[0], d.q), bool)
    t = re * re + im * im < DN_TINY
    tiny[:, 0:2 * d.half:2], tiny[:, 1:2 * d.half:2], tiny[:, 2 * d.half] = t, t, nyq * nyq < DN_TINY
    return tiny


def dn_interior(cfg, T, mut=None):
    """``(t_lo, t_hi)`` of ``dn_estimate``: the frames whose window lies wholly inside the signal, e = ceil(n_fft / 2 / hop)."""
    d = Design(cfg)
    edge = (d.half + d.hop - 1) // d.hop
    if mut == "dn_mean_over_all_frames":
        return 0, T
    if mut == "dn_interior_wide":
        edge -= 1
    return edge, T - edge


def _pairwise(x):
    return x[0] if len(x) == 1 else _pairwise(x[:len(x) // 2]) + _pairwise(x[len(x) // 2:])


def bias_reduce(mag, t_lo, t_hi, mut=None):
    """dn_bias_reduce_kernel: the fp32 terms summed in float64 strictly in ascending t, divided by the count in float64, rounded
    to fp32 once.  ``dn_bias_pairwise`` is the tree order with fp32 partial sums: in float64 the order of at most a few
    hundred fp32 terms moves the sum by 2^-53 relative, 2^-29 of the distance between two fp32 values, and no case can show it."""
    m = np.asarray(mag, dtype=np.float32)[t_lo:t_hi]
    assert t_hi > t_lo and m.shape[0] == t_hi - t_lo
    if mut == "dn_bias_sum_f32":
        total = np.add.accumulate(m, axis=0, dtype=np.float32)[-1]
        return (total / np.float32(t_hi - t_lo)).astype(np.float32)
    if mut == "dn_bias_pairwise":
        return (_pairwise(m).astype(np.float64) / np.float64(t_hi - t_lo)).astype(np.float32)
    total = np.zeros(m.shape[1], np.float64)
    for t in range(m.shape[0]):
        total = total + m[t].astype(np.float64)
    return (total / np.float64(t_hi - t_lo)).astype(np.float32)


def dn_window(cfg, m0, Mw, final, mut=None):
    """``dn::Window`` restated: ``(f_lo, f_hi, out_lo, out_count)`` of the window [hop m0, hop (m0 + Mw))."""
    d = Design(cfg)
    H, half, e = d.hop, d.half, (d.half + d.hop - 1) // d.hop
    o, end = H * m0, H * (m0 + Mw)
    f_lo = m0 + e if m0 else 0
    f_hi = max(m0 + Mw + 1 if final else m0 + Mw - e + 1, f_lo)
    lo = max(o, (f_lo + d.taps - 1) * H - half) if m0 else o
    hi = end if final else min(end, f_hi * H - half)
    count = hi - lo if f_hi > f_lo and hi > lo else 0
    return f_lo, f_hi, (lo if count else o), count


def window_slice(c, frames, s_org, Ly, cfg, tab, mut=None):
    """``launch_istft_slice`` on ``c [frames, Qp]``: samples [s_org, s_org + Ly) of the dense inverse transform of c taken as a
    whole utterance's, so no new restatement is needed.  The kernel bounds a dense slice by s_org + Ly where ``istft_launch``
    bounds by hop (frames - 1), and s_org + Ly <= hop (frames - 1) in both cases of ``dn::Window``: a final window ends at
    sample hop (m0 + Mw) = hop (f_hi - 1), so out_lo + out_count - hop f_lo = hop (frames - 1); an interior one at or before
    hop f_hi - n_fft / 2, and n_fft / 2 >= hop.  Frames outside [f_lo, f_hi) "do not exist": t < 0 or t >= frames in the
    window's coordinates, which is the rule for the staged zeros and the w^2 terms that ``istft_launch`` already restates.  A
    row's chain does not depend on the block it falls into, so the other ``first_row`` of a slice changes no bit."""
    d = Design(cfg)
    assert 0 <= s_org and Ly > 0 and s_org + Ly <= d.hop * (frames - 1), (s_org, Ly, frames)
    y, written = istft_launch(c, frames, frames, cfg, tab, False, mut)
    assert written[s_org:s_org + Ly].all()
    return y[s_org:s_org + Ly]


def dn_forward_np(wav, m, bias, strength, cfg, tab, fma, mut=None):
    """One item through ``dn_forward``: ``wav [L]``, ``m`` its mel frames or None -> ``{"frames", "acc", "c", "out"}``."""
    d = Design(cfg)
    T = len(wav) // d.hop + 1
    Tb = dn_item_frames(m, T, mut)
    out = {"frames": Tb, "acc": None, "c": np.zeros((0, d.q), np.float32)}
    if Tb:
        out["acc"] = window_acc(np.asarray(wav)[:d.hop * (Tb - 1)], 0, Tb, cfg, tab, mut)
        out["c"] = subtract_launch(out["acc"], bias, strength, cfg, fma, mut)
    out["out"], written = istft_launch(out["c"], Tb, T, cfg, tab, True, mut)
    assert written.all()
    return out


def dn_estimate_np(wav, cfg, tab, fma, mut=None):
    """``dn_estimate`` on ``wav [L]`` -> ``(mag [T, bins], bias [bins])``."""
    d = Design(cfg)
    T = len(wav) // d.hop + 1
    mag = magnitude_launch(window_acc(wav, 0, T, cfg, tab, mut), cfg, fma)
    return mag, bias_reduce(mag, *dn_interior(cfg, T, mut), mut)


# ---- the time stretch: stft_kernel<ts::Spectrum>, ts_step_kernel, ts_scan_kernel, gl_istft_kernel with sample_counts ---------------
def ts_case_id(case) -> str:
    return f"{case[0]}-B{case[1]}-M{case[2]}-r{case[3]:.4g}"


def ts_silence(name):
    """``dn_silence`` with item 1's first n_fft samples at 0.0f as well: item 0 is digital silence, item 1 has silent frames in
    front (its start phase is fixed(turns(0, 0)) = 0) and in the middle, beside live ones."""
    w = dn_silence(name, None if name in GL_CONFIGS else max(M for n, _, M, _ in TS_CASES if n == name))
    w[1, :TS_CONFIGS[name]["n_fft"]] = 0
    return w


def ts_small_angles(name, M):
    """``[1, hop M]``: the case waveform with its first n_fft / 2 samples -- all that frame 0 sees -- replaced by 0.5 at sample 0
    and 0.5e-4 at sample 1.  Sample 0 sits on the window's peak, so c[0, k] = (-1)^k (0.5 + 0.5e-4 w_1 e^(-2 pi i k / n_fft)): an
    angle of about -1e-4 sin(2 pi k / n_fft) rad in every even bin."""
    w = dn_wave(name, 1, M, seed=21)
    w[0, :TS_CONFIGS[name]["n_fft"] // 2] = 0
    w[0, 0], w[0, 1] = 0.5, 0.5e-4
    return w


def ts_counts(m, T, hop, rate, mut=None):
    """``Spectrum::item``: ``m`` an item's MEL frames (None: a dense call of T frames) -> ``(T_b, T_out_b, n_out_b)``."""
    Tb = dn_item_frames(m, T)
    q = np.float64(hop * (Tb - 1) if Tb else 0) / np.float64(rate)
    n = int({"ts_n_out_truncated": np.trunc(q), "ts_n_out_half_up": np.floor(q + 0.5)}.get(mut, np.rint(q)))
    return Tb, (int(np.ceil(np.float64(Tb) / np.float64(rate))) if Tb > 0 else 0), n


def spectrum_launch(acc, cfg, mut=None):
    """``acc`` of ``window_acc`` at y_org = 0 -> ``c [Tb, Q]`` exactly as ``Spectrum::bins4`` stores it."""
    d = Design(cfg)
    re, im, nyq = dn_parts(acc, d)
    c = np.zeros((acc.shape[0], d.q), np.float32)
    c[:, 0:2 * d.half:2], c[:, 1:2 * d.half:2], c[:, 2 * d.half] = re, im, nyq
    if mut == "ts_nyquist_im_kept":                              # the sine column that carried the value, stored like an Im
        c[:, 2 * d.half + 1] = -nyq
    return c


def u32(v):
    """The distance from fp32(|v|) to the next fp32 value above it, as float64; 0 where v is 0."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.where(v == 0, 0.0, np.spacing(v.astype(np.float32)).astype(np.float64))


def ts_turn_bar(theta):
    """``e_turn`` of the module docstring: the error allowed of ``ts::turns`` at the float64 angle ``theta``, in turns."""
    inv = 1.0 / (2.0 * np.pi)
    return TS_ATAN2_ULP * u32(theta) * inv + np.abs(theta) * abs(float(TS_INV_2PI32) - inv) + 0.5 * u32(theta * float(TS_INV_2PI32))


def ts_unit_diff(got, want):
    """``got`` (uint32 values as int64) minus ``want`` (float64 units), as the wrapped signed difference modulo 2^32."""
    diff = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    return diff - TS_UNIT * np.rint(diff / TS_UNIT)


def ts_fixed(x32, mut=None):
    """``ts::fixed``: fp32 turns -> uint32 units held in int64; the product by 2^32 is exact."""
    assert x32.dtype == np.float32
    v = x32.astype(np.float64) * TS_UNIT
    return (np.trunc(v) if mut == "ts_fixed_truncated" else np.rint(v)).astype(np.int64) & 0xFFFFFFFF


def ts_advance(d, mut=None):
    """``(advance_fixed [bins] int64, advance_turns [bins] fp32)`` of ``ts::advance_fixed`` / ``ts::advance_turns``."""
    r = np.arange(d.bins, dtype=np.int64) * d.hop
    if mut != "ts_adv_no_modulo":
        r = r % d.n_fft
    fx = ((((r << 33) // d.n_fft) + 1) >> 1) if mut == "ts_adv_fixed_rounded" else (r << 32) // d.n_fft
    return fx & 0xFFFFFFFF, r.astype(np.float32) / np.float32(d.n_fft)


def ts_rows(c, Tb, To, rate, d, mut=None):
    """``(alpha [To] fp32, re0, im0, re1, im1 [To, bins] fp32, exists [2, To])``: the two source rows of every output frame; a row
    >= Tb is 0 and does not exist."""
    t = np.arange(To)
    if mut == "ts_alpha_f32":
        step = t.astype(np.float32) * np.float32(rate)
    else:
        step = t.astype(np.float64) * np.float64(rate)
    fl = np.floor(step)
    i, alpha = fl.astype(np.int64), (step - fl).astype(np.float32)
    rows = np.zeros((Tb + 2, 2 * d.bins), np.float32)
    rows[:Tb] = np.asarray(c, dtype=np.float32)[:Tb, :2 * d.bins]
    if mut == "ts_row_past_end_kept" and Tb:
        rows[Tb] = rows[Tb - 1]
    i = np.minimum(i, Tb)
    r0, r1 = rows[i], rows[i + 1]
    return alpha, r0[:, 0::2], r0[:, 1::2], r1[:, 0::2], r1[:, 1::2], np.stack([i < Tb, i + 1 < Tb])


def step_launch(c, Tb, To, rate, cfg, mut=None):
    """``c [.., Qp]`` (or ``[.., Q]``; only rows below Tb and columns below 2 bins are read) -> a dict:
    ``mag [To, Ks]`` fp32, exact; ``inc_want``, ``inc_bar`` ``[To, Ks]`` float64 in units of 2^-32 turn (the module docstring
    derives the bar; padding bins want 0 within 0); ``tiny [To, Ks]``: float64 re^2 + im^2 of either source row that exists below DN_TINY;
    ``inc [To, Ks]`` int64: the header's line in fp32 with numpy's arctan2, for chaining on the CPU."""
    d = Design(cfg)
    alpha, re0, im0, re1, im1, exists = ts_rows(c, Tb, To, rate, d, mut)
    a = np.broadcast_to(alpha[:, None], re0.shape)
    m0 = np.sqrt(sum_sq(re0, im0, {"ts_mag_fma_re": 1, "ts_mag_fma_im": 2}.get(mut, 0)))
    m1 = np.sqrt(sum_sq(re1, im1, {"ts_mag_fma_re": 1, "ts_mag_fma_im": 2}.get(mut, 0)))
    if mut == "ts_lerp_fma_swapped":                             # (1 - alpha) m0 fused, alpha m1 rounded
        mag = co.fmaf32(np.float32(1) - a, m0, a * m1)
    else:
        mag = co.fmaf32(a, m1, (np.float32(1) - a) * m0)
    adv_fixed, adv32 = ts_advance(d, mut)
    # the wanted increment and its bar, from float64
    th0, th1 = np.arctan2(im0.astype(np.float64), re0.astype(np.float64)), np.arctan2(im1.astype(np.float64), re1.astype(np.float64))
    inv = 1.0 / (2.0 * np.pi)
    d1 = th1 * inv - th0 * inv
    d2 = d1 - adv32.astype(np.float64)[None, :]
    want = adv_fixed[None, :].astype(np.float64) + TS_UNIT * d2
    bar = TS_UNIT * (ts_turn_bar(th1) + ts_turn_bar(th0) + 0.5 * u32(d1) + 0.5 * u32(d2)) + 0.5
    bar = np.where((th0 == 0) & (th1 == 0), 0.0, bar)
    # the same line in fp32
    t0, t1 = np.arctan2(im0, re0) * TS_INV_2PI32, np.arctan2(im1, re1) * TS_INV_2PI32
    dphi = t1 - t0 - adv32[None, :]
    if mut != "ts_no_wrap":                                      # an equivalent form, not a mutation
        dphi = dphi - np.rint(dphi)
    assert dphi.dtype == np.float32
    inc = (adv_fixed[None, :] + ts_fixed(dphi, mut)) & 0xFFFFFFFF
    sq0 = re0.astype(np.float64) ** 2 + im0.astype(np.float64) ** 2
    sq1 = re1.astype(np.float64) ** 2 + im1.astype(np.float64) ** 2
    pad = lambda v, dt: np.concatenate([v.astype(dt), np.zeros((To, d.ks - d.bins), dt)], axis=1)
    return {"mag": pad(mag, np.float32), "inc_want": pad(want, np.float64), "inc_bar": pad(bar, np.float64), "inc": pad(inc, np.int64),
            "tiny": pad(((sq0 < DN_TINY) & exists[0][:, None]) | ((sq1 < DN_TINY) & exists[1][:, None]), bool), "alpha": alpha}


def ts_sincospi(x):
    """``(cospi x, sinpi x)`` in float64 for fp32 ``x`` in [-1, 1], the argument reduced exactly first."""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x)
    r = x - n                                                    # exact, [-1/2, 1/2]
    sgn = 1.0 - 2.0 * np.mod(n, 2.0)
    cos = np.where(np.abs(r) > 0.25, np.sin(np.pi * (0.5 - np.abs(r))), np.cos(np.pi * r))
    return sgn * cos, sgn * np.sin(np.pi * r)


def scan_launch(c_row0, mag, inc, To, cfg, acc0=None, mut=None):
    """``c_row0 [>= Q]``: row 0 of the item's spectrum; ``mag [To, Ks]`` fp32 and ``inc [To, Ks]`` (uint32 values as int64): the
    launch's own inputs; ``acc0 [Ks]``: the launch's own acc[0] (None: the fp32 line with numpy's arctan2) -> a dict:
    ``acc0_want``, ``acc0_bar`` ``[Ks]`` float64 units; ``acc [To, Ks]`` int64, exact from ``inc`` and ``acc0``;
    ``out_want``, ``out_bar`` ``[To, Qp]`` float64: mag (cospi x, sinpi x) on ``mag`` and ``acc``, interleaved, and its bar;
    ``out_c [To, Qp]`` fp32: ``out_want`` rounded, for chaining on the CPU."""
    import time_stretch_restatement as R
    d = Design(cfg)
    row = np.asarray(c_row0, dtype=np.float32)[:2 * d.bins]
    re, im = row[0::2], row[1::2]
    th = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    pad = lambda v, dt: np.concatenate([v.astype(dt), np.zeros(d.ks - d.bins, dt)])
    want0 = pad(TS_UNIT * th / (2.0 * np.pi), np.float64)
    bar0 = pad(np.where(th == 0, 0.0, TS_UNIT * ts_turn_bar(th) + 0.5), np.float64)
    if acc0 is None:
        acc0 = pad(np.zeros(d.bins, np.int64) if mut == "ts_start_phase_0" else ts_fixed(np.arctan2(im, re) * TS_INV_2PI32, mut), np.int64)
    acc0 = np.asarray(acc0, dtype=np.int64)
    inc = np.asarray(inc, dtype=np.int64)[:To]
    if mut == "ts_scan_inclusive":
        acc = (acc0[None, :] + np.cumsum(inc, axis=0)) & R.MASK
    else:
        acc = R.scan_fixed(acc0, inc)
    if mut == "ts_unfixed_u32":
        x = np.float32(2) * (acc.astype(np.float32) * np.float32(2.0 ** -32))
    else:
        x = np.float32(2) * R.unfixed(acc)
    assert x.dtype == np.float32
    cos, sin = ts_sincospi(x)
    if mut == "ts_sin_cos_swapped":
        cos, sin = sin, cos
    m = np.asarray(mag, dtype=np.float32)[:To].astype(np.float64)
    want, bar = np.empty((To, d.qp)), np.empty((To, d.qp))
    for o, trig in ((0, cos), (1, sin)):
        want[:, o::2] = m * trig
        bar[:, o::2] = TS_SINCOSPI_ULP * np.abs(m) * u32(trig) + 0.5 * u32(m * trig) + TS_FLOOR
    return {"acc0_want": want0, "acc0_bar": bar0, "acc0": acc0, "acc": acc, "out_want": want, "out_bar": bar, "out_c": want.astype(np.float32)}


def ts_forward_np(wav, m, rate, cfg, tab, mut=None):
    """One item through ``ts_forward``: ``wav [L]``, ``m`` its mel frames or None -> ``{"counts", "acc", "c", "step", "scan", "out"}``;
    ``out [rint(L / rate)]`` is laid out by the dense call as the device's row is."""
    d = Design(cfg)
    L = len(wav)
    T = L // d.hop + 1
    _, T_out, n_out = ts_counts(None, T, d.hop, rate, mut)
    Tb, To, n = ts_counts(m, T, d.hop, rate, mut)
    out = {"counts": (Tb, To, n), "acc": None, "c": np.zeros((0, d.q), np.float32)}
    if Tb:
        out["acc"] = window_acc(np.asarray(wav)[:d.hop * (Tb - 1)], 0, Tb, cfg, tab, mut)
        out["c"] = spectrum_launch(out["acc"], cfg, mut)
    out["step"] = step_launch(out["c"], Tb, To, rate, cfg, mut)
    out["scan"] = scan_launch(out["c"][0] if Tb else np.zeros(d.q, np.float32), out["step"]["mag"], out["step"]["inc"], To, cfg, mut=mut)
    out["out"], written = istft_launch(out["scan"]["out_c"], To, T_out, cfg, tab, True, mut, sample_count=n, Ly=n_out)
    assert written.all()
    return out


# ---- a forward on the CPU (the restatements fed with their own outputs) -------------------------------------------------------------
def forward_np(logmel, phase, cfg, tab, n_iter, fma, length=None, nnls_iters=NNLS_ITERS, mut=None):
    """One item through ``gl_forward``: ``{"S", "c0", "wav": {n: out_n}, "r": [..], "c": [..], "y": [..]}`` for n <= n_iter."""
    T = logmel.shape[1]
    Tb = item_frames(length, T)
    S, c, _, _ = invert_launch(logmel, phase, Tb, cfg, tab, nnls_iters, fma, mut)
    out = {"S": S, "c0": c, "wav": {}, "r": [], "c": [c], "y": []}
    r = None
    for it in range(n_iter + 1):
        out["wav"][it] = istft_launch(c, Tb, T, cfg, tab, length is not None, mut)[0]
        if it == n_iter:
            break
        y = istft_launch(c, Tb, T, cfg, tab, False, mut)[0]
        r, c = update_launch(update_acc(y, Tb, cfg, tab, mut), pad_cols(S, Design(cfg).ks), r, cfg, it == 0, fma, mut)
        out["y"].append(y), out["r"].append(r), out["c"].append(c)
    return out


# ---- judging on the device's own tensors ---------------------------------------------------------------------------------------
class Session:
    """What a GPU test module keeps: per kernel the contraction assignments that still reproduce every element judged so far,
    and per launch kind the counts the issue asks to print."""

    def __init__(self):
        self.alive = {"mel_kernel": assignments(MEL_SITES), "gl_invert_kernel": assignments(INVERT_SITES),
                      "gl_stft_update_kernel": assignments(UPDATE_SITES),
                      "dn_stft_kernel<subtract>": assignments(DN_SITES), "dn_stft_kernel<magnitude>": assignments(DN_SITES)}
        self.stats, self.judged = {}, set()

    def count(self, kind, exact=0, undecided=0, frames=0, ratio=0.0):
        s = self.stats.setdefault(kind, {"exact": 0, "undecided": 0, "frames": 0, "worst": 0.0})
        s["exact"] += int(exact)
        s["undecided"] += int(undecided)
        s["frames"] += int(frames)
        s["worst"] = max(s["worst"], float(ratio))

    def judge(self, kernel, kind, where, restate, compare):
        """``restate(fma)`` -> the restatement under one assignment; ``compare(restated)`` -> the number of elements that
        differ from the device.  Keeps the assignments with no difference; fails, naming the launch, when none is left."""
        left, seen = [], []
        self.judged.add(kernel)
        for fma in self.alive[kernel]:
            bad = compare(restate(fma))
            seen.append((fma, bad))
            if bad == 0:
                left.append(fma)
        assert left, f"{kind} {where}: no single contraction assignment of {kernel} reproduces the device; differing elements per assignment: {seen}"
        self.alive[kernel] = left
        return left[0]

    def report(self):
        for kind, s in sorted(self.stats.items()):
            print(f"{kind}: {s['exact']} elements exact, {s['undecided']} of {s['frames']} frames undecided, worst error / bar {s['worst']:.3f}")
        for kernel, left in self.alive.items():
            if kernel not in self.judged:                       # another module's kernels
                continue
            print(f"{kernel}: contraction assignment(s) that reproduce every element: {left}")


def differing(got, want, mask=None):
    """Elements of ``got`` that differ from ``want`` by value (NaN differs from everything), within ``mask``."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    return int(bad.sum() if mask is None else (bad & mask).sum())
