"""The time stretch without a GPU: the restatement against librosa's loop and against its own identities, the cases' reasons for
being there, the library's host-only arithmetic, the pitch composition on the host resampler, and every refusal that must
come before any device work."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.pipeline import MelToWavePipeline
from iris.resample import design_bank, resample_host
from iris.synthesis_output import build_parser, check_pitch_steps, check_tempo, main, vocode_to_wav
from iris.time_stretch import RATE_RANGE, TimeStretch, check_rate, pitch_compose, pitch_rates, semitone_ratio

import griffin_lim_restatement as G
import time_stretch_cases as C
import time_stretch_restatement as R

CASE_IDS = [C.case_id(c) for c in C.CASES]


# ---- the cases are what they claim to be -----------------------------------------------------------------------------------
def test_every_property_the_cases_are_chosen_for_holds():
    sh = {c: C.shape(c) for c in C.CASES}
    blocks = lambda n: -(-n // C.BLOCK_FRAMES)
    assert any(s["T_out"] == C.BLOCK_FRAMES + 1 for s in sh.values())                       # one past a block edge
    assert any(blocks(s["T_out"]) == 3 for s in sh.values())                                # three blocks
    assert any(c[0] == "small" and c[2] == 2 and s["T"] < s["taps"] for c, s in sh.items())   # fewer frames than taps
    assert any(s["T"] == 2 and c[3] == 4.0 and s["T_out"] == 1 for c, s in sh.items())
    assert any(c[3] == 1.0 for c in C.CASES)
    assert any(c[3] < 1 and s["n_out"] < s["hop"] * (s["T_out"] - 1) for c, s in sh.items())  # the crop is live
    assert any(c[3] > 1 and s["hop"] * (s["T_out"] - 1) < s["n_out"] < s["hop"] * (s["T_out"] - 1) + s["n_fft"] // 2
               for c, s in sh.items())                                                      # the tail rule is live
    assert any(c[3] == 2.0 ** (-1.0 / 12.0) and np.frexp(c[3])[0] != 0.5 for c in C.CASES)    # not a power of two
    run = lambda s: -(-s["T_out"] // C.SCAN_RUNS)
    assert any(s["T_out"] > C.SCAN_RUNS and s["T_out"] % run(s) for s in sh.values())       # a short last run
    assert any(1 < s["T_out"] < C.SCAN_RUNS for s in sh.values())                           # fewer frames than runs
    assert {c[0] for c in C.CASES} == {"default", "small", "two_tap"}
    for c, s in sh.items():
        ts = TimeStretch(*C.stft_args(c[0]))
        assert ts.out_frames_samples(s["L"], c[3]) == (s["T_out"], s["n_out"])
        assert ts.launch_count(c[1], s["L"], c[3]) == 4


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small", "two_tap", "default"))
def test_rate_one_returns_the_round_trip(name):
    n_fft, hop, win = C.stft_args(name)
    y = C.waveform_item(hop * 37, C.CONFIGS[name], seed=3)
    want = G.istft(G.stft(y, n_fft, hop, win), n_fft, hop, win)
    got = R.stretch(y, 1.0, n_fft, hop, win)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9
    assert np.abs(got - y).max() <= 1e-6                                              # and the round trip returns the input


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_restatement_equals_librosas_loop(case):
    name, rate = case[0], case[3]
    n_fft, hop, win = C.stft_args(name)
    out, taps = C.restated(case)
    for b, y in enumerate(C.waveform(case)):
        D = G.stft(y, n_fft, hop, win)
        D.imag[:, 0] = 0
        D.imag[:, -1] = 0
        want = R.librosa_loop(D.T.copy(), rate, n_fft, hop).T                          # [T_out, K]
        got = taps[b]["out_re"] + 1j * taps[b]["out_im"]
        assert got.shape == want.shape == (C.shape(case)["T_out"], n_fft // 2 + 1)
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        wav = R.istft_length(want.real.copy(), want.imag.copy(), C.shape(case)["n_out"], n_fft, hop, win)
        assert np.abs(out[b] - wav).max() <= 1e-9


def test_istft_length_crops_pads_and_keeps_the_tail():
    n_fft, hop, win = C.stft_args("small")
    y = C.waveform_item(hop * 9, C.CONFIGS["small"], seed=1)
    c = G.stft(y, n_fft, hop, win)
    full = G.istft(c, n_fft, hop, win)
    for n_out in (5, hop * 9, hop * 9 + 7, hop * 9 + n_fft // 2, hop * 9 + n_fft):
        got = R.istft_length(c.real.copy(), c.imag.copy(), n_out, n_fft, hop, win)
        assert got.shape == (n_out,)
        k = min(n_out, hop * 9)
        assert np.array_equal(got[:k], full[:k])
        assert not got[hop * 9 + n_fft // 2:].any()
        if n_out > hop * 9 + 4:
            assert np.abs(got[hop * 9:hop * 9 + 4]).max() > 0                           # the samples librosa's trim keeps


def test_fixed_point_scan_is_the_cumsum_modulo_a_turn():
    rng = np.random.default_rng(5)
    for To in (1, 2, 31, 32, 33, 75, 640):
        inc = rng.integers(0, 1 << 32, size=(To, 7), dtype=np.int64)
        acc0 = rng.integers(0, 1 << 32, size=7, dtype=np.int64)
        want = (acc0[None, :] + np.concatenate([np.zeros((1, 7), np.int64), np.cumsum(inc, axis=0)[:-1]])) & R.MASK
        assert np.array_equal(R.scan_fixed(acc0, inc), want)
    x = np.array([-0.5, -0.25, 0.0, 2.0 ** -33, 0.25, 0.5], np.float32)
    assert R.fixed(x).tolist() == [1 << 31, 3 << 30, 0, 0, 1 << 30, 1 << 31]
    assert R.unfixed(R.fixed(x)).tolist() == [-0.5, -0.25, 0.0, 0.0, 0.25, -0.5]
    assert R.advance_fixed(1024, 256).tolist()[:5] == [0, 1 << 30, 1 << 31, 3 << 30, 0]


# ---- the library's host-only arithmetic --------------------------------------------------------------------------------------
def test_out_samples_is_round_and_arange_over_a_sweep():
    ts = TimeStretch(64, 16, 48)
    rates = [0.25, 0.3, 0.5, 2.0 / 3.0, 0.8, 2.0 ** (-1 / 12), 1.0, 2.0 ** (1 / 12), 1.25, 1.5, 2.0, 3.0, 3.7, 4.0]
    rates += list(np.random.default_rng(11).uniform(0.25, 4.0, 40))
    for M in list(range(1, 70)) + [255, 256, 1000, 4097]:
        for rate in rates:
            L = 16 * M
            assert ts.out_frames_samples(L, rate) == (len(np.arange(0, M + 1, rate)), int(round(L / rate))), (M, rate)
            assert ts.out_samples(L, rate) == R.out_samples(L, rate)


def test_layout_and_workspace_agree():
    for args, B, M, rate in (((2048, 512, None), 3, 11, 0.8), ((1024, 256, 1024), 1, 1000, 1.25), ((64, 16, 48), 2, 1, 4.0)):
        ts = TimeStretch(*args)
        L = ts.hop_length * M
        layout, floats = ts._workspace_layout(B, L, rate)
        assert list(layout)[:5] == ["c", "mag", "inc", "acc", "out_c"]
        assert 4 * floats == ts.workspace_bytes(B, L, rate)
        assert ts.launch_count(B, L, rate) == 4 and ts.launch_count(0, L, rate) == 0 and ts.launch_count(B, 0, rate) == 0


def test_refusals_before_any_device_work():
    ts = TimeStretch()
    assert (ts.n_fft, ts.hop_length, ts.win_length) == (2048, 512, 2048)
    for bad in (0.2, 4.5, float("nan"), float("inf"), -1.0, 0.0):
        with pytest.raises(ValueError, match="rate"):
            check_rate(bad)
        with pytest.raises(ValueError, match="rate"):
            ts.forward_device(np.zeros((1, 1024), np.float32), bad)
        with pytest.raises(_native.NativeCallError) as exc:
            ts.workspace_bytes(1, 1024, bad)
        assert exc.value.status == _native.STATUS_INVALID_ARGUMENT
    assert check_rate(RATE_RANGE[0]) == 0.25 and check_rate(RATE_RANGE[1]) == 4.0
    with pytest.raises(ValueError, match="hop_length"):
        ts.forward_device(np.zeros((1, 1000), np.float32), 1.0)
    with pytest.raises(ValueError, match="float32"):
        ts.forward_device(np.zeros((1024,), np.float32), 1.0)
    with pytest.raises(ValueError, match="lengths"):
        ts.forward_device(np.zeros((2, 1024), np.float32), 1.0, lengths=[1, 3])
    with pytest.raises(ValueError, match="positive"):
        TimeStretch(n_fft=0)
    for args, status in (((1000, 250, 1000), _native.STATUS_UNSUPPORTED),      # n_fft no multiple of 32
                         ((1024, 96, 1024), _native.STATUS_UNSUPPORTED),       # hop does not divide n_fft
                         ((8192, 2048, 8192), _native.STATUS_UNSUPPORTED),
                         ((1024, 256, 2048), _native.STATUS_UNSUPPORTED)):
        with pytest.raises(_native.NativeCallError) as exc:
            TimeStretch(*args).launch_count(1, args[1] * 4, 1.0)
        assert exc.value.status == status, args
    with pytest.raises(_native.NativeCallError) as exc:                       # 2^31 elements of c
        TimeStretch(1024, 256).workspace_bytes(65535, 256 * 40, 1.0)
    assert exc.value.status == _native.STATUS_UNSUPPORTED
    with pytest.raises(_native.NativeCallError) as exc:
        ts.launch_count(-1, 1024, 1.0)
    assert exc.value.status == _native.STATUS_INVALID_ARGUMENT


# ---- pitch -------------------------------------------------------------------------------------------------------------------
def test_semitone_ratio_and_the_rates_it_asks_of_the_resampler():
    assert semitone_ratio(0) == 1 and semitone_ratio(12) == 2 and semitone_ratio(-12) == Fraction(1, 2)
    for n in (-7.0, -3.0, -1.0, 0.5, 1.0, 2.0, 5.0, 11.0):
        r = semitone_ratio(n)
        assert r == Fraction(2.0 ** (n / 12.0)).limit_denominator(640) and r.denominator <= 640
        # a best approximation: the next convergent's denominator is past 640, so the error is below 1 / (640 q)
        assert abs(r - Fraction(2.0 ** (n / 12.0))) < Fraction(1, 640 * r.denominator)
        assert semitone_ratio(n, max_den=20).denominator <= 20
        rate_in, rate_out = pitch_rates(r)
        assert Fraction(rate_out, rate_in) == 1 / r and 4000 <= min(rate_in, rate_out) and max(rate_in, rate_out) <= 192000
        bank, up, down = design_bank(rate_out, rate_in)
        assert (up, down) == (r.denominator, r.numerator)
    with pytest.raises(ValueError):
        pitch_rates(Fraction(1, 100))


def test_pitch_composition_moves_a_tone_and_keeps_the_length():
    name = "two_tap"
    n_fft, hop, win = C.stft_args(name)
    L, f0 = hop * 48, 20.0 / 256.0                                                   # cycles per sample: bin 20 of n_fft
    y = (0.5 * np.sin(2.0 * np.pi * f0 * np.arange(L))).astype(np.float32)
    for n_steps in (12.0, -12.0, 7.0):
        ratio = semitone_ratio(n_steps)
        rate_in, rate_out = pitch_rates(ratio)
        bank, up, down = design_bank(rate_out, rate_in)
        stretched = R.stretch(y, ratio.denominator / ratio.numerator, n_fft, hop, win).astype(np.float32)
        got = pitch_compose(stretched[None], [len(stretched)], L, lambda x, n: resample_host(x, bank, up, down, lengths=n))[0]
        assert got.shape == (L,) and got.dtype == np.float32
        want = R.pitch_host(y, ratio, n_fft, hop, win, lambda x: resample_host(x.astype(np.float32), bank, up, down))
        assert np.array_equal(got, want)
        spec = np.abs(np.fft.rfft(got[L // 4:3 * L // 4] * np.hanning(L // 2)))
        peak = np.argmax(spec) / (L // 2)
        assert abs(peak / (f0 * float(ratio)) - 1.0) < 0.02, (n_steps, peak)
        assert 0.3 < np.abs(got[L // 4:3 * L // 4]).max() < 0.7


# ---- the pipeline and the command line ---------------------------------------------------------------------------------------
class _Stretch:
    hop_length = 256

    def out_samples(self, L):
        return L

    def forward_device(self, wav, lengths=None):
        raise AssertionError("a refusal launches nothing")


def test_pipeline_refuses_to_stream_a_stretch():
    pipe = MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256, stretch=_Stretch())
    assert pipe.stretch is not None and MelToWavePipeline(None, lambda mel, **kw: mel, hop_length=256).stretch is None
    mel = np.zeros((1, 80, 8), np.float32)
    with pytest.raises(ValueError, match="stretch"):
        next(iter(pipe.stream(mel)))
    with pytest.raises(ValueError, match="stretch"):
        pipe.session()
    with pytest.raises(ValueError, match="normalize"):
        pipe.infer(mel, normalize=True)


def test_cli_parses_and_checks_tempo_and_pitch(tmp_path):
    args = build_parser().parse_args(["--mel", "m.npy", "--tempo", "1.25", "--pitch_steps", "-2.5"])
    assert args.tempo == 1.25 and args.pitch_steps == -2.5
    none = build_parser().parse_args(["--mel", "m.npy"])
    assert none.tempo is None and none.pitch_steps is None
    assert check_tempo(0.25) == 0.25 and check_pitch_steps(-12) == -12.0
    for bad in (0.1, 4.01, float("nan")):
        with pytest.raises(ValueError, match="tempo"):
            check_tempo(bad)
    for bad in (-12.5, 13, float("nan")):
        with pytest.raises(ValueError, match="pitch_steps"):
            check_pitch_steps(bad)
    for argv in (["--tempo", "9"], ["--pitch_steps", "40"], ["--tempo", "1.1", "--pcm16"], ["--pitch_steps", "1", "--pcm16"]):
        with pytest.raises(SystemExit):
            main(["--mel", str(tmp_path / "absent.npy")] + argv)
    with pytest.raises(ValueError, match="tempo"):
        vocode_to_wav(np.zeros((80, 4), np.float32), tmp_path / "x.wav", tempo=7.0)
    with pytest.raises(ValueError, match="float"):
        vocode_to_wav(np.zeros((80, 4), np.float32), tmp_path / "x.wav", "iris.hifigan_pretrained:infer_hifigan_pcm16", tempo=1.5)
    assert not (tmp_path / "x.wav").exists()
