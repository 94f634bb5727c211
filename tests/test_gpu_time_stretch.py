"""The time stretch (iris_time_stretch_*, ``iris.time_stretch``, ``MelToWavePipeline(stretch=)``) on the MI355X, held to the
float64 restatement of the arithmetic it commits to (tests/time_stretch_restatement.py).  Cases and inputs are
tests/time_stretch_cases.py's; tests/test_time_stretch.py shows what each case is there for.

Bars, the project's ``e32`` scheme (tests/test_gpu_denoiser.py): ``e32`` = the largest difference between the restatement run
in fp32 on the library's own tables and itself in float64, relative to ``max(1, max |want|)``, over the cases; the device must
stay within ``4 * e32`` (another summation order, another atan2f).  ``out`` is the whole stretch from the waveform; ``mag`` and
``out_c`` are launches 2 and 3 alone, both on the same fp32 spectrum (``time_stretch_cases.e32``), and the device's are held to
the float64 step on the ``c`` it stored itself.  The bars are measured when first asked for (they depend on the host BLAS's
summation order); on the CPU e32 was 5.571e-05 for the waveform (bar 2.23e-04) -- the phases of near-empty bins, which the
spectrum's own rounding moves, are in it -- 1.150e-07 for ``mag`` (bar 4.60e-07) and 1.370e-06 for ``out_c`` (bar 5.48e-06).

These bars are relative to an array's maximum and say nothing of a quiet bin.  The per-launch claims -- each launch on its own
input, ``==`` wherever the source fixes every rounding, ``inc``, ``acc[0]`` and ``out_c`` element by element to derived bars,
the rows and columns that must stay unwritten -- are tests/test_gpu_time_stretch_chain.py's.
"""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.denoiser import Denoiser
from iris.pipeline import MelToWavePipeline
from iris.resample import Resampler
from iris.synthesis_output import pcm16_from_float
from iris.time_stretch import TimeStretch, pitch_rates, pitch_shift_device, semitone_ratio
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import time_stretch_cases as C
import time_stretch_restatement as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAN = float("nan")
CASE_IDS = [C.case_id(c) for c in C.CASES]

_state = {}


def bars() -> dict:
    if "bars" not in _state:
        e = C.e32()
        _state["bars"] = {k: 4 * e[k] for k in ("out", "mag", "out_c")}
        print("e32:", {k: f"{e[k]:.3e}" for k in ("out", "mag", "out_c")})
        assert all(v > 0.0 for v in _state["bars"].values())
    return _state["bars"]


def model(name: str) -> TimeStretch:
    if name not in _state:
        _state[name] = TimeStretch(*C.stft_args(name), device=DEV)
    return _state[name]


def rel_err(got: np.ndarray, want: np.ndarray) -> float:
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    return C.rel(got, want)


def poisoned_forward(ts: TimeStretch, wav, rate, lengths=None):
    """A forward into a workspace that held NaN in every byte the layout names."""
    wav = wav if isinstance(wav, torch.Tensor) else torch.from_numpy(np.array(wav))      # a copy: the cases' arrays are read-only
    ts._ensure()
    ts._ws(int(wav.shape[0]), int(wav.shape[1]), rate).view(torch.float32).fill_(NAN)
    return ts.forward_device(wav, rate, lengths=lengths)


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_forward_matches_the_restatement(case):
    name, B, M, rate = case
    ts, wav, sh = model(name), C.waveform(case), C.shape(case)
    got, counts = poisoned_forward(ts, wav, rate)
    assert got.shape == (B, sh["n_out"]) and got.dtype == torch.float32 and got.device == DEV
    assert counts.dtype == torch.int32 and counts.tolist() == [sh["n_out"]] * B == [ts.out_samples(sh["L"], rate)] * B
    assert ts.launch_count(B, sh["L"], rate) == 4
    err = rel_err(got.cpu().numpy(), C.restated(case)[0])
    print(f"{C.case_id(case)} out: e_dev={err:.3e} bar={bars()['out']:.3e}")
    assert err <= bars()["out"]
    assert torch.equal(ts.forward_device(wav, rate)[0], got)                         # a second call: equal bits
    assert np.array_equal(ts(wav[0], rate), got[0].cpu().numpy())                    # numpy in, numpy out


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_middle_step_on_its_own_inputs_and_the_scan(case):
    name, B, M, rate = case
    ts, wav, sh = model(name), C.waveform(case), C.shape(case)
    n_fft, hop, K = sh["n_fft"], sh["hop"], sh["n_fft"] // 2 + 1
    poisoned_forward(ts, wav, rate)
    buf = {k: v.cpu().numpy() for k, v in ts._read_buffers(B, sh["L"], rate).items()}
    assert buf["frames"].tolist() == [sh["T"]] * B and buf["frames_out"].tolist() == [sh["T_out"]] * B
    assert buf["counts"].tolist() == [sh["n_out"]] * B
    for b in range(B):
        c = buf["c"][b]
        re, im = c[:, 0:2 * K:2], c[:, 1:2 * K:2]
        assert np.isfinite(re).all() and np.isfinite(im).all() and not im[:, 0].any() and not im[:, -1].any()
        want = R.middle(re, im, rate, n_fft, hop, np.float64)
        e_mag = rel_err(np.ascontiguousarray(buf["mag"][b][:, :K]), want["mag"])
        oc = buf["out_c"][b]
        got_c = np.stack([oc[:, 0:2 * K:2], oc[:, 1:2 * K:2]])
        e_c = rel_err(got_c, np.stack([want["out_re"], want["out_im"]]))
        print(f"{C.case_id(case)} item {b}: mag e_dev={e_mag:.3e} bar={bars()['mag']:.3e}; out_c e_dev={e_c:.3e} bar={bars()['out_c']:.3e}")
        assert e_mag <= bars()["mag"] and e_c <= bars()["out_c"]
        # the scan, exactly: acc = acc[0] + the exclusive cumsum of inc, modulo 2^32 -- the padding bins included
        inc, acc = buf["inc"][b], buf["acc"][b]
        want_acc = (acc[0][None, :] + np.concatenate([np.zeros((1, inc.shape[1]), np.int64), np.cumsum(inc, axis=0)[:-1]])) & R.MASK
        assert np.array_equal(acc, want_acc)
        # its start: angle(c[0]) -- atan2f within 4 ulp of numpy's at half a turn, where an fp32 ulp is 2^7 of these units
        start = R.fixed(np.arctan2(im[0], re[0]) * R.INV_2PI32)
        assert np.abs(((acc[0][:K] - start + (1 << 31)) & R.MASK) - (1 << 31)).max() <= 1 << 9 and not acc[0][K:].any()


def test_rate_one_is_the_strength_zero_denoiser():
    case = C.CASES[0]
    assert case[3] == 1.0
    wav = C.waveform(case)
    got = model(case[0]).forward_device(wav, 1.0)[0].cpu().numpy()
    want = Denoiser(*C.stft_args(case[0]), strength=0.0, device=DEV).forward_device(wav).cpu().numpy()
    err = rel_err(got, want.astype(np.float64))
    print(f"rate 1 against Denoiser(strength=0): e_dev={err:.3e} bar={bars()['out']:.3e}")
    assert err <= bars()["out"]


# ---- ragged batches ------------------------------------------------------------------------------------------------------
RAGGED_M = 40
RAGGED_LENGTHS = (0, 1, 2, 31, 32, 33, 40)


@pytest.mark.parametrize("name,rate", (("default", 0.8), ("small", 1.25), ("small", 4.0)))
def test_ragged_items_are_their_batch_of_one_calls(name, rate):
    ts, cfg = model(name), C.CONFIGS[name]
    hop = cfg["hop_length"]
    wav = torch.from_numpy(np.stack([C.waveform_item(hop * RAGGED_M, cfg, seed=50 + b) for b in range(len(RAGGED_LENGTHS))])).to(DEV)
    B, L = wav.shape
    alone = [ts.forward_device(wav[b:b + 1, :hop * m].contiguous(), rate)[0].clone() for b, m in enumerate(RAGGED_LENGTHS)]
    padded = wav.clone()
    for b, m in enumerate(RAGGED_LENGTHS):
        padded[b, hop * m:] = NAN
    want_counts = [ts.out_samples(hop * m, rate) for m in RAGGED_LENGTHS]
    assert want_counts == [R.out_samples(hop * m, rate) for m in RAGGED_LENGTHS]
    for lengths in (list(RAGGED_LENGTHS), torch.tensor(RAGGED_LENGTHS, dtype=torch.int32, device=DEV)):
        out, counts = poisoned_forward(ts, padded, rate, lengths=lengths)
        assert out.shape == (B, ts.out_samples(L, rate)) and counts.tolist() == want_counts
        for b, n in enumerate(want_counts):
            assert alone[b].shape == (1, n)
            assert torch.equal(out[b:b + 1, :n], alone[b]), (name, rate, b)
            assert torch.equal(out[b, n:], torch.zeros(out.shape[1] - n, device=DEV)), (name, rate, b)
    assert alone[0].numel() == 0 and not out[0].any()                                # a zero-length item gives zeros


# ---- pitch ---------------------------------------------------------------------------------------------------------------
def test_pitch_shift_is_stretch_then_resample_then_crop():
    name = "default"
    ts, cfg = model(name), C.CONFIGS[name]
    hop = cfg["hop_length"]
    wav = torch.from_numpy(np.stack([C.waveform_item(hop * 24, cfg, seed=70 + b) for b in range(2)])).to(DEV)
    for n_steps, lengths in ((2.0, None), (-3.0, [24, 9])):
        ratio = semitone_ratio(n_steps)
        assert isinstance(ratio, Fraction) and ratio.denominator <= 640
        got = pitch_shift_device(ts, wav, n_steps, lengths=lengths)
        stretched, counts = ts.forward_device(wav, ratio.denominator / ratio.numerator, lengths=lengths)
        rate_in, rate_out = pitch_rates(ratio)
        rs = Resampler(rate_out, rate_in=rate_in, device=DEV)
        assert (rs.up, rs.down) == (ratio.denominator, ratio.numerator)
        y = rs.forward(stretched, lengths=counts, row_scale=1)
        want = torch.zeros_like(wav)
        n = min(wav.shape[1], y.shape[1])
        want[:, :n] = y[:, :n]
        assert got.shape == wav.shape and torch.equal(got, want) and torch.isfinite(got).all() and got.abs().max() > 0.1
        if lengths is not None:
            assert not got[1, hop * 9 + rs.taps:].any()                              # the short item ends where its own samples end


# ---- the pipeline --------------------------------------------------------------------------------------------------------
def test_pipeline_with_a_stretch():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        ts = model("default")
        plain = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64)
        pipe = MelToWavePipeline(None, eng.forward, device=DEV, chunk_frames=64, stretch=ts.at(0.8))
        mel = torch.from_numpy(seeded_mel(3, 2, 40, log_mel=True)).to(DEV)
        want = ts.forward_device(plain.infer(mel), 0.8)[0]
        got = pipe.infer(mel)
        assert got.shape == (2, ts.out_samples(256 * 40, 0.8)) and torch.equal(got, want)
        pcm = pipe.infer(mel, pcm16=True)
        assert pcm.dtype == torch.int16 and np.array_equal(pcm.cpu().numpy(), pcm16_from_float(want.cpu().numpy()))
        rs = Resampler(16000, device=DEV)
        assert torch.equal(pipe.infer(mel, resampler=rs), rs.forward(want))
        with pytest.raises(ValueError, match="stretch"):
            next(iter(pipe.stream(mel)))
        with pytest.raises(ValueError, match="stretch"):
            pipe.session()
        mels = [mel[0], mel[1, :, :17], mel[0, :, :33]]
        outs, pcms, res = pipe.infer_batch(mels), pipe.infer_batch(mels, pcm16=True), pipe.infer_batch(mels, resampler=rs)
        for m, out, p, r in zip(mels, outs, pcms, res):
            one = ts.forward_device(plain.infer(m[None]), 0.8)[0][0]
            assert out.shape == (ts.out_samples(256 * m.shape[1], 0.8),) and torch.equal(out, one)
            assert np.array_equal(p.cpu().numpy(), pcm16_from_float(one.cpu().numpy()))
            assert torch.equal(r, rs.forward(one[None])[0])
    finally:
        eng.close()


def test_the_vocoder_plan_is_unchanged():
    """The forward is untouched: the launch plan of 1 x 1000 fp32 is the one recorded before this stage existed."""
    plan = _native.describe_plan(GeneratorConfig(), 1, 1000, _native.DTYPE_F32, 256)
    import json
    want = json.loads((Path(__file__).resolve().parent / "golden" / "plan_f32_1x1000.json").read_text())
    assert plan["n_launches"] == want["n_launches"] and plan["workspace_bytes"] == want["workspace_bytes"]
    assert [[l["kernel"], list(l["grid"]), l["block"], l["lds_bytes"]] for l in plan["launches"]] == want["launches"]
