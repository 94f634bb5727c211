"""The spectral-distance stage on the device (iris.metrics, csrc/spectral_distance.h) against its float64 restatement
(tests/spectral_distance_restatement.py) on the seeded cases of tests/spectral_distance_cases.py.

The bar, by the project's rule ("The bar is measured"): per output, ``e32`` is the relative error of the restatement's
float32 chain against float64 on exactly these inputs, and the device may differ from float64 by 4 x e32.  The sample-domain
sums e2 and x2 have no float32 step (e32 == 0); they are float64 sums of at most n = 20000 non-negative float64 terms taken in
another order than numpy's, so their bar is the bound of such a sum, n 2^-53 relative, doubled for the term's own rounding.
Measured on an MI355X (largest over all items of both cases): spec 1.899e-07 relative where the largest e32 is 1.899e-07 -- the
float32 chain is the project's chain oracle, and the device's error equals e32 in every printed digit of all 45 outputs; e2, x2
1.97e-16; emax and frames exact.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris.metrics import SpectralDistance
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

import spectral_distance_cases as C
import spectral_distance_restatement as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_state = {}


def stage() -> SpectralDistance:
    if "stage" not in _state:
        _state["stage"] = SpectralDistance(device=DEV)
    return _state["stage"]


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def poisoned_call(ref, test, lengths=None, row_scale=1):
    """``forward_device`` with every byte of the workspace set beforehand (0xFF: NaN as float32 and as float64)."""
    sd = stage()
    sd._ensure()
    sd._ws(*ref.shape).fill_(0xFF)
    return [t.cpu().numpy() for t in sd.forward_device(ref, test, lengths, row_scale)]


def ragged_outputs():
    if "ragged" not in _state:
        ref, test, _ = C.ragged()
        _state["ragged"] = poisoned_call(ref, test, list(C.RAGGED_LENGTHS), C.ROW_SCALE)
    return _state["ragged"]


def dense_outputs():
    if "dense" not in _state:
        _state["dense"] = poisoned_call(*C.dense())
    return _state["dense"]


def outputs_by_item():
    """``{name: (spec [R, 3], wave [3], frames [R])}`` of the device, every item of both cases."""
    spec, wave, frames = ragged_outputs()
    out = {f"ragged[{b}]": (spec[b], wave[b], frames[b]) for b in range(len(C.RAGGED_LENGTHS))}
    spec, wave, frames = dense_outputs()
    out["dense[0]"] = (spec[0], wave[0], frames[0])
    return out


def test_ragged_outputs_are_finite_and_the_empty_item_is_zero():
    spec, wave, frames = ragged_outputs()
    assert np.isfinite(spec).all() and np.isfinite(wave).all()
    assert not frames[0].any() and not spec[0].any() and not wave[0].any()
    assert (spec[1:, :, 1] > 0).all() and (wave[1:, 1] > 0).all()
    rec = stage().finish(spec, wave, frames)
    assert np.isnan(rec["spectral_convergence"][0]).all() and np.isnan(rec["log_stft_l1"][0]).all() and np.isnan(rec["snr_db"][0])
    assert np.isfinite(rec["spectral_convergence"][1:]).all() and np.isfinite(rec["log_stft_l1"][1:]).all() and np.isfinite(rec["snr_db"][1:]).all()


def test_frames_are_one_plus_samples_over_hop():
    for name, x, _ in C.items():
        want = [1 + len(x) // hop if len(x) else 0 for _, hop, _ in C.RESOLUTIONS]
        assert outputs_by_item()[name][2].tolist() == want, name
    assert outputs_by_item()["ragged[2]"][2].tolist() == [7, 4, 2]           # 3 * 256 samples at hop 512: two frames


def test_an_item_is_its_batch_of_one_call_bit_for_bit():
    ref, test, counts = C.ragged()
    spec, wave, frames = ragged_outputs()
    for b, n in enumerate(counts):
        if n == 0:
            continue
        s1, w1, f1 = poisoned_call(np.ascontiguousarray(ref[b:b + 1, :n]), np.ascontiguousarray(test[b:b + 1, :n]))
        assert np.array_equal(bits(s1[0]), bits(spec[b])) and np.array_equal(bits(w1[0]), bits(wave[b])), b
        assert np.array_equal(f1[0], frames[b])


def test_two_runs_give_the_same_bits():
    ref, test, _ = C.ragged()
    again = poisoned_call(ref, test, list(C.RAGGED_LENGTHS), C.ROW_SCALE)
    for a, b in zip(again, ragged_outputs()):
        assert np.array_equal(bits(a), bits(b))
    dref, dtest = C.dense()
    for a, b in zip(poisoned_call(dref, dtest), dense_outputs()):
        assert np.array_equal(bits(a), bits(b))


def test_every_output_of_every_item_is_inside_four_e32():
    r64, e32, got = C.restated(), C.e32(), outputs_by_item()
    worst_spec = worst_wave = worst_e32 = 0.0
    failures = []
    for name, x, _ in C.items():
        spec, wave, _ = got[name]
        if not len(x):
            assert not spec.any() and not wave.any()
            continue
        fp64_bar = 2.0 * len(x) * 2.0 ** -53
        for r in range(len(C.RESOLUTIONS)):
            for w in range(3):
                err, bar = C.relative(spec[r, w], r64[name]["spec"][r, w]), 4.0 * e32[name]["spec"][r, w]
                worst_spec, worst_e32 = max(worst_spec, err), max(worst_e32, e32[name]["spec"][r, w])
                print(f"{name} res {r} {'d2 a2 l1'.split()[w]}: device {err:.3e}  e32 {e32[name]['spec'][r, w]:.3e}")
                if err > bar:
                    failures.append((name, r, w, err, bar))
        for w in range(2):
            err = C.relative(wave[w], r64[name]["wave"][w])
            worst_wave = max(worst_wave, err)
            print(f"{name} {'e2 x2'.split()[w]}: device {err:.3e}  bar {fp64_bar:.3e}")
            if err > fp64_bar:
                failures.append((name, "wave", w, err, fp64_bar))
    print(f"largest: spec {worst_spec:.3e} (e32 {worst_e32:.3e}), e2/x2 {worst_wave:.3e}")
    assert not failures, failures


def test_emax_is_numpys_float32_maximum_bit_for_bit():
    got = outputs_by_item()
    for name, x, y in C.items():
        if len(x):
            want = np.max(np.abs(x - y))
            assert want.dtype == np.float32 and got[name][1][2] == float(want) and np.float32(got[name][1][2]) == want, name


def test_measure_finishes_the_sums_as_the_restatement_does():
    dref, dtest = C.dense()
    rec = stage().measure(dref, dtest)
    assert rec.shape == (1,)
    spec, wave, frames = dense_outputs()
    want = R.finish({"spec": spec[0], "wave": wave[0], "frames": frames[0]}, C.RESOLUTIONS)
    for key in ("spectral_convergence", "log_stft_l1", "mr_spectral_convergence", "mr_log_stft_l1", "snr_db", "emax"):
        assert np.array_equal(np.asarray(rec[key][0]), np.asarray(want[key])), key
    same = stage().measure(dref, dref)[0]
    assert not same["spectral_convergence"].any() and not same["log_stft_l1"].any() and same["snr_db"] == np.inf and same["emax"] == 0.0


@pytest.fixture(scope="module")
def engine():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg), DEV)
    yield eng
    eng.close()


def test_compare_dtypes(engine):
    mel = torch.from_numpy(seeded_mel(3, 2, 24, log_mel=True)).to(DEV)
    sd = stage()
    same = sd.compare_dtypes(engine, mel, "f32", "f32")
    assert same.shape == (2,) and (same["frames"] == [[1 + 24 * 256 // hop for _, hop, _ in C.RESOLUTIONS]] * 2).all()
    assert not same["spectral_convergence"].any() and not same["log_stft_l1"].any() and not same["emax"].any()
    assert np.isinf(same["snr_db"]).all()
    ragged = sd.compare_dtypes(engine, mel, "f32", "f32", lengths=[24, 10])
    assert ragged["frames"][1].tolist() == [1 + 10 * 256 // hop for _, hop, _ in C.RESOLUTIONS] and not ragged["emax"].any()
    rec = sd.compare_dtypes(engine, mel, "f32", "bf16")
    by_hand = sd.measure(engine.forward(mel, dtype="f32"), engine.forward(mel, dtype="bf16"))
    assert rec.tobytes() == by_hand.tobytes()
    print("bf16 against f32:", {k: rec[k].tolist() for k in ("mr_spectral_convergence", "mr_log_stft_l1", "snr_db", "emax")})
    assert np.isfinite(rec["snr_db"]).all() and (rec["snr_db"] > 0).all()
    assert (rec["spectral_convergence"] > 0).all() and (rec["emax"] > 0).all()
