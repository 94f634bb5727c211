"""The output stage, host side: ``pcm16_from_float`` (the float32 restatement of what the device computes, and what the GPU
tests compare against), int16 WAV writing, the CLI flags and the checks of ``forward_pcm16`` that need no device."""
import ctypes
import wave

import numpy as np
import pytest
import torch

from iris import _native
from iris import synthesis_output as so
from iris._weights import GeneratorConfig


def test_pcm16_plain_hand_cases():
    f = np.float32
    got = so.pcm16_from_float(np.array([1.0, -1.0, 0.0, 2.5, -7.0, np.inf, -np.inf, 0.5, 1e-9], np.float32))
    # 0.5 * 32767 = 16383.5 exactly: a tie, to even
    assert got.tolist() == [32767, -32767, 0, 32767, -32767, 32767, -32767, 16384, 0]
    assert got.dtype == np.dtype("<i2")
    # exact .5 ties go to the even neighbour, both signs (k + 0.5) / 32767 is not exact in general, so build the ties
    # from products that are: x = (2k + 1) / 2 / 32767 only ties if the product rounds to k + 0.5 -- check that first
    for k in (0, 1, 2, 3, 100, 101, 16382, 16383):
        x = f(f(k + 0.5) / f(32767.0))
        if f(x * f(32767.0)) != f(k + 0.5):
            continue
        even = k if k % 2 == 0 else k + 1
        assert so.pcm16_from_float(np.array([x, -x], np.float32)).tolist() == [even, -even], k
    assert so.pcm16_from_float(np.array([f(0.5), f(-0.5)])).tolist() == [16384, -16384]      # 16383.5 -> 16384
    # shape is kept; float64 input is cast first
    assert so.pcm16_from_float(np.zeros((2, 3), np.float64)).shape == (2, 3)


def test_pcm16_normalised_hand_cases():
    f = np.float32
    w = np.array([[0.25, -0.5, 0.125], [0.0, 0.0, 0.0], [2.0, -4.0, 1.0]], np.float32)
    got = so.pcm16_from_float(w, normalize=True, peak_target=1.0)
    for b in range(3):
        peak = np.abs(w[b]).max()
        q = (w[b] / (f(peak) + f(1e-8))) * f(1.0)
        want = np.round(np.clip(q, -1, 1) * f(32767.0)).astype(np.int16)
        assert got[b].tolist() == want.tolist()
    assert got[1].tolist() == [0, 0, 0]                          # a silent item stays silent
    assert got[0, 1] == -32767 and got[2, 1] == -32767           # (0.5 + 1e-8 rounds to 0.5 in float32)
    # per item: a 1-D call on the row gives the row
    assert np.array_equal(so.pcm16_from_float(w[0], normalize=True, peak_target=1.0), got[0])
    # the default target is the reference demo's 0.95
    d = so.pcm16_from_float(w[0], normalize=True)
    assert d[1] == np.round(f(f(-0.5) / (f(0.5) + f(1e-8))) * f(0.95) * f(32767.0))
    assert so.pcm16_from_float(np.zeros((0,), np.float32), normalize=True).shape == (0,)
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            so.pcm16_from_float(w, normalize=True, peak_target=bad)
    so.pcm16_from_float(w, normalize=False, peak_target=7.0)     # ignored without normalize


def _frames(path):
    with wave.open(str(path), "rb") as r:
        return r.getnchannels(), r.getsampwidth(), r.getframerate(), r.readframes(r.getnframes())


def test_write_wav_int16_is_verbatim(tmp_path):
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, size=4001).astype(np.int16)
    p = so.write_wav(tmp_path / "a.wav", pcm, 16000)
    assert p.suffix == ".wav"
    assert _frames(p) == (1, 2, 16000, pcm.astype("<i2").tobytes())
    p2 = so.write_wav(tmp_path / "b.wav", pcm[None, :], 22050)              # [1, samples] squeezes like float input
    assert _frames(p2)[3] == pcm.astype("<i2").tobytes()


def test_write_wav_float_bytes_unchanged(tmp_path, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "soundfile", None)          # the standard-library path, whatever is installed
    rng = np.random.default_rng(4)
    audio = (rng.standard_normal(5000) * 0.6).astype(np.float32)
    audio[:4] = [1.0, -1.0, 0.5, -0.5]
    before = np.round(np.clip(audio, -1.0, 1.0) * 32767.0).astype("<i2")     # write_wav's formula before pcm16_from_float
    p = so.write_wav(tmp_path / "f.wav", audio, 22050)
    assert _frames(p) == (1, 2, 22050, before.tobytes())
    assert np.array_equal(so.pcm16_from_float(audio), before)


def test_cli_flags_parse():
    parser = so.build_parser()
    a = parser.parse_args(["--mel", "m.npy"])
    assert a.pcm16 is False and a.normalize_peak is None and a.vocoder_entry == so.DEFAULT_VOCODER_ENTRY
    a = parser.parse_args(["--mel", "m.npy", "--pcm16", "--normalize_peak", "0.9"])
    assert a.pcm16 is True and a.normalize_peak == pytest.approx(0.9)
    with pytest.raises(SystemExit):
        so.main(["--mel", "m.npy", "--normalize_peak", "1.5"])
    from iris import hifigan_pretrained as hp
    assert so.resolve_vocoder_entry(so.PCM16_VOCODER_ENTRY) is hp.infer_hifigan_pcm16
    assert hp.infer_hifigan_pcm16.returns_pcm16 is True


def test_vocode_to_wav_keeps_int16(tmp_path, monkeypatch):
    import sys
    import types
    mod = types.ModuleType("pcm_entry_for_test")
    calls = []

    def entry(mel, sample_rate, hop_length, normalize=False, peak_target=0.95):
        calls.append((normalize, peak_target))
        return np.arange(-5, 5, dtype=np.int16)[None, :]

    entry.returns_pcm16 = True
    mod.entry = entry
    mod.float_entry = lambda mel, sr, hop: np.array([0.5, -0.25], np.float32)
    monkeypatch.setitem(sys.modules, "pcm_entry_for_test", mod)
    out = so.vocode_to_wav(np.zeros((80, 3), np.float32), tmp_path / "o.wav", "pcm_entry_for_test:entry", 8000, 256)
    assert out.dtype == np.int16 and out.shape == (10,)
    assert _frames(tmp_path / "o.wav")[3] == np.arange(-5, 5, dtype="<i2").tobytes()
    so.vocode_to_wav(np.zeros((80, 3), np.float32), tmp_path / "n.wav", "pcm_entry_for_test:entry", 8000, 256, normalize_peak=0.5)
    assert calls == [(False, 0.95), (True, 0.5)]
    # a float entry is normalised on the host
    out = so.vocode_to_wav(np.zeros((80, 3), np.float32), tmp_path / "h.wav", "pcm_entry_for_test:float_entry", 8000, 256,
                           normalize_peak=1.0)
    assert out.tolist() == so.pcm16_from_float(np.array([0.5, -0.25], np.float32), True, 1.0).tolist()


def test_symbols_declared_and_exported():
    assert {"iris_hifigan_forward_pcm16", "iris_hifigan_op_pcm16"} <= set(_native.SYMBOLS)
    lib = _native.load()
    assert hasattr(lib, "iris_hifigan_forward_pcm16") and hasattr(lib, "iris_hifigan_op_pcm16")
    assert lib.iris_hifigan_abi_version() == 4


def test_cabi_argument_checks_without_device():
    lib = _native.load()
    null = ctypes.c_void_p(None)
    # NULL handle
    assert lib.iris_hifigan_forward_pcm16(null, null, 1, 1, null, null, null, null, 0, ctypes.c_float(0.95), null, 0,
                                          _native.DTYPE_F32, null) == _native.STATUS_INVALID_ARGUMENT
    one = ctypes.c_void_p(256)                       # never dereferenced: the checks come first
    assert lib.iris_hifigan_op_pcm16(null, null, 1, one, null, 1, 4, 0, ctypes.c_float(0.95), null) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_hifigan_op_pcm16(one, null, 1, one, null, 1, 4, 1, ctypes.c_float(0.95), null) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_hifigan_op_pcm16(one, null, 1, one, one, 0, 4, 0, ctypes.c_float(0.95), null) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_hifigan_op_pcm16(one, null, 0, one, one, 1, 4, 0, ctypes.c_float(0.95), null) == _native.STATUS_INVALID_ARGUMENT
    for bad in (0.0, 1.5, -1.0, float("nan")):
        assert lib.iris_hifigan_op_pcm16(one, null, 1, one, one, 1, 4, 1, ctypes.c_float(bad), null) == _native.STATUS_INVALID_ARGUMENT


def test_forward_pcm16_argument_validation_without_device():
    from iris._engine import GeneratorEngine
    eng = GeneratorEngine.__new__(GeneratorEngine)          # no device: only the checks in front of the first launch run
    eng.cfg = GeneratorConfig()
    eng.default_dtype = "f32"
    eng.device = torch.device("cpu")
    eng.hop_length = 256
    eng._handle = None
    mel = torch.zeros((1, 80, 4))
    with pytest.raises(ValueError, match="expected mel"):
        eng.forward_pcm16(torch.zeros((1, 79, 4)))
    with pytest.raises(ValueError, match="expected mel"):
        eng.forward_pcm16(torch.zeros((80, 4)))
    with pytest.raises(ValueError, match="dtype"):
        eng.forward_pcm16(mel, dtype="fp16")
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="peak_target"):
            eng.forward_pcm16(mel, normalize=True, peak_target=bad)
    with pytest.raises(ValueError, match="lengths"):
        eng.forward_pcm16(mel, lengths=[5])
    with pytest.raises(ValueError, match="out must be"):
        eng.forward_pcm16(mel, out=torch.zeros((1, 1024), dtype=torch.float32))
    with pytest.raises(ValueError, match="wav goes with"):
        eng.forward_pcm16(mel, wav=torch.zeros((1, 1024), dtype=torch.float32))
    # an empty input needs no launch
    out = eng.forward_pcm16(torch.zeros((0, 80, 4)))
    assert out.shape == (0, 1024) and out.dtype == torch.int16
    pcm, peaks = eng.forward_pcm16(torch.zeros((2, 80, 0)), normalize=True)
    assert pcm.shape == (2, 0) and peaks.tolist() == [0.0, 0.0]


def test_plain_forward_plan_keeps_its_conv_post():
    """The plain forward launches the conv_post it always launched (the PCM forms are other instantiations)."""
    for dtype in (_native.DTYPE_F32, _native.DTYPE_BF16, _native.DTYPE_F32_SPLIT):
        for B, T in ((1, 1), (3, 40), (1, 1000)):
            assert _native.describe_plan(GeneratorConfig(), B, T, dtype)["launches"][-1]["kernel"] == "conv_post_rows_kernel"
    odd = GeneratorConfig(in_channels=20, upsample_rates=(3, 3), upsample_kernel_sizes=(5, 5), upsample_initial_channel=48,
                          resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))
    assert _native.describe_plan(odd, 3, 1)["launches"][-1]["kernel"] == "conv_post_tanh_kernel<0>"
