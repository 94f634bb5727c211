"""Ragged Griffin-Lim batches and the device-drawn start phase without a GPU: the numpy restatement of the Philox draw
(``iris.griffin_lim.philox4x32_10_np`` / ``philox_phase_np``) against known answers, the host logic of
``MelToWavePipeline.infer_batch`` with a whole-utterance vocoder that takes ``lengths``, the argument errors
``GriffinLim.forward_device(lengths=)`` raises before any device work, and the C-ABI's new symbols.  The device side is
tests/test_gpu_griffin_lim_ragged.py."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import griffin_lim as GL
from iris.griffin_lim import GriffinLim
from iris.pipeline import MelToWavePipeline


# ---- the Philox restatement --------------------------------------------------------------------------------------------
def _hex(words) -> str:
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_known_answers():
    """Random123's known answers for philox4x32-10 (its ``kat_vectors`` file: counter, key -> output), quoted from memory:
    no copy of that file was found in the ROCm installation this was written against.  What was found there is rocRAND's
    ``rocrand_philox4x32_10.h``, whose multipliers (0xD2511F53, 0xCD9E8D57) and Weyl constants (0x9E3779B9, 0xBB67AE85) are
    the ones used here; the third vector (digits of pi as counter and key) exercises every word of both."""
    kat = (
        ([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    )
    for counter, key, want in kat:
        assert _hex(GL.philox4x32_10_np(np.array(counter, dtype=np.uint64), key)) == want
    # vectorised over leading axes: the same words
    both = GL.philox4x32_10_np(np.array([kat[0][0], kat[0][0]], dtype=np.uint64), (0, 0))
    assert both.shape == (2, 4) and _hex(both[1]) == kat[0][2]


def test_counter_layout_of_the_draw():
    """Bin k of frame t of item s is output word k & 3 of counter (k >> 2, t, s, 0) under key (seed lo, seed hi)."""
    seed, item, bins, T = (0x12345678 << 32) | 0x9ABCDEF0, 5, 9, 3
    u = GL.philox_uniform_np(seed, item, bins, T)
    assert u.shape == (T, bins) and u.dtype == np.float32
    for t, k in ((0, 0), (2, 3), (1, 4), (2, 8)):
        words = GL.philox4x32_10_np(np.array([k >> 2, t, item, 0], dtype=np.uint64), (0x9ABCDEF0, 0x12345678))
        assert u[t, k] == np.float32(int(words[k & 3]) >> 8) * np.float32(2.0 ** -24)
    # a longer or wider draw starts with the shorter one: the counter knows no shape
    assert np.array_equal(GL.philox_uniform_np(seed, item, bins + 4, T + 2)[:T, :bins], u)


def test_uniforms_and_phase():
    u = GL.philox_uniform_np(1337, 0, 513, 64)
    assert (u >= 0.0).all() and (u < 1.0).all()
    assert 0.45 < float(u.mean()) < 0.55 and float(u.max()) > 0.99 and float(u.min()) < 0.01
    assert not np.array_equal(u, GL.philox_uniform_np(1337, 1, 513, 64))          # another item
    assert not np.array_equal(u, GL.philox_uniform_np(1338, 0, 513, 64))          # another seed (low word)
    assert not np.array_equal(u, GL.philox_uniform_np(1337 + (1 << 32), 0, 513, 64))      # another seed (high word)
    ph = GL.philox_phase_np(1337, 0, 513, 64)
    assert ph.shape == (64, 513, 2) and ph.dtype == np.float64
    ang = (np.float32(6.2831855) * u).astype(np.float64)                          # ONE fp32 product
    assert np.array_equal(ph[..., 0], np.cos(ang)) and np.array_equal(ph[..., 1], np.sin(ang))
    assert np.abs(ph[..., 0] ** 2 + ph[..., 1] ** 2 - 1.0).max() < 1e-15


# ---- host logic of the pipeline ----------------------------------------------------------------------------------------
class _RaggedWhole:
    """GriffinLim's call surface with ``takes_lengths``: hop (T - 1) samples a row, sample i of item b is the mean of frame
    i // hop up to its own hop (T_b - 1), 0 past them."""
    whole_utterance = True
    takes_lengths = True
    hop_length = 4

    def __init__(self):
        self.calls = []

    def forward_device(self, mel, lengths=None):
        self.calls.append(None if lengths is None else [int(n) for n in lengths])
        wav = mel.mean(dim=1)[:, :-1].repeat_interleave(self.hop_length, dim=1).clone()
        if lengths is not None:
            for b, n in enumerate(lengths):
                wav[b, self.hop_length * max(int(n) - 1, 0):] = 0.0
        return wav


class _Resampler:
    """``Resampler.forward`` / ``out_range``'s call surface: every second sample."""

    def __init__(self):
        self.calls = []

    def out_range(self, origin, L):
        return 0, (L + 1) // 2

    def forward(self, wav, lengths=None, row_scale=1, pcm16=False, normalize=False):
        self.calls.append((None if lengths is None else [int(n) for n in lengths], row_scale))
        out = wav[:, ::2]
        out = (out * 100).to(torch.int16) if pcm16 else out
        return (out, wav.abs().amax(dim=1)) if normalize else out


def _mels():
    mel = torch.arange(3 * 3 * 6, dtype=torch.float32).reshape(3, 3, 6) + 1.0
    return [mel[0], mel[1][:, :4], mel[2][:, :2]]


def test_pipeline_ragged_route_lengths_and_slicing():
    voc = _RaggedWhole()
    pipe = MelToWavePipeline(None, voc)
    mels = _mels()
    outs = pipe.infer_batch(mels)
    assert voc.calls == [[6, 4, 2]]                                   # ONE call with the items' frame counts
    assert [tuple(o.shape) for o in outs] == [(20,), (12,), (4,)]
    for o, m in zip(outs, mels):
        assert torch.equal(o, pipe.infer(m[None])[0])
    # a PostNet gets the same lengths, once
    seen = []
    refine = lambda mel, lengths=None: (seen.append(None if lengths is None else list(lengths)), mel + 1)[1]
    outs = MelToWavePipeline(refine, _RaggedWhole()).infer_batch(mels)
    assert seen == [[6, 4, 2]] and torch.equal(outs[1], voc.forward_device(mels[1][None] + 1)[0])
    # equal lengths go the same way, so item i stays its own infer
    voc.calls.clear()
    same = pipe.infer_batch([mels[0], mels[0] * 2])
    assert voc.calls == [[6, 6]] and torch.equal(same[1], pipe.infer(mels[0][None] * 2)[0])
    assert pipe.infer_batch([]) == []


def test_pipeline_ragged_route_output_stages():
    voc, rs = _RaggedWhole(), _Resampler()
    pipe = MelToWavePipeline(None, voc)
    mels = _mels()
    plain = pipe.infer_batch(mels)
    outs = pipe.infer_batch(mels, resampler=rs)
    assert rs.calls == [([5, 3, 1], 4)]                               # T_i - 1 rows of hop samples each
    assert [tuple(o.shape) for o in outs] == [(10,), (6,), (2,)]
    assert all(torch.equal(o, p[::2]) for o, p in zip(outs, plain))
    pcm = pipe.infer_batch(mels, resampler=rs, pcm16=True)
    assert all(o.dtype == torch.int16 and torch.equal(o, (p[::2] * 100).to(torch.int16)) for o, p in zip(pcm, plain))
    norm = pipe.infer_batch(mels, resampler=rs, pcm16=True, normalize=True)      # (pcm, peaks): the list is cut from pcm
    assert len(norm) == 3 and all(torch.equal(o, q) for o, q in zip(norm, pcm))
    with pytest.raises(ValueError, match="normalize=True goes with pcm16=True"):
        pipe.infer_batch(mels, normalize=True)


def test_a_vocoder_without_takes_lengths_is_still_refused():
    class Plain(_RaggedWhole):
        takes_lengths = False

    mels = _mels()
    for voc in (Plain(), GriffinLim(n_iter=1)):
        if isinstance(voc, GriffinLim):
            mels = [torch.zeros(80, 6), torch.zeros(80, 4)]
        with pytest.raises(NotImplementedError, match="one length"):
            MelToWavePipeline(None, voc).infer_batch(mels)
    assert GriffinLim().takes_lengths is False and GriffinLim(ragged=True).takes_lengths is True
    assert GriffinLim().phase == "host" and GriffinLim(phase="device").phase == "device"
    with pytest.raises(ValueError, match="phase must be"):
        GriffinLim(phase="gpu")


# ---- argument errors (raised before any device is asked for) -----------------------------------------------------------
@pytest.mark.parametrize("lengths,text", [
    ([33, 1], "= 1"),                                   # one frame has no sample
    ([33, -2], "outside"),
    ([34, 33], "outside"),
    ([33.0, 20.0], "integers"),
    ([33], "one per item"),
    ([[33, 20]], "one per item"),
    (torch.tensor([33, 20], dtype=torch.float32), "integers"),
])
def test_length_errors(lengths, text):
    gl = GriffinLim(ragged=True)
    with pytest.raises(ValueError, match=text):
        gl.forward_device(np.zeros((2, 80, 33), np.float32), lengths=lengths)
    assert gl._handle is None


def test_other_argument_errors():
    gl = GriffinLim()
    lm = np.zeros((2, 80, 33), np.float32)
    for kw in (dict(phase0="host"), dict(phase0="device", seed=-1), dict(phase0="device", seed=2 ** 64),
               dict(phase0="device", first_item=-1), dict(phase0="device", first_item=2 ** 31 - 2), dict(phase0="device", seed=1.5)):
        with pytest.raises(ValueError):
            gl.forward_device(lm, **kw)
    for args in ((1, 1), (-1, 33), (1, 33, -1), (1, 33, 0, -1)):
        with pytest.raises(ValueError):
            gl.draw_phase(*args)
    assert gl._handle is None
    assert np.array_equal(GL.check_lengths([0, 2, 33], 3, 33), np.array([0, 2, 33], dtype=np.int32))
    assert GL.check_lengths(np.array([33, 0], dtype=np.int64), 2, 33).dtype == np.int32


def test_host_phase_of_a_ragged_call_is_each_items_own_draw():
    gl = GriffinLim(n_fft=64, hop_length=16, win_length=48, n_mels=12, sample_rate=8000, fmax=None)
    packed = gl._ragged_host_phase(np.array([5, 0, 3, 5], dtype=np.int32), 7, seed=11)
    assert packed.shape == (4, 7, 33, 2) and packed.dtype == np.float32
    for b, n in enumerate((5, 0, 3, 5)):
        assert (packed[b, n:] == 0).all()
        if n:
            assert np.array_equal(packed[b, :n], GL.pack_phase(GL.start_phase(1, 33, n, 11))[0])
    assert not np.array_equal(packed[2, :3], GL.pack_phase(GL.start_phase(4, 33, 7, 11))[2, :3])     # not a slice of the dense draw


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_refusals_without_a_device():
    lib = _native.load()
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION
    for name in ("iris_griffin_lim_forward_ragged", "iris_griffin_lim_draw_phase"):
        assert name in _native.GRIFFIN_LIM_SYMBOLS and hasattr(lib, name)
    assert len(_native.GRIFFIN_LIM_SYMBOLS["iris_griffin_lim_forward_ragged"][1]) == 12
    assert len(_native.GRIFFIN_LIM_SYMBOLS["iris_griffin_lim_draw_phase"][1]) == 7
    header = (Path(__file__).resolve().parents[1] / "include" / "iris_hifigan.h").read_text()
    assert "int32_t iris_griffin_lim_forward_ragged(" in header and "int32_t iris_griffin_lim_draw_phase(" in header
    assert ctypes.sizeof(_native.GriffinLimConfig) == 64              # the config struct is the dense call's, unchanged
    null = ctypes.c_void_p(None)
    assert lib.iris_griffin_lim_forward_ragged(null, null, null, 1337, 0, 1, 33, null, null, null, 0, null) == _native.STATUS_INVALID_ARGUMENT
    assert "NULL handle" in lib.iris_hifigan_last_error().decode()
    assert lib.iris_griffin_lim_draw_phase(null, 1337, 0, 1, 33, null, null) == _native.STATUS_INVALID_ARGUMENT
    # the launch count and the workspace are the dense call's: no launch is added
    gl = GriffinLim()
    assert gl.launch_count(8, 1024) == 2 * 60 + 2
