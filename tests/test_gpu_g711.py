"""G.711 on the device: the stand-alone op (``iris_hifigan_op_g711``, csrc/pcm_out.h: ``g711_kernel``) on every 16-bit sample and on
a ragged batch at odd addresses, so the scalar head and tail run beside the 16-byte loads; and the resampler's ragged G.711 form
against the host's encoding of its int16 form.  The rules are restated in numpy here (``ulaw_rule`` / ``alaw_rule``), not taken
from the package."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.resample import Resampler
from iris.synthesis_output import g711_on_device, pcm16_from_float

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LAWS = (("ulaw", 0xFF), ("alaw", 0xD5))
LENGTHS = (0, 1, 5, 1023)


def floor_log2(m):
    e = np.zeros_like(m)
    for k in range(1, 16):
        e += (m >> k) > 0
    return e


def ulaw_rule(s):
    s = np.asarray(s).astype(np.int32)
    m = np.minimum(np.abs(s), 32635) + 132
    e = floor_log2(m) - 7
    return (~((s < 0).astype(np.int32) << 7 | e << 4 | (m >> (e + 3)) & 15) & 0xFF).astype(np.uint8)


def alaw_rule(s):
    a = np.asarray(s).astype(np.int32) >> 3
    neg = a < 0
    a = np.where(neg, ~a, a)
    seg = np.where(a < 32, 0, floor_log2(np.maximum(a, 1)) - 4)
    mant = np.where(seg < 2, a >> 1, a >> seg) & 15
    return ((seg << 4 | mant) ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


RULE = {"ulaw": ulaw_rule, "alaw": alaw_rule}


@pytest.mark.parametrize("law,zero", LAWS)
def test_op_g711_on_every_sample(law, zero):
    s = np.arange(-32767, 32768, dtype=np.int32)
    w = (s / np.float32(32767.0)).astype(np.float32)
    assert np.array_equal(pcm16_from_float(w), s)                              # on the host first: s / 32767 comes back as s
    got = g711_on_device(torch.from_numpy(w[None]).to(DEV), law)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy()[0], RULE[law](s))
    # the ends of the clamp and the sample the division cannot reach
    edge = torch.tensor([[-1.0, -1.5, 1.5, 0.0, -0.0]], device=DEV)
    assert np.array_equal(g711_on_device(edge, law).cpu().numpy()[0], RULE[law]([-32767, -32767, 32767, 0, 0]))
    assert int(RULE[law]([0])[0]) == zero


def ragged_batch():
    rng = np.random.default_rng(711)
    wav = rng.uniform(-1.2, 1.2, (len(LENGTHS), 1023)).astype(np.float32)
    for b, n in enumerate(LENGTHS):
        wav[b, n:] = np.nan                                                    # never encoded: the padding is the code of 0
    return wav


@pytest.mark.parametrize("law,zero", LAWS)
@pytest.mark.parametrize("out_shift", [1, 2])
def test_op_g711_ragged_at_odd_addresses(law, zero, out_shift):
    """Rows of 1023 samples from float 1 of an aligned buffer: every row starts off 16 bytes, at another offset each.  With the
    bytes from byte 1 the two alignments agree (16-byte loads, 4-byte stores, a scalar head and tail); from byte 2 they do
    not, and the rows are scalar.  The bytes around the output stay as they were."""
    host = ragged_batch()
    B, L = host.shape
    buf = torch.zeros(1 + B * L + 3, dtype=torch.float32, device=DEV)
    wav = buf[1:1 + B * L].view(B, L)
    wav.copy_(torch.from_numpy(host))
    mark = 0x3C
    raw = torch.full((16 + out_shift + B * L + 16,), mark, dtype=torch.uint8, device=DEV)
    out = raw[16 + out_shift:16 + out_shift + B * L].view(B, L)
    assert buf.data_ptr() % 16 == 0 and raw.data_ptr() % 16 == 0 and wav.data_ptr() % 16 == 4 and out.data_ptr() % 4 == out_shift
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _native.check("iris_hifigan_op_g711", _native.load().iris_hifigan_op_g711(
            ctypes.c_void_p(wav.data_ptr()), B, L, ctypes.c_void_p(lengths.data_ptr()), 1, _native.OUT_FORMS[law],
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    got = out.cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert np.array_equal(got[b, :n], RULE[law](pcm16_from_float(host[b, :n]))), (law, b)
        assert (got[b, n:] == zero).all(), (law, b)                            # never byte 0
    edges = raw.cpu().numpy()
    assert (edges[:16 + out_shift] == mark).all() and (edges[16 + out_shift + B * L:] == mark).all()
    # the wrapper with lengths and without: rows of the whole length
    assert torch.equal(g711_on_device(wav, law, lengths=lengths), out)
    full = g711_on_device(wav[3:4], law).cpu().numpy()
    assert np.array_equal(full[0], RULE[law](pcm16_from_float(host[3])))


@pytest.mark.parametrize("law,zero", LAWS)
def test_resampler_forward_g711_ragged(law, zero):
    host = ragged_batch()
    rs = Resampler(8000, device=DEV)
    try:
        wav = torch.from_numpy(host).to(DEV)
        pcm = rs.forward(wav, lengths=list(LENGTHS), pcm16=True).cpu().numpy()
        got = rs.forward(wav, lengths=list(LENGTHS), encoding=law)
        assert got.dtype == torch.uint8 and got.shape == pcm.shape == (4, rs.out_range(0, 1023)[1])
        assert np.array_equal(got.cpu().numpy(), RULE[law](pcm))
        counts = [rs.out_range(0, n)[1] for n in LENGTHS]
        assert counts[0] == 0 and counts[1] == 1 and counts[3] == got.shape[1]
        for b, n in enumerate(counts):
            assert (got[b, n:] == zero).all()                                  # an item's row behind its own outputs: the code of 0
        assert np.abs(pcm[3]).max() > 8000 and len(set(got[3].tolist())) > 64  # a signal, not silence
    finally:
        rs.close()
