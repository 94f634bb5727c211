"""G.711 without a GPU: the two companding rules of include/iris_hifigan.h restated here in plain Python integers, sample by
sample, and held against ``iris.synthesis_output`` over all 65 536 int16 values; the properties the rules promise; the WAV
header of a G.711 file read back with ``struct``; and the refusals of the writer and the command line.  The device's bytes are
tests/test_gpu_g711.py's.

The contract is the rule, not a library: A-law equals CPython's ``audioop.lin2alaw`` everywhere (checked where it imports),
mu-law does not equal ``audioop.lin2ulaw`` -- that one shifts by 2 before it takes the sign -- and is not compared with it."""
import struct

import numpy as np
import pytest

from iris import synthesis_output as so

ALL = np.arange(-32768, 32768, dtype=np.int32)


def ulaw_rule(s: int) -> int:
    sign = 1 if s < 0 else 0
    m = min(abs(s), 32635) + 132
    e = m.bit_length() - 1 - 7
    mant = (m >> (e + 3)) & 15
    return ~(sign << 7 | e << 4 | mant) & 0xFF


def alaw_rule(s: int) -> int:
    a = s >> 3
    mask = 0xD5
    if a < 0:
        a, mask = ~a, 0x55
    seg = 0 if a < 32 else a.bit_length() - 1 - 4
    mant = (a >> 1) & 15 if seg < 2 else (a >> seg) & 15
    return (seg << 4 | mant) ^ mask


_codes = {}


def codes(law):
    if law not in _codes:
        rule = ulaw_rule if law == "ulaw" else alaw_rule
        _codes[law] = np.array([rule(int(s)) for s in ALL], dtype=np.uint8)
    return _codes[law]


ENCODE = {"ulaw": so.ulaw_from_pcm16, "alaw": so.alaw_from_pcm16}
DECODE = {"ulaw": so.pcm16_from_ulaw, "alaw": so.pcm16_from_alaw}


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_the_numpy_restatement_is_the_rule_on_every_sample(law):
    got = ENCODE[law](ALL.astype(np.int16))
    assert got.dtype == np.uint8 and np.array_equal(got, codes(law))
    assert np.array_equal(ENCODE[law](ALL.astype(np.int16).reshape(256, 256)), codes(law).reshape(256, 256))   # any shape


@pytest.mark.parametrize("law,zero,worst", [("ulaw", 0xFF, 644), ("alaw", 0xD5, 512)])
def test_properties_of_the_rules(law, zero, worst):
    code = codes(law)
    assert len(set(code.tolist())) == 256                                   # every code is used
    assert code[32768] == zero == so.G711_ZERO[law]                          # the code of sample 0
    decoded = DECODE[law](code).astype(np.int64)
    assert (np.diff(decoded) >= 0).all()                                     # decoding the codes of rising samples never falls
    err = np.abs(decoded - ALL)
    print(f"{law}: worst |decode(encode(s)) - s| = {int(err.max())} at s = {int(ALL[err.argmax()])}")
    assert int(err.max()) == worst and int(ALL[err.argmax()]) == -32768
    every = np.arange(256, dtype=np.uint8)
    back = ENCODE[law](DECODE[law](every))
    off = np.nonzero(back != every)[0].tolist()
    assert off == ([0x7F] if law == "ulaw" else [])                          # but for mu-law's negative zero
    assert int(DECODE[law](np.uint8(0))) == (-32124 if law == "ulaw" else -5504)   # byte 0 is no silence


def test_alaw_is_audioop_where_it_imports():
    audioop = pytest.importorskip("audioop")
    pcm = ALL.astype("<i2")
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(pcm.tobytes(), 2), dtype=np.uint8), codes("alaw"))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(np.arange(256, dtype=np.uint8).tobytes(), 2), dtype="<i2"),
                          so.pcm16_from_alaw(np.arange(256, dtype=np.uint8)))


def test_g711_from_float_is_the_law_of_the_pcm16_sample():
    w = np.concatenate([ALL[1:] / np.float32(32767.0), [-1.5, 1.5]]).astype(np.float32)
    pcm = so.pcm16_from_float(w)
    assert np.array_equal(pcm[:65535], ALL[1:])                              # s / 32767 comes back as s
    for law in ("ulaw", "alaw"):
        assert np.array_equal(so.g711_from_float(w, law), ENCODE[law](pcm))
    with pytest.raises(ValueError, match="encoding must be one of"):
        so.g711_from_float(w, "pcm16")


@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [0, 1, 160, 161])
def test_wav_header(tmp_path, law, tag, n):
    code = ENCODE[law]((np.arange(n) * 97 % 65536 - 32768).astype(np.int16))
    path = so.write_wav(tmp_path / f"{law}_{n}.wav", code, 8000, encoding=law)
    data = path.read_bytes()
    assert path.suffix == ".wav" and data == so.g711_wav_bytes(code, 8000, law)
    riff, size, wave_id = struct.unpack_from("<4sI4s", data, 0)
    assert (riff, wave_id) == (b"RIFF", b"WAVE") and size == len(data) - 8 and len(data) % 2 == 0
    fmt_id, fmt_len, fmt_tag, channels, rate, byte_rate, align, bits, cb = struct.unpack_from("<4sIHHIIHHH", data, 12)
    assert (fmt_id, fmt_len, fmt_tag, channels, rate, byte_rate, align, bits, cb) == (b"fmt ", 18, tag, 1, 8000, 8000, 1, 8, 0)
    fact_id, fact_len, samples = struct.unpack_from("<4sII", data, 12 + 8 + 18)
    assert (fact_id, fact_len, samples) == (b"fact", 4, n)
    data_id, data_len = struct.unpack_from("<4sI", data, 12 + 8 + 18 + 12)
    start = 12 + 8 + 18 + 12 + 8
    assert (data_id, data_len) == (b"data", n) and data[start:start + n] == code.tobytes()
    assert len(data) == start + n + (n & 1)                                  # the pad byte of an odd chunk


def test_writer_and_command_line_refusals(tmp_path):
    code = np.full(8, 0xFF, dtype=np.uint8)
    with pytest.raises(ValueError, match="G.711 bytes are a uint8 array"):
        so.write_wav(tmp_path / "a.wav", code, 8000)                        # bytes without a law
    with pytest.raises(ValueError, match="G.711 bytes are a uint8 array"):
        so.write_wav(tmp_path / "a.wav", np.zeros(8, dtype=np.float32), 8000, encoding="ulaw")
    with pytest.raises(ValueError, match="single waveform"):
        so.write_wav(tmp_path / "a.wav", np.full((2, 8), 0xFF, dtype=np.uint8), 8000, encoding="alaw")
    assert not (tmp_path / "a.wav").exists()
    # int16 and float keep going where they went
    assert so.write_wav(tmp_path / "p.wav", np.zeros(8, dtype=np.int16), 8000, encoding="pcm16").read_bytes()[20:22] == b"\x01\x00"
    parser = so.build_parser()
    assert parser.parse_args(["--mel", "m.npy"]).encoding is None
    assert parser.parse_args(["--mel", "m.npy", "--encoding", "ulaw", "--resample_to", "8000"]).encoding == "ulaw"
    for argv in (["--encoding", "g722"], ["--encoding", "ulaw", "--pcm16"], ["--encoding", "alaw", "--normalize_peak", "0.9"]):
        with pytest.raises(SystemExit):
            so.main(["--mel", str(tmp_path / "none.npy")] + argv)
    mel = np.zeros((80, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="normalize_peak does not go with a G.711 encoding"):
        so.vocode_to_wav(mel, tmp_path / "b.wav", normalize_peak=0.9, encoding="ulaw")
    with pytest.raises(ValueError, match="float waveform"):
        so.vocode_to_wav(mel, tmp_path / "b.wav", vocoder_entry=so.PCM16_VOCODER_ENTRY, encoding="alaw")
    with pytest.raises(ValueError, match="encoding must be"):
        so.vocode_to_wav(mel, tmp_path / "b.wav", encoding="f32")
