"""The sample-rate conversion stage (iris_resampler_*, csrc/resample.h, iris/resample.py): everything that needs no GPU.

The reference never resamples, so the contract is the filter of include/iris_hifigan.h: the library's host-only design
against the formula in numpy float64, the output ranges of consecutive windows, the host restatement against a float64
evaluation of the same fp32 bank, a tone through the designed filter, and the argument rules."""
import ctypes
import ctypes.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "iris-tts_amd")]

from iris import _native, resample, synthesis_output  # noqa: E402

RATE_IN = 22050
RATES = (8000, 11025, 16000, 24000, 44100, 48000)
ZEROS, BETA, ROLLOFF = 16, 9.0, 0.945


def formula_bank(rate_out, rate_in=RATE_IN, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """The bank of include/iris_hifigan.h in numpy float64 (np.i0 for the Bessel function)."""
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    s = min(1.0, up / down)
    fc = rolloff * s
    hw = int(math.ceil(zeros / s))
    taps = 2 * hw
    j = np.arange(taps, dtype=np.float64)[None, :]
    p = np.arange(up, dtype=np.float64)[:, None]
    t = (j - hw + 1) - p / up
    inside = np.abs(t) <= hw
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / hw) ** 2, 0.0, None))) / np.i0(beta)
    bank = np.where(inside, fc * np.sinc(fc * t) * win, 0.0)
    return bank, up, down, hw


@pytest.mark.parametrize("rate_out", RATES)
def test_design_matches_the_formula(rate_out):
    want, up, down, hw = formula_bank(rate_out)
    bank, got_up, got_down = resample.design_bank(rate_out)
    assert (got_up, got_down, bank.shape) == (up, down, (up, 2 * hw))
    assert bank.dtype == np.float32
    err = float(np.abs(bank.astype(np.float64) - want).max())
    dc = float(np.abs(bank.astype(np.float64).sum(axis=1) - 1.0).max())
    print(f"{rate_out}: up {up} down {down} taps {2 * hw}, max coefficient error {err:.3e}, DC deviation {dc:.3e}")
    assert np.abs(want).max() <= 1.0
    assert err <= 2.0 ** -23
    assert dc <= 2e-5


def test_design_takes_other_parameters():
    want, up, down, hw = formula_bank(16000, zeros=7, beta=6.5, rolloff=0.9)
    bank, got_up, got_down = resample.design_bank(16000, zeros=7, beta=6.5, rolloff=0.9)
    assert (got_up, got_down, bank.shape) == (up, down, (up, 2 * hw))
    assert np.abs(bank.astype(np.float64) - want).max() <= 2.0 ** -23
    other, _, down2 = resample.design_bank(16000, rate_in=44100)
    assert down2 == 441 and other.shape[0] == 160


def test_out_range_partitions_consecutive_windows():
    rng = np.random.default_rng(7)
    for rate_out in RATES:
        _, up, down = resample.design_bank(rate_out)
        for _ in range(40):
            origin = int(rng.integers(0, 1 << 36))
            cuts = np.sort(rng.integers(0, 50000, size=int(rng.integers(1, 6))))
            edges = [0, *map(int, cuts), 50000]
            lo0, total = resample.out_range(up, down, origin, 50000)
            nxt, count = lo0, 0
            for a, b in zip(edges[:-1], edges[1:]):
                lo, n = resample.out_range(up, down, origin + a, b - a)
                assert lo == nxt and n >= 0                     # adjacent: no gap, no overlap
                nxt, count = lo + n, count + n
            assert count == total
        for L in (1, 2, 255, 4099):
            assert resample.out_range(up, down, 0, L) == (0, -(-L * up // down))
        # every output of a range sits inside its window, the neighbours outside
        lo, n = resample.out_range(up, down, 12345, 777)
        assert 12345 * up <= lo * down and (lo - 1) * down < 12345 * up
        assert (lo + n - 1) * down < (12345 + 777) * up <= (lo + n) * down
        # positions near 2^31 / down and beyond 2^32 do not wrap
        for origin in ((1 << 31) // down - 1, (1 << 31) // down + 1, (1 << 31) + 5, (1 << 33) + 11):
            lo, n = resample.out_range(up, down, origin, 1000)
            assert lo == -(-origin * up // down) and lo + n == -(-(origin + 1000) * up // down)


def test_fmaf32_is_libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, 6000).astype(np.float32)
    b = rng.uniform(-1, 1, 6000).astype(np.float32)
    c = (rng.uniform(-1, 1, 6000) * 10.0 ** rng.integers(-8, 2, 6000)).astype(np.float32)
    # products exactly halfway between two float32 (1 + (k + 1) 2^-12 + k 2^-24, k odd) plus a term below float64's
    # resolution: a float64 add returns the halfway point and the second rounding then goes to even, whatever c's sign
    a[:2000] = (1.0 + (2 * rng.integers(0, 1 << 11, 2000) + 1) * 2.0 ** -12).astype(np.float32)
    b[:2000] = np.float32(1.0 + 2.0 ** -12)
    c[:2000] = (2.0 ** -60 * rng.choice([-1.0, 1.0], 2000)).astype(np.float32)
    c[2000:2100] = 0.0
    a[2100:2200] = 0.0
    got = resample.fmaf32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(twice, want)          # the inputs do contain double-rounding cases


@pytest.mark.parametrize("rate_out", (8000, 16000, 44100, 48000))
def test_resample_host_within_the_chain_bound(rate_out):
    bank, up, down = resample.design_bank(rate_out)
    taps = bank.shape[1]
    hw = taps // 2
    rng = np.random.default_rng(rate_out)
    L, origin = 700, 1234567
    wav = rng.uniform(-1, 1, (2, L)).astype(np.float32)
    got = resample.resample_host(wav, bank, up, down, origin=origin)
    n_lo, n = resample.out_range(up, down, origin, L)
    assert got.shape == (2, n) and got.dtype == np.float32
    q = (np.arange(n, dtype=np.int64) + n_lo) * down
    idx = (q // up - hw + 1 - origin)[:, None] + np.arange(taps)[None, :]
    ok = (idx >= 0) & (idx < L)
    rows = bank[q % up].astype(np.float64)
    worst = 0.0
    for b in range(2):
        x = np.where(ok, wav[b, np.clip(idx, 0, L - 1)], 0.0).astype(np.float64)
        exact = (x * rows).sum(axis=1)
        bound = taps * 2.0 ** -24 * np.abs(x * rows).sum(axis=1)
        err = np.abs(got[b].astype(np.float64) - exact)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    print(f"{rate_out}: largest error / bound = {worst:.3f}")
    # ragged: an item is its own samples alone, zeros behind its own outputs
    own = np.array([L, 333])
    ragged = resample.resample_host(np.where(np.arange(L) < own[:, None], wav, np.nan), bank, up, down, lengths=own, origin=origin)
    alone = resample.resample_host(wav[1:2, :333], bank, up, down, origin=origin)
    assert np.array_equal(ragged[0], got[0]) and np.array_equal(ragged[1, :alone.shape[1]], alone[0])
    assert not ragged[1, alone.shape[1]:].any() and np.isfinite(ragged).all()


@pytest.mark.parametrize("rate_out", RATES)
def test_tones_through_the_designed_filter(rate_out):
    bank, up, down = resample.design_bank(rate_out)
    bank = bank.astype(np.float64)
    taps = bank.shape[1]
    hw = taps // 2
    L = 6000
    n = -(-L * up // down)
    q = np.arange(n, dtype=np.int64) * down
    idx = (q // up - hw + 1)[:, None] + np.arange(taps)[None, :]
    ok = (idx >= 0) & (idx < L)
    rows = bank[q % up]
    skip = int(math.ceil(2 * hw * up / down))
    tones = [100.0, 1000.0, 3000.0, 0.8 * min(RATE_IN, rate_out) / 2]
    for f in tones:
        x = np.sin(2 * np.pi * f * np.arange(L) / RATE_IN)
        y = (np.where(ok, x[np.clip(idx, 0, L - 1)], 0.0) * rows).sum(axis=1)
        want = np.sin(2 * np.pi * f * np.arange(n) / rate_out)
        err = float(np.abs(y - want)[skip:n - skip].max())
        print(f"{rate_out} Hz, tone {f:.0f} Hz: max interior error {err:.3e}")
        assert n - 2 * skip > 500
        assert err <= 5e-3


def test_argument_errors_and_limits():
    lib = _native.load()
    assert set(_native.RESAMPLER_SYMBOLS) == {"iris_resampler_design", "iris_resampler_create", "iris_resampler_destroy",
                                              "iris_resampler_info", "iris_resampler_out_range", "iris_resampler_forward"}
    assert lib.iris_hifigan_abi_version() == 4
    up, down, taps = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()

    def design(rate_in, rate_out, zeros=0, beta=0.0, rolloff=0.0, bank=None, capacity=0):
        return lib.iris_resampler_design(rate_in, rate_out, zeros, beta, rolloff, ctypes.byref(up), ctypes.byref(down),
                                         ctypes.byref(taps), bank, capacity)

    for rate, want_taps in ((8000, 90), (11025, 64), (16000, 46), (24000, 32), (32000, 32), (44100, 32), (48000, 32)):
        assert design(RATE_IN, rate) == 0
        assert taps.value == want_taps and up.value * taps.value * 4 <= 80 * 1024       # (32 000: 640 phases)
    inv, uns = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    assert design(RATE_IN, RATE_IN) == inv
    assert design(RATE_IN, 0) == inv and design(0, 16000) == inv
    assert design(RATE_IN, 16000, zeros=-1) == inv
    assert design(RATE_IN, 16000, beta=-1.0) == inv
    assert design(RATE_IN, 16000, rolloff=-0.5) == inv and design(RATE_IN, 16000, rolloff=1.5) == inv
    assert design(RATE_IN, 3999) == uns and design(RATE_IN, 192001) == uns
    assert design(RATE_IN, 22051) == uns                 # up = 22051 > 640
    assert design(RATE_IN, 4000, zeros=32) == uns        # taps = 2 * ceil(32 * 441 / 80) > 256
    assert b"rate_out" in lib.iris_hifigan_last_error()
    assert design(RATE_IN, 4000) == 0 and taps.value == 2 * 89
    small = (ctypes.c_float * 8)()
    assert design(RATE_IN, 16000, bank=small, capacity=8) == inv
    assert lib.iris_resampler_design(RATE_IN, 16000, 0, 0.0, 0.0, None, None, None, None, 0) == inv
    assert lib.iris_resampler_destroy(None) == 0
    with pytest.raises(_native.NativeCallError) as exc:
        resample.design_bank(RATE_IN)
    assert exc.value.status == inv


def test_cli_resample_to(tmp_path, monkeypatch):
    args = synthesis_output.build_parser().parse_args(["--mel", "m.npy", "--resample_to", "16000"])
    assert args.resample_to == 16000 and args.sample_rate == 22050
    assert synthesis_output.build_parser().parse_args(["--mel", "m.npy"]).resample_to is None
    for bad in ("3999", "192001", "-1"):
        with pytest.raises(SystemExit):
            synthesis_output.main(["--mel", "m.npy", "--resample_to", bad])
    with pytest.raises(SystemExit):
        synthesis_output.build_parser().parse_args(["--mel", "m.npy", "--resample_to", "16k"])
    with pytest.raises(ValueError):
        synthesis_output.check_resample_to(16000.5)

    # the entry receives sample_rate_out, --sample_rate stays a label, and the WAV header carries the new rate
    calls = {}

    def entry(mel, sample_rate, hop_length, sample_rate_out=None):
        calls.update(sample_rate=sample_rate, sample_rate_out=sample_rate_out)
        return np.zeros(1600, dtype=np.float32)

    monkeypatch.setattr(synthesis_output, "resolve_vocoder_entry", lambda spec: entry)
    mel_path, wav_path = tmp_path / "m.npy", tmp_path / "o.wav"
    np.save(mel_path, np.zeros((80, 4), dtype=np.float32))
    assert synthesis_output.main(["--mel", str(mel_path), "--output_wav", str(wav_path), "--resample_to", "16000"]) == 0
    assert calls == {"sample_rate": 22050, "sample_rate_out": 16000}
    import wave
    written = wav_path if wav_path.exists() else None
    assert written is not None
    try:
        with wave.open(str(written), "rb") as w:
            assert w.getframerate() == 16000 and w.getnframes() == 1600
    except wave.Error:                                   # (soundfile wrote a subtype `wave` does not read)
        import soundfile as sf
        assert sf.info(str(written)).samplerate == 16000


class _FakeEngine:
    """A 'generator' without context (every frame becomes `hop` samples of its first mel bin) and the host restatement
    behind it: the chunk arithmetic of StreamingVocoder(resampler=) on the CPU."""

    class cfg:
        hop_length = 4
        upsample_rates = (2, 2)
        upsample_kernel_sizes = (4, 4)
        resblock_kernel_sizes = (3,)
        resblock_dilation_sizes = ((1,),)

    def __init__(self, rate_out):
        self.bank, self.up, self.down = resample.design_bank(rate_out)
        self.half_width = self.bank.shape[1] // 2

    def out_range(self, origin, L):
        return resample.out_range(self.up, self.down, origin, L)

    def forward(self, mel):
        return np.repeat(mel[:, 0, :], 4, axis=1).astype(np.float32)

    def forward_resampled(self, mel, resampler, origin_frames=0):
        return resample.resample_host(self.forward(mel), self.bank, self.up, self.down, origin=origin_frames * 4)


@pytest.mark.parametrize("rate_out", (16000, 48000))
def test_streaming_chunks_partition_the_resampled_output(rate_out):
    from iris.streaming import StreamingVocoder, receptive_field_frames
    eng = _FakeEngine(rate_out)
    mel = np.random.default_rng(2).uniform(-1, 1, (2, 3, 103)).astype(np.float32)
    one_shot = eng.forward_resampled(mel, eng)
    need = receptive_field_frames(eng.cfg, extra_samples=eng.half_width)
    assert need * 4 >= eng.half_width and need > receptive_field_frames(eng.cfg)
    for group in (1, 3):
        sv = StreamingVocoder(eng.forward, chunk_frames=16, group_chunks=group, resampler=eng)
        assert sv.halo_frames == need
        chunks = list(sv.stream(mel))
        assert len(chunks) == 7
        for k, c in enumerate(chunks):                      # chunk k is outputs n_lo(16 k hop) .. n_lo(16 (k + 1) hop) - 1
            lo, hi = eng.out_range(16 * k * 4, 0)[0], eng.out_range(min(16 * (k + 1), 103) * 4, 0)[0]
            assert c.shape[1] == hi - lo
        assert np.array_equal(np.concatenate(chunks, axis=1).view(np.uint32), one_shot.view(np.uint32))
    with pytest.raises(ValueError):
        StreamingVocoder(eng.forward, chunk_frames=16, halo_frames=1, resampler=eng)           # Hw > halo * hop
    with pytest.raises(ValueError):
        StreamingVocoder(lambda m: m, chunk_frames=16, resampler=eng)
    # the default stays today's path
    plain = StreamingVocoder(eng.forward, hop_length=4, chunk_frames=16, halo_frames=13)
    assert plain.resampler is None and np.array_equal(plain.infer(mel), eng.forward(mel))
