"""The sample-rate conversion stage on the device (iris_resampler_forward, csrc/resample.h).  The reference never resamples,
so every comparison is exact against the host restatement ``iris.resample.resample_host`` (the same fp32 bank, an exact
fmaf chain), ``synthesis_output.pcm16_from_float`` for the int16 forms, and the stage composed by hand for the engine,
the chunked vocoder and the drop-in entry point."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.resample import Resampler, design_bank, resample_host
from iris.streaming import StreamingVocoder
from iris.synthesis_output import pcm16_from_float
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
V1 = GeneratorConfig()
HOP = 256


def _wave(seed, B, L):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, L)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(
        got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want)


@pytest.fixture(scope="module")
def rs16():
    rs = Resampler(16000, device=DEV)
    yield rs
    rs.close()


@pytest.fixture(scope="module")
def engine():
    from iris._engine import GeneratorEngine
    eng = GeneratorEngine(V1, seeded_state_dict(V1, seed=11, gain=1.1, post_gain=10.0), DEV)
    yield eng
    eng.close()


@pytest.mark.parametrize("rate_out", (8000, 16000, 44100, 48000, 11025))
def test_device_equals_host_bit_for_bit(rate_out):
    bank, up, down = design_bank(rate_out)
    rs = Resampler(rate_out, device=DEV)
    assert (rs.up, rs.down, rs.taps, rs.half_width) == (up, down, bank.shape[1], bank.shape[1] // 2)
    hw = rs.half_width
    lengths = sorted({1, 2, hw - 1, hw, 255, 1023, 1025, 4099})
    for B in (1, 3):
        for L in lengths:
            wav = _wave(1000 * B + L, B, L)
            wav_dev = _dev(wav)
            for origin in (0, 7, 3328 * 5 + 3, 2 ** 33 + 11):
                got = rs.forward(wav_dev, origin=origin)
                want = resample_host(wav, bank, up, down, origin=origin)
                assert rs.out_range(origin, L)[1] == want.shape[1]
                assert _same_bits(got, want), (rate_out, B, L, origin)
    rs.close()


def test_other_filter_parameters_and_unaligned_rows():
    bank, up, down = design_bank(16000, zeros=5, beta=6.5, rolloff=0.9)
    rs = Resampler(16000, device=DEV, zeros=5, beta=6.5, rolloff=0.9)
    assert rs.taps == bank.shape[1] and rs.taps % 4 == 2          # the two-coefficient tail of a bank row
    wav = _wave(5, 3, 1025)                                       # odd L: items 1 and 2 start off a 16-byte boundary
    assert _same_bits(rs.forward(_dev(wav), origin=7), resample_host(wav, bank, up, down, origin=7))
    # a caller's own pointer, one float past a 16-byte boundary
    flat = _dev(np.concatenate([np.zeros(1, np.float32), wav[0]]))
    assert _same_bits(rs.forward(flat[1:].view(1, -1)), resample_host(wav[:1], bank, up, down))
    rs.close()


@pytest.mark.parametrize("rate_out", (16000, 48000))
def test_ragged_items(rate_out):
    bank, up, down = design_bank(rate_out)
    rs = Resampler(rate_out, device=DEV)
    B, L = 4, 2048
    for own, lengths, row_scale in (([2048, 777, 1, 0], [2048, 777, 1, 0], 1), ([2048, 768, 256, 0], [8, 3, 1, 0], 256)):
        wav = _wave(21, B, L)
        for b in range(B):
            wav[b, own[b]:] = np.nan
        wav_dev = _dev(wav)
        for origin in (0, 3328 * 5 + 3):
            got = rs.forward(wav_dev, lengths=lengths, row_scale=row_scale, origin=origin).cpu().numpy()
            assert np.isfinite(got).all()
            assert _same_bits(got, resample_host(wav, bank, up, down, lengths=own, origin=origin))
            for b in range(B):
                if own[b] == 0:
                    assert not got[b].any()
                    continue
                alone = rs.forward(wav_dev[b:b + 1, :own[b]].contiguous(), origin=origin).cpu().numpy()
                n = alone.shape[1]
                assert np.array_equal(got[b, :n].view(np.uint32), alone[0].view(np.uint32)) and not got[b, n:].any()
    rs.close()


@pytest.mark.parametrize("rate_out", (16000, 48000))
def test_windows_concatenate_to_the_one_shot(rate_out):
    rs = Resampler(rate_out, device=DEV)
    wav_dev = _dev(_wave(8, 1, 6000))
    whole = rs.forward(wav_dev)
    ctx = rs.half_width + 64
    parts = []
    for start in range(0, 6000, 1500):
        lo, hi = max(0, start - ctx), min(6000, start + 1500 + ctx)
        out = rs.forward(wav_dev[:, lo:hi].contiguous(), origin=lo)
        first = rs.out_range(lo, 0)[0]
        a, n = rs.out_range(start, 1500)
        parts.append(out[:, a - first:a - first + n])
    assert torch.equal(torch.cat(parts, dim=1).view(torch.int32), whole.view(torch.int32))
    rs.close()


def test_output_forms(rs16):
    bank, up, down = design_bank(16000)
    wav = _wave(30, 3, 3001) * np.array([[1.0], [0.3], [1.4]], dtype=np.float32)
    for own in (None, [3001, 500, 0]):
        host = resample_host(wav, bank, up, down, lengths=own, origin=7)
        kw = dict(lengths=own, origin=7)
        assert _same_bits(rs16.forward(_dev(wav), pcm16=True, **kw), pcm16_from_float(host).astype(np.int16))
        pcm, peaks = rs16.forward(_dev(wav), pcm16=True, normalize=True, peak_target=0.9, **kw)
        assert _same_bits(pcm, pcm16_from_float(host, normalize=True, peak_target=0.9).astype(np.int16))
        assert _same_bits(peaks, np.abs(host).max(axis=1))
        if own is not None:
            assert float(peaks[2]) == 0.0 and not pcm[2].any()


def test_engine_chunks_and_entry_point(engine, rs16, tmp_path):
    T = 70
    mel = torch.from_numpy(seeded_mel(3, 2, T, n_mels=V1.in_channels, log_mel=True)).to(DEV)
    before = engine.forward(mel).clone()
    for dtype in ("f32", "bf16", "f32s"):
        want = rs16.forward(engine.forward(mel, dtype=dtype).clone())
        got = engine.forward_resampled(mel, rs16, dtype=dtype)
        assert got.shape == (2, rs16.out_range(0, T * HOP)[1])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), dtype
    lengths = [70, 33]
    want = rs16.forward(engine.forward(mel, dtype="f32", lengths=lengths).clone(), lengths=lengths, row_scale=HOP)
    got = engine.forward_resampled(mel, rs16, dtype="f32", lengths=lengths)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not got[1, rs16.out_range(0, 33 * HOP)[1]:].any()
    for dtype in ("bf16", "f32s"):
        with pytest.raises(_native.NativeCallError) as exc:
            engine.forward_resampled(mel, rs16, dtype=dtype, lengths=lengths)
        assert exc.value.status == _native.STATUS_UNSUPPORTED
    # a window of a longer mel carries its origin
    shifted = engine.forward_resampled(mel, rs16, origin_frames=5)
    assert torch.equal(shifted.view(torch.int32), rs16.forward(before, origin=5 * HOP).view(torch.int32))
    one_shot = engine.forward_resampled(mel, rs16).clone()
    for group in (1, 3):
        sv = StreamingVocoder(engine.forward, chunk_frames=16, group_chunks=group, config=V1, resampler=rs16)
        chunks = list(sv.stream(mel))
        assert len(chunks) == 5
        assert torch.equal(torch.cat(chunks, dim=1).view(torch.int32), one_shot.view(torch.int32)), group
        assert torch.equal(sv.infer(mel).view(torch.int32), one_shot.view(torch.int32))
    with pytest.raises(ValueError):
        StreamingVocoder(engine.forward, chunk_frames=16, halo_frames=0, config=V1, resampler=rs16)
    with pytest.raises(ValueError):
        StreamingVocoder(lambda m: engine.forward(m), chunk_frames=16, resampler=rs16)
    assert torch.equal(engine.forward(mel).view(torch.int32), before.view(torch.int32))       # the stage leaves no state behind

    import iris.hifigan_pretrained as hp
    ck = tmp_path / "g.ckpt"
    torch.save({k: torch.from_numpy(v) for k, v in seeded_state_dict(V1, seed=4).items()}, ck)
    m = seeded_mel(9, 1, 24, log_mel=True)[0]
    plain = hp.infer_hifigan(m, checkpoint_path=ck)
    res = hp.infer_hifigan(m, 22050, 256, ck, sample_rate_out=16000)
    assert res.ndim == 1 and res.dtype == np.float32
    assert _same_bits(res, rs16.forward(_dev(plain[None])).cpu().numpy()[0])
    pcm = hp.infer_hifigan_pcm16(m, checkpoint_path=ck, sample_rate_out=16000)
    assert np.array_equal(pcm, pcm16_from_float(res))


def test_pipeline_takes_a_resampler(engine, rs16):
    from iris.pipeline import MelToWavePipeline
    pipe = MelToWavePipeline(None, engine.forward, device=DEV, chunk_frames=16)
    mel = torch.from_numpy(seeded_mel(5, 1, 40, n_mels=V1.in_channels, log_mel=True)).to(DEV)
    one_shot = engine.forward_resampled(mel, rs16).clone()
    assert torch.equal(pipe.infer(mel, resampler=rs16).view(torch.int32), one_shot.view(torch.int32))
    assert torch.equal(pipe.infer(mel, pcm16=True, resampler=rs16), engine.forward_resampled(mel, rs16, pcm16=True))
    mels = [mel[0], mel[0, :, :17]]
    outs = pipe.infer_batch(mels, resampler=rs16)
    assert torch.equal(outs[0].view(torch.int32), one_shot[0].view(torch.int32))
    short = engine.forward_resampled(mel[:, :, :17].contiguous(), rs16)
    assert torch.equal(outs[1].view(torch.int32), short[0].view(torch.int32))


def test_cabi_errors_and_capture(engine, rs16):
    lib = _native.load()
    wav = _dev(_wave(1, 2, 512))
    n = rs16.out_range(0, 512)[1]
    out = torch.empty((2, n), dtype=torch.float32, device=DEV)
    pcm = torch.empty((2, n), dtype=torch.int16, device=DEV)
    peak = torch.empty((2,), dtype=torch.float32, device=DEV)

    def call(wav_p, B, L, out_p, pcm_p, peak_p, normalize=0, target=0.95, origin=0):
        return lib.iris_resampler_forward(rs16._handle, wav_p, B, L, None, 1, origin, out_p, pcm_p, peak_p, normalize,
                                          ctypes.c_float(target), None)

    w, o, p, k = wav.data_ptr(), out.data_ptr(), pcm.data_ptr(), peak.data_ptr()
    inv, uns = _native.STATUS_INVALID_ARGUMENT, _native.STATUS_UNSUPPORTED
    assert call(None, 2, 512, o, None, None) == inv
    assert call(w, 2, 512, None, None, None) == inv
    assert call(w, 2, 512, None, p, k, normalize=1) == inv            # normalising without the fp32 output
    assert call(w, 2, 512, o, p, None, normalize=1) == inv            # ... without the peaks
    for target in (0.0, -0.5, 1.5, float("nan")):
        assert call(w, 2, 512, o, p, k, normalize=1, target=target) == inv
    assert call(w, 2, 512, o, None, None, origin=-1) == inv
    assert call(w, 65536, 512, o, None, None) == uns
    assert call(None, 0, 512, None, None, None) == 0 and call(None, 2, 0, None, None, None) == 0
    torch.cuda.synchronize()
    h = ctypes.c_void_p()
    assert lib.iris_resampler_create(22050, 22050, 0, 0.0, 0.0, ctypes.byref(h)) == inv
    assert lib.iris_resampler_create(22050, 3999, 0, 0.0, 0.0, ctypes.byref(h)) == uns
    assert lib.iris_resampler_create(22050, 192001, 0, 0.0, 0.0, ctypes.byref(h)) == uns
    with pytest.raises(_native.NativeCallError):
        Resampler(22050, device=DEV)

    # one forward_resampled inside a capture replays to the eager bits
    mel = torch.from_numpy(seeded_mel(6, 1, 30, n_mels=V1.in_channels, log_mel=True)).to(DEV)
    eager = engine.forward_resampled(mel, rs16).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = engine.forward_resampled(mel, rs16)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int32), eager.view(torch.int32))
