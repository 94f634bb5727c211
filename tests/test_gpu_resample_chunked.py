"""The chunked resampler on the device: a ``ResamplerSession`` against ``Resampler.forward`` of the whole in all four store forms,
raw ``forward_window`` calls against the numpy restatement, the library's own window plan against its closed form, and a real
pipeline that streams 8 kHz mu-law behind a chunked denoiser, stretch and limiter.  Every comparison is an equality of bits."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.denoiser import Denoiser
from iris.limiter import Limiter
from iris.pipeline import MelToWavePipeline
from iris.resample import Resampler, ResamplerSession, resample_host, window_plan
from iris.synthesis_output import alaw_from_pcm16, pcm16_from_float, ulaw_from_pcm16
from iris.time_stretch import TimeStretch
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENCODINGS = (("f32", torch.float32), ("pcm16", torch.int16), ("ulaw", torch.uint8), ("alaw", torch.uint8))
_state = {}


def model(rate) -> Resampler:
    if rate not in _state:
        _state[rate] = Resampler(rate, device=DEV)
    return _state[rate]


def ceil_div(a, b):
    return -((-a) // b)


def utterance(B, L, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, L)).astype(np.float32)


def same(x: torch.Tensor, y: torch.Tensor) -> bool:
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


@pytest.mark.parametrize("rate,L,outputs", [(8000, 6000, 2177), (48000, 3000, 6531)])
def test_windows_equal_the_whole_call_in_every_form(rate, L, outputs):
    """2177 outputs at 8 kHz are three kernel blocks of 1024, and the pushes cut elsewhere: block edges and window seams fall in
    different places."""
    rs = model(rate)
    hw = rs.half_width
    wav = torch.from_numpy(utterance(2, L, rate)).to(DEV)
    pieces = [700, 1, 1500, 0, L - 2201]
    assert rs.out_range(0, L) == (0, outputs)
    for enc, dtype in ENCODINGS:
        want = rs.forward(wav, encoding=enc)
        assert want.dtype == dtype and want.shape == (2, outputs)
        session, got, at = rs.open_session(enc), [], 0
        for n in pieces:
            got.append(session.push(wav[:, at:at + n]))
            at += n
            assert session.samples_emitted == ceil_div(max(0, at - hw) * rs.up, rs.down)
            assert session.samples_buffered <= 2 * hw + ceil_div(rs.down, rs.up) + n
        got.append(session.flush())
        assert got[3].shape == (2, 0) and got[-1].shape[1] > 0 and session.samples_buffered == 0
        assert same(torch.cat(got, dim=1), want), (rate, enc)
    # encoding= says what pcm16= says, and the G.711 forms are the law of the int16 form
    pcm = rs.forward(wav, pcm16=True)
    assert same(rs.forward(wav, encoding="pcm16"), pcm) and same(rs.forward(wav, encoding="f32"), rs.forward(wav))
    assert np.array_equal(rs.forward(wav, encoding="ulaw").cpu().numpy(), ulaw_from_pcm16(pcm.cpu().numpy()))
    assert np.array_equal(rs.forward(wav, encoding="alaw").cpu().numpy(), alaw_from_pcm16(pcm.cpu().numpy()))
    with pytest.raises(ValueError, match="no normalised form"):
        rs.forward(wav, pcm16=True, normalize=True, encoding="ulaw")


@pytest.mark.parametrize("rate", [8000, 48000])
def test_forward_window_against_the_numpy_restatement(rate):
    """One interior window (neither end is an end of the utterance) and one final window, at origins off any multiple of 4."""
    rs = model(rate)
    bank, up, down, hw = _bank(rate), rs.up, rs.down, rs.half_width
    host = utterance(2, 2600, rate + 1)
    for origin, Lw, final in ((1001, 1203, False), (1397, 1203, True)):
        n_next = ceil_div((origin + hw - 1) * up, down) + 2                    # its first tap lies inside the window
        window = host[:, origin:origin + Lw]
        n_hi, keep = rs.window_plan(origin, Lw, n_next, final)
        assert (n_hi, keep) == window_plan(up, down, hw, origin, Lw, n_next, final)
        assert n_hi == ceil_div((origin + Lw - (0 if final else hw)) * up, down) and n_hi - n_next > 300
        n_lo = ceil_div(origin * up, down)
        want = resample_host(window, bank, up, down, origin=origin)[:, n_next - n_lo:n_hi - n_lo]
        got = rs.forward_window(torch.from_numpy(window.copy()).to(DEV), origin, n_next, final)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (rate, origin)
        if not final:                                                          # ... and those are the whole utterance's samples
            whole = resample_host(host, bank, up, down)
            assert np.array_equal(want.view(np.uint32), whole[:, n_next:n_hi].view(np.uint32))
        for enc, fn in (("pcm16", pcm16_from_float), ("ulaw", lambda y: ulaw_from_pcm16(pcm16_from_float(y))),
                        ("alaw", lambda y: alaw_from_pcm16(pcm16_from_float(y)))):
            got = rs.forward_window(torch.from_numpy(window.copy()).to(DEV), origin, n_next, final, encoding=enc)
            assert np.array_equal(got.cpu().numpy(), fn(want)), (rate, origin, enc)


def _bank(rate):
    from iris.resample import design_bank
    return design_bank(rate)[0]


def test_window_refusals_and_windows_that_emit_nothing():
    rs = model(8000)
    hw, inv = rs.half_width, _native.STATUS_INVALID_ARGUMENT
    wav = torch.from_numpy(utterance(2, 1000, 3)).to(DEV)

    def status(fn, *args, **kw):
        with pytest.raises(_native.NativeCallError) as err:
            fn(*args, **kw)
        return err.value.status

    assert status(rs.window_plan, 5, 1000, 0, False) == inv                    # output 0 reads in front of sample 5
    assert status(rs.forward_window, wav, 5, 0, False) == inv
    assert status(rs.window_plan, -1, 10, 0, False) == inv and status(rs.window_plan, 0, -1, 0, False) == inv
    assert status(rs.window_plan, 0, 1000, -1, False) == inv
    assert status(rs.window_plan, 0, 1000, rs.out_range(0, 1000)[1] + 1, True) == inv      # past the window's last output
    out = torch.full((2, 400), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        raw = _native.load().iris_resampler_forward_window
        stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        args = (rs._handle, ctypes.c_void_p(wav.data_ptr()), 2, 1000, 0, 0, 0)
        assert raw(*args, ctypes.c_void_p(out.data_ptr()), 2, stream) == inv                # no normalised form
        assert raw(*args, None, _native.OUT_F32, stream) == inv
        assert raw(*args, ctypes.c_void_p(out.data_ptr() + 2), _native.OUT_F32, stream) == inv   # fp32 off 4 bytes
        # nothing is final yet: OK, and nothing is launched -- not even with no output to write to
        assert raw(rs._handle, ctypes.c_void_p(wav.data_ptr()), 2, hw, 0, 0, 0, None, _native.OUT_F32, stream) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                              # no refused call launched
    assert rs.window_plan(0, hw, 0, False) == (0, 0) and rs.forward_window(wav[:, :hw], 0, 0, False).shape == (2, 0)
    assert rs.window_plan(0, 0, 0, True) == (0, 0)
    far = (1 << 40) - 1000                                                     # 64-bit origins
    assert rs.window_plan(far, 1000, ceil_div((far + hw) * rs.up, rs.down), True)[0] == ceil_div((1 << 40) * rs.up, rs.down)


def test_pipeline_streams_telephony_bytes():
    from iris._engine import GeneratorEngine
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), DEV, dtype="f32")
    try:
        dn = Denoiser(1024, 256, 1024, strength=0.5, bias=np.full(513, 0.5, dtype=np.float32), device=DEV)
        ts = TimeStretch(1024, 256, device=DEV)
        lm = Limiter(22050, ceiling_dbtp=-12.0, lookahead_ms=1.5, device=DEV)
        rs = model(8000)
        mel = torch.from_numpy(seeded_mel(3, 1, 40, log_mel=True)).to(DEV)
        kw = dict(device=DEV, chunk_frames=16)
        stages = dict(denoiser=dn.chunked(), stretch=ts.at(0.8).chunked(), limiter=lm.chunked())
        pipe = MelToWavePipeline(None, eng.forward, output=rs.chunked("ulaw"), **stages, **kw)
        want = pipe.infer(mel)
        fp32 = MelToWavePipeline(None, eng.forward, **stages, **kw).infer(mel)
        assert want.dtype == torch.uint8 and want.shape == (1, rs.out_range(0, fp32.shape[1])[1])
        assert torch.equal(want, rs.forward(fp32, encoding="ulaw"))
        assert len(set(want[0].tolist())) > 32                                  # speech-like: many codes, not silence
        pieces = list(pipe.stream(mel))
        assert all(p.shape[1] > 0 and p.dtype == torch.uint8 for p in pieces) and len(pieces) >= 3
        assert torch.equal(torch.cat(pieces, dim=1), want)
        session, got, at = pipe.session(), [], 0
        for t in (7, 1, 0, 20, 12):
            got += session.push(mel[:, :, at:at + t])
            at += t
        assert torch.equal(torch.cat(got + session.flush(), dim=1), want)
        # directly behind the vocoder, as 16-bit PCM at 8 kHz
        only = MelToWavePipeline(None, eng.forward, output=rs.chunked("pcm16"), **kw)
        want16 = only.infer(mel)
        assert want16.dtype == torch.int16 and torch.equal(want16, rs.forward(MelToWavePipeline(None, eng.forward, **kw).infer(mel), pcm16=True))
        assert torch.equal(torch.cat(list(only.stream(mel)), dim=1), want16)
        assert torch.equal(only.infer_batch([mel[0]])[0], want16[0])
        with pytest.raises(ValueError, match="output=: it decides the rate and the encoding"):
            only.infer(mel, pcm16=True)
    finally:
        eng.close()
