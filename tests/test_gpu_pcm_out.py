"""The output stage on the device (iris_hifigan_forward_pcm16, csrc/pcm_out.h): 16-bit PCM stored by conv_post, and
per-item peak-normalised PCM.  Every comparison is exact: plain PCM against the formula applied to ``engine.forward``'s
fp32 waveform, normalised PCM against ``synthesis_output.pcm16_from_float`` (float32 numpy), peaks against ``abs().max()``."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris.pipeline import MelToWavePipeline
from iris.streaming import StreamingVocoder
from iris.synthesis_output import pcm16_from_float
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict

pytestmark = pytest.mark.gpu

HOP = 256
V1 = GeneratorConfig()
# two conv pairs per ResBlock: the bf16 forward's last pair cannot be the summing one, conv_post reads three bf16 tensors
V1_EVEN = GeneratorConfig(resblock_dilation_sizes=((1, 3), (1, 3), (1, 3)))
# last stage C = 12 (the scalar conv_post), hop 9 (items of T = 1 start at odd sample offsets)
ODD_C12 = GeneratorConfig(in_channels=20, upsample_rates=(3, 3), upsample_kernel_sizes=(5, 5), upsample_initial_channel=48,
                          resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))
# last stage C = 16 (the 16-byte-staging conv_post), hop 9
ODD_C16 = GeneratorConfig(in_channels=20, upsample_rates=(3, 3), upsample_kernel_sizes=(5, 5), upsample_initial_channel=64,
                          resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))
# last stage C = 24: the bf16 path's own scalar conv_post (conv_post_tanh_bf16_kernel)
B16_C24 = GeneratorConfig(in_channels=16, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=96,
                          resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))


def _engine(cfg, post_gain=10.0):
    from iris._engine import GeneratorEngine
    return GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=post_gain), torch.device("cuda", 0))


@pytest.fixture(scope="module")
def engine():
    eng = _engine(V1)
    yield eng
    eng.close()


def _mel(cfg, seed, B, T, dev):
    return torch.from_numpy(seeded_mel(seed, B, T, n_mels=cfg.in_channels, log_mel=True)).to(dev)


def _formula(w):
    return torch.round(torch.clamp(w, -1, 1) * 32767).to(torch.int16)


def _check_all_forms(eng, mel, dtype, lengths=None, targets=(0.95,)):
    """Plain and normalised PCM of one input against engine.forward; returns the fp32 waveform."""
    w = eng.forward(mel, dtype=dtype, lengths=lengths).clone()
    pcm = eng.forward_pcm16(mel, dtype=dtype, lengths=lengths)
    assert pcm.dtype == torch.int16 and pcm.shape == w.shape
    assert torch.equal(pcm, _formula(w)), "plain PCM differs from the formula on forward's output"
    for target in targets:
        wav = torch.full_like(w, float("nan"))
        npcm, peaks = eng.forward_pcm16(mel, dtype=dtype, lengths=lengths, normalize=True, peak_target=target, wav=wav)
        assert torch.equal(wav, w), "the normalising call's waveform differs from forward's"
        assert torch.equal(peaks, w.abs().amax(dim=1)), "peaks differ from abs().max()"
        want = pcm16_from_float(w.cpu().numpy(), normalize=True, peak_target=target)
        assert np.array_equal(npcm.cpu().numpy(), want), f"normalised PCM (target {target}) differs from pcm16_from_float"
    return w


# ---- plain and normalised PCM of whole forwards ------------------------------------------------------------
def test_bf16_cases_reach_both_conv_post_inputs():
    """V1 (three pairs per ResBlock) ends in the summing pair's fp32 mean; the two-pair variant in three bf16 tensors."""
    for B, T in ((1, 1), (1, 5), (3, 40), (4, 100)):
        a = [l["kernel"] for l in _native.describe_plan(V1, B, T, _native.DTYPE_BF16)["launches"]]
        b = [l["kernel"] for l in _native.describe_plan(V1_EVEN, B, T, _native.DTYPE_BF16)["launches"]]
        assert a[-2:] == ["mrf_pair_bf16_sum_kernel", "conv_post_rows_kernel"], a[-2:]
        assert b[-2].startswith("mrf_pair_bf16_kernel") and b[-1] == "conv_post_rows_kernel", b[-2:]


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
def test_v1_pcm_equals_formula(engine, dtype):
    for B, T in ((1, 1), (1, 5), (3, 40), (4, 100)):
        mel = _mel(V1, 40 + B + T, B, T, engine.device)
        w = _check_all_forms(engine, mel, dtype, targets=(0.95, 1.0))
        assert w.abs().max() > 0


def test_bf16_three_input_conv_post():
    eng = _engine(V1_EVEN)
    for B, T in ((1, 5), (3, 40)):
        _check_all_forms(eng, _mel(V1_EVEN, 5 + T, B, T, eng.device), "bf16")
    eng.close()


def test_bf16_scalar_conv_post():
    assert _native.describe_plan(B16_C24, 3, 70, _native.DTYPE_BF16)["launches"][-1]["kernel"] == "conv_post_tanh_bf16_kernel"
    eng = _engine(B16_C24)
    for B, T in ((1, 1), (3, 70)):                       # 280 samples: two conv_post blocks per item
        _check_all_forms(eng, _mel(B16_C24, 9 + T, B, T, eng.device), "bf16")
    eng.close()


@pytest.mark.parametrize("cfg,name", [(ODD_C12, "conv_post_tanh_kernel<0>"), (ODD_C16, "conv_post_rows_kernel")],
                         ids=["C12-scalar", "C16-rows"])
def test_generic_configs_odd_hop(cfg, name):
    assert cfg.hop_length == 9
    assert _native.describe_plan(cfg, 3, 1)["launches"][-1]["kernel"] == name
    eng = _engine(cfg)
    for B, T in ((3, 1), (3, 31), (2, 57)):              # 9, 279 (two blocks) and 513 (three) samples per item, all odd
        w = _check_all_forms(eng, _mel(cfg, 3 + T, B, T, eng.device), "f32", targets=(0.95, 1.0))
        assert w.shape == (B, 9 * T)
    # ragged, with NaN in the padding
    mel = _mel(cfg, 8, 4, 31, eng.device)
    lengths = [31, 0, 1, 30]
    for b, n in enumerate(lengths):
        mel[b, :, n:] = float("nan")
    _check_all_forms(eng, mel, "f32", lengths=lengths)
    eng.close()


def test_sub_batch_passes(engine):
    """70 x 1000 frames run as two passes (65 + 5 items): every buffer advances per pass."""
    assert _native.describe_plan(V1, 70, 1000)["passes"] == 2
    mel = _mel(V1, 170, 70, 1000, engine.device)
    w = engine.forward(mel, dtype="f32")
    pcm = engine.forward_pcm16(mel, dtype="f32")
    assert torch.equal(pcm, _formula(w))
    del pcm
    wav = torch.empty_like(w)
    npcm, peaks = engine.forward_pcm16(mel, dtype="f32", normalize=True, wav=wav)
    assert torch.equal(wav, w)
    assert torch.equal(peaks, w.abs().amax(dim=1))
    for b in (0, 64, 65, 69):                            # the items on either side of the pass boundary
        assert np.array_equal(npcm[b].cpu().numpy(), pcm16_from_float(w[b].cpu().numpy(), normalize=True)), b


# ---- ragged ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,lengths", [(5, [5, 0, 1, 3]), (100, [100, 0, 1, 37])], ids=["T5", "T100"])
def test_ragged(engine, T, lengths):
    dev = engine.device
    mel = _mel(V1, 60 + T, 4, T, dev)
    alone = [engine.forward_pcm16(mel[b:b + 1, :, :n].contiguous(), dtype="f32")[0].clone() if n else None
             for b, n in enumerate(lengths)]
    alone_n = [engine.forward_pcm16(mel[b:b + 1, :, :n].contiguous(), dtype="f32", normalize=True) if n else None
               for b, n in enumerate(lengths)]
    for b, n in enumerate(lengths):
        mel[b, :, n:] = float("nan")
    _check_all_forms(engine, mel, "f32", lengths=lengths, targets=(0.95, 1.0))
    pcm = engine.forward_pcm16(mel, dtype="f32", lengths=lengths)
    npcm, peaks = engine.forward_pcm16(mel, dtype="f32", lengths=lengths, normalize=True)
    for b, n in enumerate(lengths):
        assert not pcm[b, HOP * n:].any() and not npcm[b, HOP * n:].any(), f"item {b}: PCM past its length is not 0"
        if n:
            assert torch.equal(pcm[b, :HOP * n], alone[b]), f"item {b} differs from forward_pcm16 of the item alone"
            assert torch.equal(npcm[b, :HOP * n], alone_n[b][0][0]) and peaks[b] == alone_n[b][1][0]
        else:
            assert peaks[b] == 0


def test_ragged_needs_fp32(engine):
    mel = _mel(V1, 3, 2, 40, engine.device)
    for dtype in ("bf16", "f32s"):
        with pytest.raises(_native.NativeCallError) as err:
            engine.forward_pcm16(mel, dtype=dtype, lengths=[40, 20])
        assert err.value.status == _native.STATUS_UNSUPPORTED


def test_normalised_calls_repeat(engine):
    """The peaks are re-zeroed by every call: a loud utterance does not leak into the next, quieter one."""
    loud = _mel(V1, 1, 2, 40, engine.device)
    quiet = loud - 6.0
    first = engine.forward_pcm16(loud, dtype="f32", normalize=True)
    a = engine.forward_pcm16(quiet, dtype="f32", normalize=True)
    b = engine.forward_pcm16(quiet, dtype="f32", normalize=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    wq = engine.forward(quiet, dtype="f32")
    assert torch.equal(a[1], wq.abs().amax(dim=1))
    # the same buffers reused: out= and a stale peak
    again = engine.forward_pcm16(loud, dtype="f32", normalize=True, out=a[0])
    assert again[0] is a[0] and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


# ---- the stand-alone kernels -------------------------------------------------------------------------------
def _op_pcm16(wav, lengths, row_scale, normalize, target, B, L):
    lib = _native.load()
    dev = wav.device
    pcm = torch.full((B * L + 8,), 12345, dtype=torch.int16, device=dev)         # guard samples behind the output
    peak = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    ldev = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    _native.check("iris_hifigan_op_pcm16", lib.iris_hifigan_op_pcm16(
        ctypes.c_void_p(wav.data_ptr()), ctypes.c_void_p(ldev.data_ptr() if ldev is not None else None), row_scale,
        ctypes.c_void_p(pcm.data_ptr()), ctypes.c_void_p(peak.data_ptr()), B, L, int(normalize), ctypes.c_float(target),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    assert (pcm[B * L:] == 12345).all(), "wrote past the output"
    return pcm[:B * L].view(B, L).cpu().numpy(), peak.cpu().numpy()


@pytest.mark.parametrize("L", [1, 3, 4, 255, 256, 257, 1025])
def test_op_pcm16(L):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(L)
    for B in (1, 3):                                     # B = 3 with odd L: unaligned item starts
        w = (rng.standard_normal((B, L)) * 0.7).astype(np.float32)
        w.flat[::7] = 0.5                                # ties: 0.5 * 32767 = 16383.5
        w.flat[::11] *= 3.0                              # beyond +-1
        wav = torch.from_numpy(w).to(dev)
        for lengths, scale in ((None, 1), ([L, 0, 1][:B], 1), ([(L + 1) // 2] * B, 2), ([max(L // 3, 0)] * B, 3)):
            n = [L] * B if lengths is None else [min(L, v * scale) for v in lengths]
            for normalize, target in ((False, 0.95), (True, 0.95), (True, 1.0)):
                got, peak = _op_pcm16(wav, lengths, scale, normalize, target, B, L)
                for b in range(B):
                    want = np.zeros((L,), np.int16)
                    want[:n[b]] = pcm16_from_float(w[b, :n[b]], normalize=normalize, peak_target=target)
                    assert np.array_equal(got[b], want), (B, L, lengths, scale, normalize, target, b)
                    if normalize:
                        assert peak[b] == (np.abs(w[b, :n[b]]).max() if n[b] else 0.0)


def test_op_pcm16_unaligned_base():
    """A caller's own pointers: the waveform and the PCM buffer start at different offsets from their 16- / 8-byte boundaries."""
    dev = torch.device("cuda", 0)
    lib = _native.load()
    L, B = 301, 2
    w = (np.random.default_rng(9).standard_normal((B * L + 3,)) * 0.8).astype(np.float32)
    wav = torch.from_numpy(w).to(dev)
    pcm = torch.zeros((B * L + 5,), dtype=torch.int16, device=dev)
    for woff, poff in ((1, 1), (1, 3), (3, 0), (2, 2)):
        pcm.fill_(777)
        _native.check("iris_hifigan_op_pcm16", lib.iris_hifigan_op_pcm16(
            ctypes.c_void_p(wav.data_ptr() + 4 * woff), None, 1, ctypes.c_void_p(pcm.data_ptr() + 2 * poff), None, B, L, 0,
            ctypes.c_float(0.95), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        got = pcm.cpu().numpy()
        assert np.array_equal(got[poff:poff + B * L], pcm16_from_float(w[woff:woff + B * L]))
        assert (got[:poff] == 777).all() and (got[poff + B * L:] == 777).all()


# ---- streaming, capture, errors ----------------------------------------------------------------------------
def test_streaming_int16(engine):
    mel = _mel(V1, 77, 1, 300, engine.device)
    whole = engine.forward_pcm16(mel, dtype="f32").clone()
    sv = StreamingVocoder(lambda m: engine.forward_pcm16(m.contiguous(), dtype="f32"), chunk_frames=64, config=V1)
    parts = list(sv.stream(mel))
    assert len(parts) == 5 and all(p.dtype == torch.int16 for p in parts)
    assert torch.equal(torch.cat(parts, dim=1), whole)
    assert torch.equal(sv.infer(mel), whole)
    # pushed input, uneven pieces
    pipe = MelToWavePipeline(None, engine.forward_pcm16, device=engine.device, chunk_frames=64)
    assert pipe.config is V1
    sess = pipe.session()
    out, t = [], 0
    for n in (1, 70, 13, 150, 0, 66):
        out += sess.push(mel[:, :, t:t + n])
        t += n
    out += sess.flush()
    assert t == 300 and all(p.dtype == torch.int16 for p in out)
    assert torch.equal(torch.cat(out, dim=1), whole)
    assert torch.equal(pipe.infer(mel, pcm16=True), whole)
    fp = MelToWavePipeline(None, engine.forward, device=engine.device, chunk_frames=64)
    assert torch.equal(fp.infer(mel, pcm16=True), whole) and fp.infer(mel).dtype == torch.float32
    npcm, peaks = fp.infer(mel, pcm16=True, normalize=True)
    assert np.array_equal(npcm.cpu().numpy(), pcm16_from_float(engine.forward(mel, dtype="f32").cpu().numpy(), normalize=True))
    batch = fp.infer_batch([mel[0, :, :37], mel[0, :, :120]], pcm16=True)
    assert [tuple(b.shape) for b in batch] == [(37 * HOP,), (120 * HOP,)] and batch[0].dtype == torch.int16
    assert torch.equal(batch[0], engine.forward_pcm16(mel[:, :, :37].contiguous(), dtype="f32")[0])


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalised"])
def test_capture(engine, normalize):
    dev = engine.device
    mels = [_mel(V1, s, 1, 40, dev) for s in (21, 22)]
    engine.prepare("f32")
    eager = []
    for m in mels:
        r = engine.forward_pcm16(m, dtype="f32", normalize=normalize)
        eager.append(tuple(t.clone() for t in r) if normalize else (r.clone(),))
    static_mel = mels[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = engine.forward_pcm16(static_mel, dtype="f32", normalize=normalize)
    captured = r if normalize else (r,)
    for i in (1, 0):
        static_mel.copy_(mels[i])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager[i]):
            assert torch.equal(got, want), f"replay with mel {i} differs from eager"


def test_drop_in_entry_points(tmp_path):
    from iris import hifigan_pretrained as hp
    from iris.vocoder import HiFiGANVocoder
    rng = np.random.default_rng(19)
    mels = [(rng.standard_normal((80, n)) * 2.0 - 5.0).astype(np.float32) for n in (37, 64, 1)]
    ck = tmp_path / "generator.ckpt"
    torch.save({k: torch.from_numpy(v) for k, v in seeded_state_dict(V1, seed=4).items()}, ck)
    for m in mels[:2]:
        w = hp.infer_hifigan(m, checkpoint_path=ck)
        assert np.array_equal(hp.infer_hifigan_pcm16(m, checkpoint_path=ck), pcm16_from_float(w))
        assert np.array_equal(hp.infer_hifigan_pcm16(m[None], 22050, 256, ck, normalize=True), pcm16_from_float(w, normalize=True))
    gen = hp.get_pretrained_hifigan(ck)
    assert gen.infer_pcm16(np.stack([mels[0], mels[0]])).shape == (2, 37 * HOP)
    for got, m in zip(gen.infer_batch(mels, pcm16=True), mels):
        assert got.dtype == np.int16 and np.array_equal(got, gen.infer_pcm16(m))
    voc = HiFiGANVocoder()
    for got, m in zip(voc.infer_batch(mels, pcm16=True), mels):
        assert got.dtype == np.int16 and np.array_equal(got, pcm16_from_float(voc.infer(m)))


def test_error_statuses(engine):
    lib = _native.load()
    dev = engine.device
    B, T = 2, 40
    mel = _mel(V1, 3, B, T, dev)
    pcm = torch.empty((B, HOP * T), dtype=torch.int16, device=dev)
    wav = torch.empty((B, HOP * T), dtype=torch.float32, device=dev)
    peak = torch.empty((B,), dtype=torch.float32, device=dev)
    lengths = torch.tensor([40, 20], dtype=torch.int32, device=dev)
    ws = torch.empty(engine.workspace_bytes(B, T, "f32"), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)      # noqa: E731

    def call(B=B, T=T, lengths=None, pcm=pcm, wav=wav, peak=peak, normalize=0, target=0.95, dtype=_native.DTYPE_F32, ws=ws):
        return lib.iris_hifigan_forward_pcm16(engine._handle, P(mel), B, T, P(lengths), P(pcm), P(wav), P(peak), normalize,
                                              ctypes.c_float(target), P(ws), ctypes.c_uint64(ws.numel()), dtype, stream)

    engine.prepare("bf16")
    engine.prepare("f32s")
    assert call(lengths=lengths, dtype=_native.DTYPE_BF16) == _native.STATUS_UNSUPPORTED
    assert call(lengths=lengths, dtype=_native.DTYPE_F32_SPLIT) == _native.STATUS_UNSUPPORTED
    assert call(dtype=7) == _native.STATUS_UNSUPPORTED
    assert call(normalize=1, wav=None) == _native.STATUS_INVALID_ARGUMENT
    assert call(normalize=1, peak=None) == _native.STATUS_INVALID_ARGUMENT
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        assert call(normalize=1, target=bad) == _native.STATUS_INVALID_ARGUMENT
    assert call(pcm=None) == _native.STATUS_INVALID_ARGUMENT
    assert call(B=-1) == _native.STATUS_INVALID_ARGUMENT
    assert call(ws=ws[:1024]) == _native.STATUS_WORKSPACE_TOO_SMALL
    assert call(B=0) == 0 and call(T=0) == 0 and call(B=0, pcm=None) == 0
    # plain PCM needs neither wav nor peak; 1.0 is a valid target
    assert call(wav=None, peak=None) == 0
    assert call(normalize=1, target=1.0, lengths=lengths) == 0
    torch.cuda.synchronize()
    assert torch.equal(wav, engine.forward(mel, dtype="f32", lengths=[40, 20]))
