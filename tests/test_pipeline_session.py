"""Pushed input for the PostNet -> vocoder pipeline (MelToWavePipeline.session): the raw mel of one utterance arrives
piece by piece, refined and vocoded audio leaves chunk by chunk, and the concatenation equals the one-shot pipeline."""
import numpy as np
import pytest
import torch

from iris.pipeline import MelToWavePipeline, PipelineSession

HOP = 4
HV = 13           # the vocoder stand-in's (and the V1 generator's) receptive field
HP = 4            # two stacked k5 'same' convolutions


def _stand_ins():
    """Stages with finite receptive fields: the PostNet stand-in is two stacked conv1d(k=5, padding=2) (+-4 frames), the
    vocoder stand-in is the one of tests/test_pipeline.py (+-13 frames)."""
    g = torch.Generator().manual_seed(3)
    w1 = torch.randn(8, 8, 5, generator=g) * 0.2
    w2 = torch.randn(8, 8, 5, generator=g) * 0.2
    b1 = torch.randn(8, generator=g) * 0.1          # a bias: zero padding is then visible one layer in

    def postnet(m):
        h = torch.tanh(torch.nn.functional.conv1d(m, w1, b1, padding=2))
        return m + torch.nn.functional.conv1d(h, w2, padding=2)

    def vocode(m):
        k = torch.ones(1, m.shape[1], 27) / 27.0
        y = torch.nn.functional.conv1d(m, k, padding=13)
        return y.repeat_interleave(HOP, dim=2)[:, 0, :]

    return postnet, vocode


class Counting:
    """A PostNet stand-in that counts its passes and knows its halo."""

    def __init__(self, fn, halo):
        self.fn, self.receptive_field_frames, self.calls, self.widths = fn, halo, 0, []

    def __call__(self, m):
        self.calls += 1
        self.widths.append(int(m.shape[2]))
        return self.fn(m)


def _splittings(T):
    rng = np.random.default_rng(12)
    pieces = []
    while sum(pieces) < T:
        pieces.append(int(rng.choice([0, 0, 1, 2, 5, 17, 40, 130, 300])))
    pieces[-1] -= sum(pieces) - T
    assert 0 in pieces and sum(pieces) == T
    return {"whole": [T], "single_frames": [1] * T, "random": pieces}


@pytest.mark.parametrize("name", ["whole", "single_frames", "random"])
def test_session_control_flow_cpu(name):
    T, chunk = 700, 256
    pieces = _splittings(T)[name]
    postnet, vocode = _stand_ins()
    post = Counting(postnet, HP)
    mel = torch.randn(2, 8, T, generator=torch.Generator().manual_seed(1))
    pipe = MelToWavePipeline(post, vocode, hop_length=HOP, chunk_frames=chunk)
    want = pipe.infer(mel)
    post.calls, post.widths = 0, []
    ses = pipe.session()
    assert isinstance(ses, PipelineSession) and ses.postnet_halo_frames == HP and ses.halo_frames == HV
    out, pos, returned_at = [], 0, {}
    for t in pieces:
        got = ses.push(mel[:, :, pos:pos + t].numpy() if pos % 2 else mel[:, :, pos:pos + t])    # host and torch pieces
        pos += t
        assert ses.frames_received == pos
        # latency: chunk [s, s + chunk) leaves with the push that brings frames_received to s + chunk + hv + hp
        assert ses.frames_emitted == max(0, (pos - HV - HP) // chunk * chunk)
        for c in got:
            returned_at[len(out)] = pos
            out.append(c)
        # memory: chunk + 2 (hv + hp) frames, plus the piece just pushed
        assert ses.frames_buffered <= chunk + 2 * (HV + HP) + t
        # work: a pass only where a chunk is returned
        assert post.calls <= len(out)
    out += ses.flush()
    assert ses.frames_emitted == T
    assert [c.shape[1] for c in out] == [256 * HOP, 256 * HOP, 188 * HOP]
    assert torch.allclose(torch.cat(out, dim=1), want, atol=1e-6)
    assert post.calls <= len(out) + 1
    # every refinement window is bounded too: never the whole utterance again (unless it came in one piece)
    if name != "whole":
        assert max(post.widths) <= chunk + HV + 2 * HP + max(pieces)
    for i in (0, 1):                                  # neither earlier nor later than the frame that completes the context
        first_possible = (i + 1) * chunk + HV + HP
        reached = np.cumsum(pieces)
        assert returned_at[i] == int(reached[np.searchsorted(reached, first_possible)])
    with pytest.raises(RuntimeError):
        ses.push(mel[:, :, :1])


def test_session_a_smaller_halo_is_visibly_wrong():
    """The equality above is not vacuous: with hp - 1 frames the seams differ."""
    postnet, vocode = _stand_ins()
    mel = torch.randn(2, 8, 700, generator=torch.Generator().manual_seed(1))
    pipe = MelToWavePipeline(postnet, vocode, hop_length=HOP, chunk_frames=256)
    want = pipe.infer(mel)
    for halo, ok in ((HP, True), (HP - 1, False)):
        ses = pipe.session(postnet_halo_frames=halo)
        out = []
        for s in range(0, 700, 50):
            out += ses.push(mel[:, :, s:s + 50])
        out += ses.flush()
        assert torch.allclose(torch.cat(out, dim=1), want, atol=1e-6) == ok


def test_session_without_postnet_and_errors():
    postnet, vocode = _stand_ins()
    mel = torch.randn(2, 8, 300, generator=torch.Generator().manual_seed(2))
    pipe = MelToWavePipeline(None, vocode, hop_length=HOP, chunk_frames=64)
    ses = pipe.session()
    assert ses.postnet_halo_frames == 0
    out = []
    for s in range(0, 300, 7):
        out += ses.push(mel[:, :, s:s + 7])
        assert ses.frames_emitted == max(0, (ses.frames_received - HV) // 64 * 64)
    out += ses.flush()
    assert [c.shape[1] for c in out] == [64 * HOP] * 4 + [44 * HOP]
    assert torch.allclose(torch.cat(out, dim=1), vocode(mel), atol=1e-6)
    # a bare callable: its halo cannot be guessed
    bare = MelToWavePipeline(postnet, vocode, hop_length=HOP, chunk_frames=64)
    with pytest.raises(ValueError):
        bare.session()
    assert bare.session(postnet_halo_frames=HP).postnet_halo_frames == HP
    with pytest.raises(ValueError):
        bare.session(postnet_halo_frames=-1)
    # an object that knows its halo: a smaller one is refused, a larger one is taken
    knows = MelToWavePipeline(Counting(postnet, HP), vocode, hop_length=HOP, chunk_frames=64)
    with pytest.raises(ValueError):
        knows.session(postnet_halo_frames=HP - 1)
    assert knows.session(postnet_halo_frames=HP + 2).postnet_halo_frames == HP + 2
    with pytest.raises(ValueError):
        MelToWavePipeline(None, vocode, hop_length=HOP, chunk_frames=0).session()
    # the error rules of StreamingSession
    ses = bare.session(postnet_halo_frames=HP)
    ses.push(mel[:, :, :10])
    with pytest.raises(ValueError):
        ses.push(mel[:1, :, :10])                     # another batch size
    with pytest.raises(ValueError):
        ses.push(mel[:, :7, :10])                     # other mel bins
    with pytest.raises(ValueError):
        ses.push(mel[0])                              # not [B, n_mels, t]
    ses.flush()
    with pytest.raises(RuntimeError):
        ses.push(mel[:, :, :1])
    # an utterance that ends before its first chunk, and an empty one
    ses = bare.session(postnet_halo_frames=HP)
    assert ses.push(mel[:, :, :3]) == []
    (only,) = ses.flush()
    assert torch.allclose(only, bare.infer(mel[:, :, :3]), atol=1e-6)
    assert bare.session(postnet_halo_frames=HP).flush() == []


def test_session_on_the_oracles():
    """The two CPU restatements as the stages: PostNet oracle -> generator oracle, pushed in pieces against one shot."""
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    from iris.postnet import PostNet
    from oracle import hifigan_oracle as orc
    from oracle import postnet_oracle as porc
    cfg = GeneratorConfig()
    folded = orc.to_torch_folded(seeded_state_dict(cfg, seed=2025, gain=1.18, post_gain=20.0))
    pn = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    T = 150
    mel = seeded_mel(1007, 1, T, log_mel=True)

    def postnet(m):
        return torch.from_numpy(porc.postnet_forward_np(pn.weights, m.numpy(), 3))

    def vocode(m):
        return orc.generator_forward_torch(folded, m)[:, 0, :]

    want = vocode(postnet(torch.from_numpy(mel)))                     # the same two oracles, one shot
    pipe = MelToWavePipeline(postnet, vocode, chunk_frames=64, config=cfg)
    ses = pipe.session(postnet_halo_frames=pn.receptive_field_frames)
    out, pos = [], 0
    for t in (1, 70, 0, 79):
        out += ses.push(mel[:, :, pos:pos + t])
        pos += t
        assert len(out) == (2 if pos == 150 else 0)                    # 128 + 13 + 6 = 147 frames arrive with the last push only
    out += ses.flush()
    assert [c.shape[1] for c in out] == [64 * 256, 64 * 256, 22 * 256]
    got = torch.cat(out, dim=1)
    err = float((got - want).abs().max())
    print(f"pushed session vs one shot on the oracles: max abs diff {err:.3e}")
    # the figure tests/test_streaming.py uses for chunked-versus-one-shot on the torch oracle (ATen picks kernels by length)
    assert got.shape == want.shape and err <= 2e-5


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f32s"])
def test_session_on_gpu_equals_one_shot_pipeline(dtype):
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
    from iris.postnet import PostNet
    dev = torch.device("cuda", 0)
    cfg = GeneratorConfig()
    eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=10.0), dev, dtype=dtype)
    post = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, dropout=0.3, seed=5)
    T = 300
    mel = seeded_mel(23, 1, T, log_mel=True)
    pipe = MelToWavePipeline(post, eng.forward, device=dev, chunk_frames=64)
    want = pipe.infer(mel).clone()
    ses = pipe.session()
    assert ses.postnet_halo_frames == 6 and ses.halo_frames == 13
    out, pos = [], 0
    for t in (1, 7, 150, 0, 142):
        out += [c.clone() for c in ses.push(mel[:, :, pos:pos + t])]
        pos += t
        assert ses.frames_emitted == max(0, (pos - 13 - 6) // 64 * 64)
    out += [c.clone() for c in ses.flush()]
    assert [tuple(c.shape) for c in out] == [(1, 64 * 256)] * 4 + [(1, 44 * 256)]
    got = torch.cat(out, dim=1)
    assert got.is_cuda and torch.isfinite(got).all()
    assert torch.equal(got, want)
    eng.close()
