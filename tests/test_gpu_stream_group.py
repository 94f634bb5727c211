"""``iris.stream_group.StreamGroup`` on the device, end to end: three members with utterances of 40, 70 and 23 frames join at
different steps, push pieces at different cadences and are stepped together -- one ragged PostNet pass, one ragged vocoder
forward, one limiter group call and one resampler group call per step -- and each member's concatenated pieces equal
``pipeline.infer`` of its own mel, bit for bit: 8 kHz mu-law bytes behind the limiter, with a PostNet and without, then once with
no limiter and once with no ``output=``.  The small generator configuration of tests/test_gpu_parity.py (hop 24)."""
import pytest
import torch

from iris._engine import GeneratorEngine
from iris._weights import seeded_mel
from iris.limiter import Limiter
from iris.pipeline import MelToWavePipeline
from iris.postnet import PostNet
from iris.resample import Resampler
from iris.stream_group import StreamGroup

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CHUNK = 16
FRAMES, OPENED_AT, PIECE = (40, 70, 23), (0, 1, 3), (5, 16, 23)


@pytest.fixture(scope="module")
def parts(case_setup):
    cfg, sd = case_setup("small_cfg_B3_T19")
    eng = GeneratorEngine(cfg, sd, DEV, dtype="f32")
    postnet = PostNet(n_mels=cfg.in_channels, num_layers=3, channels=32, kernel_size=5, seed=5)
    lim = Limiter(22050, ceiling_dbtp=-12.0, lookahead_ms=1.5, device=DEV)
    res = Resampler(8000, device=DEV)
    mels = [torch.from_numpy(seeded_mel(50 + i, 1, T, n_mels=cfg.in_channels, log_mel=True)).to(DEV) for i, T in enumerate(FRAMES)]
    yield dict(eng=eng, postnet=postnet, lim=lim, res=res, mels=mels)
    eng.close()


def drive(group, mels):
    members, at, got = [None] * len(mels), [0] * len(mels), [[] for _ in mels]
    shared = 0
    for step in range(100):
        for i, mel in enumerate(mels):
            if step == OPENED_AT[i]:
                members[i] = group.open()
            m = members[i]
            if m is None or m._ended:
                continue
            m.push(mel[:, :, at[i]:at[i] + PIECE[i]])
            at[i] += PIECE[i]
            if at[i] >= mel.shape[2]:
                m.end()
        pieces = group.step()
        shared += len(pieces) > 1
        for m, piece in pieces.items():
            got[members.index(m)].append(piece)
        if all(m is not None and m.closed for m in members):
            break
    assert all(m.closed for m in members) and group.members == [] and shared > 0
    return [torch.cat(g, dim=1) for g in got]


@pytest.mark.parametrize("with_postnet,with_limiter,with_output", [(True, True, True), (False, True, True), (False, False, True),
                                                                   (True, True, False)])
def test_every_member_equals_infer_of_its_own_mel(parts, with_postnet, with_limiter, with_output):
    pipe = MelToWavePipeline(parts["postnet"] if with_postnet else None, parts["eng"].forward, device=DEV, chunk_frames=CHUNK,
                             limiter=parts["lim"].chunked() if with_limiter else None,
                             output=parts["res"].chunked("ulaw") if with_output else None)
    got = drive(StreamGroup(pipe, chunk_frames=CHUNK), parts["mels"])
    torch.cuda.synchronize()
    for mel, mine in zip(parts["mels"], got):
        want = pipe.infer(mel)
        assert mine.dtype == want.dtype == (torch.uint8 if with_output else torch.float32) and mine.shape == want.shape
        assert torch.equal(mine.view(torch.int32) if mine.dtype == torch.float32 else mine,
                           want.view(torch.int32) if want.dtype == torch.float32 else want), (with_postnet, with_limiter, with_output)
    if with_limiter and not with_output:
        raw = MelToWavePipeline(parts["postnet"] if with_postnet else None, parts["eng"].forward, device=DEV,
                                chunk_frames=CHUNK).infer(parts["mels"][1])
        assert float(raw.abs().max()) > parts["lim"].ceiling >= float(got[1].abs().max())                     # the limiter acts
