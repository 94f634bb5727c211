"""The ragged VAE decoder without a GPU: the C symbol, the host-side checks of ``lengths=`` (iris.vae) and the way
``MelToWavePipeline.infer_from_phonemes`` feeds a batch to an acoustic stage that takes lengths -- one call -- or to one that
does not -- one call per item.  The device side is tests/test_gpu_vae_ragged.py."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import encoder as E
from iris.pipeline import MelToWavePipeline
from iris.vae import TextConditionedVAE

from vae_cases import make_vae

SYMBOL = "iris_vae_decoder_forward_ragged"


def test_symbol_is_declared_bound_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "iris_hifigan.h").read_text()
    assert SYMBOL in set(re.findall(r"\b(iris_vae_decoder_[a-z0-9_]+)\s*\(", header))
    assert SYMBOL in _native.VAE_SYMBOLS
    # the dense forward's arguments with lengths_dev between T and the outputs
    dense = _native.VAE_SYMBOLS["iris_vae_decoder_forward"]
    ragged = _native.VAE_SYMBOLS[SYMBOL]
    assert ragged[0] is dense[0] and len(ragged[1]) == len(dense[1]) + 1
    lib = _native.load()
    assert getattr(lib, SYMBOL) is not None
    assert lib.iris_hifigan_abi_version() == 4
    assert TextConditionedVAE.takes_lengths is True


@pytest.mark.parametrize("name", ["default", "small"])
def test_bad_host_lengths_are_rejected_before_a_device_is_required(name):
    vae = make_vae(name)
    f = vae.downsample_factor
    B, T = 2, 4 * f
    cond = np.zeros((B, T, vae.cond_dim), np.float32)
    bad = [([T], "hold 2"), ([T, T, T], "hold 2"), ([[T, T]], "hold 2"),          # wrong count
           ([T, -f], "outside"), ([-1, T], "outside"),                             # negative
           ([T + f, T], "outside"), ([0, T + 1], "outside"),                       # above T
           ([T, f + 1], "multiple of 2\\^down_stages"), ([2 * f - 1, T], "multiple of 2\\^down_stages"),
           ([T, 1.5], "integers")]
    for lengths, match in bad:
        for call, arg in ((vae.generate, cond), (vae.generate, torch.from_numpy(cond)),
                          (vae.generate_device, torch.from_numpy(cond))):
            with pytest.raises(ValueError, match=match):
                call(arg, lengths=lengths)
            with pytest.raises(ValueError, match=match):
                call(arg, lengths=np.asarray(lengths))
    assert vae._handle is None                                                     # nothing reached the device side
    # good lengths pass the check in every host form and come back as int32
    for good in ([T, 0], (f, T), np.array([2 * f, 3 * f], np.int64), torch.tensor([T, f])):
        got = vae._check_lengths(good, B, T)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.tolist() == [int(v) for v in good]


# ---- pipeline: stub stages, as in test_vae.test_infer_from_cond_chains_acoustic_postnet_vocoder ---------------------------
FACTOR, LATENT, N_MELS, HOP = 4, 6, 4, 2
TOTALS = [9, 4, 6]                                     # frames per item -> padded 12, 4, 8
PADDED = [12, 4, 8]


class _StubEngine:
    def forward(self, mel, lengths=None):
        return mel.sum(dim=1).repeat_interleave(HOP, dim=1)


def _mel_of(cond, z):
    """A mel that depends on every conditioning frame and on the prior of its latent row."""
    return cond.sum(dim=2)[:, None, :] * torch.ones(1, N_MELS, 1) + z.sum(dim=2).repeat_interleave(FACTOR, dim=1)[:, None, :]


class _RaggedVae:
    takes_lengths = True
    downsample_factor, latent_dim = FACTOR, LATENT

    def __init__(self):
        self.calls = []

    def generate_device(self, cond, z_prior=None, want_residual=True, generator=None, lengths=None):
        self.calls.append((tuple(cond.shape), z_prior.clone(), want_residual, lengths))
        mel = _mel_of(cond, z_prior)
        if lengths is not None:
            for b, n in enumerate(lengths):
                mel[b, :, n:] = 0.0
        return mel, None


class _PlainAcoustic:
    downsample_factor = FACTOR

    def __init__(self):
        self.calls = []

    def __call__(self, cond, z_prior):
        if z_prior is None:
            z_prior = torch.randn(cond.shape[0], cond.shape[1] // FACTOR, LATENT)
        self.calls.append((tuple(cond.shape), z_prior.clone()))
        return _mel_of(cond, z_prior), None


@pytest.fixture
def stub_text(monkeypatch):
    """frame_conditioning replaced by a host stand-in: an item's frame total is its first id, its conditioning rows count
    up from that total, and rows from the total on are 0 -- so a batch of one yields the item's own rows of the batch."""
    def frame_conditioning(encoder, head, ids, lengths=None, durations=None, factor=4, max_frames=None):
        assert factor == FACTOR
        totals = [int(n) for n in np.asarray(ids)[:, 0]]
        T = -(-max(totals) // factor) * factor
        cond = torch.zeros(len(totals), T, 3)
        for b, n in enumerate(totals):
            cond[b, :n] = float(n) + torch.arange(n, dtype=torch.float32)[:, None]
        return cond, totals
    monkeypatch.setattr(E, "frame_conditioning", frame_conditioning)
    return ("encoder", "head")


def _pipe(acoustic, text):
    return MelToWavePipeline(None, _StubEngine().forward, hop_length=HOP, chunk_frames=64, acoustic=acoustic, text=text)


def test_batch_goes_through_a_lengths_taking_stage_once(stub_text):
    ids = np.array(TOTALS, np.int32)[:, None]
    zs = [torch.full((1, n // FACTOR, LATENT), float(i + 1)) for i, n in enumerate(PADDED)]
    vae = _RaggedVae()
    wavs, per_item = _pipe(vae, stub_text).infer_from_phonemes(ids, z_prior=zs)
    assert per_item == TOTALS and len(vae.calls) == 1
    shape, z, want_residual, lengths = vae.calls[0]
    assert shape == (3, 12, 3) and want_residual is False
    assert list(lengths) == PADDED == [-(-t // FACTOR) * FACTOR for t in TOTALS]
    assert tuple(z.shape) == (3, 3, LATENT)
    for i, n in enumerate(PADDED):
        assert torch.equal(z[i, :n // FACTOR], zs[i][0]) and not z[i, n // FACTOR:].any()
    # item for item what the B == 1 call returns
    for i in range(3):
        one = _RaggedVae()
        wav, n_i = _pipe(one, stub_text).infer_from_phonemes(ids[i:i + 1], z_prior=zs[i])
        assert one.calls[0][3] is None and n_i == [TOTALS[i]]                # B == 1: today's dense call
        assert tuple(wavs[i].shape) == (HOP * PADDED[i],) and torch.equal(wavs[i], wav[0])
    with pytest.raises(ValueError, match="z_prior"):
        _pipe(_RaggedVae(), stub_text).infer_from_phonemes(ids, z_prior=zs[:2])
    with pytest.raises(ValueError, match="z_prior\\[1\\]"):
        _pipe(_RaggedVae(), stub_text).infer_from_phonemes(ids, z_prior=[zs[0], zs[0], zs[2]])


def test_batch_goes_through_a_plain_callable_item_by_item(stub_text):
    ids = np.array(TOTALS, np.int32)[:, None]
    zs = [torch.full((1, n // FACTOR, LATENT), float(i + 1)) for i, n in enumerate(PADDED)]
    plain = _PlainAcoustic()
    wavs, per_item = _pipe(plain, stub_text).infer_from_phonemes(ids, z_prior=zs)
    assert per_item == TOTALS and [c[0] for c in plain.calls] == [(1, n, 3) for n in PADDED]
    ragged, _ = _pipe(_RaggedVae(), stub_text).infer_from_phonemes(ids, z_prior=zs)
    for a, b in zip(wavs, ragged):
        assert torch.equal(a, b)
    # a generate_device without takes_lengths keeps the loop too
    class _OldVae:
        downsample_factor = FACTOR
        calls = 0

        def generate_device(self, cond, z_prior=None, want_residual=True):
            _OldVae.calls += 1
            return _mel_of(cond, z_prior), None
    _pipe(_OldVae(), stub_text).infer_from_phonemes(ids, z_prior=zs)
    assert _OldVae.calls == 3


def test_priors_are_drawn_per_item_in_item_order(stub_text):
    ids = np.array(TOTALS, np.int32)[:, None]
    torch.manual_seed(77)
    want = [torch.randn(1, n // FACTOR, LATENT) for n in PADDED]            # what three B == 1 calls draw, in order
    after = torch.randn(4)
    vae = _RaggedVae()
    torch.manual_seed(77)
    wavs, _ = _pipe(vae, stub_text).infer_from_phonemes(ids)
    assert torch.equal(torch.randn(4), after)                               # the same stream was consumed
    z = vae.calls[0][1]
    for i, n in enumerate(PADDED):
        assert torch.equal(z[i, :n // FACTOR], want[i][0]) and not z[i, n // FACTOR:].any()
    # and the per-item loop of a plain callable draws the same numbers
    plain = _PlainAcoustic()
    torch.manual_seed(77)
    loop, _ = _pipe(plain, stub_text).infer_from_phonemes(ids)
    for a, b in zip(wavs, loop):
        assert torch.equal(a, b)
