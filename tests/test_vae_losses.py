"""The ragged posterior side and the masked VAE losses without a GPU: the new C symbols, the loss restatement
(tests/vae_losses_restatement.py) against the reference's formulas written with explicit 0/1 masks, and the host-side checks
of ``lengths=`` in ``VAEPosteriorEncoder.encode`` / ``encode_device``, ``reconstruct``, ``decode_posterior_device``,
``vae_losses`` and the list form of ``MelToWavePipeline.resynthesize`` -- all of which raise before any device work.  The
device side is tests/test_gpu_vae_posterior_ragged.py and tests/test_gpu_vae_losses.py."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import vae as V
from iris.pipeline import MelToWavePipeline

from vae_losses_restatement import kl_terms, losses_np
from vae_posterior_cases import make_pair

# new symbol -> (its binding table, the dense forward's signature)
NEW = {"iris_vae_posterior_encode_ragged": (_native.VAE_POSTERIOR_SYMBOLS, _native.VAE_ENCODER_SYMBOLS["iris_vae_encoder_forward"]),
       "iris_vae_decoder_forward_posterior_ragged": (_native.VAE_SYMBOLS, _native.VAE_SYMBOLS["iris_vae_decoder_forward_posterior"])}


def test_symbols_are_declared_bound_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "iris_hifigan.h").read_text()
    declared = set(re.findall(r"\b(iris_vae_[a-z0-9_]+)\s*\(", header))
    lib = _native.load()
    for name, (table, dense) in NEW.items():
        assert name in declared and name in table
        # the dense forward's arguments with lengths_dev between T and the outputs
        assert table[name][0] is dense[0] and len(table[name][1]) == len(dense[1]) + 1
        assert getattr(lib, name) is not None
    losses = {n for n in declared if n.startswith("iris_vae_losses")}
    assert losses == set(_native.VAE_LOSSES_SYMBOLS) == {"iris_vae_losses", "iris_vae_losses_workspace_bytes"}
    assert lib.iris_vae_losses and lib.iris_vae_losses_workspace_bytes
    assert lib.iris_hifigan_abi_version() == 4
    assert V.VAEPosteriorEncoder.takes_lengths is True
    # the ragged encoder forward is its own family: iris_vae_encoder_* keeps the seven functions tests/test_vae_posterior.py counts
    assert set(_native.VAE_POSTERIOR_SYMBOLS) == {n for n in declared if n.startswith("iris_vae_posterior_")}
    assert len(_native.VAE_ENCODER_SYMBOLS) == 7


def test_losses_workspace_query_needs_no_device():
    import ctypes
    lib = _native.load()
    n = ctypes.c_uint64()
    assert lib.iris_vae_losses_workspace_bytes(8, 80, 1024, 16, 2, ctypes.byref(n)) == 0
    assert n.value == 8 * (4 + 1 + 2) * 8                     # 4 tiles of 256 frames, 1 tile of 4096 latent floats, 2 item sums
    assert lib.iris_vae_losses_workspace_bytes(0, 80, 1024, 16, 2, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.iris_vae_losses_workspace_bytes(2, 80, 6, 16, 2, ctypes.byref(n)) == _native.STATUS_INVALID_ARGUMENT
    assert b"multiple" in lib.iris_hifigan_last_error()
    assert lib.iris_vae_losses_workspace_bytes(2, 80, 8, 16, 2, None) == _native.STATUS_INVALID_ARGUMENT
    assert lib.iris_vae_losses_workspace_bytes(-1, 80, 8, 16, 2, ctypes.byref(n)) == _native.STATUS_INVALID_ARGUMENT


# ---- the restatement ------------------------------------------------------------------------------
def _tensors(B=3, n_mels=5, T=12, S=2, latent=4, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, n_mels, T)), rng.standard_normal((B, n_mels, T)),
            rng.standard_normal((B, T >> S, latent)), 0.5 * rng.standard_normal((B, T >> S, latent)))


def _with_masks(target, recon, mean, logvar, mask, S):
    """compute_recon_l1 / compute_kl as the reference writes them: a 0/1 mask [B, T], multiplied in."""
    m = mask[:, None, :]
    l1 = (np.abs(target - recon) * m).sum() / (m.sum() * target.shape[1] + 1e-6)
    md = mask[:, ::1 << S][:, :, None]
    kl = (kl_terms(mean, logvar) * md).sum() / (md.sum() + 1e-8)
    return l1, kl


def test_masked_form_equals_the_formula_on_explicit_masks():
    S = 2
    target, recon, mean, logvar = _tensors(S=S)
    B, _, T = target.shape
    for lengths in ([T] * B, [12, 4, 8], [0, 12, 4]):
        mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.float64)
        want_l1, want_kl = _with_masks(target, recon, mean, logvar, mask, S)
        l1, kl, item_l1, item_kl = losses_np(target, recon, mean, logvar, S, lengths)
        assert abs(l1 - want_l1) <= 1e-14 * abs(want_l1) and abs(kl - want_kl) <= 1e-14 * abs(want_kl), lengths
        # the KL denominator counts rows, not rows x channels; the item sums are the numerators' parts
        rows = sum(n >> S for n in lengths)
        assert abs(item_kl.sum() / (rows + 1e-8) - kl) <= 1e-14 * abs(kl)
        assert abs(item_l1.sum() / (sum(lengths) * target.shape[1] + 1e-6) - l1) <= 1e-14 * abs(l1)


def test_zero_length_items_and_poisoned_tails_contribute_nothing():
    S = 1
    target, recon, mean, logvar = _tensors(B=4, T=10, S=S, seed=1)
    lengths = [10, 0, 4, 0]
    want = losses_np(target[[0, 2]], recon[[0, 2]], mean[[0, 2]], logvar[[0, 2]], S, [10, 4])
    for b, n in enumerate(lengths):
        target[b, :, n:] = recon[b, :, n:] = np.nan
        mean[b, n >> S:] = logvar[b, n >> S:] = np.nan
    got = losses_np(target, recon, mean, logvar, S, lengths)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2].tolist() == [want[2][0], 0.0, want[2][1], 0.0] and got[3].tolist() == [want[3][0], 0.0, want[3][1], 0.0]
    empty = losses_np(target, recon, mean, logvar, S, [0, 0, 0, 0])
    assert empty[0] == 0.0 and empty[1] == 0.0                                          # 0 / (0 + eps), not NaN
    f32 = losses_np(np.nan_to_num(target), np.nan_to_num(recon), np.nan_to_num(mean), np.nan_to_num(logvar), S, lengths, dtype=np.float32)
    assert f32[0].dtype == np.float32 and f32[2].dtype == np.float32 and abs(float(f32[0]) - got[0]) < 1e-5 * got[0]


def test_unmasked_form_is_the_mean():
    target, recon, mean, logvar = _tensors(seed=2)
    l1, kl, item_l1, item_kl = losses_np(target, recon, mean, logvar, 2)
    assert abs(l1 - np.abs(target - recon).mean()) <= 1e-14 * l1
    assert abs(kl - kl_terms(mean, logvar).mean()) <= 1e-14 * abs(kl)
    assert abs(item_l1.sum() - np.abs(target - recon).sum()) <= 1e-12 * item_l1.sum()
    # the masked form with full lengths differs from it exactly by the reference's normalisation of the KL
    _, kl_m, _, _ = losses_np(target, recon, mean, logvar, 2, [target.shape[2]] * target.shape[0])
    rows = mean.shape[0] * mean.shape[1]
    assert abs(kl_m * (rows + 1e-8) / (rows * mean.shape[2]) - kl) <= 1e-14 * abs(kl)


# ---- host-side checks of lengths= -------------------------------------------------------------------
def _bad_lengths(T, f):
    return [([T], "hold 2"), ([T, T, T], "hold 2"), ([[T, T]], "hold 2"),           # wrong count / shape
            ([T, 1.5], "integers"),                                                  # float dtype
            ([T, -f], "outside"), ([T + f, T], "outside"), ([0, T + 1], "outside"),  # out of range
            ([T, f + 1], "multiple of 2\\^down_stages"), ([2 * f - 1, T], "multiple of 2\\^down_stages")]


@pytest.mark.parametrize("name", ["default", "small"])
def test_bad_host_lengths_are_rejected_before_a_device_is_required(name):
    enc, vae = make_pair(name)
    f = enc.downsample_factor
    B, T = 2, 4 * f
    mel = np.zeros((B, enc.n_mels, T), np.float32)
    cond = np.zeros((B, T, enc.cond_dim), np.float32)
    z = torch.zeros(B, T // f, enc.latent_dim)
    t = torch.from_numpy
    calls = [lambda L: enc.encode(mel, cond, lengths=L), lambda L: enc.encode(t(mel), t(cond), lengths=L),
             lambda L: enc.encode_device(t(mel), t(cond), lengths=L),
             lambda L: V.reconstruct(enc, vae, mel, cond, lengths=L), lambda L: V.reconstruct(enc, vae, t(mel), t(cond), lengths=L),
             lambda L: V.reconstruct(enc, vae, mel, cond, lengths=L, losses=True),
             lambda L: vae.decode_posterior_device(t(cond), z, lengths=L),
             lambda L: V.vae_losses(mel, mel, z.numpy(), z.numpy(), enc.down_stages, lengths=L)]
    for lengths, match in _bad_lengths(T, f):
        for call in calls:
            with pytest.raises(ValueError, match=match):
                call(lengths)
            with pytest.raises(ValueError, match=match):
                call(np.asarray(lengths))
    assert enc._handle is None and vae._handle is None                               # nothing reached the device side
    # one copy of the rules: the decoder's method is the module's function
    for good in ([T, 0], (f, T), np.array([2 * f, 3 * f], np.int64), torch.tensor([T, f])):
        got = V.check_lengths(good, B, T, f)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.tolist() == [int(v) for v in good]
        assert np.array_equal(vae._check_lengths(good, B, T), got)
    # vae_losses checks its shapes on the host too
    with pytest.raises(ValueError, match="target and recon"):
        V.vae_losses(mel, mel[:, :, :f], z.numpy(), z.numpy(), enc.down_stages)
    with pytest.raises(ValueError, match="mean and logvar"):
        V.vae_losses(mel, mel, z.numpy()[:, :1], z.numpy()[:, :1], enc.down_stages)


def test_resynthesize_rejects_a_bad_list_before_a_device_is_required():
    enc, vae = make_pair("default")                                                 # factor 4
    pipe = MelToWavePipeline(None, lambda mel, lengths=None: mel.sum(dim=1), hop_length=1, posterior=enc, acoustic=vae)
    mel = lambda T: np.zeros((enc.n_mels, T), np.float32)
    cond = lambda T: np.zeros((T, enc.cond_dim), np.float32)
    for T in (6, 7, 9):
        with pytest.raises(ValueError, match="multiple of 2\\^down_stages"):
            pipe.resynthesize([mel(8), mel(T)], [cond(8), cond(T)])
    with pytest.raises(ValueError, match="conditionings"):
        pipe.resynthesize([mel(8), mel(4)], [cond(8)])
    with pytest.raises(ValueError, match="item 1"):
        pipe.resynthesize([mel(8), mel(4)], [cond(8), cond(8)])                     # rows of the conditioning != frames
    with pytest.raises(ValueError, match="item 0"):
        pipe.resynthesize([np.zeros((1, enc.n_mels, 8), np.float32)], [cond(8)])    # a batch where an utterance is expected
    assert pipe.resynthesize([], []) == []
    assert enc._handle is None and vae._handle is None


def test_resynthesize_hands_a_list_to_a_plain_callable_item_by_item():
    seen = []

    def posterior(mel, cond):
        seen.append((tuple(mel.shape), tuple(cond.shape)))
        return 0.5 * mel + cond.sum(dim=2)[:, None, :], None, None

    class _Engine:
        def forward(self, mel, lengths=None):
            return mel.sum(dim=1).repeat_interleave(2, dim=1)

    pipe = MelToWavePipeline(None, _Engine().forward, hop_length=2, chunk_frames=64, posterior=posterior)
    mels = [torch.arange(12, dtype=torch.float32).reshape(3, 4), torch.ones(3, 6)]
    conds = [torch.ones(4, 2), torch.full((6, 2), 2.0)]
    wavs = pipe.resynthesize(mels, conds)
    assert seen == [((1, 3, 4), (1, 4, 2)), ((1, 3, 6), (1, 6, 2))]
    for i in range(2):
        assert torch.equal(wavs[i], pipe.resynthesize(mels[i][None], conds[i][None])[0])
