"""The masked VAE losses on the device (iris_vae_losses, ``iris.vae.vae_losses``, ``reconstruct(..., losses=True)``) on the
MI355X against the float64 restatement (tests/vae_losses_restatement.py).  Shapes and models are those of
tests/test_gpu_vae_posterior_ragged.py; ``recon``, ``mean`` and ``logvar`` come from a ragged ``reconstruct``, so the inputs
are real, and the target is the mel that went in, NaN past each item's length.  One thing differs from make_pair's models:
the logvar head (``latent_logvar_proj``) is scaled by 1/32.  With every parameter drawn at random ``logvar`` reaches 133, the
exact KL sums are 1e47 ... 1e57 -- beyond the largest float, so no fp32 output can hold them and fp32 ``exp`` is inf, in keras
as here (the device returned inf for them, which is the faithful fp32 answer).  Scaled, ``|logvar|`` stays below 5, the
range a trained posterior lives in, and every quantity of the check is finite in fp32.

The accuracy bar is derived, not measured.  The restatement is evaluated in float64 on the device's own fp32 tensors, so
what differs is the device's arithmetic alone: each term is a handful of fp32 roundings and one expf, each of them relative
to the magnitudes that enter it, and the accumulation is fp64 (its error is 2^-29 of this and is ignored).  Hence
    L1 sums:  4 * 2^-24 * sum(|target| + |recon|)
    KL sums:  4 * 2^-24 * 0.5 * sum(1 + |lv| + m^2 + e^lv)
over the elements that enter the sum, and for the normalised pair the same quantities over the whole batch divided by the
loss's denominator.  The tests print the observed error as a share of the bar; on an MI355X the largest share over all
outputs was 0.13 ("default") and 0.23 ("small"), for the masked and the unmasked form alike.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import vae as V

from vae_losses_restatement import losses_np
from test_gpu_vae_posterior_ragged import DEV, NAN, SHAPES, _dev
from vae_posterior_cases import make_pair

pytestmark = pytest.mark.gpu

U = 4 * 2.0 ** -24
_pairs = {}


def pair_of(name):
    """make_pair(name) with the logvar head scaled by 1/32 (see above)."""
    if name not in _pairs:
        enc, vae = make_pair(name)
        w = dict(enc.weights)
        for leaf in ("kernel", "bias"):
            w[f"latent_logvar_proj.{leaf}"] = w[f"latent_logvar_proj.{leaf}"] / 32
        enc.set_weights_dict(w)
        _pairs[name] = (enc, vae)
    return _pairs[name]


@pytest.fixture(scope="module")
def recon_of():
    """name -> (target, recon, mean, logvar, S, lengths) on the device: one ragged reconstruct of the shape's poisoned inputs."""
    cache = {}

    def get(name):
        if name not in cache:
            enc, vae = pair_of(name)
            T, lengths = SHAPES[name]
            mel, cond, _ = _dev(name)
            recon, (mean, logvar), _ = V.reconstruct(enc, vae, mel, cond, lengths=lengths)
            cache[name] = (mel, recon, mean, logvar, enc.down_stages, lengths)
        return cache[name]
    return get


def _bars(target, recon, mean, logvar, S, lengths):
    """(l1 bar, kl bar, item l1 bars, item kl bars) from the magnitudes, in float64; lengths=None: whole items."""
    t, r, m, lv = (a.cpu().numpy().astype(np.float64) for a in (target, recon, mean, logvar))
    B, n_mels, T = t.shape
    full = lengths is None
    lengths = [T] * B if full else lengths
    b1 = np.array([U * (np.abs(t[b, :, :n]) + np.abs(r[b, :, :n])).sum() for b, n in enumerate(lengths)])
    bk = np.array([U * 0.5 * (1 + np.abs(lv[b, :n >> S]) + m[b, :n >> S] ** 2 + np.exp(lv[b, :n >> S])).sum() for b, n in enumerate(lengths)])
    frames, rows = sum(lengths), sum(n >> S for n in lengths)
    if full:
        return b1.sum() / (frames * n_mels), bk.sum() / (rows * m.shape[2]), b1, bk
    return b1.sum() / (frames * n_mels + 1e-6), bk.sum() / (rows + 1e-8), b1, bk


def _compare(tag, got, want, bars):
    """Every one of the 2 + 2B outputs within its bar; prints the largest share of the bar."""
    got = [float(got[0]), float(got[1]), got[2].cpu().numpy().astype(np.float64), got[3].cpu().numpy().astype(np.float64)]
    worst = 0.0
    for g, w, bar in zip(got, want, bars):
        err, bar = np.abs(np.asarray(g) - np.asarray(w, np.float64)), np.asarray(bar)
        assert np.isfinite(np.asarray(g)).all() and (err <= bar).all(), (tag, g, w, err, bar)
        if (bar > 0).any():
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()) if err.ndim else float(err / bar))
    print(f"{tag}: largest error / bar = {worst:.3f}")


@pytest.mark.parametrize("name", list(SHAPES))
def test_accuracy_independence_and_determinism(recon_of, name):
    target, recon, mean, logvar, S, lengths = recon_of(name)
    B = len(lengths)
    got = V.vae_losses(target, recon, mean, logvar, S, lengths=lengths)
    assert got[0].dim() == 0 and tuple(got[2].shape) == tuple(got[3].shape) == (B,) and got[0].device == target.device
    want = losses_np(*(a.cpu().numpy() for a in (target, recon, mean, logvar)), S, lengths)
    _compare(name, got, want, _bars(target, recon, mean, logvar, S, lengths))
    # two runs give the same bits; a device lengths tensor is the host list; reconstruct(losses=True) is this call
    again = V.vae_losses(target, recon, mean, logvar, S, lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    enc, vae = pair_of(name)
    mel, cond, _ = _dev(name)
    appended = V.reconstruct(enc, vae, mel, cond, lengths=lengths, losses=True)[3]
    assert all(torch.equal(a, b) for a, b in zip(got, appended))
    # item b's two sums are those of the batch-of-one call on its own rows
    for b, n in enumerate(lengths):
        one = V.vae_losses(target[b:b + 1, :, :n], recon[b:b + 1, :, :n], mean[b:b + 1, :n >> S], logvar[b:b + 1, :n >> S], S)
        assert torch.equal(one[2][0], got[2][b]) and torch.equal(one[3][0], got[3][b]), (name, b, n)
    # numpy in -> floats and numpy out
    host = V.vae_losses(*(a.cpu().numpy() for a in (target, recon, mean, logvar)), S, lengths=list(lengths))
    assert isinstance(host[0], float) and isinstance(host[2], np.ndarray)
    assert host[0] == float(got[0]) and host[1] == float(got[1]) and np.array_equal(host[3], got[3].cpu().numpy())


@pytest.mark.parametrize("name", list(SHAPES))
def test_poisoned_tails_are_never_read(recon_of, name):
    target, recon, mean, logvar, S, lengths = recon_of(name)
    clean = V.vae_losses(torch.nan_to_num(target), recon, mean, logvar, S, lengths=lengths)
    r, m, lv = recon.clone(), mean.clone(), logvar.clone()
    for b, n in enumerate(lengths):
        r[b, :, n:] = NAN
        m[b, n >> S:] = NAN
        lv[b, n >> S:] = NAN
    assert torch.isnan(target).any() and torch.isnan(r).any() and torch.isnan(m).any() and torch.isnan(lv).any()
    got = V.vae_losses(target, r, m, lv, S, lengths=lengths)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, clean))


@pytest.mark.parametrize("name", list(SHAPES))
def test_unmasked_form_and_zero_tails(recon_of, name):
    target, recon, mean, logvar, S, lengths = recon_of(name)
    target = torch.nan_to_num(target)
    got = V.vae_losses(target, recon, mean, logvar, S)
    want = losses_np(*(a.cpu().numpy() for a in (target, recon, mean, logvar)), S)
    bars = _bars(target, recon, mean, logvar, S, None)
    _compare(name + " unmasked", got, want, bars)
    # the encoder stores 0 past an item's latent rows, and -0.5 (1 + 0 - 0 - e^0) = 0: the masked and the unmasked KL
    # numerators agree, item by item
    masked = V.vae_losses(target, recon, mean, logvar, S, lengths=lengths)
    diff = (got[3].double() - masked[3].double()).abs().cpu().numpy()
    masked_bars = _bars(target, recon, mean, logvar, S, lengths)[3]
    print(f"{name}: masked vs unmasked KL sums differ by at most {diff.max():.3e}")
    assert (diff <= masked_bars).all()


def test_an_all_empty_batch_gives_zero():
    enc, _ = pair_of("small")
    B, T = 3, 70
    nan3 = lambda *shape: torch.full(shape, NAN, device=DEV)
    got = V.vae_losses(nan3(B, enc.n_mels, T), nan3(B, enc.n_mels, T), nan3(B, T // 2, enc.latent_dim), nan3(B, T // 2, enc.latent_dim),
                       enc.down_stages, lengths=[0] * B)
    assert float(got[0]) == 0.0 and float(got[1]) == 0.0 and not got[2].any() and not got[3].any()


def test_abi_errors_leave_out_untouched():
    lib = _native.load()
    B, n_mels, T, latent, S = 2, 80, 8, 16, 2
    target, recon = torch.zeros(B, n_mels, T, device=DEV), torch.ones(B, n_mels, T, device=DEV)
    mean, logvar = torch.zeros(B, T >> S, latent, device=DEV), torch.zeros(B, T >> S, latent, device=DEV)
    lengths = torch.tensor([8, 4], dtype=torch.int32, device=DEV)
    need = ctypes.c_uint64()
    assert lib.iris_vae_losses_workspace_bytes(B, n_mels, T, latent, S, ctypes.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    sentinel = 12345.0
    out = torch.full((2 + 2 * B,), sentinel, device=DEV)
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(tensors=(target, recon, mean, logvar), T=T, out=out, ws=ws, ws_bytes=need.value):
        rc = lib.iris_vae_losses(*(p(t) for t in tensors), B, n_mels, T, latent, S, p(lengths), p(out), p(ws), ctypes.c_uint64(ws_bytes), stream)
        torch.cuda.synchronize(DEV)
        return rc
    for i in range(4):
        tensors = [target, recon, mean, logvar]
        tensors[i] = None
        assert call(tensors=tensors) == _native.STATUS_INVALID_ARGUMENT
    assert call(out=None) == _native.STATUS_INVALID_ARGUMENT and call(ws=None) == _native.STATUS_INVALID_ARGUMENT
    assert call(ws_bytes=need.value - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
    assert call(T=6) == _native.STATUS_INVALID_ARGUMENT and b"multiple" in lib.iris_hifigan_last_error()
    assert bool((out == sentinel).all())
    assert call() == 0
    # |0 - 1| over 8 and 4 frames of 80 bins; the KL of mean = logvar = 0 is 0
    assert out[2:].tolist() == [640.0, 320.0, 0.0, 0.0] and abs(float(out[0]) - 1.0) < 1e-6 and float(out[1]) == 0.0
