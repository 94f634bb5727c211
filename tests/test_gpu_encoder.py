"""The device phoneme encoder, duration head and length regulator (iris.encoder, csrc/text_encoder.h) on the MI355X against
the numpy restatement of the reference's classes (tests/encoder_restatement.py).  Every parameter is randomised
(encoder_cases.make_models).

The bar is measured, not guessed.  For exactly the inputs of encoder_cases.CASES,
``e32 = max|restatement(fp32) - restatement(fp64)| / max(1, max|fp64|)`` on the CPU was
    case                  enc_out    pred       block 0    head layer 0
    small   1x1           3.60e-07   4.66e-08   1.66e-07   4.06e-07
    small   1x7           3.96e-07   1.92e-06   1.81e-07   4.80e-07
    small   1x32          2.65e-07   5.14e-07   2.12e-07   4.90e-07
    small   1x33          4.04e-07   7.29e-07   2.07e-07   4.66e-07
    small   1x65          4.19e-07   4.92e-07   1.96e-07   4.50e-07
    small   3x40 ragged   3.25e-07   4.06e-07   1.76e-07   4.48e-07
    default 1x7           5.57e-07   6.37e-07   2.44e-07   6.88e-07
    default 1x33          5.49e-07   8.34e-07   2.82e-07   7.64e-07
    default 1x65          5.43e-07   1.18e-06   2.89e-07   6.72e-07
    default 3x37 ragged   4.51e-07   1.22e-06   3.42e-07   7.72e-07
    default 1x1000        7.77e-07   9.04e-07   3.02e-07   8.48e-07
so the bar is 4 x 1.92e-06 = 7.68e-06 (encoder_cases.BAR; tests/test_encoder.py re-measures the table) -- the factor 4
allows for another summation order, expf and the division by the square root -- far inside the project's 1e-4 parity claim;
no scaling of the test weights was needed.  On these cases the restatement's frames run from 1 (213 positions of the
1 x 1000 case are clipped up from 0) to 132.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris import encoder as E
from iris.pipeline import MelToWavePipeline

import encoder_restatement as R
from encoder_cases import BAR, CASES, CONFIGS, RAGGED, TAP_CASE, case_id, decided, make_models, reference, valid_mask

pytestmark = pytest.mark.gpu
assert BAR <= 1e-4
DEV = torch.device("cuda", 0)


def _err(got, want):
    return float(np.abs(np.asarray(got).astype(np.float64) - want).max() / max(1.0, np.abs(want).max()))


_runs = {}


def run(case):
    """The device stage on one case, once: dict(enc_out, pred, frames, offsets, totals) as numpy, plus the taps of TAP_CASE."""
    if case not in _runs:
        name, B, P, lengths = case
        enc, head = make_models(name)
        ids = torch.from_numpy(reference(case)["ids"].copy()).to(DEV)
        enc_out = enc.forward_device(ids, lengths)
        pred, frames, offsets, totals = head.forward_device(enc_out, lengths)
        out = dict(enc_out=enc_out, pred=pred, frames=frames, offsets=offsets, totals=totals)
        if case == TAP_CASE:
            out["block0"], out["layer0"] = enc._read_block0(B, P), head._read_layer0(B, P)
        _runs[case] = {k: v.cpu().numpy() for k, v in out.items()}
    return _runs[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_parity(case):
    want, got = reference(case), run(case)
    assert got["enc_out"].shape == want["enc_out"].shape and got["enc_out"].dtype == np.float32
    e_enc, e_pred = _err(got["enc_out"], want["enc_out"]), _err(got["pred"], want["pred"])
    print(f"{case_id(case)}: enc_out {e_enc:.3e} pred {e_pred:.3e} bar {BAR:.3e}")
    assert e_enc <= BAR and e_pred <= BAR, (e_enc, e_pred, BAR)


def test_intermediate_taps():
    want, got = reference(TAP_CASE), run(TAP_CASE)
    errs = {k: _err(got[k], want[k]) for k in ("block0", "layer0")}
    print("taps", {k: f"{v:.3e}" for k, v in errs.items()}, f"bar {BAR:.3e}")
    assert got["block0"].shape == want["block0"].shape and got["layer0"].shape == want["layer0"].shape
    assert all(v <= BAR for v in errs.values()), errs


def test_integer_frames_offsets_and_totals():
    undecided = positions = 0
    for case in CASES:
        lengths = case[3]
        got, m, dec = run(case), valid_mask(case), decided(case)
        want = R.predict_frames(reference(case)["pred"], lengths)
        bad = int((got["frames"][dec] != want[dec]).sum())
        print(f"{case_id(case)}: {int(dec.sum())} of {int(m.sum())} positions decided, {bad} differ")
        assert bad == 0, case_id(case)
        assert np.all(got["frames"][m] >= 1) and np.all(got["frames"][~m] == 0)
        # the scan is exact on the frames the device itself predicted
        f = got["frames"].astype(np.int64)
        assert np.array_equal(got["offsets"], np.concatenate([np.zeros((f.shape[0], 1), np.int64), np.cumsum(f, axis=1)], axis=1))
        assert np.array_equal(got["totals"], f.sum(axis=1))
        undecided += int((m & ~dec).sum()); positions += int(m.sum())
    assert undecided <= 0.02 * positions, (undecided, positions)


def test_length_regulator_is_np_repeat_with_zero_padding():
    rng = np.random.default_rng(5)
    B, P, Ed = 3, 45, 48
    enc = rng.standard_normal((B, P, Ed)).astype(np.float32)
    d = rng.integers(0, 4, (B, P)).astype(np.int32)
    d[0, 3:6] = 0; d[0, 10] = 40; d[1, :] = 1; d[1, 0] = 0; d[2, -1] = 40
    d[0, 0] += (-int(d[0].sum())) % 4                      # item 0: a multiple of the factor already
    d[2, 0] += (1 - int(d[2].sum())) % 4                   # item 2: one past a multiple
    assert d[0].sum() % 4 == 0 and d[2].sum() % 4 == 1 and len({int(t) for t in d.sum(axis=1)}) == 3
    offsets, totals = E.scan_device(torch.from_numpy(d).to(DEV))
    assert np.array_equal(offsets.cpu().numpy(), np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(d, axis=1)], axis=1))
    assert np.array_equal(totals.cpu().numpy(), d.sum(axis=1))
    for factor in (1, 4):
        got = E.length_regulate(enc, d, factor=factor)
        want = R.length_regulate(enc, d, factor=factor)
        assert got.shape == want.shape and np.array_equal(got, want), factor
    for b in (0, 2):                                        # one item: its own total decides the padding
        got = E.length_regulate(enc[b:b + 1], d[b:b + 1], factor=4)
        assert got.shape[1] == -(-int(d[b].sum()) // 4) * 4 and np.array_equal(got, R.length_regulate(enc[b:b + 1], d[b:b + 1], factor=4))
    dev_out = E.length_regulate(torch.from_numpy(enc).to(DEV), d)
    assert isinstance(dev_out, torch.Tensor) and dev_out.is_cuda and np.array_equal(dev_out.cpu().numpy(), R.length_regulate(enc, d))
    # the reference docstring's example
    e = np.arange(1, 4, dtype=np.float32)[None, :, None] * np.ones((1, 3, 4), np.float32)
    assert E.length_regulate(e, np.array([[2, 3, 1]]))[0, :, 0].tolist() == [1, 1, 2, 2, 2, 3]


@pytest.mark.parametrize("case", RAGGED, ids=case_id)
def test_batch_independence(case):
    name, B, P, lengths = case
    enc, head = make_models(name)
    got, ids = run(case), reference(case)["ids"]
    for b, n in enumerate(lengths):
        one = torch.from_numpy(ids[b:b + 1, :n].copy()).to(DEV)
        enc_b = enc.forward_device(one)
        pred_b, frames_b, _, totals_b = head.forward_device(enc_b)
        assert np.array_equal(enc_b.cpu().numpy()[0], got["enc_out"][b, :n]), b
        assert np.array_equal(pred_b.cpu().numpy()[0], got["pred"][b, :n]), b
        assert np.array_equal(frames_b.cpu().numpy()[0], got["frames"][b, :n]), b
        assert int(totals_b.item()) == int(got["totals"][b])
        assert np.all(got["enc_out"][b, n:] == 0) and np.all(got["pred"][b, n:] == 0) and np.all(got["frames"][b, n:] == 0)


def test_determinism_device_tensors_and_mask():
    case = RAGGED[0]
    name, B, P, lengths = case
    enc, head = make_models(name)
    ids_np = reference(case)["ids"]
    ids = torch.from_numpy(ids_np.copy()).to(DEV)
    a, b = enc.forward_device(ids, lengths), enc.forward_device(ids, lengths)
    assert torch.equal(a, b) and a.is_cuda and np.array_equal(a.cpu().numpy(), run(case)["enc_out"])
    pa, pb = head.forward_device(a, lengths), head.forward_device(a, lengths)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    mask = E.create_padding_mask(np.asarray(lengths), P)
    via_mask, via_lengths = enc(ids_np, mask=mask), enc(ids_np, lengths=np.asarray(lengths))
    assert isinstance(via_mask, np.ndarray) and np.array_equal(via_mask, via_lengths) and np.array_equal(via_mask, a.cpu().numpy())
    dev_out = enc(ids, mask=torch.from_numpy(mask).to(DEV))
    assert isinstance(dev_out, torch.Tensor) and dev_out.is_cuda and torch.equal(dev_out, a)
    d = head(a, lengths=lengths)
    assert d.is_cuda and tuple(d.shape) == (B, P, 1) and torch.equal(d[..., 0], pa[0])
    assert np.array_equal(head(a.cpu().numpy(), lengths=lengths)[..., 0], pa[0].cpu().numpy())
    assert np.array_equal(E.predict_durations(a.cpu().numpy(), head, lengths), pa[1].cpu().numpy())
    assert torch.equal(E.predict_durations(a, head, lengths), pa[1])


def test_chain_phonemes_to_waveform():
    from iris._engine import GeneratorEngine
    from iris._weights import GeneratorConfig, seeded_state_dict
    from iris.postnet import PostNet
    from vae_cases import make_vae
    enc, head = make_models("default")
    vae = make_vae("default")
    cfg = GeneratorConfig()
    engine = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.1, post_gain=1.0), DEV)
    postnet = PostNet(n_mels=80, num_layers=3, channels=256, kernel_size=5, seed=5)
    pipe = MelToWavePipeline(postnet, engine.forward, device=DEV, acoustic=vae, text=(enc, head))
    ids = reference(("default", 1, 7, None))["ids"]
    cond, per_item = E.frame_conditioning(enc, head, ids, factor=vae.downsample_factor)
    T = cond.shape[1]
    assert cond.is_cuda and T % 4 == 0 and 0 <= T - per_item[0] < 4 and per_item[0] == int(run(("default", 1, 7, None))["totals"][0])
    z = torch.from_numpy(np.random.default_rng(3).standard_normal((1, T // 4, vae.latent_dim)).astype(np.float32)).to(DEV)
    refined = postnet.forward_device(vae.generate_device(cond, z)[0])
    want = engine.forward(refined).clone()
    got, frames = pipe.infer_from_phonemes(ids, z_prior=z)
    assert frames == per_item and tuple(got.shape) == (1, T * 256) and torch.equal(got, want)
    want_pcm = engine.forward_pcm16(refined).clone()
    got_pcm, _ = pipe.infer_from_phonemes(ids, z_prior=z, pcm16=True)
    assert got_pcm.dtype == torch.int16 and torch.equal(got_pcm, want_pcm)
    # B = 2, ragged: a list, item i bit for bit the B = 1 call on its own ids
    ids2 = reference(("default", 3, 37, (1, 37, 20)))["ids"][1:3, :9]
    lengths = np.array([9, 4])
    rng = np.random.default_rng(4)
    singles, zs = [], []
    for i in range(2):
        _, n_i = E.frame_conditioning(enc, head, ids2[i:i + 1, :lengths[i]], factor=4)
        zs.append(torch.from_numpy(rng.standard_normal((1, -(-n_i[0] // 4), vae.latent_dim)).astype(np.float32)).to(DEV))
        singles.append(pipe.infer_from_phonemes(ids2[i:i + 1, :lengths[i]], z_prior=zs[i], pcm16=True))
    batch, frames2 = pipe.infer_from_phonemes(ids2, lengths=lengths, z_prior=zs, pcm16=True)
    assert isinstance(batch, list) and frames2 == [s[1][0] for s in singles]
    for i in range(2):
        assert torch.equal(batch[i], singles[i][0][0]), i
    # durations= replaces the head
    durs = np.array([[3, 0, 5, 1, 1, 2, 1]])
    wav, frames3 = pipe.infer_from_phonemes(ids, durations=durs, pcm16=True)
    assert frames3 == [13] and tuple(wav.shape) == (1, 16 * 256)
    cond3, _ = E.frame_conditioning(enc, None, ids, durations=durs, factor=4)
    enc_out = run(("default", 1, 7, None))["enc_out"]
    assert np.array_equal(cond3.cpu().numpy(), R.length_regulate(enc_out, durs, factor=4))
    with pytest.raises(ValueError, match="max_frames"):
        E.frame_conditioning(enc, head, ids, max_frames=per_item[0] - 1)


def test_abi_errors_leave_the_outputs_untouched():
    lib = _native.load()
    enc, head = make_models("small")
    fp = ctypes.POINTER(ctypes.c_float)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    sentinel = 12345.0
    B, P, Ed = 1, 8, enc.embed_dim
    he, hd = ctypes.c_void_p(), ctypes.c_void_p()
    eb, db = enc.blob(), head.blob()
    ecfg, dcfg = enc.native_config(), head.native_config()
    with torch.cuda.device(DEV):
        assert lib.iris_phoneme_encoder_create(ctypes.byref(ecfg), eb.ctypes.data_as(fp), ctypes.c_uint64(eb.size - 1),
                                               ctypes.byref(he)) == _native.STATUS_INVALID_ARGUMENT
        assert b"weight blob" in lib.iris_hifigan_last_error() and not he.value
        bad = enc.native_config(); bad.num_heads = 4
        assert lib.iris_phoneme_encoder_create(ctypes.byref(bad), eb.ctypes.data_as(fp), ctypes.c_uint64(eb.size),
                                               ctypes.byref(he)) == _native.STATUS_UNSUPPORTED and not he.value
        badd = head.native_config(); badd.kernel_size = 4
        assert lib.iris_duration_predictor_create(ctypes.byref(badd), db.ctypes.data_as(fp), ctypes.c_uint64(db.size),
                                                  ctypes.byref(hd)) == _native.STATUS_UNSUPPORTED and not hd.value
        assert lib.iris_duration_predictor_create(ctypes.byref(dcfg), db.ctypes.data_as(fp), ctypes.c_uint64(db.size + 1),
                                                  ctypes.byref(hd)) == _native.STATUS_INVALID_ARGUMENT and not hd.value
        assert lib.iris_phoneme_encoder_create(ctypes.byref(ecfg), eb.ctypes.data_as(fp), ctypes.c_uint64(eb.size), ctypes.byref(he)) == 0
        assert lib.iris_duration_predictor_create(ctypes.byref(dcfg), db.ctypes.data_as(fp), ctypes.c_uint64(db.size), ctypes.byref(hd)) == 0
    try:
        big = enc.max_length + 1
        ids = torch.zeros((1, big), dtype=torch.int32, device=DEV)
        out = torch.full((1, big, Ed), sentinel, device=DEV)
        ws = torch.empty(max(enc.workspace_bytes(B, P), head.workspace_bytes(B, P)), dtype=torch.uint8, device=DEV)
        pred = torch.full((B, P), sentinel, device=DEV)
        ints = [torch.full(s, 12345, dtype=torch.int32, device=DEV) for s in ((B, P), (B, P + 1), (B,))]

        def enc_fwd(P_, ws_bytes, null_out=False):
            return lib.iris_phoneme_encoder_forward(he, vp(ids), None, B, P_, None if null_out else vp(out), vp(ws), ctypes.c_uint64(ws_bytes), stream)

        def dur_fwd(ws_bytes, null_pred=False):
            return lib.iris_duration_predictor_forward(hd, vp(out), None, B, P, None if null_pred else vp(pred), vp(ints[0]), vp(ints[1]), vp(ints[2]),
                                                       vp(ws), ctypes.c_uint64(ws_bytes), stream)
        assert enc_fwd(big, ws.numel()) == _native.STATUS_INVALID_ARGUMENT and b"max_length" in lib.iris_hifigan_last_error()
        assert enc_fwd(0, ws.numel()) == _native.STATUS_INVALID_ARGUMENT
        assert enc_fwd(P, enc.workspace_bytes(B, P) - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
        assert enc_fwd(P, ws.numel(), null_out=True) == _native.STATUS_INVALID_ARGUMENT
        assert dur_fwd(head.workspace_bytes(B, P) - 1) == _native.STATUS_WORKSPACE_TOO_SMALL
        assert dur_fwd(ws.numel(), null_pred=True) == _native.STATUS_INVALID_ARGUMENT
        torch.cuda.synchronize(DEV)
        assert bool((out == sentinel).all()) and bool((pred == sentinel).all()) and all(bool((t == 12345).all()) for t in ints)
        assert enc_fwd(P, ws.numel()) == 0 and dur_fwd(ws.numel()) == 0
        torch.cuda.synchronize(DEV)
        assert not bool((out[:, :P] == sentinel).any()) and bool((out[:, P:] == sentinel).all())
        assert not bool((pred == sentinel).any()) and int(ints[2][0]) == int(ints[0].sum()) == int(ints[1][0, P])
    finally:
        lib.iris_phoneme_encoder_destroy(he)
        lib.iris_duration_predictor_destroy(hd)


def test_launch_budget():
    for name in CONFIGS:
        enc, head = make_models(name)
        c, d = enc.get_config(), head.get_config()
        for B, P in ((1, 1), (3, 40), (1, c["max_length"])):
            assert enc.launch_count(B, P) <= 5 * c["num_blocks"] + 2 and head.launch_count(B, P) <= d["num_layers"] + 2
    enc, head = make_models("default")
    assert enc.launch_count(1, 1000) == 22 and head.launch_count(1, 1000) == 4
