"""Every PostNet launch against its fmaf chain, on the launch's OWN input tensor (oracle/postnet_cases.py).

The PostNet runs the generic fp32 conv kernel (csrc/conv_mfma_f32.h) in forms no other chain test reaches: the tanh epilogue
(``out_act = 1``) in the 16-byte and in the scalar store path, channels-first staging at C_in = 80 with k = 5, C_out = 80 behind
C_in = 256, k = 5 at 256 channels, the 64-row (MT = 2) tiles, and ``postnet_residual_kernel``.  After a forward the layer
outputs still lie in the workspace (``PostNet._read_layers``: every layer of a 2- or 3-layer net, the layers L-3 .. L-1 of a
deeper one); a launch whose input AND output survive is judged:

* hidden layer:  |got - tanh_fp64(chain pre-activation)| <= TOL, every element finite;
* last layer:    ``np.array_equal(got, chain)``;
* output:        out[b, c, t] == float32(mel[b, c, t] + res[b, t, c]) bit for bit, exactly 0 past an item's length;
* ragged:        rows < lengths[b] of item b meet the same claims, the chain being that of mel[b, :, :lengths[b]] alone; the
                 mel is NaN at and past each item's length; hidden rows at or past it are unspecified and not judged.
Of a net of four or more layers that is the launches L-2 and L-1 (and the output); layer L-3's output survives but its input
does not.  The layout rule itself is pinned: the helper's total equals ``iris_postnet_workspace_bytes`` at every shape.

Configs (oracle/postnet_cases.CONFIGS): the table of the issue, with the one row it leaves open set to n_mels 6, 12 layers,
14 channels, k 7 (``iris_postnet_create`` accepts it; 14 is no multiple of 4, so the hidden layers take the scalar staging and
the scalar epilogue with the tanh), and "narrow2" (6, 2 layers, 12 channels, k 7) added so that the channels-first k = 7
launch, which a 12-layer net overwrites, is judged too.  Two weight seeds; dense T = 1 .. 97 at B = 1 and 3; ragged (6, 70),
(4, 70) and the (8, 2048) of tests/test_postnet_ragged.py, the one case with 64-row tiles at 256 CUs (re-checked with the
device's CU count; skipped with a message on a chip where that shape does not reach them).

TOL.  ``f32_cases.TOL_TANH`` = 2e-6, the project's bar for ``tanhf`` behind an exact chain.  Measured on the CPU over the
dense cases (pre-activations up to |27|): max |float32 tanh of the chain - tanh_fp64| = 6.02e-08 for numpy's fp32 tanh and
2.98e-08 (half an ulp below 1) for the correctly rounded one; 2e-6 is the larger and stands.
e32 (CPU, tests/test_oracle_postnet.py, 2 x 65 frames, both weight seeds): default 1.69e-07 / 2.35e-07, deeper 2.33e-07 /
2.37e-07, small 9.83e-08 / 1.24e-07, narrow 5.28e-08 / 5.73e-08, narrow2 1.15e-07 / 5.70e-08.
Worst tanh error per config as observed on the first run on an MI355X (measured on the DEVICE; every figure above is CPU only):
    default 8.09e-08 dense, 8.37e-08 ragged ((8, 2048), 64-row tiles: 8.03e-08);  deeper 8.16e-08;  small 7.55e-08;
    narrow 7.75e-08;  narrow2 7.63e-08
and every last layer and every output equal, bit for bit: no launch differed from its chain, no device code changed.
Every test prints its worst tanh error, the elements judged and its wall time (``pytest -s``).
"""
import time

import numpy as np
import pytest
import torch

from oracle import f32_cases as fc
from oracle import postnet_cases as pc

pytestmark = pytest.mark.gpu
TOL = max(fc.TOL_TANH, 6.02e-08)

_postnets = {}


def _postnet(config, seeds):
    if (config, seeds) not in _postnets:
        _postnets[(config, seeds)] = (pc.make_postnet(config, seeds), None)
        pn = _postnets[(config, seeds)][0]
        _postnets[(config, seeds)] = (pn, pc.folded_layers(pn))
    return _postnets[(config, seeds)]


def _cu():
    return torch.cuda.get_device_properties(torch.device("cuda", 0)).multi_processor_count


def _forward_and_judge(pn, layers, config, mel, lengths):
    """One forward; every claim.  Returns (worst tanh error, elements judged, launches judged)."""
    B, _, T = mel.shape
    L = pn.num_layers
    fed = mel
    if lengths is not None:
        fed = mel.copy()
        for b, n in enumerate(lengths):
            fed[b, :, n:] = np.nan
    out = pn.forward_device(torch.from_numpy(fed).cuda(), lengths=lengths)
    torch.cuda.synchronize()
    kept, total = pn._read_layers(B, T)
    assert total == pn.workspace_bytes(B, T), (config, B, T, total)
    assert sorted(kept) == list(range(max(0, L - 3), L)), sorted(kept)
    out = out.cpu().numpy()
    kept = {i: t.cpu().numpy() for i, t in kept.items()}                      # [B, T, C]
    worst, elements, launches = 0.0, 0, 0
    cu = _cu()
    for i in range(L):
        if i not in kept or not (i == 0 or i - 1 in kept):
            continue
        launches += 1
        wb = layers[i]
        chunk = pc.layer_chunk(wb, i)
        form = pc.kernel_form(pn, i, B, T, cu, ragged=lengths is not None)
        x_all = fed if i == 0 else kept[i - 1].transpose(0, 2, 1)
        items = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(n)) for b, n in enumerate(lengths) if n]
        for sl, n in items:
            x = np.ascontiguousarray(x_all[sl, :, :n])
            rows = pc.layer_rows(x.shape[0], n, wb)
            assert fc.n_rows(rows) >= fc.MIN_SHARE * n
            pre = pc.chain_layer(x, wb, chunk, rows)
            got = fc.co.take_rows(kept[i][sl, :n].transpose(0, 2, 1), rows)
            what = f"{config} {B}x{T}{'' if lengths is None else f' item {sl.start} of length {n}'} layer {i} [{form}]"
            if i < L - 1:
                worst = max(worst, pc.judge_hidden(got, pre, TOL, what))
            else:
                pc.judge_last(got, pre, what)
            elements += got.size
    pc.judge_output(out, mel, kept[L - 1], lengths, f"{config} {B}x{T} postnet_residual_kernel")
    elements += out.size
    return worst, elements, launches


DENSE = [(config, si, B) for config in pc.CONFIGS for si in range(len(pc.WEIGHT_SEEDS)) for B in pc.DENSE_B]


@pytest.mark.parametrize("config,si,B", DENSE, ids=[f"{c}-w{si}-B{B}" for c, si, B in DENSE])
def test_postnet_every_launch_is_its_chain_dense(config, si, B):
    pn, layers = _postnet(config, pc.WEIGHT_SEEDS[si])
    t0 = time.perf_counter()
    worst, elements, launches = 0.0, 0, 0
    for T in pc.DENSE_T:
        w, e, n = _forward_and_judge(pn, layers, config, pc.case_mel(config, B, T, 100 + T), None)
        worst, elements, launches = max(worst, w), elements + e, launches + n
    assert launches == len(pc.DENSE_T) * min(pn.num_layers, 2 if pn.num_layers > 3 else 3)
    print(f"postnet chain {config} w{si} B={B}: worst tanh error {worst:.3e} (bar {TOL:.1e}), {launches} launches, "
          f"{elements} elements judged in {time.perf_counter() - t0:.2f} s")


RAGGED = [(ci, si) for ci in range(len(pc.RAGGED)) for si in range(len(pc.WEIGHT_SEEDS))]


@pytest.mark.parametrize("ci,si", RAGGED, ids=[f"{pc.RAGGED[ci][0]}x{pc.RAGGED[ci][1]}-w{si}" for ci, si in RAGGED])
def test_postnet_every_launch_is_its_chain_ragged(ci, si):
    B, T, lengths = pc.RAGGED[ci]
    config = pc.RAGGED_CONFIG
    pn, layers = _postnet(config, pc.WEIGHT_SEEDS[si])
    cu = _cu()
    tiles = [pc.layer_tile(pn.n_mels if i == pn.num_layers - 1 else pn.channels, B, T, cu)[0] for i in range(pn.num_layers)]
    if (B, T) == (8, 2048):
        if cu == pc.CU:
            assert tiles == [2, 2, 1], tiles
        elif 2 not in tiles:
            pytest.skip(f"{cu} CUs: ({B}, {T}) does not reach the 64-row tiles here (it does at {pc.CU} CUs)")
    t0 = time.perf_counter()
    worst, elements, launches = _forward_and_judge(pn, layers, config, pc.case_mel(config, B, T, 201 + 2 * ci), lengths)
    assert launches == 3
    print(f"postnet chain ragged {B}x{T} w{si} (MT per layer {tiles}): worst tanh error {worst:.3e} (bar {TOL:.1e}), "
          f"{elements} elements judged in {time.perf_counter() - t0:.2f} s")
