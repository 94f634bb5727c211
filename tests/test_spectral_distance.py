"""The spectral-distance stage without a GPU: the float64 restatement against torch.stft, the identities the measures obey, the
frame rule at a length that is no multiple of the hop, the reference's own float32 error on the GPU tests' inputs (their bar),
the C ABI's declarations, the library's host-only answers and every refusal that needs no handle.  The device itself is
tests/test_gpu_spectral_distance.py's."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from iris import _native
from iris.metrics import CHUNK, DEFAULT_RESOLUTIONS, TILE_FRAMES, SpectralDistance, record_dtype

import spectral_distance_cases as C
import spectral_distance_restatement as R

REPO = Path(__file__).resolve().parents[1]
INVALID, UNSUPPORTED = 1, 4


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,win", R.DEFAULT)
@pytest.mark.parametrize("n", [20000, 768])
def test_float64_magnitudes_are_torch_stft(n_fft, hop, win, n):
    """Anchors the restatement to something not written here; 768 = 3 * 256 is shorter than n_fft / 2 at 2048 and no multiple of
    hop 512."""
    x = C.signal(5, n)
    w = torch.zeros(n_fft, dtype=torch.float64)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
    ref = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True,
                     pad_mode="constant", return_complex=True).abs().numpy().T
    own = R.magnitudes(x, n_fft, hop, win)
    assert own.shape == ref.shape == (1 + n // hop, n_fft // 2 + 1)
    worst = np.abs(own - ref).max() / np.abs(ref).max()
    print(f"n_fft {n_fft}, n {n}: {worst:.2e} of the largest magnitude")
    assert worst <= 1e-10


def test_float32_chain_tracks_float64():
    x = C.signal(6, 5000)
    for n_fft, hop, win in R.DEFAULT:
        a, b = R.magnitudes(x, n_fft, hop, win), R.magnitudes_f32(x, n_fft, hop, win)
        assert b.dtype == np.float32 and np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


# ---- identities ---------------------------------------------------------------------------------------------------------------
def test_a_signal_against_itself_is_at_distance_zero():
    x = C.signal(7, 6000)
    s = R.sums(x, x)
    assert not s["spec"][:, 0].any() and not s["spec"][:, 2].any() and s["spec"][:, 1].min() > 0
    assert s["wave"][0] == 0.0 and s["wave"][2] == 0.0 and s["wave"][1] > 0
    f = R.finish(s)
    assert not f["spectral_convergence"].any() and not f["log_stft_l1"].any() and f["snr_db"] == np.inf


@pytest.mark.parametrize("g", [0.5, 4.0])
def test_a_gain_gives_its_closed_forms(g):
    """``test = g ref`` (g a power of two, so the product is exact in float32): spectral convergence
    ``|1 - g|``, SNR ``-20 log10 |1 - g|``, and ``|ln g|`` for the log distance where every cell of both lies above the floor."""
    x = C.signal(8, 6000)
    y = (np.float32(g) * x).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), g * x.astype(np.float64))
    for n_fft, hop, win in R.DEFAULT:                        # the precondition of the third identity
        A = R.magnitudes(x, n_fft, hop, win)
        assert min(A.min(), g * A.min()) > R.FLOOR
    f = R.finish(R.sums(x, y))
    assert np.abs(f["spectral_convergence"] - abs(1 - g)).max() <= 1e-12
    assert abs(f["snr_db"] + 20 * np.log10(abs(1 - g))) <= 1e-10
    assert np.abs(f["log_stft_l1"] - abs(np.log(g))).max() <= 1e-9
    assert abs(f["mr_log_stft_l1"] - abs(np.log(g))) <= 1e-9 and abs(f["mr_spectral_convergence"] - abs(1 - g)) <= 1e-12


def test_three_rows_of_256_at_hop_512_have_two_frames_and_the_last_sample_counts():
    x, y = C.pair(9, 768)
    s = R.sums(x, y)
    assert s["frames"].tolist() == [7, 4, 2]
    y2 = y.copy()
    y2[-1] += np.float32(0.25)
    s2 = R.sums(x, y2)
    for r in range(3):
        assert s2["spec"][r, 0] != s["spec"][r, 0] and s2["spec"][r, 2] != s["spec"][r, 2] and s2["spec"][r, 1] == s["spec"][r, 1]
    assert s2["wave"][0] != s["wave"][0] and s2["wave"][1] == s["wave"][1]
    empty = R.sums(x[:0], y[:0])
    assert not empty["frames"].any() and not empty["spec"].any() and not empty["wave"].any()


def test_the_cases_are_what_they_are_chosen_for():
    ref, test, counts = C.ragged()
    assert counts == [0, 256, 768, 4096, 9472] and ref.shape == (5, 9472)
    assert all(np.isnan(ref[b, n:]).all() and np.isnan(test[b, n:]).all() and np.isfinite(ref[b, :n]).all() for b, n in enumerate(counts))
    assert 1 + counts[4] // 128 == 75 > 64 and counts[1] < 1024 and counts[2] < 1024 and counts[2] % 512
    assert all(C.DENSE_L % hop for _, hop, _ in R.DEFAULT) and 1 + C.DENSE_L // 512 == 40 > 32 and -(-C.DENSE_L // CHUNK) == 5
    assert len(C.items()) == 6


def test_e32_is_measurable_and_its_bar_stays_inside_1e_3():
    """The GPU tests' bar is 4 x e32 per output; no bar may be looser than 1e-3 relative."""
    e, worst = C.e32(), 0.0
    assert set(e) == {name for name, x, _ in C.items() if len(x)}
    for name, v in e.items():
        print(name, "spec", np.array2string(v["spec"], precision=2), "wave", v["wave"])
        assert not v["wave"].any()                           # no float32 step in the sample domain
        assert (v["spec"] > 0).all()
        worst = max(worst, float(v["spec"].max()))
    print(f"largest e32 = {worst:.3e}")
    assert 4 * worst <= 1e-3
    r64 = C.restated()
    assert all(s["spec"][:, 1].min() > 1.0 and s["wave"][1] > 1.0 for name, s in r64.items() if s["frames"].any())


# ---- the C ABI, host only --------------------------------------------------------------------------------------------------
def test_symbols_declared_and_loadable():
    header = (REPO / "include" / "iris_hifigan.h").read_text()
    declared = set(re.findall(r"\b(iris_spectral_distance_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.SPECTRAL_DISTANCE_SYMBOLS)
    assert {"iris_spectral_distance_create", "iris_spectral_distance_destroy", "iris_spectral_distance_workspace_bytes",
            "iris_spectral_distance_forward"} <= declared
    lib = _native.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert len(_native.SPECTRAL_DISTANCE_SYMBOLS["iris_spectral_distance_forward"][1]) == 13
    assert lib.iris_hifigan_abi_version() == _native.ABI_VERSION == 4


def _words(B, L, resolutions):
    """``SdWorkspace`` (csrc/iris_spectral_distance.hip) restated, in 4-byte words."""
    up = lambda n: (n + 63) & ~63
    mag = max(B * (L // hop + 1) * ((n_fft // 2 + 1 + 3) & ~3) for n_fft, hop, _ in resolutions)
    parts = sum(up(B * -(-(L // hop + 1) // TILE_FRAMES) * 6) for _, hop, _ in resolutions)
    return 2 * up(mag) + parts + up(B * -(-L // CHUNK) * 6)


@pytest.mark.parametrize("B,L", [(1, 20000), (5, 9472), (1, 1), (3, 256000)])
def test_workspace_bytes_and_a_dry_run_need_no_device(B, L):
    sd = SpectralDistance()
    assert sd.resolutions == DEFAULT_RESOLUTIONS and sd.get_config() == {"resolutions": [list(r) for r in DEFAULT_RESOLUTIONS]}
    assert sd.launch_count(B, L) == 3 * 3 + 2
    assert sd.launch_count(0, L) == 0 and sd.launch_count(B, 0) == 0
    assert sd.workspace_bytes(B, L) == max(256, 4 * _words(B, L, DEFAULT_RESOLUTIONS)) and sd.workspace_bytes(0, 0) == 256
    one = SpectralDistance([(512, 128, 400)])
    assert one.launch_count(B, L) == 5 and one.workspace_bytes(B, L) == 4 * _words(B, L, [(512, 128, 400)])
    assert record_dtype(3)["spectral_convergence"].shape == (3,)


def _status(fn, res, n_res, *args):
    out = (ctypes.c_uint64 if fn.endswith("bytes") else ctypes.c_int32)()
    arr = None if res is None else (ctypes.c_int32 * len(res))(*res)
    return getattr(_native.load(), fn)(arr, n_res, *args, ctypes.byref(out))


def test_refusals_come_before_any_device_work():
    good = [512, 128, 512, 1024, 256, 1024]
    for fn in ("iris_spectral_distance_workspace_bytes", "iris_spectral_distance_launch_count"):
        assert _status(fn, good, 2, 2, 1000) == 0
        assert _status(fn, good * 2, 4, 2, 1000) == 0 and _status(fn, good * 2 + [512, 128, 512], 5, 2, 1000) == INVALID     # more than 4
        assert _status(fn, good, 0, 2, 1000) == INVALID and _status(fn, None, 1, 2, 1000) == INVALID
        assert _status(fn, [512, 96, 512], 1, 2, 1000) == INVALID                             # hop does not divide n_fft
        assert _status(fn, [528, 132, 528], 1, 2, 1000) == UNSUPPORTED                        # n_fft % 32
        assert _status(fn, [512, 128, 513], 1, 2, 1000) == INVALID and _status(fn, [512, 0, 512], 1, 2, 1000) == INVALID
        assert _status(fn, [8192, 2048, 8192], 1, 2, 1000) == UNSUPPORTED and _status(fn, [512, 2, 512], 1, 2, 1000) == UNSUPPORTED
        assert _status(fn, good, 2, -1, 1000) == INVALID and _status(fn, good, 2, 2, -1) == INVALID
        assert _status(fn, good, 2, 65536, 10) == UNSUPPORTED and _status(fn, good, 2, 4096, 1 << 19) == UNSUPPORTED
        assert getattr(_native.load(), fn)((ctypes.c_int32 * 6)(*good), 2, 2, 1000, None) == INVALID
    lib = _native.load()
    h = ctypes.c_void_p()
    assert lib.iris_spectral_distance_create((ctypes.c_int32 * 3)(512, 96, 512), 1, ctypes.byref(h)) == INVALID
    assert lib.iris_spectral_distance_create((ctypes.c_int32 * 3)(512, 128, 512), 1, None) == INVALID
    assert lib.iris_spectral_distance_forward(None, None, None, 2, 100, None, 1, None, None, None, None, 0, None) == INVALID
    assert b"handle" in lib.iris_hifigan_last_error()
    with pytest.raises(_native.NativeCallError, match="resolutions"):
        SpectralDistance([(512, 128, 512)] * 5)
    with pytest.raises(_native.NativeCallError, match="does not divide"):
        SpectralDistance([(512, 96, 512)])
    with pytest.raises(_native.NativeCallError, match="multiple of 32"):
        SpectralDistance([(528, 132, 528)])
    with pytest.raises(ValueError, match="resolutions"):
        SpectralDistance([(512, 128)])
    with pytest.raises(ValueError, match="resolutions"):
        SpectralDistance([])


def test_shape_and_row_scale_refusals_come_before_the_handle():
    """Mismatched shapes and row_scale < 1 are refused on the host; without a device the first thing that could fail otherwise is
    the handle's creation, which these never reach."""
    sd = SpectralDistance()
    x = np.zeros((2, 100), np.float32)
    with pytest.raises(ValueError, match="row_scale"):
        sd.forward_device(x, x, lengths=[1, 1], row_scale=0)
    with pytest.raises(ValueError, match="float32"):
        sd.forward_device(torch.zeros((2, 100), dtype=torch.float64), x)
    with pytest.raises(ValueError, match="lengths"):
        sd.forward_device(x, x, lengths=[1, 1, 1])
    with pytest.raises(ValueError, match="one shape"):
        sd.forward_device(x, np.zeros((2, 99), np.float32))
    with pytest.raises(ValueError, match="one shape"):
        sd.measure(x, x[:1])
    f = sd.finish(np.zeros((1, 3, 3)), np.zeros((1, 3)), np.zeros((1, 3), np.int32))
    assert np.isnan(f["spectral_convergence"]).all() and np.isnan(f["log_stft_l1"]).all() and np.isnan(f["snr_db"][0])
