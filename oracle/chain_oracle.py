"""ctypes binding of the fp32 fmaf-chain oracle (oracle/chain_oracle.c).  TEST INFRASTRUCTURE ONLY.

Tensors are fp32 numpy in the reference's layouts ([B, C, L] activations, Conv1d weights [C_out, C_in, k], ConvTranspose1d
weights [C_in, C_out, k]); ``rows`` is a list of output row ranges ``[(a, e), ...]`` and only those rows are returned,
concatenated along the last axis (``take_rows`` cuts another tensor the same way).  ``x`` is the layer's ACTIVATED input:
``lrelu32`` and ``mean32`` are the fp32 LeakyReLU and the MRF mean ((y0 + y1) + y2) / n with a true division.  ``chunk`` is
the kernel's CIC (``chunk_of`` reads it from a recorded kernel name).  ``variant`` selects a WRONG restatement.
"""
import ctypes
import re
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
ASCENDING, TAP_MAJOR, BIAS_FIRST, RES_FIRST = 1, 2, 4, 8
SLOPE = np.float32(0.1)
_lib = None


def load():
    global _lib
    if _lib is None:
        path = _HERE / "libchain_oracle.so"
        if not path.exists():
            raise FileNotFoundError(f"{path} not built: run `make -C {_HERE}`")
        lib = ctypes.CDLL(str(path))
        vp, i = ctypes.c_void_p, ctypes.c_int
        lib.chain_conv1d.restype = i
        lib.chain_conv1d.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp, i, i]
        lib.chain_conv_transpose1d.restype = i
        lib.chain_conv_transpose1d.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, vp, i, i]
        lib.chain_conv_post_preact.restype = i
        lib.chain_conv_post_preact.argtypes = [vp, vp, vp, vp, i, i, i, i, vp, i]
        lib.chain_fmaf.restype = None
        lib.chain_fmaf.argtypes = [vp, vp, vp, vp, ctypes.c_longlong]
        lib.chain_set_portable.argtypes = [i]
        lib.chain_uses_fma_unit.restype = i
        _lib = lib
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _wpack(w_co_ci_k):
    """[C_out, C_in, k] -> [k, C_in, C_out padded to a multiple of 16 with zeros]"""
    co, ci, k = w_co_ci_k.shape
    out = np.zeros((k, ci, -(-co // 16) * 16), dtype=np.float32)
    out[:, :, :co] = np.asarray(w_co_ci_k, dtype=np.float32).transpose(2, 1, 0)
    return out


def _cl(a):
    """[B, C, L] -> contiguous channels-last [B, L, C]"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 1))


def row_index(rows, limit):
    idx = np.concatenate([np.arange(a, e, dtype=np.int32) for a, e in rows]) if len(rows) else np.zeros(0, np.int32)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < limit), (rows, limit)
    return np.ascontiguousarray(idx)


def take_rows(t, rows):
    """The rows ``rows`` of [B, C, L] (or [B, L]), as the chain functions return them."""
    return t[..., row_index(rows, t.shape[-1])]


def lrelu32(x, slope=SLOPE):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x > 0, x, x * np.float32(slope)).astype(np.float32)


def mean32(ys, n=None):
    """((y0 + y1) + y2) / n in fp32: the reference's order and a true division."""
    s = np.asarray(ys[0], dtype=np.float32)
    for y in ys[1:]:
        s = s + np.asarray(y, dtype=np.float32)
    return (s / np.float32(n or len(ys))).astype(np.float32)


def _check(rc, fn):
    if rc != 0:
        raise ValueError(f"{fn} refused its arguments (status {rc})")


def chain_conv1d(x, w, b, dilation, chunk, rows, residual=None, variant=0):
    """Conv1d ('same' zero padding) + bias (+ residual) as the kernels' chain; [B, C_out, rows]."""
    B, Ci, L = x.shape
    Co, Ci_w, k = w.shape
    assert Ci_w == Ci and k % 2 == 1
    idx = row_index(rows, L)
    xc, wc, bc = _cl(x), _wpack(w), _f32(b)
    rc_ = None if residual is None else _cl(np.asarray(residual)[:, :, idx])
    out = np.empty((B, idx.size, Co), dtype=np.float32)
    _check(load().chain_conv1d(xc.ctypes.data, wc.ctypes.data, bc.ctypes.data, None if rc_ is None else rc_.ctypes.data,
                               out.ctypes.data, B, L, Ci, Co, k, int(dilation), int(chunk), idx.ctypes.data, idx.size,
                               int(variant)), "chain_conv1d")
    return out.transpose(0, 2, 1)


def chain_conv_transpose1d(x, w, b, stride, chunk, rows, variant=0):
    """ConvTranspose1d(k, stride, padding (k - stride) / 2) + bias, phase by phase with taps ascending; [B, C_out, rows]."""
    B, Ci, L = x.shape
    Ci_w, Co, k = w.shape
    assert Ci_w == Ci
    idx = row_index(rows, L * stride)
    xc, wc, bc = _cl(x), _wpack(np.asarray(w).transpose(1, 0, 2)), _f32(b)
    out = np.empty((B, idx.size, Co), dtype=np.float32)
    _check(load().chain_conv_transpose1d(xc.ctypes.data, wc.ctypes.data, bc.ctypes.data, out.ctypes.data, B, L, Ci, Co, k,
                                         int(stride), int(chunk), idx.ctypes.data, idx.size, int(variant)),
           "chain_conv_transpose1d")
    return out.transpose(0, 2, 1)


def chain_conv_post_preact(x, w, b, rows):
    """conv_post before tanh: bias, then taps ascending, channels ascending; [B, rows]."""
    B, C, L = x.shape
    assert w.shape[0] == 1 and w.shape[1] == C
    k = w.shape[2]
    idx = row_index(rows, L)
    xc, wc, bc = _cl(x), np.ascontiguousarray(_f32(w)[0].T), _f32(b)
    out = np.empty((B, idx.size), dtype=np.float32)
    _check(load().chain_conv_post_preact(xc.ctypes.data, wc.ctypes.data, bc.ctypes.data, out.ctypes.data, B, L, C, k,
                                         idx.ctypes.data, idx.size), "chain_conv_post_preact")
    return out


def fmaf32(a, b, c):
    """``fmaf(a, b, c)`` element by element in fp32 (broadcast first): ONE rounding, where numpy's ``a * b + c`` has two."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), np.asarray(c, dtype=np.float32))
    a, b, c = _f32(a), _f32(b), _f32(c)
    out = np.empty(a.shape, dtype=np.float32)
    load().chain_fmaf(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, out.size)
    return out


# ---- the chunk (CIC) of a launch, from its recorded kernel name ---------------------------------------------------------
_CONV = re.compile(r"conv_mfma_f32_kernel(?:_ragged)?<(\d+), (\d+), (\d+), (\d+)>")
_MRF = re.compile(r"mrf_conv_mfma_f32_kernel(?:_ragged)?<(\d+), (\d+), (\d+), (\d+),")


def chunk_of(kernel, c_in):
    """Input channels per chunk of the launch ``kernel`` (a name recorded by ``describe_plan``).  The generic and the
    persistent MRF kernel carry their CIC as the fourth template argument; the other kernels have ONE instantiation of it
    and no argument to read: the ConvTranspose1d GEMM and the 16 x 16-job kernel stage 64 channels (``constexpr int CIC =
    64``, ``kSmallCic``), the fused pairs the whole C (C = 32 / 64: one chunk)."""
    m = _CONV.match(kernel) or _MRF.match(kernel)
    if m:
        return int(m.group(4))
    if kernel.startswith(("convt_mfma_f32_kernel", "mrf_small_f32_kernel")):
        return 64
    if kernel.startswith("mrf_pair_f32"):
        assert c_in in (32, 64), (kernel, c_in)
        return c_in
    raise ValueError(f"no chain chunk known for kernel {kernel!r}")
