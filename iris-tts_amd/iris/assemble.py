"""Silence trim and sentence join on the device (``iris_assemble_*``, csrc/assemble.h): a ragged batch of waveforms -- the
sentences of one text -- becomes ONE waveform.  Per item ``Assembler`` takes the decision of ``librosa.effects.trim(y, top_db=,
ref=np.max, frame_length=, hop_length=)``; librosa cannot be imported here, so the contract is the rules below, held by a
float64 and an fp32 numpy restatement (``tests/assemble_restatement.py``).

With ``F = frame_length``, ``H = hop_length`` (``F`` even, ``H`` dividing ``F / 2``) and item b owning ``L_b`` samples:

    ``T_b = L_b // H + 1`` frames; frame t covers samples ``[t H - F / 2, t H + F / 2)``, 0 outside the item; ``mse[t] = sum(y^2) / F``
    ``ref_b = max_t mse[t]``                                       (``ref ** 2`` with an absolute reference amplitude ``ref``)
    frame t is non-silent iff ``max(mse[t], 1e-10) > max(ref_b, 1e-10) * 10 ** (-top_db / 10)``          (fp32, strict)
    ``start = t0 H``, ``end = min(L_b, (t1 + 1) H)`` for the first / last non-silent frame (none: 0, 0)
    ``start' = max(0, start - pad)``, ``end' = min(L_b, end + pad)``, ``len_b = end' - start'``
    a non-empty item is stored from ``off_b = sum(len_a, a < b) + pause * (non-empty items a < b)``
    ``out[off_b + n] = (y[b, start' + n] * fade_in[n]) * fade_out[len_b - 1 - n]``, a raised-cosine ramp of ``fade`` samples

This is ``amplitude_to_db(rms, ref, top_db=None) > -top_db`` without the logarithms, so an item of digital silence keeps every
frame with ``ref=None``, as in librosa.  An empty item contributes neither samples nor a pause.  A call is 3 launches on the
current stream; the host never reads a length, and two calls agree bit for bit.

``MelToWavePipeline(..., assemble=Assembler(...))`` runs the join behind the denoiser and the stretch and in front of the output
stage.  A chunked form is not built: the reference level is the whole item's maximum.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _native
from ._native_model import _DeviceStage, _ptr, _stream, _take_shapes


class Assembler(_DeviceStage):
    """Trim and join with fixed parameters, resident on one GPU (``device``, or the current one); the handle -- it owns the
    ramp -- is built on first use.  ``ref``: None for the item's own maximum (``ref=np.max``), or an absolute amplitude > 0.
    ``pad``: samples kept beyond the decision's bounds on either side; ``fade``: samples of the ramp at every cut;
    ``pause``: samples of silence between two non-empty items."""

    _abi_name = "assemble"

    def __init__(self, frame_length: int = 2048, hop_length: int = 512, top_db: float = 60.0, ref: Optional[float] = None,
                 pad: int = 0, fade: int = 0, pause: int = 0, device: Optional[torch.device] = None):
        super().__init__(device)
        for name, v in (("frame_length", frame_length), ("hop_length", hop_length), ("pad", pad), ("fade", fade), ("pause", pause)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if ref is not None and not float(ref) > 0.0:
            raise ValueError(f"ref must be None (the item's own maximum) or an amplitude above 0, got {ref!r}")
        self.frame_length, self.hop_length = int(frame_length), int(hop_length)
        self.top_db, self.ref = float(top_db), None if ref is None else float(ref)
        self.pad, self.fade, self.pause = int(pad), int(fade), int(pause)
        self.capacity(0, 0)                                    # the library's own refusals, before any device work

    def get_config(self) -> dict:
        return {"frame_length": self.frame_length, "hop_length": self.hop_length, "top_db": self.top_db, "ref": self.ref,
                "pad": self.pad, "fade": self.fade, "pause": self.pause}

    def native_config(self) -> "_native.AssembleConfig":
        return _native.AssembleConfig(self.frame_length, self.hop_length, self.top_db, 0.0 if self.ref is None else self.ref,
                                      self.pad, self.fade, self.pause)

    # -- host-only queries -------------------------------------------------------------------
    def capacity(self, B: int, L: int) -> int:
        """``cap = B L + pause (B - 1)``: the samples ``join_device`` returns for a batch ``[B, L]`` (no device needed)."""
        return self._query("out_capacity", B, L)

    def launch_count(self, B: int, L: int) -> int:
        """Kernel launches of one call: 3 (a dry run on the host, no device needed)."""
        return self._query("launch_count", B, L)

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._query("workspace_bytes", B, L)

    def _workspace_layout(self, B: int, L: int):
        """``({buffer: (offset, shape)}, words)``: ``AsWorkspace`` (csrc/iris_assemble.hip) restated -- ``mse [B, L // H + 1]`` fp32,
        then ``spans [B, 2]`` int32.  Host only."""
        return _take_shapes({"mse": (B, L // self.hop_length + 1), "spans": (B, 2)})

    def _read_buffers(self, B: int, L: int) -> dict:
        """Test-only: copies of ``mse`` (fp32; row b is stored up to ``T_b``) and ``spans`` as the last call of shape (B, L)
        left them in the workspace."""
        layout, _ = self._workspace_layout(B, L)
        (o_m, s_m), (o_s, s_s) = layout["mse"], layout["spans"]
        return {"mse": self._workspace.view(torch.float32)[o_m:o_m + s_m[0] * s_m[1]].view(s_m).clone(),
                "spans": self._workspace.view(torch.int32)[o_s:o_s + 2 * B].view(s_s).clone()}

    # -- the calls ---------------------------------------------------------------------------
    def join_device(self, wav, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``wav [B, L]`` fp32, host or device -> ``(out [cap], offsets [B + 1] int32, spans [B, 2] int32)`` on the device,
        ``cap = capacity(B, L)``: the trimmed items end to end from ``offsets[b]`` on, ``pause`` zeros between two non-empty
        ones, ``offsets[B]`` the total and ``out[total:]`` 0; ``spans[b] = (start', end')`` in item b's own samples.
        Asynchronous on the current stream, 3 launches, nothing synchronises; two calls agree bit for bit.

        ``lengths`` (a host sequence of integers or an integer tensor ``[B]``, which the host never reads) and ``row_scale``:
        item b owns ``min(L, lengths[b] * row_scale)`` samples -- mel frames and the vocoder's hop, or a stretch's ``counts``
        and 1 -- and nothing past them is read.  Item b's span and samples are those of its batch-of-one call.
        ``offsets[B:]`` is the ``lengths`` of a following ``Resampler.forward(out[None], lengths=, row_scale=1)``."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        cap = self.capacity(B, L)
        out = torch.empty((cap,), dtype=torch.float32, device=self._device)
        offsets = torch.empty((B + 1,), dtype=torch.int32, device=self._device)      # the stage stores every element itself
        spans = torch.empty((B, 2), dtype=torch.int32, device=self._device)
        if B == 0 or L == 0:
            return out.zero_(), offsets.zero_(), spans.zero_()
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_assemble_forward", lib.iris_assemble_forward(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(out), _ptr(spans), _ptr(offsets), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, offsets, spans

    def join(self, wav, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(out[:total], spans)``: ``join_device``, then ONE read-back -- the total, which sizes the result; this is the only
        place the stage synchronises."""
        out, offsets, spans = self.join_device(wav, lengths=lengths, row_scale=row_scale)
        return out[:int(offsets[-1].item())], spans

    def trim_device(self, wav, lengths=None, row_scale: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """The same bounds with every item kept in its own row: ``(out [B, L], counts [B] int32)`` on the device,
        ``out[b, :counts[b]]`` item b's trimmed and faded samples, the rest of the row 0, ``counts`` the next stage's lengths
        (``row_scale=1``).  The same 3 launches; ``pause`` plays no part."""
        lib, wav, lengths, B, L = self._ragged_wave(wav, lengths, row_scale)
        out = torch.empty((B, L), dtype=torch.float32, device=self._device)
        counts = torch.empty((B,), dtype=torch.int32, device=self._device)
        if B == 0 or L == 0:
            return out, counts.zero_()
        ws = self._ws(B, L)
        with torch.cuda.device(self._device):
            _native.check("iris_assemble_trim_ragged", lib.iris_assemble_trim_ragged(
                self._handle, _ptr(wav), B, L, _ptr(lengths), int(row_scale), _ptr(out), None, _ptr(counts), _ptr(ws),
                ctypes.c_uint64(ws.numel()), _stream(self._device)))
        return out, counts
