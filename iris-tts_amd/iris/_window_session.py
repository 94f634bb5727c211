"""Pushed waveform input, once, for the stages that have a windowed form with exact seams (``iris.denoiser``,
``iris.time_stretch``, ``iris.limiter``, ``iris.resample``).  A stage says which samples of an utterance a window settles
(its ``window_range`` / ``window_plan``: the finality rule, written down on the C side) and runs one window
(``forward_window``); what makes the concatenation of a session's pieces equal the whole-utterance call bit for bit is here:
one window per push over everything held, only what is settled leaves, and no sample the next window reads is dropped.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch


class _WindowSession:
    """The waveform of ONE utterance (or a batch of equal lengths) arrives piece by piece (``push``), settled output leaves
    with the push that settles it, ``flush`` ends the utterance.  ``_buf`` holds samples ``[_base, _total)``; a push appends
    its piece and runs ``_window`` once, then drops what that window says the next one no longer needs.

    A stage's session supplies ``_window(final) -> (piece, keep_from)`` -- the plan, the early-out that launches nothing,
    the call of ``forward_window`` and its own counters; ``keep_from`` is the first sample the next window must still hold
    (``_base`` keeps everything) -- and ``samples_emitted``.  ``dtype``: what the pieces are made of; ``piece_multiple``: a
    piece's length must be a multiple of it (the stage's ``hop_length``, where a window is whole frames by construction);
    ``_ragged_call``: the stage's own call that takes ragged batches, which a session does not."""

    _ragged_call = "forward_device(lengths=)"

    def __init__(self, dtype: torch.dtype = torch.float32, piece_multiple: int = 1):
        self._dtype, self._piece_multiple = dtype, int(piece_multiple)
        self._buf: Optional[torch.Tensor] = None          # samples [self._base, self._total) of the utterance, [B, n]
        self._base = 0
        self._total = 0
        self._closed = False

    @property
    def samples_received(self) -> int:
        return self._total

    @property
    def samples_buffered(self) -> int:
        return self._total - self._base

    def _empty(self) -> torch.Tensor:
        if self._buf is None:
            return torch.empty((0, 0), dtype=self._dtype)
        return self._buf.new_empty((self._buf.shape[0], 0), dtype=self._dtype)

    def _window(self, final: bool) -> Tuple[torch.Tensor, int]:
        raise NotImplementedError

    def _advance(self, final: bool) -> torch.Tensor:
        if self._buf is None:
            return self._empty()
        return self._keep(*self._window(final))

    def _keep(self, piece: torch.Tensor, keep_from: int) -> torch.Tensor:
        """What follows a window: drops the samples in front of ``keep_from`` and hands ``piece`` on."""
        keep_from = min(max(keep_from, self._base), self._total)
        if keep_from > self._base:
            self._buf = self._buf[:, keep_from - self._base:]
            self._base = keep_from
        return piece

    def push(self, wav_piece, lengths=None) -> torch.Tensor:
        """Appends ``wav_piece [B, n]`` fp32 (n >= 0, host or device) and returns the device tensor ``[B, m]`` of what became
        settled; ``m`` may be 0, and then nothing was launched."""
        self._append(wav_piece, lengths)
        return self._advance(final=False)

    def _append(self, wav_piece, lengths=None) -> None:
        """The checks of ``push`` and the piece behind what is held; no window runs."""
        if lengths is not None:
            raise ValueError(f"a session takes items of one length: ragged batches stay on {self._ragged_call}")
        if self._closed:
            raise RuntimeError("the session was flushed: open a new one for the next utterance")
        if not isinstance(wav_piece, torch.Tensor):
            wav_piece = torch.from_numpy(np.ascontiguousarray(np.asarray(wav_piece, dtype=np.float32)))
        if wav_piece.dim() != 2 or wav_piece.dtype != torch.float32:
            raise ValueError(f"expected a waveform piece [B, n] float32, got {wav_piece.dtype} {tuple(wav_piece.shape)}")
        if wav_piece.shape[1] % self._piece_multiple:
            raise ValueError(f"a piece of {wav_piece.shape[1]} samples is not a multiple of hop_length = {self._piece_multiple}")
        if self._buf is not None and wav_piece.shape[0] != self._buf.shape[0]:
            raise ValueError(f"every piece of an utterance has the same batch size: {self._buf.shape[0]}, got {wav_piece.shape[0]}")
        if self._buf is None:
            self._buf = wav_piece
        elif wav_piece.shape[1]:
            self._buf = torch.cat([self._buf, wav_piece.to(self._buf.device)], dim=1)
        self._total += int(wav_piece.shape[1])

    def flush(self) -> torch.Tensor:
        """Ends the utterance and returns what was waiting for context: the right edge of this last window is the true end,
        past which the whole-utterance call reads zeros too.  Further calls return an empty tensor."""
        if self._closed:
            return self._empty()
        out = self._advance(final=True)
        self._close()
        return out

    def _close(self) -> None:
        self._closed = True
        self._buf = None if self._buf is None else self._buf[:, :0]
        self._base = self._total


class _RangeSession(_WindowSession):
    """A ``_WindowSession`` over a stage whose plan is ``window_range(origin, Lw, final) -> (out_lo, out_count)``, the samples
    a window settles, with origins on multiples of ``step`` (the denoiser's hop; 1 for the limiter).  ``halo = (left, right)``
    is what an interior window loses on either side; a window may settle samples that have left already, which are cut off.
    A stage's session supplies ``_forward_window(final) -> out [B, out_count]``.

    ``_window`` is three steps, so that something else may run the window -- ``iris.stream_group`` runs those of many sessions
    in one call: ``_plan`` says which window is due and whether it launches, ``_forward_window`` runs it, ``_take`` books what
    came back.  The rules are in ``_plan`` and ``_take`` alone."""

    def __init__(self, stage, step: int, dtype: torch.dtype = torch.float32, piece_multiple: int = 1):
        super().__init__(dtype, piece_multiple)
        self._stage, self._step = stage, int(step)
        self._emitted = 0
        self.halo = self._measure_halo()

    @property
    def samples_emitted(self) -> int:
        return self._emitted

    def _measure_halo(self) -> Tuple[int, int]:
        """``(left, right)``, read off two windows long enough to settle something -- one that starts inside an utterance and
        ends with it, one that starts with it and ends inside."""
        step = span = self._step
        while True:
            (lo_l, n_l), (lo_r, n_r) = self._stage.window_range(step, span, True), self._stage.window_range(0, span, False)
            if n_l and n_r:
                return lo_l - step, span - (lo_r + n_r)
            if span > 1 << 28:
                raise ValueError("window_range settles no sample of any window: no halo can be derived")
            span *= 2

    def _forward_window(self, final: bool) -> torch.Tensor:
        raise NotImplementedError

    def _plan(self, final: bool) -> SimpleNamespace:
        """The window over everything held: ``origin``, ``Lw``, ``final``, the range ``lo``, ``count`` it settles, and
        ``launch``: whether that holds a sample not yet emitted."""
        lo, count = self._stage.window_range(self._base, self._total - self._base, final)
        launch = not (count == 0 or lo + count <= self._emitted)
        if launch and lo > self._emitted:
            raise RuntimeError(f"the window [{self._base}, {self._total}) settles samples from {lo} on, but {self._emitted} is due")
        return SimpleNamespace(origin=self._base, Lw=self._total - self._base, final=bool(final), lo=lo, count=count, launch=launch)

    def _take(self, plan: SimpleNamespace, out) -> Tuple[torch.Tensor, int]:
        """``(piece, keep_from)`` of the planned window, whose forward returned ``out [B, count]`` (None: it did not launch)."""
        if not plan.launch:
            return self._empty(), self._base                  # nothing new is settled: no launch
        piece = out[:, self._emitted - plan.lo:] if self._emitted > plan.lo else out
        self._emitted = plan.lo + plan.count
        # the next window: the last origin (a multiple of step) whose first settled sample is not past the next one due
        return piece, (self._emitted - self.halo[0]) // self._step * self._step

    def _window(self, final: bool) -> Tuple[torch.Tensor, int]:
        plan = self._plan(final)
        return self._take(plan, self._forward_window(final) if plan.launch else None)
