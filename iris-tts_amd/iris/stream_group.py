"""Concurrent streams: many streaming sessions, each at its own place in its own utterance, stepped with one launch per stage.

A ``PipelineSession`` serves one caller, and N callers cost N times the launch-bound price of a window.  A ``StreamGroup`` holds
one session's worth of state per caller (a *member*) and ``step()`` runs, for all members that have a computable window, ONE
ragged PostNet pass (if the pipeline has a PostNet), ONE ragged vocoder forward, ONE limiter group call
(``Limiter.forward_windows``) and ONE resampler group call (``Resampler.forward_windows``):

    group = StreamGroup(pipeline, chunk_frames=256)
    m = group.open()          # a member: one caller's utterance
    m.push(mel_piece)         # [1, n_mels, t] or [n_mels, t]; only queues
    m.end()                   # the utterance is complete
    pieces = group.step()     # {member: tensor [1, n]}: what became settled, fp32, int16 or G.711 bytes as output= says

The windows of different members are just items of one ragged forward -- item b of ``iris_hifigan_forward_ragged`` and
``iris_postnet_forward_ragged`` is bit for bit its stand-alone result -- and rows of one group call on the wave side, where
row b is bit for bit ``forward_window`` of that item.  So the concatenation of a member's pieces equals ``pipeline.infer`` of
its own mel bit for bit, whoever else is in the group.

A member emits AT MOST ONE vocoder chunk per step, so one step is one forward: a member that pushed three chunks' worth of
frames takes three steps to drain.  A member that has ended and drained closes itself; members join (``open``) and leave
(``StreamMember.leave``) between steps freely.  ``step()`` is synchronous on the host and asynchronous on the current stream,
as the sessions are; the caller decides when to call it.

The bookkeeping is not restated here.  Which raw window the PostNet needs, which mel window the next chunk needs, which samples
the limiter and the resampler hold and what they settle are ``PipelineSession._plan_refine`` / ``_take_refined``,
``StreamingSession._plan_chunk`` / ``_take_chunk`` and the ``_plan`` / ``_take`` of ``LimiterSession`` and ``ResamplerSession``:
the group calls plan for everyone, one batched forward, then take for everyone.

The native group calls take at most ``_native.WINDOW_GROUP_MAX`` = 64 rows (their descriptors travel by value in the kernel
argument); ``step()`` cuts larger groups into slabs of 64 members and runs the stages once per slab.

Not built: per-item windows for the chunked denoiser and the time stretch (frame-aligned origins, the carried phase), bf16 /
f32s engines, ``assemble=`` and ``loudness=`` (whole-item measures), and a resident row buffer -- the rows of a group call are
packed from the members' held samples with one copy per member and step.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _native
from .batching import pack_mels
from .pipeline import MelToWavePipeline, PipelineSession

GROUP_MAX = _native.WINDOW_GROUP_MAX


class StreamMember:
    """One caller's utterance in a ``StreamGroup``: ``push`` queues mel frames, ``end`` says the utterance is complete, and the
    group's ``step`` returns its audio.  ``closed`` once everything has left (or after ``leave``)."""

    def __init__(self, group: "StreamGroup"):
        self._group = group
        self._session = PipelineSession(group.pipeline, group.postnet_halo_frames)
        self._session.chunk_frames = self._session._inner.chunk_frames = group.chunk_frames
        self._ended = False
        self.closed = False

    @property
    def frames_received(self) -> int:
        return self._session.frames_received

    @property
    def frames_emitted(self) -> int:
        return self._session.frames_emitted

    def push(self, mel_piece) -> None:
        """Queues ``mel_piece [1, n_mels, t]`` or ``[n_mels, t]`` (t >= 0, host or device); nothing runs until ``step``."""
        if self._ended or self.closed:
            raise RuntimeError("the member's utterance has ended: open a new member for the next one")
        if not isinstance(mel_piece, torch.Tensor):
            mel_piece = torch.as_tensor(mel_piece, dtype=torch.float32)
        if mel_piece.dim() == 2:
            mel_piece = mel_piece[None]
        if mel_piece.dim() != 3 or mel_piece.shape[0] != 1:
            raise ValueError(f"a member takes ONE utterance: expected mel [1, n_mels, t] or [n_mels, t], got {tuple(mel_piece.shape)}")
        self._session._append(mel_piece)

    def end(self) -> None:
        """The utterance is complete: the steps that follow drain it, and the member closes itself."""
        self._ended = True

    def leave(self) -> None:
        """Drops the member and whatever it held; nothing more is returned for it."""
        self.closed = True
        self._group._members = [m for m in self._group._members if m is not self]


class StreamGroup:
    """``pipeline``: a ``MelToWavePipeline`` of ``vocode`` backed by the fp32 engine's ragged forward (any callable that takes
    ``lengths=``), an optional PostNet, an optional ``limiter=lim.chunked()`` (fp32, or ``pcm16=True`` when nothing follows it)
    and an optional ``output=res.chunked(encoding)``.  A chunked denoiser or time stretch, ``assemble=``, ``loudness=``, a plain
    limiter, a whole-utterance vocoder or a non-fp32 engine is refused with a ``ValueError`` that names the stage.
    ``chunk_frames``: the frames of a vocoder chunk, for every member.  ``postnet_halo_frames``: as ``pipeline.session``'s."""

    def __init__(self, pipeline: MelToWavePipeline, chunk_frames: int = 256, postnet_halo_frames: Optional[int] = None):
        for name in ("denoiser", "stretch"):
            if getattr(pipeline, name) is not None:
                raise ValueError(f"a StreamGroup does not take a pipeline with {name}=: its windows have per-item frame origins "
                                 "and state, and no group form is built for them")
        for name in ("assemble", "loudness"):
            if getattr(pipeline, name) is not None:
                raise ValueError(f"a StreamGroup does not take a pipeline with {name}=: its measure is the whole item's, and no "
                                 "chunked form is built")
        pipeline._refuse_unstreamable(whole=ValueError(           # a plain limiter (limiter=lim.chunked()), then the vocoder
            "a StreamGroup does not take a whole-utterance vocode (Griffin-Lim): every sample depends on every frame"))
        dtype = getattr(getattr(pipeline.streamer.forward, "__self__", None), "default_dtype", "f32")
        if dtype != "f32":
            raise ValueError(f"a StreamGroup needs the fp32 engine as its vocode: only it has a ragged forward, got dtype {dtype!r}")
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames >= 1 is required, got {chunk_frames}")
        self.pipeline, self.chunk_frames, self.postnet_halo_frames = pipeline, int(chunk_frames), postnet_halo_frames
        self._members: List[StreamMember] = []
        StreamMember(self)                                       # the session's own refusals (a PostNet without a halo), now

    @property
    def members(self) -> List[StreamMember]:
        return list(self._members)

    def open(self) -> StreamMember:
        """A new member, for one caller's utterance."""
        member = StreamMember(self)
        self._members.append(member)
        return member

    def step(self) -> Dict[StreamMember, torch.Tensor]:
        """One launch per stage for every member with a computable window (per slab of 64 members); ``{member: [1, n]}`` of what
        became settled, members with nothing new left out.  Each member advances by at most one vocoder chunk."""
        out: Dict[StreamMember, torch.Tensor] = {}
        members = self.members
        for at in range(0, len(members), GROUP_MAX):
            self._step_slab(members[at:at + GROUP_MAX], out)
        self._members = [m for m in self._members if not m.closed]
        return out

    # -- one slab: plan for everyone, one forward, take for everyone, stage by stage -----------
    def _step_slab(self, members: List[StreamMember], out: Dict[StreamMember, torch.Tensor]) -> None:
        pipe = self.pipeline
        # the PostNet: every member's raw window in ONE ragged pass
        due = [(m, plan) for m in members for plan in [m._session._plan_refine(m._ended)] if plan is not None]
        if due:
            windows = [m._session._raw_window(plan) for m, plan in due]
            refine = pipe._refine_fn()
            if refine is not None:
                padded, lengths = pack_mels([w[0] for w in windows])
                refined = refine(padded, lengths=lengths)
                windows = [refined[i:i + 1, :, :int(n)] for i, n in enumerate(lengths)]
            for (m, plan), window in zip(due, windows):
                m._session._inner._append(m._session._take_refined(plan, window))
        # the vocoder: every member's next chunk in ONE ragged forward
        pieces: Dict[StreamMember, torch.Tensor] = {}
        due = []
        for m in members:
            s = m._session
            chunk = s._inner._plan_chunk(m._ended and s._refined == s._total)
            if chunk is not None:
                due.append((m, chunk))
        if due:
            padded, lengths = pack_mels([m._session._inner._chunk_window(c)[0] for m, c in due])
            wav = pipe.streamer.forward(padded, lengths=lengths)
            hop = pipe.streamer.hop_length
            for i, (m, c) in enumerate(due):
                pieces[m] = m._session._inner._take_chunk(c, wav[i:i + 1, :hop * int(lengths[i])])
        # the wave stages, in the order infer applies them: each ONE group call over the members' held samples
        final = {m: m._ended and m._session._refined == m._session._total and m._session._inner._next == m._session._inner._total
                 for m in members}
        for k in range(len(members[0]._session._sessions) if members else 0):
            rows = []
            for m in members:
                sess, piece = m._session._sessions[k], pieces.pop(m, None)
                if sess._closed:
                    continue
                if piece is not None and piece.shape[1]:
                    sess._append(MelToWavePipeline._session_input(piece) if k == 0 else piece)
                elif not final[m]:
                    continue                                      # nothing new, and the utterance goes on: no window
                if sess._buf is None:                             # an utterance of no samples
                    sess._close()
                    continue
                plan = sess._plan(final[m])
                if plan.launch:
                    rows.append((m, sess, plan))
                else:
                    sess._keep(*sess._take(plan, None))
                    if final[m]:
                        sess._close()
            for (m, sess, plan), result in zip(rows, self._forward_rows(rows)):
                pieces[m] = sess._keep(*sess._take(plan, result))
                if final[m]:
                    sess._close()
        for m in members:
            piece = pieces.get(m)
            if piece is not None and piece.shape[1]:
                out[m] = piece
            if final[m]:
                m.closed = True

    @staticmethod
    def _forward_rows(rows: list) -> list:
        """The planned windows of one stage's sessions as ONE ``forward_windows`` call; what each session's ``_take`` expects."""
        if not rows:
            return []
        sess0 = rows[0][1]
        held = [sess._buf[0] for _, sess, _ in rows]
        packed = torch.nn.utils.rnn.pad_sequence(held, batch_first=True)          # [k, in_stride]: row b = member b's held samples
        if hasattr(sess0, "pcm16"):                              # LimiterSession
            items = [(p.origin, p.Lw, p.final) for _, _, p in rows]
            wav, stats, counts = sess0._stage.forward_windows(packed, items, pcm16=sess0.pcm16)
            return [(wav[i:i + 1, :n], stats[i:i + 1]) for i, n in enumerate(counts)]
        items = [(p.origin, p.Lw, p.n_next, p.final) for _, _, p in rows]          # ResamplerSession
        wav, counts = sess0._res.forward_windows(packed, items, encoding=sess0.encoding)
        return [wav[i:i + 1, :n] for i, n in enumerate(counts)]
