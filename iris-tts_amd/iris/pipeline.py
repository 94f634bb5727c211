"""Mel -> (PostNet) -> HiFiGAN -> waveform chunks, chained on one GPU (BASELINE.json configs[4]).

In the reference the three steps are separate host round trips (``scripts/synthesize.py:148-166`` runs the PostNet
and returns a numpy mel, ``:171-216`` converts it again and calls the vocoder).  Here the refined mel never leaves
HBM: ``PostNet.forward_device`` writes a device tensor that the vocoder engine reads chunk by chunk
(``iris.streaming``: 256-frame chunks + 13-frame halo, seams identical to the one-shot forward), so the first
audio is available after one chunk instead of after the whole utterance.

Three ways in: ``infer`` / ``stream`` take one complete mel; ``infer_batch`` takes a list of mels of different lengths and
runs ONE ragged PostNet pass and ONE ragged vocoder forward over all of them; ``session()`` takes the mel of one utterance
piece by piece from a producer that is still running, and refines and vocodes each chunk as soon as its context exists.
"""
from __future__ import annotations

from typing import Callable, Iterator, List, Optional, Sequence

import numpy as np
import torch

from .batching import pack_mels, split_waveforms
from .streaming import StreamingSession, StreamingVocoder

# why each chunked stage refuses a pipeline built on ``forward_pcm16``: its session reads the vocoder's fp32 chunks
_NEEDS_FP32 = {
    "denoiser": "a chunked denoiser takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not "
                "forward_pcm16 (no chunked PCM stage runs behind the denoiser)",
    "stretch": "a chunked stretch takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not "
               "forward_pcm16 (no chunked PCM stage runs behind the stretch)",
    "limiter": "a chunked limiter takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not "
               "forward_pcm16 (the limiter's own session stores 16-bit PCM: limiter=lim.chunked(pcm16=True))",
    "output": "output= reads the fp32 waveform: build the pipeline on engine.forward, not forward_pcm16 (the "
              "output stage stores 16-bit PCM itself: output=res.chunked('pcm16'))",
}


class MelToWavePipeline:
    """``postnet``: an ``iris.postnet.PostNet`` (or any callable mapping a device mel ``[B, n_mels, T]`` to a
    refined one), or None to vocode the mel as it is.  ``vocode``: ``GeneratorEngine.forward`` (or any callable
    ``[B, n_mels, W] -> [B, hop*W]``).  ``config``: the generator's ``GeneratorConfig`` -- hop length and the
    minimal halo are derived from it (V1 values when omitted; ``vocode.__self__.cfg`` is picked up when ``vocode``
    is a bound ``GeneratorEngine.forward``).  ``acoustic``: an ``iris.vae.TextConditionedVAE`` (or any callable
    ``(frame_cond, z_prior) -> (device mel [B, n_mels, T], ...)``) for ``infer_from_cond``, or None.  ``text``: a pair
    ``(iris.encoder.PhonemeEncoder, iris.encoder.DurationPredictor)`` for ``infer_from_phonemes``, or None.  ``posterior``:
    an ``iris.vae.VAEPosteriorEncoder`` (or any callable ``(mel, frame_cond) -> (device recon [B, n_mels, T], ...)``) for
    ``resynthesize``, or None.  ``frontend``: an ``iris.mel.MelFrontend`` (or any callable ``(audio [B, L], lengths=,
    max_frames=) -> (device mel [B, n_mels, T], frames [B])``) for ``mel_from_audio`` and ``resynthesize_from_audio``, or None.

    ``vocode`` may also be an ``iris.griffin_lim.GriffinLim`` (any object with ``whole_utterance = True`` and a
    ``forward_device``): text to waveform with no trained vocoder.  Such a vocoder takes the whole mel in one call -- every
    sample depends on every frame, so nothing is chunked and ``stream`` / ``session`` are refused -- and decides the length of
    its output itself (``hop * (T - 1)`` samples).  A batch of unequal lengths goes through ONE ragged call when the vocoder
    says ``takes_lengths`` (``GriffinLim(..., ragged=True)``: ``forward_device(mel, lengths=)``, item i bit for bit its own
    ``infer``); one that does not raises ``NotImplementedError``.

    ``denoiser``: an ``iris.denoiser.Denoiser`` (or any object with ``forward_device(wav [B, L], lengths=) -> [B, L]``), or
    None.  With one, ``infer``, ``infer_batch`` and every ``infer_from_*`` / ``resynthesize*`` route take the vocoder's fp32
    waveform through it -- in the ragged routes with the batch's lengths -- and run the output stage afterwards as
    stand-alone launches: ``pcm16=`` / ``normalize=`` through ``synthesis_output.pcm16_on_device``, ``resampler=`` through
    ``Resampler.forward``.  ``stream`` and ``session`` raise ``ValueError`` for a plain ``Denoiser``: a chunk seam needs the
    frames on either side of it.  With ``denoiser=None`` nothing changes.

    ``denoiser=dn.chunked()`` (an ``iris.denoiser.ChunkedDenoiser``, or any object with ``chunked_sessions = True``, a
    ``forward_device`` and an ``open_session() -> push / flush``) lets ``stream`` and ``session`` run: every fp32 chunk the
    vocoder emits is pushed into ONE ``DenoiserSession``, what becomes final is yielded (empty pieces are skipped) and the
    end of the utterance drains it.  The concatenation equals ``infer(mel)`` bit for bit -- the session's seams are exact --
    but the pieces are no longer all ``[B, hop * chunk]``: the first is short by the denoiser's right-hand halo
    (``n_fft / hop - 1`` frames: 3 at 1024 / 256) and the last carries it.  Added latency: a sample leaves that halo after
    its chunk does, on top of ``hv + hp`` -- a chunk shorter than the halo yields nothing until a later chunk covers it.
    ``infer``, ``infer_batch`` and the ragged routes go through ``forward_device`` as before.  Such a denoiser needs fp32: a
    pipeline built on ``forward_pcm16`` refuses it (``ValueError``), and so does a stream handed an integer chunk; a
    whole-utterance vocoder stays refused.

    ``stretch``: what ``iris.time_stretch.TimeStretch.at(rate)`` returns (or any object with ``hop_length``, ``out_samples(L)``
    and ``forward_device(wav [B, L], lengths=) -> (out [B, n_out], counts [B])``), or None.  With one, ``infer``, ``infer_batch``
    and every ``infer_from_*`` / ``resynthesize*`` route take the fp32 waveform -- the denoiser's, where there is one --
    through the phase vocoder and run the output stage afterwards as stand-alone launches, as for a denoiser; an item then
    has ``out_samples(hop * T_i)`` samples, and the ragged routes hand the stretch's ``counts`` on as sample lengths
    (``row_scale=1``).  The waveform must be whole frames of the stretch's own ``hop_length`` (``ValueError`` otherwise).
    ``stream`` and ``session`` raise ``ValueError`` for a plain ``ts.at(rate)``: the phase accumulator is a running state.
    With ``stretch=None`` nothing changes.

    ``stretch=ts.at(rate).chunked()`` (an ``iris.time_stretch.ChunkedStretch``, or any object with ``chunked_sessions = True``, a
    ``forward_device`` and an ``open_session() -> push / flush``) lets ``stream`` and ``session`` run: the vocoder's fp32 chunks
    go through the chunked denoiser's session, if there is one, and then through ONE ``StretchSession``, which carries the
    phase and the last output frames on the device.  Empty pieces are skipped and the last piece carries the halo; the
    concatenation equals ``infer(mel)`` bit for bit.  It needs fp32 as the chunked denoiser does (``forward_pcm16`` as the
    ``vocode`` is refused), and a plain denoiser beside it still refuses to stream.

    ``assemble``: an ``iris.assemble.Assembler`` (or any object with ``join_device(wav [B, L], lengths=, row_scale=) -> (out
    [cap], offsets [B + 1], spans [B, 2])``), or None.  With one, a batch is taken to be the sentences of one text:
    ``infer_batch`` -- and so the batch routes of ``infer_from_phonemes`` and ``resynthesize`` -- return ``(waveform, spans)``
    instead of a list: every item trimmed of its leading and trailing silence (``librosa.effects.trim``'s decision, on the
    device) and laid end to end with the assembler's pause and fades, ``spans [B, 2]`` (device, int32) saying what was kept of
    each item.  The join runs behind the denoiser and the stretch and in front of ``pcm16=`` / ``normalize=`` /
    ``resampler=``, which then see ONE row: the peak is the joined utterance's.  Every launch is queued before the one
    read-back, the total, which sizes the result.  ``infer`` treats every row of its mel as an item of such a batch; one row
    is trimmed, a join of one.  ``stream`` and ``session`` refuse (``ValueError``): the reference level is the whole item's
    maximum, and no chunked form is built.  With ``assemble=None`` nothing changes.

    ``loudness``: an ``iris.loudness.LoudnessNormalizer`` (or any object with ``normalize_device(wav [B, L], lengths=,
    row_scale=) -> (out [B, L], stats [B, 2])``), or None.  With one, ``infer``, ``infer_batch`` and the batch routes of
    ``infer_from_phonemes`` / ``resynthesize`` bring every item to the normalizer's target loudness (ITU-R BS.1770-4, measured
    and applied on the device, per item, no read-back) behind the denoiser and the stretch and in front of ``assemble=`` --
    each sentence is levelled, then trimmed, faded and joined -- and of ``pcm16=`` / ``normalize=`` / ``resampler=``, which
    run as stand-alone launches as for a denoiser.  The lengths are the ones the stage in front handed on (the batch's frames
    and the hop, or the stretch's device ``counts``).  ``stream`` and ``session`` refuse (``ValueError``): the measure is the
    whole item's, and no chunked form is built.  With ``loudness=None`` nothing changes.

    ``limiter``: an ``iris.limiter.Limiter`` (or any object with ``limit_device(wav [B, L], lengths=, row_scale=) -> (out [B, L],
    stats [B, 2])``), or None.  With one, the same routes hold every item under the limiter's true-peak ceiling by a look-ahead
    gain that falls only around a peak -- so a ``LoudnessNormalizer(peak_ceiling=None)`` in front reaches its target -- behind
    ``loudness=`` and in front of ``assemble=`` and of ``pcm16=`` / ``normalize=`` / ``resampler=``, which run as stand-alone
    launches as for a denoiser.  It is handed the lengths and ``row_scale`` the stage in front passed on.  ``stream`` and
    ``session`` refuse a plain limiter (``ValueError``): the gain looks ``2A + 7`` samples past a chunk's end.  With
    ``limiter=None`` nothing changes.

    ``limiter=lim.chunked()`` (an ``iris.limiter.ChunkedLimiter``, or any object with ``chunked_sessions = True``, a
    ``limit_device`` and an ``open_session() -> push / flush``) lets ``stream`` and ``session`` run: the fp32 chunks go through
    the chunked denoiser's and the chunked stretch's sessions, if there are any, and then through ONE ``LimiterSession``, the
    order in which ``infer`` applies the stages.  Empty pieces are skipped; the first piece is short by ``2A + 7`` samples (73 at
    1.5 ms and 22.05 kHz) and the last carries them; the concatenation equals ``infer(mel)`` bit for bit, so a streamed
    utterance is held under the ceiling.  With ``lim.chunked(pcm16=True)`` the limiter's kernel stores 16-bit PCM itself: the
    pieces are int16 and their concatenation equals ``infer(mel, pcm16=True)``.  It needs fp32 as the chunked denoiser does
    (``forward_pcm16`` as the ``vocode`` is refused); ``infer`` and ``infer_batch`` go through ``limit_device`` as before; and
    ``assemble=`` and ``loudness=`` beside it still refuse to stream, their measures being the whole item's.

    ``output``: what ``iris.resample.Resampler.chunked(encoding)`` returns (a ``ChunkedResampler``, or any object with
    ``chunked_sessions = True``, a ``forward(wav, lengths=, row_scale=)``, an ``out_range`` and an ``open_session() -> push /
    flush``), or None: the output stage of a served utterance, the sample rate and the sample format a consumer takes -- 8 kHz
    G.711 mu-law for a phone line is ``output=Resampler(8000).chunked("ulaw")``.  ``stream`` and ``session`` open its session
    LAST, behind the limiter's, or directly behind the vocoder when no other session exists; the pieces are fp32, int16 or uint8
    at ``output.rate_out`` and their concatenation equals ``infer(mel)`` bit for bit.  ``infer`` and ``infer_batch`` without
    ``pcm16`` / ``normalize`` / ``resampler`` arguments apply the same resampler and encoding in one call behind the other
    stages; those arguments beside ``output=`` are refused (``ValueError``), and so are ``lim.chunked(pcm16=True)`` and
    ``forward_pcm16`` as the ``vocode``: the resampler reads fp32.  With ``output=None`` nothing changes."""

    def __init__(self, postnet: Optional[Callable], vocode: Callable, device: Optional[torch.device] = None,
                 hop_length: Optional[int] = None, chunk_frames: int = 256, halo_frames: Optional[int] = None,
                 group_chunks: int = 1, config=None, acoustic=None, text=None, posterior=None, frontend=None,
                 denoiser=None, stretch=None, assemble=None, loudness=None, limiter=None, output=None):
        self.postnet = postnet
        self.denoiser = denoiser
        self.stretch = stretch
        self.assemble = assemble
        self.loudness = loudness
        self.limiter = limiter
        self.output = output
        self.acoustic = acoustic
        self.text = text
        self.posterior = posterior
        self.frontend = frontend
        self.device = device
        if config is None:
            config = getattr(getattr(vocode, "__self__", None), "cfg", None)
        self.config = config
        self._whole = vocode if getattr(vocode, "whole_utterance", False) else None
        # the stages that stream, in the order ``infer`` applies them: what ``_open_sessions`` opens
        self._chunked = {name: stage for name, stage in (("denoiser", denoiser), ("stretch", stretch), ("limiter", limiter),
                                                         ("output", output)) if getattr(stage, "chunked_sessions", False)}
        if self._chunked and getattr(vocode, "__name__", "") == "forward_pcm16":
            raise ValueError(_NEEDS_FP32[next(iter(self._chunked))])         # the first of them speaks
        if output is not None and "output" not in self._chunked:
            raise ValueError("output= takes a resampler with its encoding: pass output=res.chunked(encoding), not the Resampler")
        if output is not None and getattr(self._chunked.get("limiter"), "pcm16", False):
            raise ValueError("output= reads the fp32 waveform: pass limiter=lim.chunked(), not lim.chunked(pcm16=True) (the "
                             "output stage stores 16-bit PCM itself: output=res.chunked('pcm16'))")
        if self._whole is not None and hop_length is None:
            hop_length = int(vocode.hop_length)
        self.streamer = StreamingVocoder(vocode, hop_length=hop_length, chunk_frames=chunk_frames,
                                         halo_frames=halo_frames, group_chunks=group_chunks, config=config)

    def _to_device(self, mel) -> torch.Tensor:
        if not isinstance(mel, torch.Tensor):
            mel = torch.from_numpy(np.ascontiguousarray(np.asarray(mel, dtype=np.float32)))
        if mel.dim() != 3:
            raise ValueError(f"expected mel [B, n_mels, T], got shape {tuple(mel.shape)}")
        if self.device is not None:
            mel = mel.to(self.device)
        return mel

    def _refine_fn(self) -> Optional[Callable]:
        return None if self.postnet is None else getattr(self.postnet, "forward_device", self.postnet)

    def refine(self, mel) -> torch.Tensor:
        """Host or device mel ``[B, n_mels, T]`` -> refined device mel (one PostNet pass over the whole utterance:
        0.3 % of the vocoder's work)."""
        mel = self._to_device(mel)
        if self.postnet is None:
            return mel
        return self._refine_fn()(mel)

    def stream(self, mel) -> Iterator[torch.Tensor]:
        """Yields ``[B, hop*chunk]`` device tensors in order; their concatenation equals ``infer(mel)``.  Refused with a
        plain denoiser (``ValueError``): its frames reach ``n_fft / 2`` samples across a chunk seam.  With a chunked one the
        pieces are the ``DenoiserSession``'s: the first short by its halo, the last carrying it, none empty.  Likewise with
        a chunked stretch and a chunked limiter (int16 pieces with ``lim.chunked(pcm16=True)``); the session of ``output=``
        comes last of all, and its pieces are at its rate and in its encoding."""
        self._refuse_unstreamable()
        if self._whole is not None:
            raise NotImplementedError("a whole-utterance vocoder (Griffin-Lim) cannot be streamed: every sample depends on every frame")
        sessions = self._open_sessions()
        if not sessions:
            yield from self.streamer.stream(self.refine(mel))
            return
        for chunk in self.streamer.stream(self.refine(mel)):
            piece = self._push_through(sessions, self._session_input(chunk))
            if piece.shape[1]:
                yield piece
        yield from self._flush_through(sessions)

    def _open_sessions(self) -> list:
        """The sessions a chunk goes through on its way out, in the order ``infer`` applies the stages: the chunked denoiser's,
        then the chunked stretch's, then the chunked limiter's, then the output stage's."""
        return [stage.open_session() for stage in self._chunked.values()]

    def _output_args(self, pcm16: bool, normalize: bool, resampler):
        """``resampler`` for the output stage of ``infer`` / ``infer_batch``: the caller's, or ``output=`` -- beside which the
        caller names none, and no ``pcm16`` / ``normalize`` either."""
        if self.output is None:
            return resampler
        if pcm16 or normalize or resampler is not None:
            raise ValueError("this pipeline has output=: it decides the rate and the encoding, so pcm16=, normalize= and "
                             "resampler= are not taken beside it")
        return self.output

    @staticmethod
    def _push_through(sessions: list, piece: torch.Tensor) -> torch.Tensor:
        """``piece`` through ``sessions`` in order; an empty piece is not pushed any further."""
        for session in sessions:
            if not piece.shape[1]:
                break
            piece = session.push(piece)
        return piece

    @staticmethod
    def _flush_through(sessions: list) -> List[torch.Tensor]:
        """Ends the utterance: each session is flushed in order, and what it held goes through the ones behind it first."""
        out = []
        for i, session in enumerate(sessions):
            tail = session.flush()
            out.append(MelToWavePipeline._push_through(sessions[i + 1:], tail) if i + 1 < len(sessions) else tail)
        return [p for p in out if p.shape[1]]

    @staticmethod
    def _session_input(chunk: torch.Tensor) -> torch.Tensor:
        if not chunk.is_floating_point():
            raise ValueError(f"a chunked denoiser, stretch or limiter takes fp32 chunks, the vocoder returned {chunk.dtype}")
        return chunk.float()

    def _refuse_unstreamable(self) -> None:
        """``ValueError`` where a stage of this pipeline has no chunked form, or has one that was not opted into."""
        if self.assemble is not None:
            raise ValueError("a pipeline with assemble= cannot be streamed: the trim's reference level is the whole item's "
                             "maximum, known only when the item has ended, and no chunked form is built; use infer / infer_batch")
        if self.loudness is not None:
            raise ValueError("a pipeline with loudness= cannot be streamed: the integrated loudness is the whole item's "
                             "measure, known only when the item has ended, and no chunked form is built; use infer / infer_batch")
        if self.limiter is not None and "limiter" not in self._chunked:
            raise ValueError("a pipeline with limiter= cannot be streamed: the gain at a sample looks 2 * lookahead + 7 samples "
                             "past it, across a chunk's end, and no chunked form is built into a plain limiter: pass "
                             "limiter=lim.chunked(), or use infer / infer_batch")
        if self.stretch is not None and "stretch" not in self._chunked:
            raise ValueError("a pipeline with a plain time stretch cannot be streamed: the phase accumulator runs through the whole "
                             "utterance; pass stretch=ts.at(rate).chunked(), or use infer / infer_batch")
        if self.denoiser is not None and "denoiser" not in self._chunked:
            raise ValueError("a pipeline with a denoiser cannot be streamed: a chunk seam needs n_fft / 2 samples of context on "
                             "either side, and no chunked denoiser is built; use infer / infer_batch")

    def _vocode_whole(self, mel: torch.Tensor, pcm16: bool, normalize: bool, resampler):
        """One call of a whole-utterance vocoder, then ``_output_stage`` on its waveform."""
        return self._output_stage(self._whole.forward_device(mel), pcm16, normalize, resampler)

    @staticmethod
    def _output_stage(wav: torch.Tensor, pcm16: bool, normalize: bool, resampler):
        """The stand-alone output stages on a waveform that exists, whose length is the tensor's own: ``Resampler.forward``, or
        ``synthesis_output.pcm16_on_device`` (``(pcm, peaks)`` with ``normalize``)."""
        if resampler is not None:
            return resampler.forward(wav, pcm16=pcm16, normalize=normalize)
        if not pcm16:
            return wav
        from .synthesis_output import pcm16_on_device
        return pcm16_on_device(wav, normalize=normalize)

    def _vocode_whole_ragged(self, padded: torch.Tensor, lengths, pcm16: bool, normalize: bool, resampler) -> List[torch.Tensor]:
        """A batch through a whole-utterance vocoder that takes ``lengths``: ONE ``forward_device(padded, lengths=)``, whose
        rows are 0 past ``hop * (T_i - 1)`` -- so an item's peak is its own -- then the output stage over the whole batch
        and a list cut at each item's own count.  An item of one frame is refused by the vocoder, as ``infer`` refuses it."""
        frames = [int(t) for t in lengths]
        rows = [max(t - 1, 0) for t in frames]
        return self._ragged_output_stage(self._whole.forward_device(padded, lengths=frames), rows, pcm16, normalize, resampler)

    def _denoise(self, wav: torch.Tensor, lengths=None) -> torch.Tensor:
        """The vocoder's waveform through the denoiser (``lengths``: the items' mel frames, ``hop`` samples each)."""
        wav = wav.float()
        return self.denoiser.forward_device(wav) if lengths is None else self.denoiser.forward_device(wav, lengths=lengths)

    def _level(self, wav: torch.Tensor, lengths=None, row_scale: int = 1) -> torch.Tensor:
        """The waveform through the loudness stage, if there is one: item i, ``lengths[i] * row_scale`` samples of its row (all of
        it without ``lengths``), at the target loudness and 0 behind.  ``lengths`` may be a device tensor; nothing is read back."""
        if self.loudness is None:
            return wav
        return self.loudness.normalize_device(wav.float(), lengths=lengths, row_scale=row_scale)[0]

    def _limit(self, wav: torch.Tensor, lengths=None, row_scale: int = 1) -> torch.Tensor:
        """The waveform through the limiter, if there is one, with the lengths ``_level`` was handed: every item under the
        ceiling and 0 behind its own samples.  Nothing is read back."""
        if self.limiter is None:
            return wav
        return self.limiter.limit_device(wav.float(), lengths=lengths, row_scale=row_scale)[0]

    def _stretch_ragged(self, wav: torch.Tensor, rows: Sequence[int], pcm16: bool, normalize: bool, resampler) -> List[torch.Tensor]:
        """A batch whose item i owns ``hop * rows[i]`` samples through ONE ragged stretch, then the output stage with the
        stretch's ``counts`` as sample lengths.  The host knows the counts from ``out_samples``: nothing synchronises."""
        hop, sh = self.streamer.hop_length, int(self.stretch.hop_length)
        for i, r in enumerate(rows):
            if hop * r % sh:
                raise ValueError(f"item {i}: {hop * r} samples are not whole frames of the stretch's hop_length = {sh}; nothing is padded silently")
        if wav.shape[1] % sh:                                        # the padded row itself; its tail belongs to no item
            wav = torch.nn.functional.pad(wav, (0, sh - wav.shape[1] % sh))
        out, counts = self.stretch.forward_device(wav, lengths=[hop * r // sh for r in rows])
        out = self._limit(self._level(out, counts, 1), counts, 1)
        if self.assemble is not None:
            return self._joined_output_stage(out, counts, 1, pcm16, normalize, resampler)
        return self._ragged_output_stage(out, counts, pcm16, normalize, resampler, hop=1,
                                         samples=[self.stretch.out_samples(hop * r) for r in rows])

    def _ragged_output_stage(self, wav: torch.Tensor, rows, pcm16: bool, normalize: bool, resampler, hop: Optional[int] = None,
                             samples: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """The output stage over a batch whose item i owns ``hop * rows[i]`` samples and is 0 behind them, cut per item.
        ``hop``: the vocoder's, unless the caller's rows are in another unit; ``samples``: the items' counts on the host where
        ``rows`` is a device tensor."""
        hop = self.streamer.hop_length if hop is None else hop
        samples = [hop * r for r in rows] if samples is None else list(samples)
        if resampler is not None:
            out = resampler.forward(wav, lengths=rows, row_scale=hop, pcm16=pcm16, normalize=normalize)
            samples = [resampler.out_range(0, n)[1] for n in samples]
        elif pcm16:
            from .synthesis_output import pcm16_on_device
            out = pcm16_on_device(wav, normalize=normalize)
        else:
            out = wav
        out = out[0] if normalize else out
        return [out[i, :n] for i, n in enumerate(samples)]

    def _joined_output_stage(self, wav: torch.Tensor, lengths, row_scale: int, pcm16: bool, normalize: bool, resampler):
        """A batch whose item i owns ``lengths[i] * row_scale`` samples through the assembler, then the output stage on the
        joined row with the device's total as its length.  Returns ``(what infer returns for one row, cut at the total;
        spans)``; the total is read back once, after everything is queued."""
        out, offsets, spans = self.assemble.join_device(wav.float(), lengths=lengths, row_scale=row_scale)
        row, total = out[None], offsets[-1:]
        if resampler is not None:
            res = resampler.forward(row, lengths=total, row_scale=1, pcm16=pcm16, normalize=normalize)
        elif pcm16:
            from .synthesis_output import pcm16_on_device
            res = pcm16_on_device(row, normalize=normalize)        # the row is 0 behind the total: its peak is the utterance's
        else:
            res = row
        n = int(total.item())
        if resampler is not None:
            n = resampler.out_range(0, n)[1]
        if normalize:
            return (res[0][0, :n], res[1]), spans
        return res[0, :n], spans

    def _pcm16_fn(self) -> Callable:
        fn = getattr(getattr(self.streamer.forward, "__self__", None), "forward_pcm16", None)
        if fn is None:
            raise ValueError("pcm16=True needs a vocoder with a device output stage: construct the pipeline with a bound "
                             "GeneratorEngine.forward")
        return fn

    def _resampled_fn(self) -> Callable:
        fn = getattr(getattr(self.streamer.forward, "__self__", None), "forward_resampled", None)
        if fn is None:
            raise ValueError("resampler= needs a vocoder with a device resampling stage: construct the pipeline with a bound "
                             "GeneratorEngine.forward")
        return fn

    def infer(self, mel, pcm16: bool = False, normalize: bool = False, resampler=None):
        """The whole utterance.  ``pcm16=True``: an int16 device tensor, converted by the vocoder's last launch
        (``GeneratorEngine.forward_pcm16``), chunked like the fp32 path.  ``normalize=True`` (with pcm16): every item scaled
        to 0.95 at its own peak first; the peak is the whole utterance's, so the refined mel is vocoded in ONE forward,
        and ``(pcm, peaks)`` is returned.

        ``resampler`` (an ``iris.resample.Resampler``): the waveform at its rate instead of 22 050 Hz
        (``GeneratorEngine.forward_resampled``) -- fp32 chunked like the plain path, each window at its own origin, so the
        result equals the one-shot conversion bit for bit; with ``pcm16`` the refined mel goes through ONE forward.

        With ``output=`` the arguments are refused and the result is the fp32 waveform -- behind every other stage -- through
        ``output.forward``: its rate, its encoding, what ``stream`` yields piece by piece."""
        if normalize and not pcm16:
            raise ValueError("normalize=True goes with pcm16=True")
        resampler = self._output_args(pcm16, normalize, resampler)
        if (self.denoiser is not None or self.stretch is not None or self.assemble is not None or self.loudness is not None
                or self.limiter is not None or self.output is not None):
            mel = self.refine(mel)
            wav = self._whole.forward_device(mel) if self._whole is not None else self.streamer.infer(mel)
            if self.denoiser is not None:
                wav = self._denoise(wav)
            if self.stretch is not None:
                wav = self.stretch.forward_device(wav.float())[0]
            wav = self._limit(self._level(wav))
            if self.assemble is not None:
                return self._joined_output_stage(wav, None, 1, pcm16, normalize, resampler)
            return self._output_stage(wav, pcm16, normalize, resampler)
        if self._whole is not None:
            return self._vocode_whole(self.refine(mel), pcm16, normalize, resampler)
        if resampler is not None:
            fwd = self._resampled_fn()
            if pcm16:
                return fwd(self.refine(mel), resampler, pcm16=True, normalize=normalize)
            sv = self.streamer
            return StreamingVocoder(sv.forward, hop_length=sv.hop_length, chunk_frames=sv.chunk_frames,
                                    halo_frames=sv.halo_frames, group_chunks=sv.group_chunks, config=self.config, resampler=resampler).infer(self.refine(mel))
        if not pcm16:
            return self.streamer.infer(self.refine(mel))
        fwd = self._pcm16_fn()
        if normalize:
            return fwd(self.refine(mel), normalize=True)
        sv = self.streamer
        return StreamingVocoder(fwd, hop_length=sv.hop_length, chunk_frames=sv.chunk_frames, halo_frames=sv.halo_frames,
                                group_chunks=sv.group_chunks, config=self.config).infer(self.refine(mel))

    __call__ = infer

    def infer_from_cond(self, frame_cond, z_prior=None, **kw):
        """Frame-level text conditioning ``[B, T, cond_dim]`` (and optionally the latent prior sample) -> what ``infer`` returns
        for the mel the acoustic stage generates from it (``TextConditionedVAE.generate_device``, reference
        scripts/synthesize.py:125-166): VAE decoder, PostNet and vocoder on one stream, the mel never leaves the device.
        ``**kw`` goes to ``infer`` (``pcm16``, ``normalize``, ``resampler``)."""
        if self.acoustic is None:
            raise ValueError("infer_from_cond needs an acoustic stage: construct the pipeline with acoustic=TextConditionedVAE(...)")
        gen = getattr(self.acoustic, "generate_device", None)
        mel = gen(frame_cond, z_prior, want_residual=False)[0] if gen is not None else self.acoustic(frame_cond, z_prior)[0]
        return self.infer(mel, **kw)

    def resynthesize(self, mel, frame_cond, **kw):
        """Copy-synthesis: a recorded mel ``[B, n_mels, T]`` and its frame conditioning ``[B, T, cond_dim]`` -> what ``infer``
        returns for the VAE's reconstruction of it (``iris.vae.reconstruct``: posterior encoder, forward flow, decoder), all
        on one stream -- what the acoustic model loses, heard apart from what the text side loses.  ``**kw`` goes to
        ``infer`` (``pcm16``, ``normalize``, ``resampler``).

        A sequence of mels ``[n_mels, T_i]`` with a sequence of conditionings ``[T_i, cond_dim]``: utterances of different
        lengths, packed and reconstructed in ONE ragged ``reconstruct(..., lengths=)``, whose mel then goes on the way
        ``infer_from_phonemes`` hands a batch on -- ``infer_batch`` over slices of it, one ragged PostNet pass and one ragged
        vocoder forward.  The result is a list, item i bit for bit ``resynthesize(mel[i][None], frame_cond[i][None])[0]``.
        Every ``T_i`` must be a multiple of ``acoustic.downsample_factor`` (``ValueError``; nothing is padded silently).  A
        posterior that is a plain callable gets the items one by one instead."""
        if self.posterior is None:
            raise ValueError("resynthesize needs a posterior encoder: construct the pipeline with posterior=VAEPosteriorEncoder(...)")
        if isinstance(mel, (list, tuple)):
            return self._resynthesize_batch(list(mel), list(frame_cond), **kw)
        if hasattr(self.posterior, "encode_device"):
            if self.acoustic is None:
                raise ValueError("resynthesize needs the decoder too: construct the pipeline with acoustic=TextConditionedVAE(...)")
            from .vae import reconstruct
            mel = self._to_device(mel)
            if not isinstance(frame_cond, torch.Tensor):
                frame_cond = torch.from_numpy(np.ascontiguousarray(np.asarray(frame_cond, dtype=np.float32)))
            recon = reconstruct(self.posterior, self.acoustic, mel, frame_cond.to(mel.device))[0]
        else:
            recon = self.posterior(mel, frame_cond)[0]
        return self.infer(recon, **kw)

    def _resynthesize_batch(self, mels: list, conds: list, **kw) -> List[torch.Tensor]:
        """``resynthesize`` of a list: shapes are checked on the host, then one ragged ``reconstruct`` and ``infer_batch``."""
        if len(mels) != len(conds):
            raise ValueError(f"{len(mels)} mels but {len(conds)} conditionings")
        if not mels:
            return []
        ragged = hasattr(self.posterior, "encode_device")
        if ragged and self.acoustic is None:
            raise ValueError("resynthesize needs the decoder too: construct the pipeline with acoustic=TextConditionedVAE(...)")
        factor = int(getattr(self.acoustic, "downsample_factor", 1))
        conds = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c, dtype=np.float32)))
                 for c in conds]
        for i, (m, c) in enumerate(zip(mels, conds)):
            if len(m.shape) != 2 or c.dim() != 2 or c.shape[0] != m.shape[1] or c.shape[1] != conds[0].shape[1]:
                raise ValueError(f"item {i}: expected a mel [n_mels, T] and a conditioning [T, cond_dim], got "
                                 f"{tuple(m.shape)} and {tuple(c.shape)}")
            if m.shape[1] % factor:
                raise ValueError(f"item {i}: T = {m.shape[1]} is not a multiple of 2^down_stages = {factor}: pad the mel and "
                                 "the conditioning first; nothing is padded silently")
        if not ragged:
            recons = [self.posterior(self._to_device(torch.as_tensor(m)[None]), c[None])[0][0] for m, c in zip(mels, conds)]
            return self.infer_batch(recons, **kw)
        from .vae import reconstruct
        padded, lengths = pack_mels(mels)
        padded = self._to_device(padded)
        cond = torch.zeros((len(conds), padded.shape[2], conds[0].shape[1]), dtype=torch.float32, device=padded.device)
        for i, c in enumerate(conds):
            cond[i, :c.shape[0]] = c.to(device=cond.device, dtype=torch.float32)
        recon = reconstruct(self.posterior, self.acoustic, padded, cond, lengths=lengths)[0]
        return self.infer_batch([recon[i, :, :int(n)] for i, n in enumerate(lengths)], **kw)

    def _frontend_fn(self) -> Callable:
        if self.frontend is None:
            raise ValueError("this call needs a mel front-end: construct the pipeline with frontend=MelFrontend(...)")
        return getattr(self.frontend, "forward_device", self.frontend)

    @staticmethod
    def _audio_rows(audio):
        """One waveform ``[n]`` or a batch ``[B, L]`` (numpy or tensor, float or int16) -> ``[B, L]``."""
        if not isinstance(audio, torch.Tensor):
            audio = np.asarray(audio)
            audio = torch.from_numpy(np.ascontiguousarray(audio if audio.dtype == np.int16 else audio.astype(np.float32, copy=False)))
        if audio.dim() == 1:
            audio = audio[None]
        if audio.dim() != 2:
            raise ValueError(f"expected audio [n] or [B, L], got shape {tuple(audio.shape)}")
        return audio

    def mel_from_audio(self, audio) -> torch.Tensor:
        """A waveform ``[n]`` or a batch ``[B, L]`` (float32 or int16, host or device) -> its device log-mel
        ``[B, n_mels, 1 + L // hop]`` (``iris.mel.MelFrontend.forward_device``: the reference's ``compute_mel_spectrogram``)."""
        return self._frontend_fn()(self._audio_rows(audio))[0]

    def resynthesize_from_audio(self, audio, frame_cond, **kw):
        """``resynthesize`` from the recording itself: ``audio [n]`` (float32 or int16) and its frame conditioning
        ``[T, cond_dim]`` (or ``[1, T, cond_dim]``).  The mel is the front-end's, cut at the conditioning's ``T`` frames as the
        reference's dataset trims it to the duration total (``datasets.py:621-624``), and goes to ``resynthesize``.  The
        audio must have at least ``T`` frames (``1 + n // hop >= T``) and ``T`` must be a multiple of
        ``acoustic.downsample_factor`` (``ValueError``; nothing is padded silently).

        Lists of waveforms and conditionings: ONE ragged front-end call over the padded batch (``lengths`` = the items'
        samples, ``max_frames`` = their ``T_i``), then the list form of ``resynthesize`` -- one ragged ``reconstruct`` and
        ``infer_batch``.  The result is a list."""
        fe = self._frontend_fn()
        hop = int(getattr(self.frontend, "hop_length", self.streamer.hop_length))
        factor = int(getattr(self.acoustic, "downsample_factor", 1))

        def check(i, n, T):
            if 1 + n // hop < T:
                raise ValueError(f"item {i}: {n} samples give {1 + n // hop} frames, the conditioning has {T}")
            if T % factor:
                raise ValueError(f"item {i}: T = {T} is not a multiple of 2^down_stages = {factor}: pad the conditioning "
                                 "first; nothing is padded silently")

        if isinstance(audio, (list, tuple)):
            audios, conds = list(audio), list(frame_cond)
            if len(audios) != len(conds):
                raise ValueError(f"{len(audios)} waveforms but {len(conds)} conditionings")
            if not audios:
                return []
            rows = [self._audio_rows(a) for a in audios]
            for i, (a, c) in enumerate(zip(rows, conds)):
                if a.shape[0] != 1 or len(c.shape) != 2 or a.dtype != rows[0].dtype:
                    raise ValueError(f"item {i}: expected a waveform [n] of one sample type and a conditioning [T, cond_dim], got "
                                     f"{a.dtype} {tuple(a.shape)} and {tuple(c.shape)}")
                check(i, int(a.shape[1]), int(c.shape[0]))
            counts = [int(a.shape[1]) for a in rows]
            caps = [int(c.shape[0]) for c in conds]
            packed = torch.zeros((len(rows), max(counts)), dtype=rows[0].dtype, device=rows[0].device)
            for i, a in enumerate(rows):
                packed[i, :counts[i]] = a[0].to(packed.device)
            mel = fe(packed, lengths=counts, max_frames=caps)[0]
            return self.resynthesize([mel[i, :, :t] for i, t in enumerate(caps)], conds, **kw)
        rows = self._audio_rows(audio)
        if rows.shape[0] != 1:
            raise ValueError("resynthesize_from_audio takes one waveform [n], or lists of waveforms and conditionings")
        if not isinstance(frame_cond, torch.Tensor):
            frame_cond = torch.from_numpy(np.ascontiguousarray(np.asarray(frame_cond, dtype=np.float32)))
        if frame_cond.dim() == 2:
            frame_cond = frame_cond[None]
        if frame_cond.dim() != 3 or frame_cond.shape[0] != 1:
            raise ValueError(f"expected a conditioning [T, cond_dim], got shape {tuple(frame_cond.shape)}")
        T = int(frame_cond.shape[1])
        check(0, int(rows.shape[1]), T)
        mel = fe(rows, max_frames=[T])[0]
        return self.resynthesize(mel[:, :, :T].contiguous(), frame_cond, **kw)

    def infer_from_phonemes(self, ids, lengths=None, durations=None, z_prior=None, **kw):
        """Phoneme ids ``[B, P]`` -> ``(what infer returns, frames_per_item)``: phoneme encoder, duration head and length
        regulator (``iris.encoder.frame_conditioning``, reference scripts/synthesize.py:93-122), then ``infer_from_cond``.
        The conditioning is padded to ``acoustic.downsample_factor`` frames, as the reference pads it, and so is the audio:
        item i has ``hop * T_i`` samples with ``T_i = ceil(frames_per_item[i] / factor) * factor`` (``hop * (T_i - 1)`` from a
        whole-utterance vocoder, ``iris.griffin_lim``).  ``durations`` (integer ``[B, P]``)
        replaces the duration head's prediction.

        ``B == 1``: one chain on one stream; the only read-back is the frame total.  ``B > 1``: every stage runs ONCE over
        the ragged batch -- the encoder and the head (``lengths``), then the VAE decoder over the whole conditioning with
        item i's length ``ceil(frames_per_item[i] / factor) * factor`` (``generate_device(..., lengths=)``), then
        ``infer_batch`` over slices of its one mel.  The result is then a list, item i bit for bit the ``B == 1`` call on
        ``ids[i, :lengths[i]]``; ``z_prior`` is a list of per-item priors ``[1, T_i / factor, latent_dim]`` (or None: they
        are drawn per item, in item order, as the ``B == 1`` calls would draw them), and ``**kw`` goes to ``infer`` /
        ``infer_batch``.  An acoustic stage without ``takes_lengths`` (a plain callable) gets each item's conditioning --
        cut at its own padded total -- on its own instead."""
        if self.text is None or self.acoustic is None:
            raise ValueError("infer_from_phonemes needs text=(PhonemeEncoder, DurationPredictor) and acoustic=TextConditionedVAE(...)")
        from .encoder import frame_conditioning
        encoder, head = self.text
        factor = int(getattr(self.acoustic, "downsample_factor", 1))
        cond, per_item = frame_conditioning(encoder, head, ids, lengths=lengths, durations=durations, factor=factor)
        if cond.shape[0] == 1:
            return self.infer_from_cond(cond, z_prior, **kw), per_item
        if z_prior is not None and len(z_prior) != cond.shape[0]:
            raise ValueError(f"z_prior must be a list of {cond.shape[0]} per-item priors")
        gen = getattr(self.acoustic, "generate_device", None)
        padded = [-(-total // factor) * factor for total in per_item]
        if gen is not None and getattr(self.acoustic, "takes_lengths", False):
            mel = gen(cond, self._pack_priors(z_prior, cond, padded, factor), want_residual=False, lengths=padded)[0]
            return self.infer_batch([mel[i, :, :n] for i, n in enumerate(padded)], **kw), per_item
        mels = []
        for i, n in enumerate(padded):
            c = cond[i:i + 1, :n]
            z = None if z_prior is None else z_prior[i]
            mels.append((gen(c, z, want_residual=False)[0] if gen is not None else self.acoustic(c, z)[0])[0])
        return self.infer_batch(mels, **kw), per_item

    def _pack_priors(self, z_prior, cond: torch.Tensor, padded: Sequence[int], factor: int) -> torch.Tensor:
        """Per-item priors ``[1, padded[i] / factor, latent_dim]`` -> one ``[B, T / factor, latent_dim]`` for the ragged VAE
        call; rows past an item's own stay 0 and are never read.  ``z_prior=None``: each item's prior is drawn here, in item
        order and in the shape its own ``generate_device`` call would draw, so the random stream consumed is the same."""
        latent = int(self.acoustic.latent_dim)
        packed = torch.zeros((len(padded), cond.shape[1] // factor, latent), dtype=torch.float32, device=cond.device)
        for i, n in enumerate(padded):
            if z_prior is None:
                z = torch.randn((1, n // factor, latent), device=cond.device, dtype=torch.float32)
            else:
                z = torch.as_tensor(z_prior[i])
                if tuple(z.shape) != (1, n // factor, latent):
                    raise ValueError(f"expected z_prior[{i}] [1, {n // factor}, {latent}], got {tuple(z.shape)}")
            packed[i, :n // factor] = z[0]
        return packed

    def infer_batch(self, mels: Sequence, pcm16: bool = False, normalize: bool = False, resampler=None) -> List[torch.Tensor]:
        """Utterances of different lengths, ``mels[i]`` = ``[n_mels, T_i]`` (host or device) -> one waveform
        ``[hop * T_i]`` per utterance (with ``output=``: at its rate and in its encoding), with ONE PostNet pass and ONE vocoder forward for the whole list: the mels are padded
        to the longest (``pack_mels``) and both stages bound every layer of item i by ``T_i`` (``forward_device(...,
        lengths=)``, ``vocode(..., lengths=)``), so item i is bit for bit ``infer(mels[i][None])[0]`` -- padding alone would
        let the padded frames reach the last frames of every short item (``iris.batching``).  The stages must take
        ``lengths``; a vocoder dtype without a ragged forward (bf16, f32s) fails as ``engine.forward(lengths=...)`` does.
        ``pcm16=True``: int16 waveforms from ``GeneratorEngine.forward_pcm16``; with ``normalize=True`` each is scaled to
        0.95 at its own peak first.  ``resampler``: every waveform at its rate (``GeneratorEngine.forward_resampled`` with the
        same lengths: item i has ``resampler.out_range(0, hop * T_i)[1]`` samples, bit for bit its one-item conversion).
        A whole-utterance vocoder with ``takes_lengths`` (``_vocode_whole_ragged``): ``hop * (T_i - 1)`` samples per item.
        With ``assemble=`` the result is ``(waveform, spans)``: the items trimmed and joined into one (the class docstring)."""
        if normalize and not pcm16:
            raise ValueError("normalize=True goes with pcm16=True")
        resampler = self._output_args(pcm16, normalize, resampler)
        mels = list(mels)
        if not mels:
            return []
        padded, lengths = pack_mels(mels)
        ragged_whole = self._whole is not None and getattr(self._whole, "takes_lengths", False)
        if self._whole is not None and not ragged_whole and len(set(int(n) for n in lengths)) > 1:
            raise NotImplementedError("a whole-utterance vocoder (Griffin-Lim) takes items of one length: an item's last frames "
                                      "change its own STFT, and no ragged form is built; call infer once per length")
        padded = self._to_device(padded)
        if self.postnet is not None:
            padded = self._refine_fn()(padded, lengths=lengths)
        if (self.denoiser is not None or self.stretch is not None or self.assemble is not None or self.loudness is not None
                or self.limiter is not None or self.output is not None):
            frames = [int(t) for t in lengths]
            if ragged_whole:
                rows = [max(t - 1, 0) for t in frames]
                wav = self._whole.forward_device(padded, lengths=frames)
            elif self._whole is not None:
                rows = [max(frames[0] - 1, 0)] * len(frames)
                wav = self._whole.forward_device(padded)
            else:
                rows = frames
                wav = self.streamer.forward(padded, lengths=lengths)
            if self.denoiser is not None:
                wav = self._denoise(wav, rows)
            if self.stretch is not None:
                return self._stretch_ragged(wav.float(), rows, pcm16, normalize, resampler)
            wav = self._limit(self._level(wav, rows, self.streamer.hop_length), rows, self.streamer.hop_length)
            if self.assemble is not None:
                return self._joined_output_stage(wav, rows, self.streamer.hop_length, pcm16, normalize, resampler)
            return self._ragged_output_stage(wav, rows, pcm16, normalize, resampler)
        if ragged_whole:
            return self._vocode_whole_ragged(padded, lengths, pcm16, normalize, resampler)
        if self._whole is not None:
            out = self._vocode_whole(padded, pcm16, normalize, resampler)
            return list((out[0] if normalize else out).unbind(0))
        if resampler is not None:
            wav = self._resampled_fn()(padded, resampler, lengths=lengths, pcm16=pcm16, normalize=normalize)
            wav = wav[0] if normalize else wav
            hop = self.streamer.hop_length
            return [wav[i, :resampler.out_range(0, hop * int(t))[1]] for i, t in enumerate(lengths)]
        if pcm16:
            wav = self._pcm16_fn()(padded, lengths=lengths, normalize=normalize)
            wav = wav[0] if normalize else wav
        else:
            wav = self.streamer.forward(padded, lengths=lengths)
        return split_waveforms(wav, lengths, self.streamer.hop_length)

    def session(self, postnet_halo_frames: Optional[int] = None) -> "PipelineSession":
        """A new ``PipelineSession`` for ONE utterance whose mel is still being produced.  ``postnet_halo_frames``: the
        PostNet's receptive field on either side, for a callable that has no ``receptive_field_frames`` of its own.
        Refused with a plain denoiser, stretch or limiter (``ValueError``), as ``stream`` is; with chunked ones the session's
        pieces are those of the last of their sessions."""
        self._refuse_unstreamable()
        if self._whole is not None:
            raise NotImplementedError("a whole-utterance vocoder (Griffin-Lim) cannot be streamed: every sample depends on every frame")
        return PipelineSession(self, postnet_halo_frames)


class PipelineSession:
    """Pushed input for ``MelToWavePipeline``: the raw mel of ONE utterance arrives piece by piece (``push``), refined and
    vocoded audio leaves chunk by chunk, ``flush`` ends the utterance.  The concatenation of everything returned equals
    ``pipeline.infer`` of the concatenated mel.

    The PostNet is a finite stack of 'same' convolutions (src/iris/postnet.py:48-67): refined frame t depends on the raw mel
    within +-hp frames only (``PostNet.receptive_field_frames``, 6 for the 3 x k5 net), so it is final once raw frames up to
    t + hp have arrived, or the utterance has ended.  Final refined frames go into an ordinary ``StreamingSession``, which
    cuts the chunks and keeps the generator's own halo hv (13 for V1).  A refinement window starts hp raw frames before the
    first frame not yet refined (clamped at 0: frame 0 is the true start, its zero padding is the one-shot's own) and ends
    at the last raw frame received; the frames within hp of a window edge that is not an edge of the utterance have seen
    zero padding where the utterance has frames, and are dropped.

    Latency: chunk ``[s, s + chunk)`` is returned by the push that brings ``frames_received`` to ``s + chunk + hv + hp``.
    Work: the PostNet runs only in a push that returns at least one chunk, and once in ``flush`` -- a producer that pushes
    single frames does not cause a pass per frame.  Memory: at most ``chunk + 2 * (hv + hp)`` frames are buffered (raw ones
    not yet refined with their left-hand context, refined ones not yet emitted with theirs) plus the piece just pushed.

    A pipeline built on ``engine.forward_pcm16`` yields int16 chunks.  No peak normalisation here: it needs the peak of an
    utterance that has not ended yet.

    With a chunked denoiser (``MelToWavePipeline(denoiser=dn.chunked())``) every chunk goes through one ``DenoiserSession``
    on its way out: ``push`` and ``flush`` return its non-empty pieces -- the first short by the denoiser's halo, ``flush``
    returning it -- and a chunk leaves that many samples later.  With a chunked stretch (``stretch=ts.at(rate).chunked()``) they
    then go through one ``StretchSession``, whose pieces ``push`` and ``flush`` return instead.  With a chunked limiter
    (``limiter=lim.chunked()``) one ``LimiterSession`` comes last: its pieces are what ``push`` and ``flush`` return, ``2A + 7``
    samples later still, held under the ceiling, and int16 with ``lim.chunked(pcm16=True)``."""

    def __init__(self, pipeline: MelToWavePipeline, postnet_halo_frames: Optional[int] = None):
        sv = pipeline.streamer
        if sv.chunk_frames < 1:
            raise ValueError(f"chunk_frames >= 1 is required, got {sv.chunk_frames}")
        postnet = pipeline.postnet
        if postnet_halo_frames is not None and postnet_halo_frames < 0:
            raise ValueError(f"postnet_halo_frames >= 0 is required, got {postnet_halo_frames}")
        if postnet is None:
            hp = 0
        elif hasattr(postnet, "receptive_field_frames"):
            hp = int(postnet.receptive_field_frames)
            if postnet_halo_frames is not None:
                if postnet_halo_frames < hp:
                    raise ValueError(f"postnet_halo_frames={postnet_halo_frames} is smaller than the PostNet's receptive "
                                     f"field ({hp} frames): window seams would differ from the one-shot output")
                hp = int(postnet_halo_frames)
        elif postnet_halo_frames is not None:
            hp = int(postnet_halo_frames)
        else:
            raise ValueError("the PostNet has no receptive_field_frames: pass postnet_halo_frames (the frames on either "
                             "side that reach one refined frame); a guess would make the window seams silently wrong")
        self._pipeline = pipeline
        self._refine = pipeline._refine_fn()
        self.postnet_halo_frames = hp
        self._inner = StreamingSession(sv.forward, hop_length=sv.hop_length, chunk_frames=sv.chunk_frames,
                                       halo_frames=sv.halo_frames, config=pipeline.config)
        self.hop_length, self.chunk_frames, self.halo_frames = sv.hop_length, sv.chunk_frames, sv.halo_frames
        self._raw: list = []          # raw pieces [B, n_mels, t]; together they cover raw frames [self._base, self._total)
        self._base = 0
        self._total = 0               # raw frames received so far
        self._refined = 0             # first raw frame not yet refined (== frames pushed into the inner session)
        self._lead = None             # (B, n_mels) of the utterance
        self._closed = False
        self._sessions = pipeline._open_sessions()

    @property
    def frames_received(self) -> int:
        return self._total

    @property
    def frames_emitted(self) -> int:
        return self._inner.frames_emitted

    @property
    def frames_buffered(self) -> int:
        """Frames held between calls: raw ones (with the left-hand PostNet context) + refined ones in the vocoder session."""
        return (self._total - self._base) + (self._inner._total - self._inner._base)

    def _plan_refine(self, final: bool) -> Optional[tuple]:
        """``(win_start, stop)``: the raw window ``[win_start, frames_received)`` whose refinement makes the frames ``[first not
        yet refined, stop)`` final -- or None: nothing is final, or (before the end) it would not complete a chunk.  The PostNet
        runs only when its output completes a chunk: the vocoder session emits ``[s, s + chunk)`` once it holds refined frames up
        to ``s + chunk + hv``, and those are final ``hp`` raw frames later."""
        hp = self.postnet_halo_frames
        if not final and self._total - hp < self._inner.frames_emitted + self.chunk_frames + self.halo_frames:
            return None
        stop = self._total if final else self._total - hp        # refined frames [self._refined, stop) are final
        if stop <= self._refined:
            return None
        return max(0, self._refined - hp), stop

    def _raw_window(self, plan: tuple) -> torch.Tensor:
        self._raw = [self._raw[0] if len(self._raw) == 1 else torch.cat(self._raw, dim=2)]
        return self._raw[0][:, :, plan[0] - self._base:]

    def _take_refined(self, plan: tuple, window: torch.Tensor) -> torch.Tensor:
        """The final frames of the refined window; the raw frames the next window no longer needs are dropped."""
        win_start, stop = plan
        piece = window[:, :, self._refined - win_start:stop - win_start]
        self._refined = stop
        keep_from = max(0, stop - self.postnet_halo_frames)      # the next window's left-hand context
        self._raw = [self._raw[0][:, :, keep_from - self._base:]]
        self._base = keep_from
        return piece

    def _advance(self, final: bool) -> List:
        """Refines every frame that is final now and hands it to the vocoder session: plan, forward, take
        (``iris.stream_group`` plans for many sessions and runs ONE ragged pass)."""
        plan = self._plan_refine(final)
        if plan is None:
            return []
        window = self._raw_window(plan)
        if self._refine is not None:
            window = self._refine(window)
        return self._through_sessions(self._inner.push(self._take_refined(plan, window)))

    def _through_sessions(self, chunks: List, final: bool = False) -> List:
        """The vocoder's chunks through the sessions of the chunked stages (if there are any; ``MelToWavePipeline._open_sessions``
        has the order), drained at the end with ``final``; empty pieces are dropped."""
        if not self._sessions:
            return chunks
        pieces = [MelToWavePipeline._push_through(self._sessions, MelToWavePipeline._session_input(c)) for c in chunks]
        pieces = [p for p in pieces if p.shape[1]]
        return pieces + MelToWavePipeline._flush_through(self._sessions) if final else pieces

    def push(self, mel_piece) -> List[torch.Tensor]:
        """Appends the raw ``mel_piece [B, n_mels, t]`` (t >= 0, host or device) and returns the waveform chunks
        ``[B, hop * chunk]`` that became computable, in order (possibly none)."""
        self._append(mel_piece)
        return self._advance(final=False)

    def _append(self, mel_piece) -> None:
        """The checks of ``push`` and the piece behind what is held; nothing runs."""
        if self._closed:
            raise RuntimeError("the session was flushed: start a new one for the next utterance")
        mel_piece = self._pipeline._to_device(mel_piece)
        if self._lead is not None and tuple(mel_piece.shape[:2]) != self._lead:
            raise ValueError("every piece of an utterance must have the same batch size and mel bins")
        if mel_piece.shape[2] > 0:
            self._lead = tuple(mel_piece.shape[:2])
            self._raw.append(mel_piece)
            self._total += int(mel_piece.shape[2])

    def flush(self) -> List[torch.Tensor]:
        """Ends the utterance: refines the frames that were waiting for context -- the right edge of this last window is the
        true end of the mel, as in the one-shot pass -- and returns the remaining chunks (the last may be shorter)."""
        if self._closed:
            return []
        out = self._advance(final=True)
        out += self._through_sessions(self._inner.flush(), final=True)
        self._closed = True
        self._raw = []
        return out
