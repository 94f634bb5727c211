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

from typing import Callable, Iterator, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .batching import pack_mels, split_waveforms
from .streaming import StreamingSession, StreamingVocoder


class _Waves(NamedTuple):
    """A ragged batch of waveforms, as ``forward_device(lengths=)``, ``normalize_device``, ``limit_device``, ``join_device`` and
    ``Resampler.forward`` take one: item i owns ``lengths[i] * row_scale`` samples of ``wav [B, L]`` and is 0 behind them.
    ``lengths``: None for whole rows, a host sequence, or a device tensor; ``samples``: the items' counts where the host knows
    them (None: whole rows, or a length only the device has)."""
    wav: torch.Tensor
    lengths: object = None
    row_scale: int = 1
    samples: Optional[Sequence[int]] = None


class _WaveStage(NamedTuple):
    name: str                       # the pipeline's attribute and constructor argument
    step: Optional[str]             # the method ``_chain`` calls, ``_Waves -> _Waves`` (None: the stage belongs to ``_finish``)
    unstreamable: Optional[str]     # why ``stream`` / ``session`` refuse it (a stage with a chunked form: unless it was opted into)
    needs_fp32: Optional[str]       # why its chunked form refuses a pipeline built on ``forward_pcm16`` (None: no chunked form)
    speaks: int = 0                 # where several stages refuse to stream, the one with the lowest number says why


# the stages behind the vocoder, in the order ``infer`` applies them; the next wave stage is one entry here and its step method
_WAVE_STAGES = (
    _WaveStage("denoiser", "_denoise",
               "a pipeline with a denoiser cannot be streamed: a chunk seam needs n_fft / 2 samples of context on either side, "
               "and no chunked denoiser is built; use infer / infer_batch",
               "a chunked denoiser takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not forward_pcm16 "
               "(no chunked PCM stage runs behind the denoiser)", speaks=5),
    _WaveStage("stretch", "_stretch",
               "a pipeline with a plain time stretch cannot be streamed: the phase accumulator runs through the whole utterance; "
               "pass stretch=ts.at(rate).chunked(), or use infer / infer_batch",
               "a chunked stretch takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not forward_pcm16 "
               "(no chunked PCM stage runs behind the stretch)", speaks=4),
    _WaveStage("loudness", "_level",
               "a pipeline with loudness= cannot be streamed: the integrated loudness is the whole item's measure, known only "
               "when the item has ended, and no chunked form is built; use infer / infer_batch", None, speaks=2),
    _WaveStage("limiter", "_limit",
               "a pipeline with limiter= cannot be streamed: the gain at a sample looks 2 * lookahead + 7 samples past it, across "
               "a chunk's end, and no chunked form is built into a plain limiter: pass limiter=lim.chunked(), or use infer / "
               "infer_batch",
               "a chunked limiter takes the vocoder's fp32 waveform: build the pipeline on engine.forward, not forward_pcm16 "
               "(the limiter's own session stores 16-bit PCM: limiter=lim.chunked(pcm16=True))", speaks=3),
    _WaveStage("assemble", None,
               "a pipeline with assemble= cannot be streamed: the trim's reference level is the whole item's maximum, known only "
               "when the item has ended, and no chunked form is built; use infer / infer_batch", None, speaks=1),
    _WaveStage("output", None, None,
               "output= reads the fp32 waveform: build the pipeline on engine.forward, not forward_pcm16 (the output stage "
               "stores 16-bit PCM itself: output=res.chunked('pcm16'))"),
)


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

    The wave stages -- ``denoiser``, ``stretch``, ``loudness``, ``limiter``, ``assemble``, ``output`` (the table ``_WAVE_STAGES``)
    -- are each None, and then nothing changes, or set.  With any of them ``infer``, ``infer_batch`` and every ``infer_from_*`` /
    ``resynthesize*`` route take the vocoder's fp32 waveform through the stages that are set, in that order, and run the output
    stage afterwards as stand-alone launches: ``pcm16=`` / ``normalize=`` through ``synthesis_output.pcm16_on_device``,
    ``resampler=`` through ``Resampler.forward``.  In the ragged routes every stage is handed the lengths and the ``row_scale``
    the stage in front passed on: the batch's frames (``hop * (T_i - 1)`` from a whole-utterance vocoder: its rows) and the
    hop, or behind a stretch its device ``counts`` and ``row_scale=1``; nothing is read back.  ``stream`` and ``session``
    refuse a stage as it is (``ValueError``).  The chunked form opts in with ``.chunked()``: any object with
    ``chunked_sessions = True``, the stage's own whole-utterance method and an ``open_session() -> push / flush``.  Then every fp32
    chunk the vocoder emits goes through ONE session per chunked stage, in the order ``infer`` applies the stages; what becomes
    final is yielded (empty pieces are skipped), the end of the utterance drains the sessions, and the concatenation equals
    ``infer(mel)`` bit for bit -- the sessions' seams are exact -- but the pieces are no longer all ``[B, hop * chunk]``: each
    session's first piece is short by its halo and its last carries it.  A chunked stage needs fp32: a pipeline built on
    ``forward_pcm16`` refuses it (``ValueError``), and so does a stream handed an integer chunk; a whole-utterance vocoder stays
    refused; a stage beside it that was not opted in, or has no chunked form, still refuses to stream; ``infer``,
    ``infer_batch`` and the ragged routes go through the whole-utterance method as before.

    ``denoiser``: an ``iris.denoiser.Denoiser`` (or any object with ``forward_device(wav [B, L], lengths=) -> [B, L]``;
    ``lengths``: the items' rows, ``hop`` samples each).  Not streamed as it is: a chunk seam needs the frames on either side
    of it.  ``denoiser=dn.chunked()`` (an ``iris.denoiser.ChunkedDenoiser``): one ``DenoiserSession``; its halo is the
    right-hand ``n_fft / hop - 1`` frames (3 at 1024 / 256).  Added latency: a sample leaves that halo after its chunk does, on
    top of ``hv + hp`` -- a chunk shorter than the halo yields nothing until a later chunk covers it.

    ``stretch``: what ``iris.time_stretch.TimeStretch.at(rate)`` returns (or any object with ``hop_length``, ``out_samples(L)``
    and ``forward_device(wav [B, L], lengths=) -> (out [B, n_out], counts [B])``): the phase vocoder, on the denoiser's waveform
    where there is one.  An item then has ``out_samples(hop * T_i)`` samples -- the host knows the counts from ``out_samples``,
    nothing synchronises -- and in the ragged routes the waveform must be whole frames of the stretch's own ``hop_length``
    (``ValueError`` otherwise; nothing is padded silently).  Not streamed as it is: the phase accumulator is a running state.
    ``stretch=ts.at(rate).chunked()`` (an ``iris.time_stretch.ChunkedStretch``): one ``StretchSession``, which carries the
    phase and the last output frames on the device; the last piece carries the halo.

    ``loudness``: an ``iris.loudness.LoudnessNormalizer`` (or any object with ``normalize_device(wav [B, L], lengths=,
    row_scale=) -> (out [B, L], stats [B, 2])``): every item at the normalizer's target loudness (ITU-R BS.1770-4, measured
    and applied on the device, per item, no read-back) in ``infer``, ``infer_batch`` and the batch routes of
    ``infer_from_phonemes`` / ``resynthesize`` -- each sentence is levelled, then trimmed, faded and joined.  Never streamed:
    the measure is the whole item's, and no chunked form is built.

    ``limiter``: an ``iris.limiter.Limiter`` (or any object with ``limit_device(wav [B, L], lengths=, row_scale=) -> (out [B, L],
    stats [B, 2])``): every item under the limiter's true-peak ceiling by a look-ahead gain that falls only around a peak -- so a
    ``LoudnessNormalizer(peak_ceiling=None)`` in front reaches its target.  Not streamed as it is: the gain looks ``2A + 7``
    samples past a chunk's end.  ``limiter=lim.chunked()`` (an ``iris.limiter.ChunkedLimiter``): one ``LimiterSession``; the
    first piece is short by ``2A + 7`` samples (73 at 1.5 ms and 22.05 kHz) and the last carries them, so a streamed utterance
    is held under the ceiling.  With ``lim.chunked(pcm16=True)`` the limiter's kernel stores 16-bit PCM itself: the pieces are
    int16 and their concatenation equals ``infer(mel, pcm16=True)``.

    ``assemble``: an ``iris.assemble.Assembler`` (or any object with ``join_device(wav [B, L], lengths=, row_scale=) -> (out
    [cap], offsets [B + 1], spans [B, 2])``).  With one, a batch is taken to be the sentences of one text: ``infer_batch`` --
    and so the batch routes of ``infer_from_phonemes`` and ``resynthesize`` -- return ``(waveform, spans)`` instead of a list:
    every item trimmed of its leading and trailing silence (``librosa.effects.trim``'s decision, on the device) and laid end to
    end with the assembler's pause and fades, ``spans [B, 2]`` (device, int32) saying what was kept of each item.  ``pcm16=`` /
    ``normalize=`` / ``resampler=`` then see ONE row: the peak is the joined utterance's.  Every launch is queued before the one
    read-back, the total, which sizes the result.  ``infer`` treats every row of its mel as an item of such a batch; one row is
    trimmed, a join of one.  Never streamed: the reference level is the whole item's maximum, and no chunked form is built.

    ``output``: what ``iris.resample.Resampler.chunked(encoding)`` returns (a ``ChunkedResampler``, or any object with
    ``chunked_sessions = True``, a ``forward(wav, lengths=, row_scale=)``, an ``out_range`` and an ``open_session() -> push /
    flush``): the output stage of a served utterance, the sample rate and the sample format a consumer takes -- 8 kHz G.711
    mu-law for a phone line is ``output=Resampler(8000).chunked("ulaw")``.  ``stream`` and ``session`` open its session LAST,
    behind the limiter's, or directly behind the vocoder when no other session exists; the pieces are fp32, int16 or uint8 at
    ``output.rate_out``.  ``infer`` and ``infer_batch`` without ``pcm16`` / ``normalize`` / ``resampler`` arguments apply the
    same resampler and encoding in one call behind the other stages; those arguments beside ``output=`` are refused
    (``ValueError``), and so are ``lim.chunked(pcm16=True)`` and ``forward_pcm16`` as the ``vocode``: the resampler reads fp32.

    Not built: a chunked loudness stage and a chunked assembler (above), and no chunked PCM stage behind a chunked denoiser or
    stretch -- 16-bit pieces come from ``lim.chunked(pcm16=True)`` or ``output=res.chunked('pcm16')``."""

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
        self._chunked = {s.name: getattr(self, s.name) for s in _WAVE_STAGES
                         if s.needs_fp32 and getattr(getattr(self, s.name), "chunked_sessions", False)}
        if self._chunked and getattr(vocode, "__name__", "") == "forward_pcm16":
            raise ValueError(next(s.needs_fp32 for s in _WAVE_STAGES if s.name in self._chunked))      # the first of them speaks
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

    def _output_args(self, pcm16: bool, normalize: bool, resampler) -> tuple:
        """``(pcm16, normalize, resampler)`` for the output stage of ``infer`` / ``infer_batch``: the caller's, or ``output=`` as
        the resampler -- beside which the caller names none, and no ``pcm16`` / ``normalize`` either."""
        if normalize and not pcm16:
            raise ValueError("normalize=True goes with pcm16=True")
        if self.output is None:
            return pcm16, normalize, resampler
        if pcm16 or normalize or resampler is not None:
            raise ValueError("this pipeline has output=: it decides the rate and the encoding, so pcm16=, normalize= and "
                             "resampler= are not taken beside it")
        return pcm16, normalize, self.output

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

    def _refuse_unstreamable(self, whole: Optional[Exception] = None) -> None:
        """``ValueError`` where a stage of this pipeline has no chunked form, or has one that was not opted into; of several, the
        one the table lets speak first (``speaks``).  Then the refusal of a whole-utterance vocoder: ``NotImplementedError``, or
        ``whole`` (``StreamGroup`` has its own)."""
        refused = [s for s in _WAVE_STAGES if s.unstreamable and getattr(self, s.name) is not None and s.name not in self._chunked]
        if refused:
            raise ValueError(min(refused, key=lambda s: s.speaks).unstreamable)
        if self._whole is not None:
            raise whole or NotImplementedError("a whole-utterance vocoder (Griffin-Lim) cannot be streamed: every sample "
                                               "depends on every frame")

    # -- the whole-utterance route: vocode, the chain of wave stages, finish -- every step ``_Waves -> _Waves`` -----------------
    def _has_wave_stage(self) -> bool:
        return any(getattr(self, s.name) is not None for s in _WAVE_STAGES)

    def _vocode(self, mel: torch.Tensor, frames=None, forward: Optional[Callable] = None) -> _Waves:
        """The refined ``mel`` through the vocoder, and the only place that turns frames into rows.  ``frames=None``: whole
        rows, chunked by the streamer (a whole-utterance vocoder takes the mel in one call).  ``frames``: item i's frame count,
        ONE ragged forward; item i owns ``hop`` samples per row, ``T_i`` rows -- ``T_i - 1`` from a whole-utterance vocoder, which
        takes ``lengths=`` if it says ``takes_lengths`` and else has been handed items of one length (an item of one frame is
        refused by the vocoder itself).  ``forward``: a fused route's launch in place of the streamer's (``_fused_forward``)."""
        if frames is None:
            return _Waves(self._whole.forward_device(mel) if self._whole is not None else (forward or self.streamer.infer)(mel))
        rows = [int(t) for t in frames]
        if self._whole is None:
            wav = (forward or self.streamer.forward)(mel, lengths=frames)
        else:
            ragged = getattr(self._whole, "takes_lengths", False)
            wav = self._whole.forward_device(mel, lengths=rows) if ragged else self._whole.forward_device(mel)
            rows = [max(t - 1, 0) for t in rows]
        hop = self.streamer.hop_length
        return _Waves(wav, rows, hop, [hop * r for r in rows])

    def _chain(self, waves: _Waves) -> _Waves:
        """The wave stages that are set, in the table's order."""
        for stage in _WAVE_STAGES:
            if stage.step is not None and getattr(self, stage.name) is not None:
                waves = getattr(self, stage.step)(waves)
        return waves

    def _denoise(self, waves: _Waves) -> _Waves:
        """Through the denoiser; its ``lengths`` are rows of ``hop`` samples, the vocoder's (it is the first stage)."""
        wav = waves.wav.float()
        return waves._replace(wav=self.denoiser.forward_device(wav) if waves.lengths is None
                              else self.denoiser.forward_device(wav, lengths=waves.lengths))

    def _stretch(self, waves: _Waves) -> _Waves:
        """Through the stretch.  A ragged batch goes through ONE call and leaves with the stretch's device ``counts`` as sample
        lengths; the host knows the counts from ``out_samples``: nothing synchronises."""
        wav = waves.wav.float()
        if waves.lengths is None:
            return _Waves(self.stretch.forward_device(wav)[0])
        sh = int(self.stretch.hop_length)
        for i, n in enumerate(waves.samples):
            if n % sh:
                raise ValueError(f"item {i}: {n} samples are not whole frames of the stretch's hop_length = {sh}; nothing is padded silently")
        if wav.shape[1] % sh:                                        # the padded row itself; its tail belongs to no item
            wav = torch.nn.functional.pad(wav, (0, sh - wav.shape[1] % sh))
        out, counts = self.stretch.forward_device(wav, lengths=[n // sh for n in waves.samples])
        return _Waves(out, counts, 1, [self.stretch.out_samples(n) for n in waves.samples])

    def _level(self, waves: _Waves) -> _Waves:
        """Through the loudness stage: every item at the target loudness and 0 behind its own samples.  Nothing is read back."""
        return waves._replace(wav=self.loudness.normalize_device(waves.wav.float(), lengths=waves.lengths, row_scale=waves.row_scale)[0])

    def _limit(self, waves: _Waves) -> _Waves:
        """Through the limiter: every item under the ceiling and 0 behind its own samples.  Nothing is read back."""
        return waves._replace(wav=self.limiter.limit_device(waves.wav.float(), lengths=waves.lengths, row_scale=waves.row_scale)[0])

    def _finish(self, waves: _Waves, pcm16: bool, normalize: bool, resampler, as_list: bool = False):
        """The assembler, if there is one -- the batch becomes ONE row with the device's total as its length, 0 behind it, so its
        peak is the utterance's -- then the stand-alone output stage, then the cut."""
        spans = None
        if self.assemble is not None:
            out, offsets, spans = self.assemble.join_device(waves.wav.float(), lengths=waves.lengths, row_scale=waves.row_scale)
            waves = _Waves(out[None], offsets[-1:])
        return self._cut(self._output_stage(waves, pcm16, normalize, resampler), waves, normalize, resampler, as_list, spans)

    @staticmethod
    def _output_stage(waves: _Waves, pcm16: bool, normalize: bool, resampler):
        """The stand-alone output stage on a waveform that exists: ``Resampler.forward`` with the batch's lengths, or
        ``synthesis_output.pcm16_on_device`` (``(pcm, peaks)`` with ``normalize``), or the waveform as it is."""
        if resampler is not None:
            ragged = {} if waves.lengths is None else {"lengths": waves.lengths, "row_scale": waves.row_scale}
            return resampler.forward(waves.wav, **ragged, pcm16=pcm16, normalize=normalize)
        if not pcm16:
            return waves.wav
        from .synthesis_output import pcm16_on_device
        return pcm16_on_device(waves.wav, normalize=normalize)

    @staticmethod
    def _cut(result, waves: _Waves, normalize: bool, resampler, as_list: bool, spans=None):
        """What the caller gets of ``result``, the output of the batch ``waves``: with ``spans`` ``(the joined row -- what
        ``infer`` returns for one row -- cut at the total, spans)``, the total read back once, after everything is queued; a list
        cut at each item's own count; or the rows as they are."""
        def count(n):
            return n if resampler is None else resampler.out_range(0, n)[1]
        out = result[0] if normalize else result
        if spans is not None:
            row = out[0, :count(int(waves.lengths.item()))]
            return ((row, result[1]) if normalize else row), spans
        if not as_list:
            return result
        if waves.samples is None:
            return list(out.unbind(0))
        return [out[i, :count(n)] for i, n in enumerate(waves.samples)]

    # -- the fused routes: no wave stage, so the vocoder's last launch does the conversion --------------------------------------
    def _streamer_with(self, forward: Optional[Callable] = None, resampler=None) -> StreamingVocoder:
        """This pipeline's streamer with another forward, or with a resampler behind its own."""
        sv = self.streamer
        return StreamingVocoder(forward or sv.forward, hop_length=sv.hop_length, chunk_frames=sv.chunk_frames,
                                halo_frames=sv.halo_frames, group_chunks=sv.group_chunks, config=self.config, resampler=resampler)

    def _fused_forward(self, ragged: bool, pcm16: bool, normalize: bool, resampler) -> Optional[Callable]:
        """What ``_vocode`` runs in place of the streamer's forward (None: fp32 at the vocoder's rate, nothing to fuse):
        ``GeneratorEngine.forward_pcm16`` or ``forward_resampled`` -- ONE forward for a ragged batch, for ``normalize`` (the peak is
        the whole utterance's) and for resampled PCM; chunked like the fp32 path otherwise, each resampled window at its own
        origin.  A vocoder without that forward is refused here, before anything runs."""
        if resampler is None and not pcm16:
            return None
        engine = getattr(self.streamer.forward, "__self__", None)
        if resampler is None:
            fwd = getattr(engine, "forward_pcm16", None)
            if fwd is None:
                raise ValueError("pcm16=True needs a vocoder with a device output stage: construct the pipeline with a bound "
                                 "GeneratorEngine.forward")
            if ragged or normalize:
                return lambda mel, **lengths: fwd(mel, **lengths, normalize=normalize)
            return self._streamer_with(fwd).infer
        fwd = getattr(engine, "forward_resampled", None)
        if fwd is None:
            raise ValueError("resampler= needs a vocoder with a device resampling stage: construct the pipeline with a bound "
                             "GeneratorEngine.forward")
        if ragged or pcm16:
            return lambda mel, **lengths: fwd(mel, resampler, **lengths, pcm16=pcm16, normalize=normalize)
        return self._streamer_with(resampler=resampler).infer

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
        out_args = self._output_args(pcm16, normalize, resampler)
        if self._has_wave_stage() or self._whole is not None:
            return self._finish(self._chain(self._vocode(self.refine(mel))), *out_args)
        forward = self._fused_forward(False, *out_args)
        return self._vocode(self.refine(mel), forward=forward).wav

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
        A whole-utterance vocoder with ``takes_lengths`` (``_vocode``): ``hop * (T_i - 1)`` samples per item, its rows 0 past
        them -- so an item's peak is its own.
        With ``assemble=`` the result is ``(waveform, spans)``: the items trimmed and joined into one (the class docstring)."""
        out_args = self._output_args(pcm16, normalize, resampler)
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
        if self._has_wave_stage():
            return self._finish(self._chain(self._vocode(padded, lengths)), *out_args, as_list=True)
        if self._whole is not None:                                  # items of one length and no stage behind: whole rows, as ``infer``
            return self._finish(self._vocode(padded, lengths if ragged_whole else None), *out_args, as_list=True)
        pcm16, normalize, resampler = out_args
        waves = self._vocode(padded, lengths, self._fused_forward(True, *out_args))
        if resampler is None:                                        # at the vocoder's rate: cut with its check of the row's length
            return split_waveforms(waves.wav[0] if normalize else waves.wav, lengths, self.streamer.hop_length)
        return self._cut(waves.wav, waves, normalize, resampler, as_list=True)

    def session(self, postnet_halo_frames: Optional[int] = None) -> "PipelineSession":
        """A new ``PipelineSession`` for ONE utterance whose mel is still being produced.  ``postnet_halo_frames``: the
        PostNet's receptive field on either side, for a callable that has no ``receptive_field_frames`` of its own.
        Refused with a plain denoiser, stretch or limiter (``ValueError``), as ``stream`` is; with chunked ones the session's
        pieces are those of the last of their sessions."""
        self._refuse_unstreamable()
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
