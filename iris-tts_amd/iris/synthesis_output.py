"""Output stage of the synthesis path: mel -> vocoder entry -> WAV.

What the reference does after the mel is ready (``scripts/synthesize.py:171-216``): ``np.array(mel)``,
call the vocoder, cast to float32, ``squeeze`` to 1-D, log the duration, create the output directory
and ``soundfile.write(path, audio, sample_rate)``, falling back to ``np.save(path.with_suffix(".npy"))``
when soundfile is missing or fails.  The reference also documents -- but never wired -- a pluggable
vocoder selected as ``--vocoder_entry module:function`` with the signature
``function(mel, sample_rate, hop_length) -> np.ndarray[samples]`` (``HIFIGAN_SETUP.md:61-75``,
``README.md:155-158``; ``synthesize.py`` imports ``importlib`` at :9 and never uses it).

This module wires exactly that convention and the output stage; ``python -m iris.synthesis_output``
is the CLI for a mel that already exists as a ``.npy`` file (the text front-end, encoder and VAE that
produce it are outside this repo's scope).
"""
from __future__ import annotations

import argparse
import importlib
import logging
import struct
import wave
from pathlib import Path
from typing import Callable, Optional, Union

import numpy as np

logger = logging.getLogger(__name__)

DEFAULT_VOCODER_ENTRY = "iris.hifigan_pretrained:infer_hifigan"
PCM16_VOCODER_ENTRY = "iris.hifigan_pretrained:infer_hifigan_pcm16"    # 16-bit PCM converted on the device (--pcm16)
VocoderEntry = Callable[..., np.ndarray]


def resolve_vocoder_entry(spec: str) -> VocoderEntry:
    """``"package.module:function"`` -> the callable (``HIFIGAN_SETUP.md:61-75``)."""
    if not isinstance(spec, str) or spec.count(":") != 1:
        raise ValueError(f"--vocoder_entry must look like 'module:function', got {spec!r}")
    module_name, func_name = spec.split(":")
    if not module_name or not func_name:
        raise ValueError(f"--vocoder_entry must look like 'module:function', got {spec!r}")
    module = importlib.import_module(module_name)
    try:
        fn = getattr(module, func_name)
    except AttributeError as exc:
        raise AttributeError(f"module {module_name!r} has no attribute {func_name!r}") from exc
    if not callable(fn):
        raise TypeError(f"{spec} is not callable")
    return fn


def to_mono_float32(audio) -> np.ndarray:
    """float32 cast + squeeze to 1-D, as ``synthesize.py:199-203``."""
    audio = np.asarray(audio, dtype=np.float32)
    if audio.ndim > 1:
        audio = audio.squeeze()
    if audio.ndim != 1:
        raise ValueError(f"expected a single waveform after squeeze, got shape {audio.shape}")
    return audio


def _check_peak_target(peak_target) -> np.float32:
    if not 0.0 < float(peak_target) <= 1.0:
        raise ValueError(f"peak_target must lie in (0, 1], got {peak_target}")
    return np.float32(peak_target)


def pcm16_from_float(audio, normalize: bool = False, peak_target: float = 0.95) -> np.ndarray:
    """float waveform -> 16-bit PCM (little-endian int16, same shape), in float32 arithmetic throughout:

        ``pcm = round(clip(w, -1, 1) * 32767)``            (``np.round``: half to even)

    and with ``normalize`` first ``w = (w / (peak + 1e-8)) * peak_target``, ``peak`` the largest ``|w|`` along the last
    axis -- per item of a batch; the scheme of the reference's demo_vocoder.py, 0.95 / (max|w| + 1e-8), restated with
    every operation a float32 rounding of its own.  A silent or empty item has peak 0 and stays 0.  This is the host
    restatement of the device output stage (``GeneratorEngine.forward_pcm16``, csrc/pcm_out.h): the two agree bit for bit."""
    w = np.asarray(audio, dtype=np.float32)
    if normalize:
        target = _check_peak_target(peak_target)
        peak = np.max(np.abs(w), axis=-1, keepdims=True, initial=np.float32(0.0)) if w.ndim else np.abs(w)
        w = (w / (peak.astype(np.float32) + np.float32(1e-8))) * target
    return np.round(np.clip(w, np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)).astype("<i2")


def pcm16_on_device(wav, normalize: bool = False, peak_target: float = 0.95):
    """The device output stage on a waveform that already exists (``iris_hifigan_op_pcm16``, csrc/pcm_out.h): an fp32 device
    tensor ``[B, L]`` -> int16 ``[B, L]``, bit for bit ``pcm16_from_float(wav)``; with ``normalize`` every item is scaled to
    ``peak_target`` at its own peak first and ``(pcm, peaks)`` is returned, ``peaks`` the fp32 tensor ``[B]`` of the items'
    max |w|.  Asynchronous on the current stream.  For vocoders without an output stage of their own (``iris.griffin_lim``)."""
    import ctypes

    import torch

    from . import _native
    if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
        raise ValueError(f"expected an fp32 device waveform [B, L], got {wav.dtype} {tuple(wav.shape)} on {wav.device}")
    if normalize:
        _check_peak_target(peak_target)
    wav = wav.contiguous()
    B, L = int(wav.shape[0]), int(wav.shape[1])
    pcm = torch.empty((B, L), dtype=torch.int16, device=wav.device)
    peaks = torch.zeros((B,), dtype=torch.float32, device=wav.device) if normalize else None
    if B and L:
        with torch.cuda.device(wav.device):
            _native.check("iris_hifigan_op_pcm16", _native.load().iris_hifigan_op_pcm16(
                ctypes.c_void_p(wav.data_ptr()), None, 1, ctypes.c_void_p(pcm.data_ptr()),
                ctypes.c_void_p(None if peaks is None else peaks.data_ptr()), B, L, int(bool(normalize)),
                ctypes.c_float(float(peak_target)), ctypes.c_void_p(torch.cuda.current_stream(wav.device).cuda_stream)))
    return (pcm, peaks) if normalize else pcm


ENCODINGS = ("f32", "pcm16", "ulaw", "alaw")      # what the device stores: fp32, int16, or one G.711 byte per sample
G711_ZERO = {"ulaw": 0xFF, "alaw": 0xD5}          # the code of sample 0: what padding holds (byte 0 decodes to -32 124)
G711_WAV_TAG = {"ulaw": 7, "alaw": 6}             # WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW


def check_encoding(encoding: str, g711_only: bool = False) -> str:
    allowed = tuple(G711_ZERO) if g711_only else ENCODINGS
    if encoding not in allowed:
        raise ValueError(f"encoding must be one of {allowed}, got {encoding!r}")
    return encoding


def _floor_log2(m: np.ndarray) -> np.ndarray:
    """``floor(log2 m)`` of positive int32 below 2^16, in integers (the device counts leading zeros)."""
    e = np.zeros_like(m)
    for k in range(1, 16):
        e += (m >> k) > 0
    return e


def ulaw_from_pcm16(pcm) -> np.ndarray:
    """int16 samples -> G.711 mu-law bytes (uint8, same shape), the rule of include/iris_hifigan.h in integers alone:
    ``sign = s < 0``, ``m = min(|s|, 32635) + 132``, ``e = floor(log2 m) - 7``, ``mant = (m >> (e + 3)) & 15``,
    ``byte = ~(sign << 7 | e << 4 | mant) & 0xFF``.  The host restatement of the device's store form (csrc/pcm_out.h): the two
    agree on all 65 536 samples.  Not ``audioop.lin2ulaw``, which shifts by 2 before it takes the sign (381 inputs differ)."""
    s = np.asarray(pcm).astype(np.int32)
    sign = (s < 0).astype(np.int32)
    m = np.minimum(np.abs(s), 32635) + 132
    e = _floor_log2(m) - 7
    mant = (m >> (e + 3)) & 15
    return (~(sign << 7 | e << 4 | mant) & 0xFF).astype(np.uint8)


def alaw_from_pcm16(pcm) -> np.ndarray:
    """int16 samples -> G.711 A-law bytes (uint8, same shape): ``a = s >> 3`` (arithmetic); ``a < 0``: ``a = ~a``, ``mask = 0x55``,
    else ``mask = 0xD5``; ``seg = 0 if a < 32 else floor(log2 a) - 4``; ``mant = (a >> 1) & 15 if seg < 2 else (a >> seg) & 15``;
    ``byte = (seg << 4 | mant) ^ mask``.  Equal to ``audioop.lin2alaw`` on all 65 536 samples, and to the device's store form."""
    a = np.asarray(pcm).astype(np.int32) >> 3
    neg = a < 0
    a = np.where(neg, ~a, a)
    mask = np.where(neg, 0x55, 0xD5)
    seg = np.where(a < 32, 0, _floor_log2(np.maximum(a, 1)) - 4)
    mant = np.where(seg < 2, a >> 1, a >> seg) & 15
    return ((seg << 4 | mant) ^ mask).astype(np.uint8)


def pcm16_from_ulaw(code) -> np.ndarray:
    """The standard G.711 mu-law decoder: bytes -> int16 (``((mant << 3) + 132 << e) - 132`` with the sign)."""
    u = ~np.asarray(code).astype(np.int32) & 0xFF
    t = ((((u & 15) << 3) + 132) << ((u >> 4) & 7)) - 132
    return np.where(u & 0x80, -t, t).astype(np.int16)


def pcm16_from_alaw(code) -> np.ndarray:
    """The standard G.711 A-law decoder: bytes -> int16."""
    a = np.asarray(code).astype(np.int32) ^ 0x55
    seg = (a >> 4) & 7
    t = (a & 15) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def g711_from_float(audio, encoding: str) -> np.ndarray:
    """float waveform -> G.711 bytes: the law of ``pcm16_from_float(audio)``, which is what the device stores."""
    enc = ulaw_from_pcm16 if check_encoding(encoding, g711_only=True) == "ulaw" else alaw_from_pcm16
    return enc(pcm16_from_float(audio))


def g711_on_device(wav, encoding: str, lengths=None, row_scale: int = 1):
    """The stand-alone G.711 stage on a waveform that exists (``iris_hifigan_op_g711``, csrc/pcm_out.h): an fp32 device tensor
    ``[B, L]`` -> uint8 ``[B, L]``, bit for bit ``g711_from_float(wav, encoding)``.  ``lengths`` (an int32 device tensor ``[B]``)
    and ``row_scale``: item b owns ``min(L, lengths[b] * row_scale)`` samples and the rest of its row holds the code for 0."""
    import ctypes

    import torch

    from . import _native
    law = _native.OUT_FORMS[check_encoding(encoding, g711_only=True)]
    if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
        raise ValueError(f"expected an fp32 device waveform [B, L], got {wav.dtype} {tuple(wav.shape)} on {wav.device}")
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.device != wav.device or tuple(lengths.shape) != (wav.shape[0],)):
        raise ValueError(f"lengths must be an int32 tensor [{wav.shape[0]}] on {wav.device}")
    wav = wav.contiguous()
    B, L = int(wav.shape[0]), int(wav.shape[1])
    out = torch.empty((B, L), dtype=torch.uint8, device=wav.device)
    if B and L:
        with torch.cuda.device(wav.device):
            _native.check("iris_hifigan_op_g711", _native.load().iris_hifigan_op_g711(
                ctypes.c_void_p(wav.data_ptr()), B, L, ctypes.c_void_p(None if lengths is None else lengths.data_ptr()),
                int(row_scale), law, ctypes.c_void_p(out.data_ptr()),
                ctypes.c_void_p(torch.cuda.current_stream(wav.device).cuda_stream)))
    return out


RESAMPLE_TO_RANGE = (4000, 192000)     # what the device resampler admits (include/iris_hifigan.h)


def check_resample_to(hz) -> int:
    """``--resample_to``: an integer rate inside ``RESAMPLE_TO_RANGE`` (the library decides the rest: up <= 640, taps <= 256)."""
    if isinstance(hz, bool) or int(hz) != hz or not RESAMPLE_TO_RANGE[0] <= int(hz) <= RESAMPLE_TO_RANGE[1]:
        raise ValueError(f"resample_to must be an integer rate in [{RESAMPLE_TO_RANGE[0]}, {RESAMPLE_TO_RANGE[1]}] Hz, got {hz}")
    return int(hz)


TEMPO_RANGE = (0.25, 4.0)              # what the device time stretch admits (include/iris_hifigan.h)
PITCH_STEPS_RANGE = (-12.0, 12.0)       # semitones: the stretch behind a shift stays inside TEMPO_RANGE with room to spare


def check_tempo(rate) -> float:
    """``--tempo``: a finite rate inside ``TEMPO_RANGE`` (above 1 is faster)."""
    r = float(rate)
    if not TEMPO_RANGE[0] <= r <= TEMPO_RANGE[1]:             # False for NaN too
        raise ValueError(f"tempo must be a rate in [{TEMPO_RANGE[0]}, {TEMPO_RANGE[1]}], got {rate}")
    return r


def check_pitch_steps(n_steps) -> float:
    """``--pitch_steps``: semitones inside ``PITCH_STEPS_RANGE`` (fractions are fine)."""
    n = float(n_steps)
    if not PITCH_STEPS_RANGE[0] <= n <= PITCH_STEPS_RANGE[1]:
        raise ValueError(f"pitch_steps must lie in [{PITCH_STEPS_RANGE[0]:g}, {PITCH_STEPS_RANGE[1]:g}] semitones, got {n_steps}")
    return n


def check_trim_db(top_db) -> float:
    """``--trim_db``: a finite threshold above 0, in dB below the waveform's loudest frame."""
    db = float(top_db)
    if not 0.0 < db < float("inf"):                           # False for NaN too
        raise ValueError(f"trim_db must be a finite threshold above 0 dB, got {top_db}")
    return db


def check_lufs(target) -> float:
    """``--lufs``: a finite target loudness in -70 .. 0 LUFS."""
    lufs = float(target)
    if not -70.0 <= lufs <= 0.0:                              # False for NaN too
        raise ValueError(f"lufs must be a target loudness in -70 .. 0 LUFS, got {target}")
    return lufs


def level_to_lufs(audio: np.ndarray, target_lufs: float, sample_rate: int = 22050, peak_ceiling: Optional[float] = 1.0) -> np.ndarray:
    """A float waveform ``[n]`` at ``target_lufs`` integrated loudness (ITU-R BS.1770-4, measured and applied on the device,
    ``iris.loudness``); the gain stops where the sample peak would pass ``peak_ceiling``.  A waveform shorter than 400 ms, or
    with nothing above -70 LUFS, is returned as it is."""
    from .loudness import LoudnessNormalizer
    audio = to_mono_float32(audio)
    if len(audio) == 0:
        return audio
    stage = LoudnessNormalizer(sample_rate, check_lufs(target_lufs), peak_ceiling=peak_ceiling)
    return stage.normalize_device(audio[None])[0][0].cpu().numpy()


LIMIT_DBTP_RANGE = (-20.0, 0.0)         # true-peak ceilings the command line takes


def check_limit_dbtp(ceiling) -> float:
    """``--limit_dbtp``: a finite true-peak ceiling in -20 .. 0 dBTP."""
    db = float(ceiling)
    if not LIMIT_DBTP_RANGE[0] <= db <= LIMIT_DBTP_RANGE[1]:  # False for NaN too
        raise ValueError(f"limit_dbtp must be a true-peak ceiling in -20 .. 0 dBTP, got {ceiling}")
    return db


def limit_true_peak(audio: np.ndarray, ceiling_dbtp: float, sample_rate: int = 22050) -> np.ndarray:
    """A float waveform ``[n]`` held under ``ceiling_dbtp`` by the device look-ahead limiter (``iris.limiter``, 1.5 ms of
    lookahead, at most its 256 samples): the gain falls only around a peak, and a waveform under the ceiling is returned bit
    for bit."""
    from .limiter import MAX_LOOKAHEAD, Limiter
    audio = to_mono_float32(audio)
    if len(audio) == 0:
        return audio
    ms = min(1.5, 1000.0 * MAX_LOOKAHEAD / float(sample_rate))
    return Limiter(sample_rate, check_limit_dbtp(ceiling_dbtp), ms).limit_device(audio[None])[0][0].cpu().numpy()


def g711_encode(audio: np.ndarray, encoding: str, resample_to: Optional[int] = None, sample_rate: int = 22050) -> np.ndarray:
    """A float waveform ``[n]`` -> G.711 bytes on the device: with ``resample_to`` the resampler converts from ``sample_rate`` and
    stores the bytes in its own launch (``Resampler.forward(encoding=)``), otherwise the stand-alone op encodes at the rate the
    waveform has (``g711_on_device``)."""
    import torch

    from ._engine import require_gpu
    check_encoding(encoding, g711_only=True)
    audio = to_mono_float32(audio)
    if len(audio) == 0:
        return np.zeros(0, dtype=np.uint8)
    wav = torch.from_numpy(audio[None]).to(require_gpu())
    if resample_to is None:
        return g711_on_device(wav, encoding)[0].cpu().numpy()
    from .resample import Resampler
    rs = Resampler(check_resample_to(resample_to), rate_in=int(sample_rate), device=wav.device)
    try:
        return rs.forward(wav, encoding=encoding)[0].cpu().numpy()
    finally:
        rs.close()


def trim_silence(audio: np.ndarray, top_db: float, frame_length: int = 2048, hop_length: int = 512) -> np.ndarray:
    """A float waveform ``[n]`` without its leading and trailing silence: ``librosa.effects.trim(audio, top_db=)``'s decision on
    the device (``iris.assemble``)."""
    from .assemble import Assembler
    audio = to_mono_float32(audio)
    if len(audio) == 0:
        return audio
    return Assembler(frame_length, hop_length, check_trim_db(top_db)).join(audio[None])[0].cpu().numpy()


def tempo_and_pitch(audio: np.ndarray, tempo: Optional[float] = None, pitch_steps: Optional[float] = None, n_fft: int = 1024,
                    hop_length: int = 256) -> np.ndarray:
    """A float waveform ``[n]`` through the device phase vocoder (``iris.time_stretch``): first the pitch, at its own length,
    then the tempo, to ``round(n / tempo)`` samples.  The stretch takes whole frames, so the waveform is zero-padded to a
    multiple of ``hop_length`` on the way in and the result is cut to the length ``n`` asks for."""
    import torch

    from .time_stretch import TimeStretch, pitch_shift_device
    audio = to_mono_float32(audio)
    n = len(audio)
    if n == 0 or (tempo is None and pitch_steps is None):
        return audio
    ts = TimeStretch(n_fft, hop_length)
    wav = torch.from_numpy(np.pad(audio, (0, -n % hop_length))[None])
    if pitch_steps is not None:
        wav = pitch_shift_device(ts, wav, check_pitch_steps(pitch_steps))
        wav[:, n:] = 0
    if tempo is not None:
        out = ts.forward_device(wav, check_tempo(tempo))[0][0, :int(round(n / float(tempo)))]
    else:
        out = wav[0, :n]
    return out.cpu().numpy()


def g711_wav_bytes(code: np.ndarray, sample_rate: int, encoding: str) -> bytes:
    """A mono G.711 WAV file as bytes: format tag 7 (mu-law) or 6 (A-law), 8 bits, the 18-byte ``fmt `` chunk a non-PCM format
    carries (``cbSize = 0``), a ``fact`` chunk with the sample count, then the data (padded to an even length).  Packed with
    ``struct``: the ``wave`` module writes PCM only."""
    tag = G711_WAV_TAG[check_encoding(encoding, g711_only=True)]
    data = np.ascontiguousarray(code, dtype=np.uint8).tobytes()
    n, rate = len(data), int(sample_rate)
    pad = n & 1
    fmt = struct.pack("<4sIHHIIHHH", b"fmt ", 18, tag, 1, rate, rate, 1, 8, 0)
    fact = struct.pack("<4sII", b"fact", 4, n)
    body = b"WAVE" + fmt + fact + struct.pack("<4sI", b"data", n) + data + b"\x00" * pad
    return struct.pack("<4sI", b"RIFF", len(body)) + body


def write_wav(path: Union[str, Path], audio: np.ndarray, sample_rate: int = 22050, encoding: Optional[str] = None) -> Path:
    """Writes a mono WAV.  Float samples: ``soundfile`` is used when importable (the reference's writer,
    ``synthesize.py:211-213``); otherwise the standard-library ``wave`` module writes 16-bit PCM
    (``pcm16_from_float``), which is also what soundfile's default WAV subtype produces.  An int16 array (one waveform
    after squeeze; what ``forward_pcm16`` / ``infer_hifigan_pcm16`` return) already is that PCM and is written verbatim
    by ``wave``.  On failure the samples are saved as ``.npy`` next to the requested path, like the reference
    (:214-216).  Returns the path actually written.  A uint8 array goes with ``encoding="ulaw"`` or ``"alaw"``: G.711 bytes
    (what ``Resampler.forward(encoding=)`` and a telephony stream return), written verbatim behind a header with format tag 7
    or 6 (``g711_wav_bytes``); a uint8 array without a law, or a law with anything else, is refused."""
    out_path = Path(path)
    is_g711 = isinstance(audio, np.ndarray) and audio.dtype == np.uint8
    if is_g711 != (encoding in G711_ZERO):
        raise ValueError(f"G.711 bytes are a uint8 array with encoding='ulaw' or 'alaw': got {getattr(audio, 'dtype', type(audio))} "
                         f"with encoding={encoding!r}")
    if encoding not in (None, "pcm16") and not is_g711:
        raise ValueError(f"write_wav writes 16-bit PCM or G.711: encoding={encoding!r} is neither")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    if is_g711:
        audio = audio.squeeze() if audio.ndim > 1 else audio
        if audio.ndim != 1:
            raise ValueError(f"expected a single waveform after squeeze, got shape {audio.shape}")
        try:
            out_path.write_bytes(g711_wav_bytes(audio, sample_rate, encoding))
            logger.info(f"Wrote {out_path}")
            return out_path
        except Exception as exc:  # same fallback as the reference
            npy = out_path.with_suffix(".npy")
            np.save(str(npy), audio)
            logger.warning(f"WAV write failed; wrote numpy array instead: {npy} ({exc})")
            return npy
    is_pcm = isinstance(audio, np.ndarray) and audio.dtype == np.int16
    if is_pcm:
        audio = audio.squeeze() if audio.ndim > 1 else audio
        if audio.ndim != 1:
            raise ValueError(f"expected a single waveform after squeeze, got shape {audio.shape}")
    else:
        audio = to_mono_float32(audio)
    def write_pcm(pcm: np.ndarray) -> None:
        with wave.open(str(out_path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(int(sample_rate))
            w.writeframes(pcm.astype("<i2", copy=False).tobytes())

    try:
        if is_pcm:
            write_pcm(audio)
        else:
            try:
                import soundfile as sf  # optional dependency
                sf.write(str(out_path), audio, sample_rate)
            except ImportError:
                write_pcm(pcm16_from_float(audio))
        logger.info(f"Wrote {out_path}")
        return out_path
    except Exception as exc:  # same fallback as the reference
        npy = out_path.with_suffix(".npy")
        np.save(str(npy), audio)
        logger.warning(f"WAV write failed; wrote numpy array instead: {npy} ({exc})")
        return npy


def vocode_to_wav(mel: np.ndarray, output_wav: Union[str, Path], vocoder_entry: str = DEFAULT_VOCODER_ENTRY,
                  sample_rate: int = 22050, hop_length: int = 256, normalize_peak: Optional[float] = None,
                  resample_to: Optional[int] = None, tempo: Optional[float] = None, pitch_steps: Optional[float] = None,
                  trim_db: Optional[float] = None, lufs: Optional[float] = None, limit_dbtp: Optional[float] = None,
                  encoding: Optional[str] = None) -> np.ndarray:
    """mel ``[1, n_mels, T]`` or ``[n_mels, T]`` -> waveform written to ``output_wav``; returns the samples: float32, or
    int16 when the entry returned 16-bit PCM (``PCM16_VOCODER_ENTRY``), which is kept and written as it is.
    ``normalize_peak``: scale the utterance so that its peak is this value in (0, 1] -- the entry is then called with
    ``normalize=True, peak_target=`` (an entry that converts on the device, ``infer_hifigan_pcm16``) when it returns PCM; a float result is
    normalised on the host (``pcm16_from_float``).
    ``resample_to``: the entry is called with ``sample_rate_out=`` (``infer_hifigan`` / ``infer_hifigan_pcm16`` then convert
    the generator's 22 050 Hz on the GPU, ``iris.resample``) and the WAV header carries that rate; ``sample_rate`` keeps
    labelling only, as in the reference.
    ``tempo`` / ``pitch_steps``: the entry's float waveform goes through ``tempo_and_pitch`` (the device phase vocoder) before
    it is normalised and written; an entry that returns 16-bit PCM is refused (``ValueError``), the stage takes fp32.
    ``trim_db``: the entry's float waveform loses its leading and trailing silence first (``trim_silence``); an entry that
    returns 16-bit PCM is refused in the same way.
    ``lufs``: the float waveform -- behind the tempo and pitch stage, in front of ``normalize_peak`` -- is brought to this
    integrated loudness (``level_to_lufs``, at ``resample_to`` where that is given); 16-bit PCM is refused in the same way.
    ``limit_dbtp``: behind ``lufs``, the float waveform is held under this true-peak ceiling by the look-ahead limiter
    (``limit_true_peak``); ``level_to_lufs`` then runs with no peak ceiling of its own, so the target is reached.  16-bit PCM
    is refused in the same way.
    ``encoding``: ``"ulaw"`` or ``"alaw"`` writes a G.711 WAV (``g711_encode``: one byte per sample, stored by the device) and
    returns the uint8 bytes.  The entry is then called WITHOUT ``sample_rate_out``: the float stages above run at the
    generator's rate and ``resample_to`` converts last, in the launch that stores the bytes; without ``resample_to`` the
    stand-alone op encodes at the generator's rate.  An entry that returns 16-bit PCM and ``normalize_peak`` are refused beside
    it.  ``"pcm16"`` and None change nothing."""
    g711 = encoding in G711_ZERO
    if encoding is not None and not g711 and check_encoding(encoding) != "pcm16":
        raise ValueError(f"encoding must be 'pcm16', 'ulaw' or 'alaw' here, got {encoding!r}")
    if g711 and normalize_peak is not None:
        raise ValueError("normalize_peak does not go with a G.711 encoding: the companding law is defined on the unscaled sample")
    if lufs is not None:
        check_lufs(lufs)
    if limit_dbtp is not None:
        check_limit_dbtp(limit_dbtp)
    if trim_db is not None:
        check_trim_db(trim_db)
    if tempo is not None:
        check_tempo(tempo)
    if pitch_steps is not None:
        check_pitch_steps(pitch_steps)
    fn = resolve_vocoder_entry(vocoder_entry)
    if (tempo is not None or pitch_steps is not None) and getattr(fn, "returns_pcm16", False):
        raise ValueError("tempo / pitch_steps take the vocoder's float waveform: use an entry that returns float32 (not --pcm16)")
    if trim_db is not None and getattr(fn, "returns_pcm16", False):
        raise ValueError("trim_db takes the vocoder's float waveform: use an entry that returns float32 (not --pcm16)")
    if lufs is not None and getattr(fn, "returns_pcm16", False):
        raise ValueError("lufs takes the vocoder's float waveform: use an entry that returns float32 (not --pcm16)")
    if g711 and getattr(fn, "returns_pcm16", False):
        raise ValueError("a G.711 encoding takes the vocoder's float waveform: use an entry that returns float32 (not --pcm16)")
    if limit_dbtp is not None and getattr(fn, "returns_pcm16", False):
        raise ValueError("limit_dbtp takes the vocoder's float waveform: use an entry that returns float32 (not --pcm16)")
    mel = np.array(mel)
    logger.info(f"Using vocoder entry {vocoder_entry} ...")
    if normalize_peak is not None:
        _check_peak_target(normalize_peak)
    extra = {}
    if resample_to is not None:
        out_rate = check_resample_to(resample_to)
        if not g711:
            extra["sample_rate_out"] = out_rate
        wav_rate = sample_rate if g711 else out_rate
    else:
        wav_rate = out_rate = sample_rate
    if normalize_peak is not None and getattr(fn, "returns_pcm16", False):
        audio = fn(mel, sample_rate, hop_length, normalize=True, peak_target=float(normalize_peak), **extra)
    else:
        audio = fn(mel, sample_rate, hop_length, **extra)
    if isinstance(audio, np.ndarray) and audio.dtype == np.int16:
        if g711:
            raise ValueError("a G.711 encoding takes the vocoder's float waveform, the entry returned 16-bit PCM")
        audio = audio.squeeze() if audio.ndim > 1 else audio
        if audio.ndim != 1:
            raise ValueError(f"expected a single waveform after squeeze, got shape {audio.shape}")
    else:
        audio = to_mono_float32(audio)
        if trim_db is not None:
            audio = trim_silence(audio, trim_db)
        if tempo is not None or pitch_steps is not None:
            audio = tempo_and_pitch(audio, tempo, pitch_steps, hop_length=hop_length)
        if lufs is not None:
            audio = level_to_lufs(audio, lufs, wav_rate) if limit_dbtp is None else level_to_lufs(audio, lufs, wav_rate, peak_ceiling=None)
        if limit_dbtp is not None:
            audio = limit_true_peak(audio, limit_dbtp, wav_rate)
        if normalize_peak is not None:
            audio = pcm16_from_float(audio, normalize=True, peak_target=normalize_peak)
    if g711:
        audio = g711_encode(audio, encoding, resample_to=None if resample_to is None else out_rate, sample_rate=sample_rate)
    logger.info(f"Generated audio: {audio.shape}, duration={len(audio) / out_rate:.2f}s")
    write_wav(output_wav, audio, out_rate, encoding=encoding if g711 else None)
    return audio


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Vocode a mel-spectrogram (.npy) to a WAV file")
    parser.add_argument("--mel", required=True, help=".npy file with a mel [n_mels, T] or [1, n_mels, T]")
    parser.add_argument("--output_wav", type=str, default="outputs/sample.wav")        # synthesize.py:67
    parser.add_argument("--vocoder", type=str, default="hifigan", choices=["hifigan"])  # README.md:155-158
    parser.add_argument("--vocoder_entry", type=str, default=DEFAULT_VOCODER_ENTRY)
    parser.add_argument("--sample_rate", type=int, default=22050)                       # synthesize.py:77
    parser.add_argument("--hop_length", type=int, default=256)                          # synthesize.py:78
    parser.add_argument("--pcm16", action="store_true",
                        help=f"convert to 16-bit PCM on the GPU (vocoder entry {PCM16_VOCODER_ENTRY} unless --vocoder_entry is given)")
    parser.add_argument("--normalize_peak", type=float, default=None, metavar="X",
                        help="scale the utterance so that its peak is X, 0 < X <= 1 (the reference demo uses 0.95)")
    parser.add_argument("--resample_to", type=int, default=None, metavar="HZ",
                        help="convert the generator's 22050 Hz waveform to HZ on the GPU (8000, 16000, 44100, 48000, ...); the "
                             "WAV header then carries HZ (--sample_rate keeps labelling only)")
    parser.add_argument("--tempo", type=float, default=None, metavar="RATE",
                        help="play RATE times as fast at the same pitch (0.25 .. 4; the device phase vocoder, iris.time_stretch)")
    parser.add_argument("--pitch_steps", type=float, default=None, metavar="N",
                        help="shift the pitch by N semitones at the same length (-12 .. 12, fractions allowed)")
    parser.add_argument("--trim_db", type=float, default=None, metavar="DB",
                        help="cut leading and trailing silence more than DB below the loudest frame (librosa.effects.trim's "
                             "decision on the GPU, iris.assemble), before the other output options")
    parser.add_argument("--lufs", type=float, default=None, metavar="TARGET",
                        help="bring the waveform to TARGET LUFS integrated loudness (-70 .. 0; ITU-R BS.1770-4 on the GPU, "
                             "iris.loudness), behind --trim_db / --tempo / --pitch_steps")
    parser.add_argument("--limit_dbtp", type=float, default=None, metavar="DB",
                        help="hold the waveform under a true-peak ceiling of DB dBTP (-20 .. 0; the look-ahead limiter on the GPU, "
                             "iris.limiter), behind --lufs, which then reaches its target instead of stopping at the sample peak")
    parser.add_argument("--encoding", type=str, default=None, choices=["pcm16", "ulaw", "alaw"],
                        help="what the WAV holds: pcm16 (as --pcm16), or G.711 mu-law / A-law bytes stored by the GPU -- telephony, "
                             "usually with --resample_to 8000; without it the bytes are at the generator's rate")
    return parser


def main(argv: Optional[list] = None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.normalize_peak is not None and not 0.0 < args.normalize_peak <= 1.0:
        parser.error(f"--normalize_peak must lie in (0, 1], got {args.normalize_peak}")
    if args.resample_to is not None:
        try:
            check_resample_to(args.resample_to)
        except ValueError as exc:
            parser.error(f"--{exc}")
    for name, check in (("tempo", check_tempo), ("pitch_steps", check_pitch_steps), ("trim_db", check_trim_db), ("lufs", check_lufs),
                        ("limit_dbtp", check_limit_dbtp)):
        if getattr(args, name) is not None:
            try:
                check(getattr(args, name))
            except ValueError as exc:
                parser.error(f"--{exc}")
            if args.pcm16:
                parser.error(f"--{name} takes the float waveform: it does not go with --pcm16")
    if args.encoding == "pcm16":
        args.pcm16 = True
    elif args.encoding is not None:
        if args.pcm16:
            parser.error(f"--encoding {args.encoding} takes the float waveform: it does not go with --pcm16")
        if args.normalize_peak is not None:
            parser.error(f"--encoding {args.encoding} does not go with --normalize_peak")
    if args.pcm16 and args.vocoder_entry == DEFAULT_VOCODER_ENTRY:
        args.vocoder_entry = PCM16_VOCODER_ENTRY
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    mel = np.load(args.mel, allow_pickle=False)
    vocode_to_wav(mel, args.output_wav, args.vocoder_entry, args.sample_rate, args.hop_length, args.normalize_peak,
                  args.resample_to, args.tempo, args.pitch_steps, args.trim_db, args.lufs, args.limit_dbtp,
                  None if args.encoding == "pcm16" else args.encoding)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
