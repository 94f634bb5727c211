"""Recording fakes and the case matrix behind ``tests/test_pipeline_routes.py``: which calls ``MelToWavePipeline`` makes on its
stages, for every combination of wave stages, vocoder kind, entry point and output argument.  Pure CPU, no native library.

    python tests/pipeline_routes_cases.py --write     # records tests/golden/pipeline_routes.json.gz from the pipeline in the tree
    python tests/pipeline_routes_cases.py --print     # the recorded file as the text it holds: JSON, one line or record per row

The file was written once, from the pipeline as it stood before its routes were merged into one chain, and is not written
again: a pipeline that passes the test hands every stage the calls that one did.

Every fake multiplies the waveform by its own power of two (all values stay exact integers in fp32) and appends one line to a
shared log: ``name.method(arguments)``, a tensor as dtype, shape and the sum of its values -- so the order in which the stages
ran shows in the values each one was handed -- ``lengths`` as ``None``, ``list:[...]``, ``ndarray:[...]`` or ``tensor:[...]``,
and every keyword that was passed, by name.  A keyword that was not passed is not in the line.  The host arithmetic a stage
offers (``out_samples``, ``out_range``, ``half_width``) launches nothing and is not logged; what it returned shows in the
shapes of the outcome.  A case's record is its log and its outcome: the result's structure, or the exception's type and text.
"""
from __future__ import annotations

import gzip
import io
import itertools
import json
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden" / "pipeline_routes.json.gz"       # 0.5 MB of readable JSON, stored compressed
if str(REPO / "iris-tts_amd") not in sys.path:
    sys.path.insert(0, str(REPO / "iris-tts_amd"))

HOP, N_MELS, CHUNK = 4, 2, 4
LOG: list = []


# ---- describing values ------------------------------------------------------------------------------------------------------
_DT = {torch.float32: "f32", torch.float64: "f64", torch.int16: "i16", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8"}


def _total(t: torch.Tensor):
    s = t.double().sum().item() if t.is_floating_point() else int(t.long().sum().item())
    return repr(s)


def _tensor(t: torch.Tensor) -> str:
    return f"{_DT[t.dtype]}{list(t.shape)}S{_total(t)}"


def show(v) -> str:
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, torch.Tensor):
        if v.dim() == 1 and not v.is_floating_point() and v.numel() <= 8:
            return f"tensor:{_DT[v.dtype]}{v.tolist()}"
        return _tensor(v)
    if isinstance(v, np.ndarray):
        return f"ndarray:{v.dtype}{v.tolist()}"
    if isinstance(v, np.generic):
        return f"{type(v).__name__}({v.item()!r})"
    if isinstance(v, (list, tuple)):
        return ("list:[" if isinstance(v, list) else "tuple:(") + ", ".join(show(x) for x in v) + ("]" if isinstance(v, list) else ")")
    return getattr(v, "name", type(v).__name__)


def log_call(name: str, args, kw) -> None:
    LOG.append(f"{name}({', '.join([show(a) for a in args] + [f'{k}={show(x)}' for k, x in kw.items()])})")


def _owned(lengths, row_scale, B, L):
    """Samples per item under the stages' convention, as a list of ints (the fakes may read a device tensor: they are the device)."""
    if lengths is None:
        return [L] * B
    return [int(n) * int(row_scale) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]


def _mask(wav, counts):
    out = torch.zeros_like(wav)
    for i, n in enumerate(counts):
        out[i, :n] = wav[i, :n]
    return out


# ---- vocoders ---------------------------------------------------------------------------------------------------------------
def _wave(mel, lengths=None, drop=0):
    """The fakes' vocoder arithmetic, pointwise in frames so chunk seams are exact: frame t of item b becomes the ``HOP`` samples
    ``(2 * mel[b, 0, t] + mel[b, 1, t] + 7) * (1, 2, 3, 4)``, rows 0 behind ``HOP * (lengths[b] - drop)``."""
    base = (2 * mel[:, 0] + mel[:, 1] + 7).float()
    wav = base.repeat_interleave(HOP, dim=1) * torch.arange(1, HOP + 1, dtype=torch.float32).repeat(mel.shape[2])
    wav = wav[:, :HOP * (mel.shape[2] - drop)]
    return wav if lengths is None else _mask(wav, [HOP * (int(n) - drop) for n in lengths])


def _pcm(wav, normalize=False):
    pcm = torch.remainder(wav, 32749.0).to(torch.int16)
    return (pcm, wav.abs().amax(dim=1)) if normalize else pcm


def fake_pcm16_on_device(wav, **kw):
    log_call("pcm16_on_device", (wav,), kw)
    return _pcm(wav, kw.get("normalize", False))


def plain_vocode(mel, **kw):
    log_call("vocode", (mel,), kw)
    return _wave(mel, kw.get("lengths"))


class FakeConfig:
    upsample_rates, upsample_kernel_sizes = (2, 2), (4, 4)
    resblock_kernel_sizes, resblock_dilation_sizes = (3,), ((1,),)
    hop_length = HOP


class FakeEngine:
    name, cfg = "engine", FakeConfig()

    def forward(self, mel, **kw):
        log_call("engine.forward", (mel,), kw)
        return _wave(mel, kw.get("lengths"))

    def forward_pcm16(self, mel, **kw):
        log_call("engine.forward_pcm16", (mel,), kw)
        return _pcm(_wave(mel, kw.get("lengths")), kw.get("normalize", False))

    def forward_resampled(self, mel, resampler, **kw):
        log_call("engine.forward_resampled", (mel, resampler), kw)
        wav = _wave(mel, kw.get("lengths"))[:, ::2] * 64
        return _pcm(wav, kw.get("normalize", False)) if kw.get("pcm16") else wav


class FakeWhole:
    """A whole-utterance vocoder: ``HOP * (T - 1)`` samples, an item of one frame refused."""
    whole_utterance, hop_length, name = True, HOP, "whole"

    def __init__(self, ragged: bool):
        self.takes_lengths = ragged

    def forward_device(self, mel, **kw):
        log_call("whole.forward_device", (mel,), kw)
        if min([mel.shape[2]] if kw.get("lengths") is None else [int(n) for n in kw["lengths"]]) < 2:
            raise ValueError("whole: an item needs at least two frames")
        return _wave(mel, kw.get("lengths"), drop=1)


class FakePostNet:
    name, receptive_field_frames = "postnet", 1

    def forward_device(self, mel, **kw):
        log_call("postnet.forward_device", (mel,), kw)
        return mel


# ---- wave stages ------------------------------------------------------------------------------------------------------------
class FakeSession:
    """``push`` / ``flush`` of a chunked stage: ``fn`` on what arrived, the last ``halo`` samples held back until more arrive."""

    def __init__(self, name, fn, halo):
        self.name, self.fn, self.halo, self.buf = name, fn, halo, None

    def push(self, piece):
        log_call(f"{self.name}.session.push", (piece,), {})
        piece = self.fn(piece)
        self.buf = piece if self.buf is None else torch.cat([self.buf, piece], dim=1)
        out, self.buf = self.buf[:, :max(self.buf.shape[1] - self.halo, 0)], self.buf[:, max(self.buf.shape[1] - self.halo, 0):]
        return out

    def flush(self):
        log_call(f"{self.name}.session.flush", (), {})
        out, self.buf = (torch.zeros((1, 0)) if self.buf is None else self.buf), None
        return out


class FakeDenoiser:
    name = "denoiser"

    def forward_device(self, wav, **kw):
        log_call("denoiser.forward_device", (wav,), kw)
        return wav * 2


class FakeChunkedDenoiser(FakeDenoiser):
    chunked_sessions = True

    def open_session(self):
        log_call("denoiser.open_session", (), {})
        return FakeSession("denoiser", lambda w: w * 2, 3)


class FakeStretch:
    """Rate 2 at a hop of 8: every second sample, so ``out_samples(L) = L // 2``; ``counts`` is a device tensor."""
    name, hop_length = "stretch", 8

    def out_samples(self, L):
        return int(L) // 2

    def forward_device(self, wav, **kw):
        log_call("stretch.forward_device", (wav,), kw)
        out = wav[:, ::2] * 4
        counts = [out.shape[1]] * wav.shape[0] if kw.get("lengths") is None else [int(n) * 4 for n in kw["lengths"]]
        return _mask(out, counts), torch.tensor(counts, dtype=torch.int32)


class FakeChunkedStretch(FakeStretch):
    chunked_sessions = True

    def open_session(self):
        log_call("stretch.open_session", (), {})
        return FakeSession("stretch", lambda w: w * 4, 5)          # a session of its own arithmetic: the length is kept


class FakeLoudness:
    name = "loudness"

    def normalize_device(self, wav, **kw):
        log_call("loudness.normalize_device", (wav,), kw)
        return wav * 8, torch.zeros((wav.shape[0], 2))


class FakeLimiter:
    name = "limiter"

    def limit_device(self, wav, **kw):
        log_call("limiter.limit_device", (wav,), kw)
        return wav * 16, torch.zeros((wav.shape[0], 2))


class FakeChunkedLimiter(FakeLimiter):
    chunked_sessions = True

    def __init__(self, pcm16=False):
        self.pcm16 = pcm16

    def open_session(self):
        log_call("limiter.open_session", (), {})
        return FakeSession("limiter", (lambda w: _pcm(w * 16)) if self.pcm16 else (lambda w: w * 16), 2)


class FakeAssembler:
    """The items laid end to end (nothing trimmed): ``out [B * L]``, ``offsets [B + 1]``, ``spans [B, 2]``, all "on the device"."""
    name = "assemble"

    def join_device(self, wav, **kw):
        log_call("assemble.join_device", (wav,), kw)
        counts = _owned(kw.get("lengths"), kw.get("row_scale", 1), *wav.shape)
        out = torch.zeros(wav.numel(), dtype=wav.dtype)
        offsets = [0]
        for i, n in enumerate(counts):
            out[offsets[-1]:offsets[-1] + n] = wav[i, :n] * 32
            offsets.append(offsets[-1] + n)
        spans = torch.tensor([[0, n] for n in counts], dtype=torch.int32)
        return out, torch.tensor(offsets, dtype=torch.int32), spans


class FakeResampler:
    """Half the rate: global output n is input 2n and reads no other, so ``half_width`` is 0."""
    name, half_width, rate_out = "resampler", 0, 11025

    def out_range(self, origin, L):
        lo = -(-int(origin) // 2)
        return lo, -(-(int(origin) + int(L)) // 2) - lo

    def forward(self, wav, **kw):
        log_call(f"{self.name}.forward", (wav,), kw)
        wav = wav[:, ::2] * 64
        return _pcm(wav, kw.get("normalize", False)) if kw.get("pcm16") else wav


class FakeOutput(FakeResampler):
    """``output=``: a chunked resampler with its encoding (fp32 here)."""
    name, chunked_sessions = "output", True

    def open_session(self):
        log_call("output.open_session", (), {})
        return _OutputSession()


class _OutputSession:
    def __init__(self):
        self.base, self.buf = 0, None                              # ``buf`` holds the inputs from global index ``base`` on

    def _emit(self, final):
        stop = self.base + self.buf.shape[1] - (0 if final else min(2, self.buf.shape[1]))
        first = -(-self.base // 2) * 2
        out = self.buf[:, first - self.base:stop - self.base:2] * 64 if first < stop else self.buf[:, :0]
        self.buf, self.base = self.buf[:, stop - self.base:], stop
        return out

    def push(self, piece):
        log_call("output.session.push", (piece,), {})
        self.buf = piece if self.buf is None else torch.cat([self.buf, piece], dim=1)
        return self._emit(False)

    def flush(self):
        log_call("output.session.flush", (), {})
        return torch.zeros((1, 0)) if self.buf is None else self._emit(True)


# ---- the matrix -------------------------------------------------------------------------------------------------------------
STAGES = ("denoiser", "stretch", "loudness", "limiter", "assemble", "output")
PLAIN = {"denoiser": FakeDenoiser, "stretch": FakeStretch, "loudness": FakeLoudness, "limiter": FakeLimiter,
         "assemble": FakeAssembler, "output": FakeOutput}
CHUNKED = {"denoiser": FakeChunkedDenoiser, "stretch": FakeChunkedStretch, "limiter": FakeChunkedLimiter,
           "limiter16": lambda: FakeChunkedLimiter(pcm16=True), "output": FakeOutput}
VOCODERS = ("callable", "engine", "whole", "whole_ragged")
OUTPUT_ARGS = {"none": {}, "pcm16": {"pcm16": True}, "pcm16+normalize": {"pcm16": True, "normalize": True},
               "resampler": {"resampler": True}, "resampler+pcm16+normalize": {"resampler": True, "pcm16": True, "normalize": True},
               "normalize": {"normalize": True}}
# entry points: name -> (method, frames of the items); the first five take every output argument, the others the two ends
CALLS = {"infer_b1": ("infer", [8]), "infer_b2": ("infer", [8, 8]), "batch_8_8": ("infer_batch", [8, 8]),
         "batch_8_5": ("infer_batch", [8, 5]), "batch_8_6": ("infer_batch", [8, 6]), "infer_t1": ("infer", [1]),
         "batch_9_7": ("infer_batch", [9, 7]), "batch_8_1": ("infer_batch", [8, 1]), "stream": ("stream", [10, 10]),
         "session": ("session", [10]), "group": ("group", [])}
THIN = ("infer_t1", "batch_9_7", "batch_8_1")
NO_ARGS = ("stream", "session", "group")


def mel_of(frames: int, seed: int) -> torch.Tensor:
    """``[N_MELS, frames]`` of the integers -2 .. 2."""
    t = torch.arange(frames)
    return torch.stack([((seed * 7 + m * 3 + t * 5) % 5 - 2).float() for m in range(N_MELS)])


def build_vocoder(kind: str):
    if kind == "callable":
        return plain_vocode, {"hop_length": HOP}
    if kind in ("engine", "engine_pcm16"):
        return (FakeEngine().forward if kind == "engine" else FakeEngine().forward_pcm16), {}
    return FakeWhole(ragged=kind == "whole_ragged"), {}


def stage_sets():
    return [tuple(s for s, on in zip(STAGES, bits) if on) for bits in itertools.product((0, 1), repeat=len(STAGES))]


def main_cases():
    """``(group, case name, vocoder, {stage: fake class}, call, output arguments)`` for the main matrix."""
    for voc in VOCODERS:
        for call in CALLS:
            names = ("none",) if call in NO_ARGS else ("none", "resampler+pcm16+normalize") if call in THIN else tuple(OUTPUT_ARGS)
            for chosen in stage_sets():
                for arg in names:
                    yield f"{voc}/{call}", f"{'+'.join(chosen) or '-'}/{arg}", voc, {s: PLAIN[s] for s in chosen}, call, OUTPUT_ARGS[arg]


def chunked_cases():
    """The chunked forms: every mix of absent / plain / chunked denoiser, stretch and limiter (fp32 and ``pcm16=True``) with and
    without ``output=``, on ``forward`` and ``forward_pcm16``; ``loudness=`` or ``assemble=`` beside them for the streaming calls."""
    forms = {"denoiser": ("-", "plain", "chunked"), "stretch": ("-", "plain", "chunked"),
             "limiter": ("-", "plain", "chunked", "chunked16"), "output": ("-", "chunked")}
    for voc in ("callable", "engine", "engine_pcm16"):
        for call in ("stream", "session", "group", "infer_b1", "batch_8_6"):
            for extra in ("-", "loudness", "assemble") if call in NO_ARGS else ("-",):
                for combo in itertools.product(*forms.values()):
                    stages = {} if extra == "-" else {extra: PLAIN[extra]}
                    for stage, form in zip(forms, combo):
                        if form == "plain":
                            stages[stage] = PLAIN[stage]
                        elif form != "-":
                            stages[stage] = CHUNKED["limiter16" if form == "chunked16" else stage]
                    name = "/".join(f"{s}:{f}" for s, f in zip(forms, combo)) + f"/{extra}"
                    yield f"chunked/{voc}/{call}", name, voc, stages, call, {}


def all_cases():
    yield from main_cases()
    yield from chunked_cases()


# ---- running one case -------------------------------------------------------------------------------------------------------
def describe(result):
    if isinstance(result, torch.Tensor):
        return _tensor(result)
    if isinstance(result, (list, tuple)):
        return {"list" if isinstance(result, list) else "tuple": [describe(r) for r in result]}
    return repr(result)


@contextmanager
def patched_output_stage():
    """``synthesis_output.pcm16_on_device`` replaced by its fake for the duration: the real one needs the device."""
    import iris.synthesis_output as so
    real, so.pcm16_on_device = so.pcm16_on_device, fake_pcm16_on_device
    try:
        yield
    finally:
        so.pcm16_on_device = real


def run_case(voc: str, stages: dict, call: str, args: dict) -> dict:
    """Builds the pipeline of the case, makes the call, and returns ``{"log": [...], "outcome": ...}``."""
    from iris.pipeline import MelToWavePipeline
    del LOG[:]
    try:
        vocode, kw = build_vocoder(voc)
        pipe = MelToWavePipeline(FakePostNet(), vocode, chunk_frames=CHUNK, **kw, **{s: make() for s, make in stages.items()})
        method, frames = CALLS[call]
        args = dict(args, resampler=FakeResampler()) if args.get("resampler") else args
        if method == "infer":
            result = pipe.infer(torch.stack([mel_of(t, i) for i, t in enumerate(frames)]), **args)
        elif method == "infer_batch":
            result = pipe.infer_batch([mel_of(t, i) for i, t in enumerate(frames)], **args)
        elif method == "stream":
            result = list(pipe.stream(torch.stack([mel_of(t, i) for i, t in enumerate(frames)])))
        elif method == "session":
            session, mel = pipe.session(), mel_of(frames[0], 0)[None]
            result = [session.push(mel[:, :, :3]), session.push(mel[:, :, 3:7]), session.push(mel[:, :, 7:]), session.flush()]
        else:
            from iris.stream_group import StreamGroup
            result = type(StreamGroup(pipe, chunk_frames=CHUNK)).__name__
        outcome = describe(result)
    except Exception as exc:                                       # the refusal is the outcome
        outcome = f"{type(exc).__name__}: {exc}"
    return {"log": list(LOG), "outcome": outcome}


def run_all() -> dict:
    """``{group: [(case name, record)]}`` for the whole matrix, in matrix order."""
    out: dict = {}
    with patched_output_stage():
        for group, name, voc, stages, call, args in all_cases():
            out.setdefault(group, []).append((name, run_case(voc, stages, call, args)))
    return out


# ---- the file: distinct log lines and distinct records once, cases by index ------------------------------------------------------
def write_golden(path: Path = GOLDEN) -> None:
    lines, records, name_lists, groups = {}, {}, {}, {}
    for group, cases in run_all().items():
        names, refs = [], []
        for name, rec in cases:
            key = json.dumps([[lines.setdefault(line, len(lines)) for line in rec["log"]], rec["outcome"]])
            names.append(name)
            refs.append(records.setdefault(key, len(records)))
        groups[group] = {"names": name_lists.setdefault(json.dumps(names), len(name_lists)), "records": refs}
    with open(path, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as packed, io.TextIOWrapper(packed) as f:
        f.write('{"lines": [\n' + ",\n".join(json.dumps(line) for line in lines) + '\n],\n"records": [\n')
        f.write(",\n".join(records) + '\n],\n"name_lists": [\n' + ",\n".join(name_lists) + '\n],\n"groups": {\n')
        f.write(",\n".join(f"{json.dumps(g)}: {json.dumps(v)}" for g, v in groups.items()) + "\n}}\n")
    print(f"{path}: {sum(len(v['records']) for v in groups.values())} cases, {len(records)} distinct records, {len(lines)} distinct lines, "
          f"{path.stat().st_size} bytes")


def read_golden(path: Path = GOLDEN) -> dict:
    """``{group: [(case name, record)]}`` as ``run_all`` returns it, from the file."""
    data = json.loads(gzip.decompress(path.read_bytes()))
    records = [{"log": [data["lines"][i] for i in log], "outcome": outcome} for log, outcome in data["records"]]
    return {g: [(n, records[r]) for n, r in zip(data["name_lists"][v["names"]], v["records"], strict=True)] for g, v in data["groups"].items()}


if __name__ == "__main__":
    if sys.argv[1:] == ["--print"]:
        sys.stdout.write(gzip.decompress(GOLDEN.read_bytes()).decode())
    elif sys.argv[1:] == ["--write"]:
        write_golden()
    else:
        sys.exit("usage: python tests/pipeline_routes_cases.py --write | --print")
