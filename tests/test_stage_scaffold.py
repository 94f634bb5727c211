"""The seven waveform stages share one base (``iris._native_model._DeviceStage``); this holds that by behaviour, without a GPU:
every stage's ``workspace_bytes`` and ``launch_count`` answer what the library's own entry point answers when called directly,
the three ragged-wave stages refuse a bad call with one text before any device work, and no stage carries a copy of what the
base owns."""
import ctypes

import numpy as np
import pytest
import torch

from iris import _native
from iris._window_session import _WindowSession
from iris.assemble import Assembler
from iris.denoiser import Denoiser, DenoiserSession
from iris.griffin_lim import GriffinLim
from iris.limiter import Limiter, LimiterSession
from iris.loudness import LoudnessNormalizer
from iris.mel import MelFrontend
from iris.resample import ResamplerSession
from iris.time_stretch import StretchSession, TimeStretch

B, HOPS = 2, 4

# (class, constructor arguments, the shape (B, n) of a tiny call given the stage, further arguments of its two queries)
STAGES = [
    (MelFrontend, {}, lambda s: (B, HOPS * s.hop_length), ()),
    (GriffinLim, {"n_iter": 3}, lambda s: (B, 4), ()),
    (Denoiser, {}, lambda s: (B, HOPS * s.hop_length), ()),
    (TimeStretch, {}, lambda s: (B, HOPS * s.hop_length), (1.25,)),
    (Assembler, {}, lambda s: (B, HOPS * s.hop_length), ()),
    (LoudnessNormalizer, {}, lambda s: (B, HOPS * 256), ()),
    (Limiter, {}, lambda s: (B, HOPS * 256), ()),
]
IDS = [cls.__name__ for cls, *_ in STAGES]
RAGGED = [(Assembler, "join_device"), (Assembler, "trim_device"), (LoudnessNormalizer, "normalize_device"),
          (LoudnessNormalizer, "measure_device"), (Limiter, "limit_device"), (Limiter, "true_peak_device")]


def _direct(stage, what, *args):
    """``iris_<abi>_<what>(config, *args, &out)`` through the bare library, with the out type its declaration names."""
    name = f"iris_{stage._abi_name}_{what}"
    out = (ctypes.c_uint64 if what.endswith("bytes") else ctypes.c_int32)()
    cfg = stage.native_config()
    status = getattr(_native.load(), name)(ctypes.byref(cfg), *args, ctypes.byref(out))
    assert status == 0, (name, status)
    return int(out.value)


@pytest.mark.parametrize("cls, kwargs, shape_of, extra", STAGES, ids=IDS)
def test_queries_answer_what_the_library_answers(cls, kwargs, shape_of, extra):
    stage = cls(**kwargs)
    shape = shape_of(stage)
    assert stage.workspace_bytes(*shape, *extra) == _direct(stage, "workspace_bytes", *shape, *extra) >= 256
    flags = (0,) if cls in (LoudnessNormalizer, Limiter) else ()            # measure_only, which these two take last
    assert stage.launch_count(*shape, *extra) == _direct(stage, "launch_count", *shape, *extra, *flags) > 0
    assert stage.launch_count(0, shape[1], *extra) == _direct(stage, "launch_count", 0, shape[1], *extra, *flags) == 0
    assert stage._handle is None and stage._workspace is None               # no query built anything


@pytest.mark.parametrize("cls, call", RAGGED, ids=[f"{c.__name__}.{m}" for c, m in RAGGED])
def test_ragged_wave_refusals_are_one_text(cls, call, monkeypatch):
    stage = cls()

    def no_device(*a, **k):
        raise AssertionError("a refused call reached the handle")
    monkeypatch.setattr(stage, "_ensure", no_device)
    wav = np.zeros((2, 64), dtype=np.float32)
    refusals = [
        (dict(wav=np.zeros(64, np.float32)), "expected a waveform [B, L] float32, got torch.float32 (64,)"),
        (dict(wav=torch.zeros((2, 64), dtype=torch.float64)), "expected a waveform [B, L] float32, got torch.float64 (2, 64)"),
        (dict(wav=wav, row_scale=0), "row_scale must be an integer >= 1, got 0"),
        (dict(wav=wav, row_scale=True), "row_scale must be an integer >= 1, got True"),
        (dict(wav=wav, lengths=[1, 2, 3]), "lengths must be 2 integers, got int64 (3,)"),
        (dict(wav=wav, lengths=[1.0, 2.0]), "lengths must be 2 integers, got float64 (2,)"),
    ]
    for kwargs, text in refusals:
        with pytest.raises(ValueError) as err:
            getattr(stage, call)(**kwargs)
        assert str(err.value) == text, (kwargs.keys(), str(err.value))


@pytest.mark.parametrize("cls", [cls for cls, *_ in STAGES], ids=IDS)
def test_no_stage_keeps_a_copy_of_the_base(cls):
    own = set(vars(cls))
    allowed = {"close"} if cls is Denoiser else set()
    assert not (own & {"_ensure", "close", "_ws_for", "_prepare", "_ws", "_query", "_window_range"}) - allowed, sorted(own)
    if cls not in (GriffinLim, Denoiser):                                   # these two hand an array to their create
        assert "_create" not in own and "_upload_blob" not in own


@pytest.mark.parametrize("cls", [DenoiserSession, StretchSession, LimiterSession, ResamplerSession], ids=lambda c: c.__name__)
def test_no_session_keeps_a_copy_of_the_base(cls):
    """The four chunked stages' sessions share ``iris._window_session._WindowSession``: the buffer, ``push`` and ``flush`` are its."""
    own = set(vars(cls))
    assert issubclass(cls, _WindowSession)
    assert not own & {"push", "flush", "samples_received", "samples_buffered", "_empty", "_advance"}, sorted(own)
    assert cls.push is _WindowSession.push and cls.flush is _WindowSession.flush
    if cls in (DenoiserSession, LimiterSession):                            # one plan form, one halo
        assert "_measure_halo" not in own and "_window" not in own
