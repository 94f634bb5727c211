"""Every route through ``MelToWavePipeline`` against a recorded trace (``tests/golden/pipeline_routes.json.gz``): for every set of
wave stages, vocoder kind, entry point and output argument, the calls each stage receives -- their order, the shapes, dtypes
and sums of the tensors, ``lengths`` as a host list or a device tensor, ``row_scale``, and which keywords were passed at all --
and what comes back, or the refusal word for word.  ``tests/pipeline_routes_cases.py`` has the fakes and the matrix; the file
was recorded once, from the pipeline before its routes became one chain, and is only ever read here.  CPU only."""
import pytest
import torch

import pipeline_routes_cases as routes

_state = {}


def _golden():
    if "golden" not in _state:
        _state["golden"] = routes.read_golden()
    return _state["golden"]


def _cases():
    if "cases" not in _state:
        _state["cases"] = {}
        for group, *case in routes.all_cases():
            _state["cases"].setdefault(group, []).append(case)
    return _state["cases"]


def _side_by_side(want: dict, got: dict) -> str:
    rows = ["    expected" + " " * 88 + "| actual"]
    for i in range(max(len(want["log"]), len(got["log"]))):
        a, b = (r["log"][i] if i < len(r["log"]) else "" for r in (want, got))
        rows.append(f"  {' ' if a == b else '!'} {a:<98}| {b}")
    return "\n".join(rows + [f"    -> {want['outcome']}", f"    -> {got['outcome']}"])


def test_the_matrix_is_the_recorded_one():
    """Same groups and the same cases in each, so no case can leave the comparison unnoticed; 64 stage sets in every group."""
    golden = _golden()
    mine = {group: [case[0] for case in cases] for group, cases in _cases().items()}
    assert list(mine) == list(golden)
    for group, names in mine.items():
        assert names == [n for n, _ in golden[group]], group
        if not group.startswith("chunked/"):
            assert len({n.split("/")[0] for n in names}) == 64, group


@pytest.mark.parametrize("group", list(_cases()))
def test_every_case_replays_its_record(group):
    want = dict(_golden()[group])
    wrong = []
    with routes.patched_output_stage():
        for name, voc, stages, call, args in _cases()[group]:
            got = routes.run_case(voc, stages, call, args)
            if got != want[name]:
                wrong.append(f"{group} :: {name}\n{_side_by_side(want[name], got)}")
    assert not wrong, f"{len(wrong)} of {len(want)} cases differ from the record; the first three:\n" + "\n\n".join(wrong[:3])


# ---- what the recorded fakes cannot show: they return whole rows, and fp32 ------------------------------------------------------
def _pipeline(vocode, **stages):
    from iris.pipeline import MelToWavePipeline
    kw = {} if getattr(vocode, "whole_utterance", False) else {"hop_length": routes.HOP}
    return MelToWavePipeline(None, vocode, chunk_frames=routes.CHUNK, **kw, **stages)


@pytest.mark.parametrize("args", [{}, {"pcm16": True}, {"pcm16": True, "normalize": True}])
def test_a_row_shorter_than_its_items_is_refused(args):
    """A vocoder whose rows are shorter than ``hop * T`` (a wrong ``hop_length``, a short output): ``infer_batch`` refuses with
    ``split_waveforms``' sentence where nothing stands behind the vocoder; it does not hand back a truncated item."""
    class Short(routes.FakeEngine):
        def forward(self, mel, **kw):
            return super().forward(mel, **kw)[:, :24]

        def forward_pcm16(self, mel, **kw):
            out = super().forward_pcm16(mel, **kw)
            return (out[0][:, :24], out[1]) if kw.get("normalize") else out[:, :24]

    with pytest.raises(ValueError, match=r"lengths must lie in \[0, 6\] for 24 samples at hop 4"):
        _pipeline(Short().forward).infer_batch([routes.mel_of(8, 0), routes.mel_of(5, 1)], **args)


def _f64(mel, **kw):
    return routes.plain_vocode(mel, **kw).double()


@pytest.mark.parametrize("stage", ["denoiser", "stretch", "loudness", "limiter", "assemble"])
def test_every_stage_is_handed_fp32(stage):
    """``.float()`` stands in front of every wave stage: a vocoder that returns float64 reaches each of them as fp32, from
    ``infer`` and from ``infer_batch``."""
    pipe = _pipeline(_f64, **{stage: routes.PLAIN[stage]()})
    for call in (lambda: pipe.infer(routes.mel_of(8, 0)[None]), lambda: pipe.infer_batch([routes.mel_of(8, 0), routes.mel_of(6, 1)])):
        del routes.LOG[:]
        call()
        assert [line.split("(")[1][:4] for line in routes.LOG if line.startswith(stage + ".")] == ["f32["], routes.LOG


def test_no_float_where_no_stage_takes_the_waveform():
    """Without a wave stage the vocoder's dtype goes through: the fused routes return it, and a whole-utterance vocoder's
    waveform reaches the stand-alone output stage as it is."""
    pipe = _pipeline(_f64)
    assert pipe.infer(routes.mel_of(8, 0)[None]).dtype == torch.float64
    assert [w.dtype for w in pipe.infer_batch([routes.mel_of(8, 0), routes.mel_of(5, 1)])] == [torch.float64] * 2

    class Whole64(routes.FakeWhole):
        def forward_device(self, mel, **kw):
            return super().forward_device(mel, **kw).double()

    for ragged in (False, True):
        del routes.LOG[:]
        _pipeline(Whole64(ragged)).infer_batch([routes.mel_of(8, 0), routes.mel_of(8, 1)], resampler=routes.FakeResampler())
        assert routes.LOG[-1].startswith("resampler.forward(f64["), routes.LOG
