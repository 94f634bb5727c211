"""Prints the host-only launch plan (``iris_hifigan_describe_plan``: kernel names, grids, blocks, LDS bytes, workspace bytes,
passes) or the error text of a fixed list of (config, dtype, cu_count, batch, frames) cases as canonical JSON, one line per
case: two builds of the library plan the same launches exactly when their dumps are byte-identical.  Needs no GPU.
usage (from the repository root): [IRIS_HIFIGAN_LIB=<libiris_hifigan_*.so>] python tools/plan_dump.py > plans.jsonl"""
import dataclasses, json, sys
sys.path[:0] = ["iris-tts_amd", ".", "tests"]
from iris import _native
from iris._weights import GeneratorConfig
from test_planner_sweep import SWEEP_SHAPES

CONFIGS = {"v1": GeneratorConfig(),
           "small": dataclasses.replace(GeneratorConfig(), upsample_initial_channel=128, upsample_rates=(4, 4), upsample_kernel_sizes=(8, 8))}
SHAPES = list(SWEEP_SHAPES) + [(1, 1), (1, 2), (1, 7), (1, 31), (1, 64), (1, 100), (1, 1000), (1, 1600), (8, 300), (16, 1000),
                               (32, 500), (70, 1000), (3, 70000), (65536, 10)]

for name, cfg in CONFIGS.items():
    for dtype in (0, 1, 2):
        for cu in (256, 64):
            for B, T in SHAPES:
                case = {"config": name, "dtype": dtype, "cu_count": cu, "B": B, "T": T}
                try:
                    case["plan"] = _native.describe_plan(cfg, B, T, dtype, cu)
                except _native.NativeCallError as exc:
                    case["error"] = str(exc)
                print(json.dumps(case, sort_keys=True))
