"""The configurations, shapes and seeded inputs shared by tests/test_encoder.py and tests/test_gpu_encoder.py."""
from __future__ import annotations

import functools

import numpy as np

# the reference's (scripts/synthesize.py:94-98) with an 80-phoneme vocabulary
DEFAULT = dict(encoder=dict(vocab_size=80), head=dict(hidden_dim=256))
# channels that are not multiples of 32 (48 = 32 + 16, 80, 40), key_dim 16 (half an MFMA tile), an odd block count, a head
# whose input and hidden widths differ, three layers (the ping-pong wraps) and k = 5
SMALL = dict(encoder=dict(vocab_size=11, embed_dim=48, num_heads=3, ffn_dim=80, num_blocks=3, max_length=150),
             head=dict(hidden_dim=40, num_layers=3, kernel_size=5, in_dim=48))
CONFIGS = {"default": DEFAULT, "small": SMALL}
KEY_TILE = 32          # keys per tile of txt_attention_kernel as built (csrc/text_encoder.h, kRows)
# (config, B, P, lengths): P = 1; P = 7; 32 and 33 cross a query tile; 33 and 65 are just above one and two key tiles; the
# ragged cases hold an item of one phoneme and one of the full P, with a batch offset that is no multiple of the tile
CASES = [("small", 1, 1, None), ("small", 1, 7, None), ("small", 1, 32, None), ("small", 1, 33, None), ("small", 1, 65, None),
         ("small", 3, 40, (1, 40, 17)), ("default", 1, 7, None), ("default", 1, 33, None), ("default", 1, 65, None),
         ("default", 3, 37, (1, 37, 20)), ("default", 1, 1000, None)]
RAGGED = [c for c in CASES if c[3] is not None]
TAP_CASE = ("default", 3, 37, (1, 37, 20))
WEIGHT_SEED = {"default": 303, "small": 404}


def case_id(case) -> str:
    name, B, P, lengths = case
    return f"{name}-{B}x{P}" + ("-ragged" if lengths else "")


@functools.lru_cache(maxsize=None)
def make_models(name: str):
    """(PhonemeEncoder, DurationPredictor) of config `name` with EVERY parameter randomised (encoder_restatement.randomise)."""
    from iris.encoder import DurationPredictor, PhonemeEncoder
    from encoder_restatement import randomise
    enc = PhonemeEncoder(**CONFIGS[name]["encoder"], seed=1)
    head = DurationPredictor(**CONFIGS[name]["head"], seed=2)
    randomise(enc, WEIGHT_SEED[name])
    randomise(head, WEIGHT_SEED[name] + 1, duration_bias=1.0, duration_gain=1.0)
    return enc, head


def make_ids(name: str, B: int, P: int) -> np.ndarray:
    rng = np.random.default_rng(7000 * B + P)
    return rng.integers(0, CONFIGS[name]["encoder"]["vocab_size"], (B, P)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name: str = "float64"):
    """The restatement on one case, computed once and shared: dict(ids, enc_out, block0, pred, layer0) -- read-only.
    The duration head reads the restatement's own encoder output of the same dtype."""
    import encoder_restatement as R
    name, B, P, lengths = case
    dtype = np.dtype(dtype_name).type
    enc, head = make_models(name)
    ids = make_ids(name, B, P)
    enc_out, taps = R.encoder_forward(enc.get_config(), enc.weights, ids, lengths, dtype)
    pred, dtaps = R.duration_forward(head.get_config(), head.weights, enc_out, lengths, dtype)
    out = dict(ids=ids, enc_out=enc_out, block0=taps["block0"], pred=pred, layer0=dtaps["layer0"])
    for v in out.values():
        v.setflags(write=False)
    return out

# max |restatement(fp32) - restatement(fp64)| / max(1, max |fp64|) over CASES and the four tensors of `reference`, measured
# on the CPU (tests/test_encoder.py asserts it; the table is in tests/test_gpu_encoder.py); the GPU bar is 4 x that.
E32_WORST = 1.92e-6
BAR = 4 * E32_WORST


def e32(case) -> dict:
    a, b = reference(case, "float64"), reference(case, "float32")
    return {k: float(np.abs(b[k].astype(np.float64) - a[k]).max() / max(1.0, np.abs(a[k]).max()))
            for k in ("enc_out", "pred", "block0", "layer0")}


def valid_mask(case) -> np.ndarray:
    _, B, P, lengths = case
    return np.ones((B, P), bool) if lengths is None else np.arange(P)[None, :] < np.asarray(lengths)[:, None]


def decided(case, max_frames_per_phoneme: int = 1_000_000) -> np.ndarray:
    """Positions whose integer frame count the float64 restatement decides: ``exp(pred) - 1`` lies further than
    ``BAR * max(1, exp(pred))`` from every half-integer and from the clip edges."""
    import encoder_restatement as R
    pred = reference(case, "float64")["pred"]
    raw = R.raw_frames(pred)
    margin = BAR * np.maximum(1.0, np.exp(pred))
    to_half = np.abs(raw - (np.floor(raw) + 0.5))
    to_clip = np.minimum(np.abs(raw - 1.0), np.abs(raw - max_frames_per_phoneme))
    return valid_mask(case) & (to_half > margin) & (to_clip > margin)
