"""The configurations, shapes and seeded inputs shared by tests/test_vae.py and tests/test_gpu_vae.py."""
from __future__ import annotations

import numpy as np

DEFAULT = dict(n_mels=80, cond_dim=256)
# channels that are not multiples of 32, a dilation cycle that wraps to 1 at block 4, one down/up stage, an odd coupling count
SMALL = dict(n_mels=20, cond_dim=24, model_channels=48, latent_dim=4, decoder_blocks=5, wavenet_kernel_size=3, down_stages=1,
             flow_layers=3, flow_hidden=12)
CONFIGS = {"default": DEFAULT, "small": SMALL}
# (config, B, T): T' = 1 (all taps but one are padding); T' = 9 (the dilation-8 taps land inside the item); T' = 33 and 66
# cross a 32-row MFMA tile with a batch offset; T' = 65 crosses two tiles
CASES = [("default", 1, 4), ("default", 2, 8), ("default", 1, 36), ("default", 3, 132), ("default", 1, 260),
         ("small", 3, 6), ("small", 2, 70)]
WEIGHT_SEED = {"default": 101, "small": 202}


def make_vae(name: str):
    """A TextConditionedVAE of config `name` with EVERY parameter randomised (vae_restatement.randomise)."""
    from iris.vae import TextConditionedVAE
    from vae_restatement import randomise
    vae = TextConditionedVAE(**CONFIGS[name], seed=1)
    randomise(vae, WEIGHT_SEED[name])
    return vae


def make_inputs(vae, B: int, T: int):
    rng = np.random.default_rng(1000 * B + T)
    cond = rng.standard_normal((B, T, vae.cond_dim)).astype(np.float32)
    z = rng.standard_normal((B, T // vae.downsample_factor, vae.latent_dim)).astype(np.float32)
    return cond, z
