"""The configurations, shapes and seeded inputs shared by tests/test_vae_posterior.py and tests/test_gpu_vae_posterior.py."""
from __future__ import annotations

import numpy as np

import vae_cases

ENC_KEYS = ("n_mels", "cond_dim", "model_channels", "latent_dim", "num_wavenet_blocks", "wavenet_kernel_size", "down_stages")
# "default": the reference constructor's defaults.  "small": vae_cases.SMALL with 5 encoder blocks -- the dilation cycle
# wraps to 1 at block 4, channels are not multiples of 32, one down stage.
CONFIGS = {"default": dict(vae_cases.DEFAULT), "small": dict(vae_cases.SMALL, num_wavenet_blocks=5)}
# (config, B, T): T = 4: every tap but one is padding; (2, 36): a partial second 32-row tile, a batch offset, the dilation-8
# taps inside the item; (3, 132): five tiles at the frame rate, 33 latent rows; (1, 260): 65 latent rows
CASES = [("default", 1, 4), ("default", 2, 36), ("default", 3, 132), ("default", 1, 260), ("small", 3, 6), ("small", 2, 70)]
WEIGHT_SEED = {"default": 303, "small": 404}


def make_pair(name: str):
    """(VAEPosteriorEncoder, TextConditionedVAE) of config `name`, EVERY parameter randomised (``latent_logvar_proj``
    included), sharing one ``downsample.blocks.*`` set: the decoder's."""
    from iris.vae import TextConditionedVAE, VAEPosteriorEncoder
    from vae_restatement import randomise
    cfg = CONFIGS[name]
    vae = TextConditionedVAE(**cfg, seed=1)
    randomise(vae, vae_cases.WEIGHT_SEED[name])
    enc = VAEPosteriorEncoder(**{k: cfg[k] for k in ENC_KEYS if k in cfg}, seed=2)
    w = randomise(enc, WEIGHT_SEED[name])
    w.update({k: v for k, v in vae.weights.items() if k.startswith("downsample.blocks.")})
    enc.set_weights_dict(w)
    return enc, vae


def full_config(enc, vae) -> dict:
    cfg = vae.get_config()
    cfg["num_wavenet_blocks"] = enc.num_wavenet_blocks
    return cfg


def make_inputs(enc, B: int, T: int):
    rng = np.random.default_rng(7000 + 1000 * B + T)
    mel = rng.standard_normal((B, enc.n_mels, T)).astype(np.float32)
    cond = rng.standard_normal((B, T, enc.cond_dim)).astype(np.float32)
    return mel, cond
