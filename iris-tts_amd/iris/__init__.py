"""iris (MI355X build) -- the HiFiGAN vocoder path of ZECTBynmo/iris-tts, rebuilt for gfx950.

Only the vocoder hot path exists here: ``iris.vocoder`` and
``iris.hifigan_pretrained`` are drop-ins for the reference modules of the same names; the
arithmetic runs in hand-written HIP behind the C-ABI of ``include/iris_hifigan.h``.  ``iris.postnet``,
``iris.vae`` (inference half: ``generate()``) and ``iris.encoder`` (phoneme encoder, duration head, length regulator)
cover the stages in front of the vocoder; ``iris.denoiser`` (spectral bias subtraction) sits behind it, in front of the
output stage.
Put this directory's parent (``iris-tts_amd/``) on ``PYTHONPATH`` in place of the reference's
``src/``.
"""

__version__ = "0.1.0"
