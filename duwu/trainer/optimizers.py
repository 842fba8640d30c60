"""reference src/duwu/trainer/optimizers.py: ``AdamWFP16`` (AdamW with both moments in fp16, no first-moment bias
correction, weight decay accumulated per tensor and applied when it crosses ``decay_threshold``), so that
``optimizer: duwu.trainer.optimizers.AdamWFP16`` in a config resolves.  The class is the fused flat-buffer one
(``uwudiff_amd.optim.FusedAdamWFP16``: one HIP launch per buffer or reduced chunk, the decay a launch per decaying tensor).

The reference module's free function ``adamw_make_step`` is not built: the update lives in the kernel
(``uwu_adamw_fp16_step`` / ``uwu_param_decay``, uwudiff_amd/csrc/optimizer.hip) and has no tensor-level entry here.
"""
from uwudiff_amd.optim import FusedAdamWFP16 as AdamWFP16  # noqa: F401
