"""reference src/duwu/sampling/__init__.py (its ``gbc_sampling`` import names a module the reference does not ship: left out)."""
from .sampling import diffusion_sampling  # noqa: F401
from .k_diffusion_euler import sample_euler_ancestral, sample_euler_ancestral_cfgpp  # noqa: F401
from .k_diffusion_dpm2 import sample_dpm2, sample_dpm2_cfgpp  # noqa: F401
