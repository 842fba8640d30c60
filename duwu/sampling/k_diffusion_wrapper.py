"""reference src/duwu/sampling/k_diffusion_wrapper.py: the discrete-sigma eps denoiser (host-side table logic, uwudiff_amd/sampling.py)."""
from uwudiff_amd.sampling import DiscreteEpsDDPMDenoiser  # noqa: F401
