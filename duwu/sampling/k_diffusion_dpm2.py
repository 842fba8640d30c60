"""reference src/duwu/sampling/k_diffusion_dpm2.py with its call signatures (plus an optional ``noise_sampler`` for the churn noise);
the loops run fused on the HIP kernels (uwudiff_amd/sampling.py: guided_dpm2)."""
from uwudiff_amd.sampling import guided_dpm2

from .k_diffusion_euler import _check


def sample_dpm2(model, x, sigmas, extra_args=None, disable=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                single_call: bool = False, image_to_noise: bool = False, noise_sampler=None):
    """DPM-Solver-2 (k_diffusion_dpm2.py:8-57); ``single_call`` reuses the midpoint derivative as the next step's first one."""
    _check(model, image_to_noise, "sample_dpm2")
    return guided_dpm2(model, x, sigmas, extra_args, s_churn, s_tmin, s_tmax, s_noise, single_call, noise_sampler)


def sample_dpm2_cfgpp(model, x, sigmas, extra_args=None, disable=None, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                      single_call: bool = False, image_to_noise: bool = False, noise_sampler=None):
    """DPM-Solver-2 with CFG++ (k_diffusion_dpm2.py:60-111; ``single_call`` does not work there either and is refused)."""
    _check(model, image_to_noise, "sample_dpm2_cfgpp")
    return guided_dpm2(model, x, sigmas, extra_args, s_churn, s_tmin, s_tmax, s_noise, single_call, noise_sampler, cfgpp=True)
