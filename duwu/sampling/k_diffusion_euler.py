"""reference src/duwu/sampling/k_diffusion_euler.py with its call signatures; the loops run fused on the HIP kernels
(uwudiff_amd/sampling.py: guided_euler_ancestral) and therefore take the model object of ``cfg_wrapper`` / ``cond_text_wrapper``."""
from uwudiff_amd.sampling import GuidedModel, guided_euler_ancestral


def _check(model, image_to_noise, name):
    if image_to_noise:
        raise NotImplementedError(f"{name}(image_to_noise=True): the inversion of euler_latent.py is not built")
    if not isinstance(model, GuidedModel):
        raise TypeError(f"{name} runs the fused sampling loop and needs the model returned by duwu.sampling.cfg.cfg_wrapper or "
                        f"duwu.sampling.cfg.cond_text_wrapper, got {type(model).__name__}")


def sample_euler_ancestral(model, x, sigmas, extra_args=None, callback=None, disable=None, eta=1.0, s_noise=1.0,
                           noise_sampler=None, image_to_noise: bool = False):
    """Ancestral sampling with Euler steps (k_diffusion_euler.py:8-48).  ``disable`` (the progress bar's switch) is accepted and unused."""
    _check(model, image_to_noise, "sample_euler_ancestral")
    return guided_euler_ancestral(model, x, sigmas, extra_args, callback, eta, s_noise, noise_sampler)


def sample_euler_ancestral_cfgpp(model, x, sigmas, extra_args=None, callback=None, disable=None, eta=1.0, s_noise=1.0,
                                 noise_sampler=None, image_to_noise: bool = False):
    """The same with CFG++, https://arxiv.org/abs/2406.08070 (k_diffusion_euler.py:51-106)."""
    _check(model, image_to_noise, "sample_euler_ancestral_cfgpp")
    return guided_euler_ancestral(model, x, sigmas, extra_args, callback, eta, s_noise, noise_sampler, cfgpp=True)
