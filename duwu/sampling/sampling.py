"""reference src/duwu/sampling/sampling.py: prompts + a trained denoiser -> PIL images.  Text encoding, the sampling loop, the latent
de-normalisation, the VAE decode and the uint8 conversion all run on the device; the host draws the starting noise
(so a seed gives the reference's starting latents), owns the sigma grid and receives one uint8 copy at the end."""
from collections.abc import Callable
from typing import Literal

import torch
from PIL import Image

from duwu.sampling.cfg import cfg_wrapper
from duwu.sampling.k_diffusion_euler import sample_euler_ancestral
from duwu.sampling.k_diffusion_wrapper import DiscreteEpsDDPMDenoiser
from duwu.utils import truncate_or_pad_to_length
from uwudiff_amd import sampling as S
from uwudiff_amd.engine import seed_everything


def sampling_sigmas(train_scheduler, num_steps, sample_scheduler=None, get_sigma_func=None):
    """sampling.py:79-100: ``num_steps + 1`` descending sigmas, host fp32.  Default: the scheduler's own table (descending, with
    the final 0 appended) read at linspace(0, num_train_timesteps, num_steps + 1) -- which ends on that 0."""
    if get_sigma_func is not None:
        return torch.as_tensor(get_sigma_func(num_steps)).float()
    sched = sample_scheduler or train_scheduler  # e.g. a Laplace training schedule whose sigmas[0] is too large to start from
    return sched.sigmas[torch.linspace(0, sched.config.num_train_timesteps, num_steps + 1).long()].float()


@torch.no_grad()
def diffusion_sampling(
    unet,
    te,
    vae,
    train_scheduler,
    prompt: str | list[str] | list[list[str]],
    neg_prompt: str | list[str],
    num_steps: int = 16,
    sample_scheduler=None,
    get_sigma_func: Callable[[int], list[float]] | None = None,
    num_samples: int = 1,
    padding_mode: Literal["repeat_last", "cycling", "uniform_expansion"] = "cycling",
    cfg_scale: float = 3.0,
    seed: int = 42,
    width: int = 1024,
    height: int = 1024,
    rescale: bool = False,
    vae_std: float | None = None,
    vae_mean: float | None = None,
    internal_sampling_func: Callable | None = None,
    trace: dict | None = None,
):
    """The reference's signature and defaults.  ``trace`` (not in the reference): a dict that receives the run's intermediates --
    ``sigmas``, ``init_x``, ``latents`` (the loop's output), ``decoded`` (the VAE's images) and ``noise_draws`` (step, seed, offset)."""
    seed_everything(seed)
    sampler = internal_sampling_func or sample_euler_ancestral
    vae_std = vae_std or 1 / vae.config.scaling_factor
    vae_mean = vae_mean or 0.0

    prompt = [prompt] if isinstance(prompt, str) else list(prompt)
    neg_prompt = [neg_prompt] if isinstance(neg_prompt, str) else list(neg_prompt)
    assert len(prompt) == len(neg_prompt)
    prompt = truncate_or_pad_to_length(prompt, num_samples, padding_mode=padding_mode)
    neg_prompt = truncate_or_pad_to_length(neg_prompt, num_samples, padding_mode=padding_mode)

    device = next(unet.parameters()).device
    denoiser = DiscreteEpsDDPMDenoiser(unet, train_scheduler.alphas_cumprod, False)
    model = cfg_wrapper(prompt=prompt, neg_prompt=neg_prompt, width=width, height=height, unet=denoiser, te=te, cfg=cfg_scale)
    sigmas = sampling_sigmas(train_scheduler, num_steps, sample_scheduler, get_sigma_func)

    init_x = torch.randn(num_samples, unet.config.in_channels, height // 8, width // 8) * torch.sqrt(1 + sigmas[0] ** 2)
    latents = sampler(model, init_x.to(device), sigmas)
    finished = S.latent_finish(latents, rescale, vae_std, vae_mean)
    # one latent at a time, as the reference decodes: the decoder's activations of the whole batch never coexist
    decoded = torch.cat([vae.decode(finished[i:i + 1]).sample for i in range(num_samples)])
    pixels = S.image_u8(decoded).cpu().numpy()  # the only device-to-host copy
    if trace is not None:
        trace.update(sigmas=sigmas, init_x=init_x, latents=latents, decoded=decoded, noise_draws=list(model.noise_draws))
    return [Image.fromarray(p) for p in pixels]
