"""GPU: what the four models inherit from the shared flat-parameter store (uwudiff_amd/flat.py), on the device, each at the smallest
configuration its own GPU test file builds: the bf16 shadow after a load, dtype casts that leave the forward's bits alone, and
the adapters' dirty mark."""
import os

import pytest
import torch

from tests import clip_oracle
from tests.conftest import ROOT
from tests.test_flat_params_cpu import TINY_UNET

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DIT = dict(depth=3, hidden=128, heads=2, patch=2, sample_size=16, in_channels=4, out_channels=4, cond_dim=32)
TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")


def _unet():
    from uwudiff_amd.unet import UNet2DConditionModel

    return UNet2DConditionModel(TINY_UNET, compute_dtype="bf16")


def _unet_inputs(B=2, S=8, Tk=7):
    """8 x 8 latents: every GroupNorm of the model sums a sample in ONE workgroup (at 16 x 16 the 96-channel norms take four, whose
    fp32 atomics land in any order), so two forwards on the same weights give the same bits"""
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(B, 4, S, S, generator=g), torch.randint(0, 1000, (B,), generator=g)
    ctx, pooled = torch.randn(B, Tk, TINY_UNET["cross_attention_dim"], generator=g), torch.randn(B, 16, generator=g)
    ids = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B)
    return x.cuda(), t.cuda(), ctx.cuda(), {"text_embeds": pooled.cuda(), "time_ids": ids.cuda()}


def _unet_forward(m):
    x, t, ctx, added = _unet_inputs()
    return [m(x, t, encoder_hidden_states=ctx, added_cond_kwargs=added)[0]]


def _dit():
    from uwudiff_amd.dit import DiT, DiTConfig

    return DiT(DiTConfig(compute_dtype="bf16", **DIT), init="random")


def _dit_forward(m):
    g = torch.Generator().manual_seed(2)
    x, t, c = torch.randn(3, 4, 16, 16, generator=g), torch.randint(0, 1000, (3,), generator=g), torch.randn(3, 32, generator=g)
    return [m(x.cuda(), t.cuda(), added_cond_kwargs={"text_embeds": c.cuda()})[0]]


def _vae():
    from uwudiff_amd.vae import AutoencoderKL

    return AutoencoderKL.from_pretrained("sdxl-vae", compute_dtype="bf16")


def _vae_forward(m):
    g = torch.Generator().manual_seed(3)
    x, z = torch.randn(1, 3, 32, 40, generator=g).cuda(), torch.randn(1, 4, 4, 5, generator=g).cuda()
    dist = m.encode(x).latent_dist
    return [dist.mean, dist.logvar, m.decode(z).sample]


def _clip(projection):
    from uwudiff_amd.text_model import CLIPTextModel, CLIPTextModelWithProjection

    return (CLIPTextModelWithProjection if projection else CLIPTextModel)(clip_oracle.TINY_QUICK, compute_dtype="bf16")


def _clip_forward(m):
    ids, mask = clip_oracle.tokens(clip_oracle.TINY_QUICK, [5, 40, 77], seed=11)
    first, second, hidden = m(ids.cuda(), attention_mask=mask.cuda(), output_hidden_states=True)
    return [first, second, *hidden]


MODELS = {"unet": (_unet, _unet_forward), "dit": (_dit, _dit_forward), "vae": (_vae, _vae_forward),
          "clip": (lambda: _clip(False), _clip_forward), "clip_proj": (lambda: _clip(True), _clip_forward)}


@pytest.mark.parametrize("name", list(MODELS))
def test_shadow_after_a_device_load_and_casts_that_change_nothing(name):
    build, forward = MODELS[name]
    torch.manual_seed(2)
    sd = build().state_dict()  # (host tensors)
    torch.manual_seed(1)
    m = build().cuda()
    assert m.shadow.is_cuda and m.shadow.numel() == m.P.n
    before = m.shadow.clone()
    m.load_state_dict(sd)
    torch.cuda.synchronize()
    assert m.flat.is_cuda and m.flat.dtype == torch.float32 and not torch.equal(m.shadow, before)
    assert torch.equal(m.shadow, m.flat.detach().to(BF)) and m.P.shadow is m.shadow and m.P.flat is m.flat
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())
    with torch.no_grad():
        y0 = [y.clone() for y in forward(m)]
        flat, shadow = m.flat.detach().clone(), m.shadow.clone()
        assert m.half().to(BF) is m
        assert m.flat.dtype == torch.float32 and m.shadow.dtype == BF and torch.equal(m.flat, flat) and torch.equal(m.shadow, shadow)
        assert all(b.dtype != torch.float16 for b in m.buffers())
        y1 = forward(m)
        torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(y0, y1)):
        print(f"[flat {name}] output {i}: max |before - after the casts| = {float((a.float() - b.float()).abs().max()):.3e}")
    assert len(y0) == len(y1) and all(torch.equal(a, b) for a, b in zip(y0, y1))


def test_refresh_shadow_marks_the_adapters_dirty():
    """refresh_shadow() rewrites the shadow from the base weights, wiping the merged W + dW: the adapters must be merged again
    before the next forward, which then runs on the same bits as a freshly attached network's"""
    from uwudiff_amd.adapters import LycorisNetwork

    torch.manual_seed(4)
    m = _unet().cuda().requires_grad_(False)
    net = LycorisNetwork(m, TOML).cuda()
    with torch.no_grad():
        net.flat.data.copy_(torch.randn(net.n, generator=torch.Generator().manual_seed(13)).cuda() * 0.1)
        net.apply_to(m)
        y_merged = _unet_forward(m)[0].clone()
        merged = m.shadow.clone()
        assert not net._dirty and not torch.equal(merged, m.flat.detach().to(BF))
        m.refresh_shadow()
        torch.cuda.synchronize()
        assert net._dirty and torch.equal(m.shadow, m.flat.detach().to(BF))
        y_again = _unet_forward(m)[0].clone()
        assert not net._dirty and torch.equal(m.shadow, merged)
        net.restore()
        assert m.P.ad is None and torch.equal(m.shadow, m.flat.detach().to(BF))
        y_bare = _unet_forward(m)[0].clone()
        net.apply_to(m)
        y_fresh = _unet_forward(m)[0]
        torch.cuda.synchronize()
        assert torch.equal(m.shadow, merged)
    d = lambda a, b: float((a.float() - b.float()).abs().max())  # noqa: E731
    print(f"[flat lycoris] max |after refresh - freshly attached| {d(y_again, y_fresh):.3e}, |first - freshly attached| "
          f"{d(y_merged, y_fresh):.3e}, |bare - freshly attached| {d(y_bare, y_fresh):.3e}")
    assert torch.equal(y_again, y_fresh) and torch.equal(y_merged, y_fresh) and not torch.equal(y_bare, y_fresh)
