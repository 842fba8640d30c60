"""The Stable Diffusion 1.x family end to end through its shipped config files, cut down to the small four-level UNet of
tests/test_sd15_unet_gpu.py (head widths 40 / 80 / 160), a two-layer CLIP ViT-L/14-width text encoder and a small VAE: the
classes, names and settings are the YAML's."""
import os

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

UNET = dict(block_out_channels=[40, 80, 160, 160], layers_per_block=1, attention_head_dim=1, transformer_layers_per_block=1,
            norm_num_groups=8)  # the rest (block types, context 768, no pooled conditioning, 1x1-conv projections): the preset's
TEXT = dict(num_hidden_layers=2)
VAE = dict(block_out_channels=[32, 32, 64, 64], layers_per_block=1, mid_block_add_attention=False, scaling_factor=0.18215)


@pytest.fixture(scope="module")
def sd_stack():
    from duwu.loader import load_any
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import seed_everything

    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "sampling", "demo_sampling_sd.yaml")),
                {"sampling_func": {"prompt": ["a cat sitting on a table", "dogs with pumpkins"], "neg_prompt": ["", "blurry"],
                                   "num_samples": 2, "num_steps": 2, "width": 64, "height": 64},
                 "model_config": {"unet": {"config": UNET}, "vae": {"pretrained_model_name_or_path": VAE}}})
    cfg.model_config.te.text_model_and_configs[0][0]["config"] = TEXT
    seed_everything(cfg.sampling_func.seed)
    models = {name: load_any(cfg.model_config[name]) for name in ("unet", "te", "vae")}
    # the seeded initial weights leave every residual branch's output near zero (eps ~ 1e-5: guidance could not show in 8-bit
    # images); give every branch signal, as the oracle comparisons do
    g = torch.Generator().manual_seed(3)
    sd = models["unet"].state_dict()
    for n, v in sd.items():
        if v.dim() > 1:
            sd[n] = (torch.randn(v.shape, generator=g) * (0.5 / v[0].numel() ** 0.5)).to(v.device)
    models["unet"].load_state_dict(sd)
    return cfg, models


def _sample(sd_stack, **kw):
    from duwu.utils import instantiate_any

    cfg, models = sd_stack
    return instantiate_any(cfg.sampling_func)(**models, **kw)


def test_sd15_sampling_through_the_shipped_yaml(sd_stack):
    from uwudiff_amd.text_model import CLIPTextModel
    from uwudiff_amd.unet import UNet2DConditionModel

    cfg, models = sd_stack
    unet, te, vae = models["unet"], models["te"], models["vae"]
    assert type(unet) is UNet2DConditionModel and len(unet.plan_down) == 4 and unet.cfg.addition_embed_type is None
    assert not unet.cfg_dict["use_linear_projection"] and unet.cfg.cross_attention_dim == 768
    assert [type(m) for m in te.text_models] == [CLIPTextModel] and te.use_normed_ctx
    assert vae.config.scaling_factor == 0.18215
    seen = []
    hook = unet.register_forward_pre_hook(
        lambda mod, args, kwargs: seen.append((kwargs.get("added_cond_kwargs", None), tuple(kwargs["encoder_hidden_states"].shape))),
        with_kwargs=True)
    trace = {}
    images = _sample(sd_stack, trace=trace)
    hook.remove()
    assert len(images) == 2 and all(im.mode == "RGB" and im.size == (64, 64) for im in images)
    assert tuple(trace["latents"].shape) == (2, 4, 8, 8) and bool(torch.isfinite(trace["latents"]).all())
    # no pooled vector: the UNet is called without added conditioning, on [prompt rows, negative rows] x tokens x 768
    assert len(seen) == 2 and all(added is None and (shape[0], shape[2]) == (4, 768) for added, shape in seen)
    again = _sample(sd_stack)
    assert [im.tobytes() for im in again] == [im.tobytes() for im in images]
    unguided = _sample(sd_stack, cfg_scale=1)
    assert [im.tobytes() for im in unguided] != [im.tobytes() for im in images]


def test_sd15_trainer_from_the_shipped_yaml():
    """two steps of DMTrainer from configs/demo_training_sd15.yaml: the denoiser's context is the text encoder's NORMED hidden
    state (te_use_normed_ctx), and nothing consumes the batch's time_ids"""
    from duwu.trainer import DMTrainer
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.text_model import CLIPTextModel
    from uwudiff_amd.unet import SD15_UNET_CONFIG

    node = load_yaml(os.path.join(ROOT, "configs", "demo_training_sd15.yaml")).trainer
    assert node["_target_"] == "duwu.trainer.DMTrainer" and node.te_use_normed_ctx is True
    mc = node.model_config
    mc.te.text_model_and_configs[0][0]["config"] = TEXT
    mc.unet["config"] = dict(SD15_UNET_CONFIG, **UNET)
    mc.vae["pretrained_model_name_or_path"] = VAE
    torch.manual_seed(1215)
    tr = DMTrainer(mc, te_use_normed_ctx=node.te_use_normed_ctx, loss_config=node.loss_config, use_warm_up=False).cuda()
    assert [type(m) for m in tr.te.text_models] == [CLIPTextModel] and len(tr.unet.plan_down) == 4
    seen = []
    tr.unet.register_forward_pre_hook(lambda mod, args, kwargs: seen.append(kwargs["encoder_hidden_states"].detach().clone()),
                                      with_kwargs=True)
    opt = tr.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    captions = ["a photo of a cat", "DUMMY TEST with a few more words in it"]
    tokens = tr.te.tokenize(captions)
    batch = (torch.randn(2, 3, 128, 128).cuda(), captions, tokens, {"time_ids": torch.tensor([[1024, 1024, 0, 0, 1024, 1024.0]] * 2)}, {})
    p0 = tr.unet.flat.data.clone()
    for step in range(2):
        out = tr.training_step(batch, step)
        assert bool(torch.isfinite(out["loss"])), step
        out["loss"].backward()
        opt.step()
        opt.zero_grad()
    assert (tr.unet.flat.data - p0).abs().max().item() > 0
    with torch.no_grad():
        embedding, normed, pooled, _ = tr.te(tokens)
    assert pooled is None and len(seen) == 2
    assert tuple(seen[0].shape) == (2, 77, 768) and torch.equal(seen[0].float(), normed.float())
    assert not torch.equal(normed.float(), embedding.float())
