"""The Stable Diffusion 1.x family without a GPU: names, presets, the parameter count, the config files, the LyCORIS preset."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD_NAMES = ["CompVis/stable-diffusion-v1-4", "runwayml/stable-diffusion-v1-5", "bdsqlsz/stable-diffusion-v1-5"]


@pytest.fixture(scope="module")
def sd15():
    from uwudiff_amd.unet import UNet2DConditionModel

    return UNet2DConditionModel.from_pretrained("sd15", init_weights=False, device="meta")


@pytest.mark.parametrize("name", SD_NAMES)
def test_every_stage_resolves_the_sd1_names(name):
    from duwu.modules.unet_patch import UNet2DFromScratch
    from uwudiff_amd.scheduler import EulerDiscreteScheduler
    from uwudiff_amd.text_model import CLIPTextModel
    from uwudiff_amd.unet import SD15_UNET_CONFIG, UNet2DConditionModel
    from uwudiff_amd.vae import PRESETS

    assert UNet2DConditionModel._preset(name) is SD15_UNET_CONFIG
    for unet in (UNet2DConditionModel.from_pretrained(name, subfolder="unet", init_weights=False, device="meta"),
                 UNet2DConditionModel.from_config(name, subfolder="unet", init_weights=False, device="meta"),
                 UNet2DFromScratch.from_config(name, subfolder="unet", init_weights=False, device="meta")):
        assert tuple(unet.cfg.block_out_channels) == (320, 640, 1280, 1280) and unet.cfg.cross_attention_dim == 768
        assert unet.config.sample_size == 64 and unet.cfg.addition_embed_type is None
    sched = EulerDiscreteScheduler.from_pretrained(name, subfolder="scheduler")
    assert sched.config.prediction_type == "epsilon" and sched.config.beta_schedule == "scaled_linear"
    assert PRESETS[name]["scaling_factor"] == 0.18215 and PRESETS[name]["sample_size"] == 512
    te = CLIPTextModel.from_pretrained(name, subfolder="text_encoder", device="meta")  # CLIP ViT-L/14
    assert (te.config["hidden_size"], te.config["num_hidden_layers"], te.config["num_attention_heads"]) == (768, 12, 12)


def test_sd_vae_preset():
    from uwudiff_amd.vae import PRESETS, SDXL_VAE_CONFIG

    sd = PRESETS["sd-vae"]
    assert sd["scaling_factor"] == 0.18215 and sd["sample_size"] == 512
    assert {k: v for k, v in sd.items() if k not in ("scaling_factor", "sample_size")} == {
        k: v for k, v in SDXL_VAE_CONFIG.items() if k not in ("scaling_factor", "sample_size")}
    assert PRESETS["sdxl-vae"]["scaling_factor"] == 0.13025  # SDXL untouched


def test_unet_preset_parameter_count_and_layout(sd15):
    tensors = dict(sd15.named_tensors())
    assert sum(v.numel() for v in tensors.values()) == 859_520_964
    assert not any(n.startswith("add_embedding.") for n in tensors)
    # use_linear_projection=False: the Transformer2D projections are 1x1 convolutions in the checkpoint layout
    assert tuple(tensors["down_blocks.0.attentions.0.proj_in.weight"].shape) == (320, 320, 1, 1)
    assert tuple(tensors["mid_block.attentions.0.proj_out.weight"].shape) == (1280, 1280, 1, 1)
    assert tuple(tensors["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"].shape) == (320, 768)
    # 8 heads at every level: head widths 40, 80, 160
    assert [b["ch"] // b["heads"] for b in sd15.plan_down[:3]] == [40, 80, 160] and sd15.mid_heads == 8
    assert "down_blocks.3.attentions.0.proj_in.weight" not in tensors and "up_blocks.0.attentions.0.proj_in.weight" not in tensors


def test_int_and_tuple_config_forms_are_the_same_model(sd15):
    from uwudiff_amd.unet import SD15_UNET_CONFIG, UNet2DConditionModel

    tup = UNet2DConditionModel(dict(SD15_UNET_CONFIG, attention_head_dim=(8, 8, 8, 8), transformer_layers_per_block=(1, 1, 1, 1)),
                               init_weights=False, device="meta")
    assert tup.P.registry == sd15.P.registry
    assert tup._t2d_heads == sd15._t2d_heads and set(tup._t2d_heads.values()) == {8}


def test_linear_projection_layouts():
    from uwudiff_amd.unet import UNet2DConditionModel

    cfg = dict(block_out_channels=(40, 80), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), attention_head_dim=1, transformer_layers_per_block=1,
               layers_per_block=1, cross_attention_dim=24, norm_num_groups=8, addition_embed_type=None)
    conv = UNet2DConditionModel(dict(cfg, use_linear_projection=False), compute_dtype="fp32")
    lin = UNet2DConditionModel(dict(cfg), compute_dtype="fp32")  # the default stays True
    name = "down_blocks.0.attentions.0.proj_in.weight"
    sd_conv, sd_lin = conv.state_dict(), lin.state_dict()
    assert tuple(sd_conv[name].shape) == (40, 40, 1, 1) and tuple(sd_lin[name].shape) == (40, 40)
    assert all(v.dim() == 2 for n, v in sd_lin.items() if ".proj_in." in n and n.endswith("weight"))
    lin.load_state_dict({n: v.reshape(v.shape[:2]) if ".proj_" in n and v.dim() == 4 else v for n, v in sd_conv.items()})
    assert torch.equal(lin.state_dict()[name], sd_conv[name][:, :, 0, 0])
    conv.load_state_dict(sd_conv)
    with pytest.raises(RuntimeError, match="size mismatch"):
        conv.load_state_dict(sd_lin)
    with pytest.raises(RuntimeError, match="size mismatch"):
        lin.load_state_dict(sd_conv)


@pytest.mark.parametrize("path", ["configs/model/pretrained_sd.yaml", "configs/sampling/demo_sampling_sd.yaml",
                                  "configs/demo_training_sd15.yaml"])
def test_config_files_load_and_their_targets_resolve(path):
    from uwudiff_amd.config import get_obj_from_str, load_yaml

    cfg = load_yaml(os.path.join(ROOT, path))
    targets = []

    def walk(x):
        if isinstance(x, dict):
            if "_target_" in x:
                targets.append(x["_target_"])
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)

    walk(cfg)
    assert len(targets) >= 5
    for t in targets:
        assert callable(get_obj_from_str(t)), t
    mc = cfg["trainer"]["model_config"] if "trainer" in cfg else cfg["model_config"]
    te = mc["te"]
    assert te["use_normed_ctx"] is True and te["zero_for_padding"] is False and len(te["text_model_and_configs"]) == 1
    extra = te["text_model_and_configs"][0][1]
    assert (extra["use_pooled"], extra["concat_bucket"], extra["layer_idx"]) == (False, 0, -1)
    if "trainer" in cfg:
        assert cfg["trainer"]["te_use_normed_ctx"] is True
    if "sampling_func" in cfg:
        sf = cfg["sampling_func"]
        assert (sf["width"], sf["height"], sf["num_samples"], sf["num_steps"], sf["cfg_scale"]) == (512, 512, 8, 24, 7)
        assert sf["internal_sampling_func"]["_target_"].endswith("sample_euler_ancestral")
        assert sf["internal_sampling_func"]["eta"] == 0.0
    if path.endswith("pretrained_sd.yaml"):
        assert set(mc) == {"scheduler", "unet", "te", "vae"}


def test_lycoris_preset_adapts_the_sd15_projections(sd15):
    from uwudiff_amd import adapters as A

    specs = {s.name: s for s in A.match_layers(sd15, os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml"))}
    s = specs["down_blocks.0.attentions.0.proj_in"]
    assert s.algo == "lora" and dict(s.tensors)["lora_down.weight"] == (4, 320)
    assert sorted(specs) == sorted(n for n in sd15.module_kinds if ".attentions." in n)
