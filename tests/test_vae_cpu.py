"""CPU: the host side of uwudiff_amd.vae.AutoencoderKL -- target resolution, presets, the diffusers key set and layout round
trip against tests/vae_oracle.py, parameter counts, loading, and the refusals that need no device."""
import json
import os

import pytest
import torch

from tests import vae_oracle

NODE = {"_target_": "diffusers.AutoencoderKL.from_pretrained",
        "_load_config_": {"precision": "torch.float16", "to_freeze": True},
        "pretrained_model_name_or_path": "madebyollin/sdxl-vae-fp16-fix"}
HUB_NAMES = [("madebyollin/sdxl-vae-fp16-fix", None), ("stabilityai/stable-diffusion-xl-base-1.0", "vae"), ("sdxl-vae", None)]


@pytest.fixture(scope="module")
def vae():
    from uwudiff_amd.vae import AutoencoderKL

    torch.manual_seed(3)
    return AutoencoderKL.from_pretrained("sdxl-vae")


@pytest.fixture(scope="module")
def oracle():
    torch.manual_seed(4)
    return vae_oracle.AutoencoderKL().eval()


def test_target_resolves():
    from uwudiff_amd.config import get_obj_from_str
    from uwudiff_amd.vae import AutoencoderKL

    fn = get_obj_from_str("diffusers.AutoencoderKL.from_pretrained")
    assert fn.__self__ is AutoencoderKL and fn.__func__ is AutoencoderKL.from_pretrained.__func__
    assert get_obj_from_str("diffusers.AutoencoderKL") is AutoencoderKL


@pytest.mark.parametrize("name,subfolder", HUB_NAMES)
def test_hub_names_build_the_sdxl_preset(name, subfolder):
    from uwudiff_amd.vae import AutoencoderKL

    m = AutoencoderKL.from_pretrained(name, subfolder=subfolder, init_weights=False)
    c = m.config
    assert (c.in_channels, c.out_channels, c.latent_channels) == (3, 3, 4)
    assert tuple(c.block_out_channels) == (128, 256, 512, 512) and c.layers_per_block == 2 and c.norm_num_groups == 32
    assert c.act_fn == "silu" and c.mid_block_add_attention is True
    assert c.scaling_factor == 0.13025 and c["scaling_factor"] == 0.13025
    assert m.compute_dtype == "bf16"
    assert sum(v.numel() for _, v in m.named_tensors()) == 83_653_863


def test_unknown_name_is_a_value_error():
    from uwudiff_amd.vae import AutoencoderKL

    with pytest.raises(ValueError, match="sdxl-vae"):
        AutoencoderKL.from_pretrained("nobody/no-such-vae")
    with pytest.raises(ValueError):
        AutoencoderKL.from_pretrained("sdxl-vae", compute_dtype="fp16")


def test_dict_is_a_config():
    from uwudiff_amd.vae import AutoencoderKL

    m = AutoencoderKL.from_pretrained({"block_out_channels": [32, 64], "layers_per_block": 1, "mid_block_add_attention": False},
                                      compute_dtype="fp32")
    o = vae_oracle.AutoencoderKL(block_out_channels=(32, 64), layers_per_block=1, mid_block_add_attention=False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in o.state_dict().items()}
    assert m.compute_dtype == "fp32" and m.config.scaling_factor == 0.13025


def test_state_dict_is_the_diffusers_key_set(vae, oracle):
    got = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in oracle.state_dict().items()}
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert got["encoder.down_blocks.0.downsamplers.0.conv.weight"] == (128, 128, 3, 3)
    assert got["encoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert got["quant_conv.weight"] == (8, 8, 1, 1) and got["decoder.conv_out.weight"] == (3, 128, 3, 3)


def test_parameter_count_and_split(vae, oracle):
    sd = vae.state_dict()
    count = lambda p: sum(v.numel() for k, v in sd.items() if k.startswith(p))  # noqa: E731
    assert sum(v.numel() for v in sd.values()) == 83_653_863
    assert (count("encoder."), count("decoder."), count("quant_conv."), count("post_quant_conv.")) == (34_163_592, 49_490_179, 72, 20)
    assert sum(p.numel() for p in oracle.parameters()) == 83_653_863


def test_load_state_dict_round_trip_is_bit_exact(vae, oracle):
    ref = oracle.state_dict()
    vae.load_state_dict(ref)
    got = vae.state_dict()
    for k, v in ref.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k], v), k
    # the stored layout: [Cout][3][3][C] for 3x3 convolutions, channels padded to 8 with zeros
    w = vae.P.base32("encoder.down_blocks.1.resnets.0.conv1.weight")
    assert tuple(w.shape) == (256, 9 * 128)
    assert torch.equal(w.view(256, 3, 3, 128), ref["encoder.down_blocks.1.resnets.0.conv1.weight"].permute(0, 2, 3, 1))
    w = vae.P.base32("encoder.conv_in.weight").view(128, 3, 3, 8)
    assert torch.equal(w[..., :3], ref["encoder.conv_in.weight"].permute(0, 2, 3, 1)) and not w[..., 3:].any()
    w = vae.P.base32("decoder.conv_out.weight").view(8, 3, 3, 128)
    assert not w[3:].any() and not vae.P.base32("decoder.conv_out.bias")[3:].any()
    w = vae.P.base32("post_quant_conv.weight")
    assert tuple(w.shape) == (8, 8) and torch.equal(w[:4, :4], ref["post_quant_conv.weight"][:, :, 0, 0]) and not w[4:].any()


def test_load_state_dict_refuses_missing_keys_and_wrong_shapes(vae, oracle):
    ref = oracle.state_dict()
    before = vae.state_dict()
    bad = dict(ref)
    del bad["decoder.up_blocks.2.upsamplers.0.conv.bias"]
    with pytest.raises(RuntimeError, match="upsamplers.0.conv.bias"):
        vae.load_state_dict(bad)
    bad = dict(ref)
    bad["encoder.conv_in.weight"] = torch.zeros(128, 4, 3, 3)
    with pytest.raises(RuntimeError, match="encoder.conv_in.weight"):
        vae.load_state_dict(bad)
    bad = dict(ref)
    bad["encoder.mid_block.attentions.0.query.weight"] = torch.zeros(512, 512)
    with pytest.raises(RuntimeError, match="query"):
        vae.load_state_dict(bad)
    after = vae.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)  # a refused load writes nothing


def test_every_parameter_is_frozen(vae):
    ps = list(vae.parameters())
    assert len(ps) == 1 and ps[0] is vae.flat and ps[0].dtype == torch.float32
    assert not any(p.requires_grad for p in ps) and not vae.training
    assert vae._uwu_keep_fp32_master is True


def test_load_any_keeps_the_fp32_master():
    from duwu.loader import load_any
    from uwudiff_amd.vae import AutoencoderKL

    m = load_any(dict(NODE))
    assert isinstance(m, AutoencoderKL)
    assert m.flat.dtype == torch.float32 and not m.flat.requires_grad and not m.training
    assert m.config.scaling_factor == 0.13025 and m.config.latent_channels == 4
    assert bool(m.flat.abs().sum() > 0)  # seeded default initialisation, not zeros


def test_seeded_initialisation_is_reproducible():
    from uwudiff_amd.vae import AutoencoderKL

    small = {"block_out_channels": [32, 64], "layers_per_block": 1, "mid_block_add_attention": False}
    torch.manual_seed(11)
    a = AutoencoderKL(small).state_dict()
    torch.manual_seed(11)
    b = AutoencoderKL(small).state_dict()
    torch.manual_seed(12)
    c = AutoencoderKL(small).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["encoder.conv_in.weight"], c["encoder.conv_in.weight"])
    w = a["encoder.down_blocks.1.resnets.0.conv1.weight"]  # Conv2d default: U(+-1/sqrt(fan_in)), fan_in = 9 * 32
    assert float(w.abs().max()) <= (9 * 32) ** -0.5 and float(w.abs().max()) > 0.9 * (9 * 32) ** -0.5
    assert torch.equal(a["encoder.conv_norm_out.weight"], torch.ones(64)) and not a["encoder.conv_norm_out.bias"].any()


def test_local_directory_loads(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from uwudiff_amd.vae import AutoencoderKL
    from uwudiff_amd.flat import FlatModule

    calls, inner = [], FlatModule._from_local_dir.__func__  # every local directory goes through the one loader in flat.py
    monkeypatch.setattr(FlatModule, "_from_local_dir", classmethod(lambda c, *a, **kw: calls.append(c) or inner(c, *a, **kw)))

    cfg = {"_class_name": "AutoencoderKL", "_diffusers_version": "0.0", "in_channels": 3, "out_channels": 3, "latent_channels": 4,
           "block_out_channels": [32, 64], "layers_per_block": 1, "norm_num_groups": 32, "act_fn": "silu",
           "mid_block_add_attention": False, "scaling_factor": 0.5, "force_upcast": False}
    torch.manual_seed(5)
    o = vae_oracle.AutoencoderKL(block_out_channels=(32, 64), layers_per_block=1, mid_block_add_attention=False)
    d = tmp_path / "repo" / "vae"
    os.makedirs(d)
    (d / "config.json").write_text(json.dumps(cfg))
    sd = {k: v.detach().half().contiguous() for k, v in o.state_dict().items()}
    save_file(sd, str(d / "diffusion_pytorch_model.safetensors"))
    for m in (AutoencoderKL.from_pretrained(str(d)), AutoencoderKL.from_pretrained(str(tmp_path / "repo"), subfolder="vae")):
        assert m.config.scaling_factor == 0.5 and tuple(m.config.block_out_channels) == (32, 64)
        got = m.state_dict()
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k].float()) for k in sd)
        assert "force_upcast" not in m.config and "_class_name" not in m.config
    assert calls == [AutoencoderKL] * 2
    assert AutoencoderKL.from_pretrained(str(d), config={"scaling_factor": 0.25}).config.scaling_factor == 0.25  # as the text models
    with pytest.raises(ValueError):
        AutoencoderKL.from_pretrained(str(tmp_path / "repo"))  # a directory without config.json is not a known name


def test_shape_and_device_refusals(vae):
    from uwudiff_amd.lib import UwuError

    for shape in ((1, 3, 60, 64), (1, 3, 64, 68)):
        with pytest.raises(ValueError, match="multiples of 8"):
            vae.encode(torch.zeros(shape))
    with pytest.raises(UwuError, match="no CPU fallback"):
        vae.encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(UwuError, match="no CPU fallback"):
        vae.decode(torch.zeros(1, 4, 8, 8))


def test_pixel_config_names_the_vae():
    from uwudiff_amd.config import load_yaml
    from tests.conftest import ROOT

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_pixels.yaml"))
    assert list(cfg.data.dataset_config.sample_size) == [3, 256, 256] and cfg.data.dataloader_config.batch_size == 16
    node = cfg.trainer.model_config.vae
    assert node["_target_"] == "diffusers.AutoencoderKL.from_pretrained"
    assert node["pretrained_model_name_or_path"] == "madebyollin/sdxl-vae-fp16-fix"
    assert dict(node["_load_config_"]) == {"precision": "torch.float16", "to_freeze": True}
    assert cfg.trainer.model_config.unet["config"] == "stabilityai/stable-diffusion-xl-base-1.0"
