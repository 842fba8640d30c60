"""CPU: LyCORIS adapter configuration, factorization, layer matching over the SDXL UNet names (a UNet on the meta device:
no parameter storage), adapter shapes / parameter count / state-dict keys, and the refusals."""
import math
import os

import pytest
import torch

from tests.conftest import ROOT
from uwudiff_amd import adapters as A
from uwudiff_amd.unet import SDXL_UNET_CONFIG, TINY_UNET_CONFIG, UNet2DConditionModel

TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")
PRESET = {
    "config": {"algo": "lora", "linear_dim": 4, "linear_alpha": 1, "conv_dim": 4, "conv_alpha": 1, "use_tucker": True,
               "train_norm": True},
    "preset": {"enable_conv": False, "target_module": ["Transformer2DModel"], "target_name": [],
               "module_algo_map": {"Attention": {"algo": "lokr", "factor": 64, "full_matrix": True},
                                  "FeedForward": {"algo": "lokr", "factor": 6, "full_matrix": True}}},
}


@pytest.fixture(scope="module")
def sdxl():
    return UNet2DConditionModel(SDXL_UNET_CONFIG, init_weights=False, device="meta")


@pytest.mark.parametrize("d,f,want", [(640, 64, (10, 64)), (1280, 64, (20, 64)), (2048, 64, (32, 64)), (640, 6, (5, 128)),
                                      (1280, 6, (5, 256)), (2560, 6, (5, 512)), (5120, 6, (5, 1024)),
                                      (10240, 6, (5, 2048)), (320, -1, (16, 20)), (77, 6, (1, 77))])
def test_factorization(d, f, want):
    assert A.factorization(d, f) == want


def test_toml_and_dict_parse_alike():
    cfg_t, pre_t = A.load_config(TOML)
    cfg_d, pre_d = A.load_config(PRESET)
    assert cfg_t == cfg_d and pre_t == pre_d
    assert cfg_t["algo"] == "lora" and cfg_t["linear_dim"] == 4 and cfg_t["train_norm"] is True
    assert cfg_t["factor"] == -1 and cfg_t["full_matrix"] is False  # defaults
    assert pre_t["module_algo_map"]["Attention"] == {"algo": "lokr", "factor": 64, "full_matrix": True}


def _expected(name, shape):
    """the adapter of one UNet layer under the shipped preset, from the contract alone"""
    if len(shape) == 1:
        return "norm", [("w_norm", shape), ("b_norm", shape)]
    out, inn = shape
    leaf = name.rsplit(".", 1)[-1]
    if ".attn1." in name or ".attn2." in name:
        f = 64
    elif ".ff." in name:
        f = 6
    else:
        assert leaf in ("proj_in", "proj_out"), name
        return "lora", [("lora_down.weight", (4, inn)), ("lora_up.weight", (out, 4))]
    (ol, ok), (im, in_) = A.factorization(out, f), A.factorization(inn, f)
    return "lokr", [("lokr_w1", (ol, im)), ("lokr_w2", (ok, in_))]


def test_sdxl_preset_assignment(sdxl):
    specs = A.match_layers(sdxl, TOML)
    got = {s.name: s for s in specs}
    # every layer inside a Transformer2DModel stack, nothing outside
    t2d = [n for n in sdxl.module_kinds if ".attentions." in n]
    assert sorted(got) == sorted(t2d)
    for n, s in got.items():
        kind = sdxl.module_kinds[n]
        assert kind in ("Linear", "LayerNorm", "GroupNorm")
        algo, tensors = _expected(n, s.shape)
        assert s.algo == algo and s.tensors == tensors, (n, s)
    assert got["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"].tensors == [("lokr_w1", (10, 10)),
                                                                                         ("lokr_w2", (64, 64))]
    assert got["mid_block.attentions.0.transformer_blocks.9.attn2.to_k"].tensors == [("lokr_w1", (20, 32)),
                                                                                     ("lokr_w2", (64, 64))]
    assert got["up_blocks.0.attentions.2.transformer_blocks.3.ff.net.0.proj"].tensors == [("lokr_w1", (5, 5)),
                                                                                          ("lokr_w2", (2048, 256))]
    assert got["down_blocks.2.attentions.1.transformer_blocks.0.ff.net.2"].tensors == [("lokr_w1", (5, 5)),
                                                                                      ("lokr_w2", (256, 1024))]
    assert got["down_blocks.1.attentions.1.norm"].algo == "norm"  # the GroupNorm of the stack
    assert got["mid_block.attentions.0.transformer_blocks.0.norm3"].algo == "norm"
    assert all(s.scale == 1.0 for s in specs if s.algo == "lokr")  # full w2
    assert all(s.scale == 0.25 for s in specs if s.algo == "lora")  # alpha / dim
    # counts: 70 transformer blocks (2 + 2 + 10 + 10 + 3*2 + 3*10 ... of the SDXL shape)
    nblocks = sum(1 for n in sdxl.module_kinds if n.endswith(".attn1.to_q"))
    nstacks = sum(1 for n in sdxl.module_kinds if n.endswith(".proj_in"))
    assert (nblocks, nstacks) == (70, 11)
    assert sum(s.algo == "lokr" for s in specs) == 10 * nblocks
    assert sum(s.algo == "lora" for s in specs) == 2 * nstacks
    assert sum(s.algo == "norm" for s in specs) == 3 * nblocks + nstacks
    # total adapter parameters, computed from the contract over the registry
    total = 0
    for n in t2d:
        _, tensors = _expected(n, sdxl.P.registry[n + ".weight"][1])
        total += sum(math.prod(sh) for _, sh in tensors)
    assert sum(s.numel for s in specs) == total == 52_377_500


def test_state_dict_keys_and_zero_delta():
    unet = UNet2DConditionModel(TINY_UNET_CONFIG, init_weights=False, device="meta")
    torch.manual_seed(0)
    net = A.LycorisNetwork(unet, TOML)
    assert net.flat.device.type == "cpu" and net.flat.requires_grad
    sd = net.state_dict()
    name = "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"
    base = "lycoris_" + name.replace(".", "_")
    assert {base + ".lokr_w1", base + ".lokr_w2", base + ".alpha"} <= set(sd)
    lora = "lycoris_down_blocks_1_attentions_0_proj_in"
    assert {lora + ".lora_down.weight", lora + ".lora_up.weight", lora + ".alpha"} <= set(sd)
    nrm = "lycoris_down_blocks_1_attentions_0_transformer_blocks_0_norm1"
    assert {nrm + ".w_norm", nrm + ".b_norm"} <= set(sd) and nrm + ".alpha" not in sd
    # zero deltas at initialisation: up / w2 / norm offsets are zero, down / w1 are not
    assert float(sd[lora + ".lora_up.weight"].abs().max()) == 0 and float(sd[lora + ".lora_down.weight"].abs().max()) > 0
    assert float(sd[base + ".lokr_w2"].abs().max()) == 0 and float(sd[base + ".lokr_w1"].abs().max()) > 0
    assert float(sd[nrm + ".w_norm"].abs().max()) == 0
    bound = 1 / math.sqrt(64)  # kaiming_uniform(a = sqrt 5) over fan_in = 64
    assert float(sd[lora + ".lora_down.weight"].abs().max()) <= bound
    # round trip through the flat buffer
    sd2 = {k: torch.randn_like(v) if not k.endswith(".alpha") else v for k, v in sd.items()}
    net2 = A.LycorisNetwork(unet, TOML)
    net2.load_state_dict(sd2)
    back = net2.state_dict()
    assert all(torch.equal(back[k], sd2[k]) for k in sd2)
    with pytest.raises(RuntimeError):
        net2.load_state_dict({**sd2, "lycoris_nope.lokr_w1": torch.zeros(1)})


def test_lowrank_w2_and_module_algo_override():
    unet = UNet2DConditionModel(TINY_UNET_CONFIG, init_weights=False, device="meta")
    cfg = {"config": {"algo": "lokr", "linear_dim": 3, "linear_alpha": 6, "factor": 8},
           "preset": {"target_module": ["BasicTransformerBlock"], "module_algo_map": {"GEGLU": {"algo": "lora", "linear_dim": 2}}}}
    specs = {s.name: s for s in A.match_layers(unet, cfg)}
    q = specs["down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"]  # 128 x 128: (8, 16) x (8, 16), 3 < 16 / 2
    assert q.algo == "lokr" and q.lowrank and q.scale == 2.0
    assert q.tensors == [("lokr_w1", (8, 8)), ("lokr_w2_a", (16, 3)), ("lokr_w2_b", (3, 16))]
    g = specs["down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj"]
    assert g.algo == "lora" and g.r == 2 and g.scale == 3.0  # GEGLU's table overrides dim; alpha from config
    assert "down_blocks.1.attentions.0.proj_in" not in specs  # outside the BasicTransformerBlocks
    assert not any(s.algo == "norm" for s in specs.values())  # train_norm defaults to false
    # target_name: fnmatch patterns over module names
    cfg = {"config": {"algo": "lora"}, "preset": {"target_name": ["*.attn2.to_[kv]"]}}
    names = sorted(s.name for s in A.match_layers(unet, cfg))
    assert names and all(n.endswith((".attn2.to_k", ".attn2.to_v")) for n in names)


def test_refusals(sdxl):
    with pytest.raises(ValueError, match="bogus"):
        A.load_config({"config": {"bogus": 1}, "preset": {"target_module": ["Transformer2DModel"]}})
    with pytest.raises(ValueError, match="weird"):
        A.load_config({"config": {}, "preset": {"target_module": [], "weird": True}})
    with pytest.raises(ValueError, match="dropout"):
        A.load_config({"config": {}, "preset": {"module_algo_map": {"Attention": {"dropout": 0.1}}}})
    for algo in ("loha", "ia3", "dylora", "glora", "full", "oft", "boft"):
        with pytest.raises(NotImplementedError, match=algo):
            A.load_config({"config": {"algo": algo}, "preset": {"target_module": ["Transformer2DModel"]}})
    with pytest.raises(NotImplementedError, match="conv"):
        A.match_layers(sdxl, {"config": {}, "preset": {"target_module": ["ResnetBlock2D"], "enable_conv": True}})
    # without enable_conv a ResNet target adapts its Linears only (conv_shortcut: a 1x1 convolution seen as a Linear)
    names = {s.name for s in A.match_layers(sdxl, {"config": {}, "preset": {"target_module": ["ResnetBlock2D"]}})}
    assert "down_blocks.1.resnets.0.conv_shortcut" in names and "down_blocks.1.resnets.0.time_emb_proj" in names
    assert not any(n.endswith((".conv1", ".conv2")) for n in names)


def test_dit_refused():
    from uwudiff_amd.dit import DiT

    dit = DiT(hidden=64, depth=1, heads=1, patch=2, sample_size=8, in_channels=4, out_channels=4, cond_dim=8)
    with pytest.raises(NotImplementedError, match="UNet"):
        A.LycorisNetwork(dit, PRESET)


def test_trainer_refuses_dit_and_bad_config(tmp_path):
    from duwu.trainer.trainer import DMTrainer

    loss = {"_target_": "duwu.loss.DiffusionLoss", "scheduler": {"_target_": "uwudiff_amd.scheduler.EulerDiscreteScheduler"}}
    dit = {"unet": {"_target_": "uwudiff_amd.dit.DiT", "hidden": 64, "depth": 1, "heads": 1, "patch": 2,
                    "sample_size": 8, "in_channels": 4, "out_channels": 4, "cond_dim": 8}}
    with pytest.raises(NotImplementedError):
        DMTrainer(dit, lycoris_config=PRESET, loss_config=loss)
    unet = {"unet": {"_target_": "duwu.modules.unet_patch.UNet2DFromScratch.from_config", "config": "tiny-unet"}}
    with pytest.raises(NotImplementedError, match="loha"):
        DMTrainer(unet, lycoris_config={"config": {"algo": "loha"}, "preset": PRESET["preset"]}, loss_config=loss)


def test_trainer_builds_adapters_on_cpu(tmp_path):
    from duwu.trainer.trainer import DMTrainer

    loss = {"_target_": "duwu.loss.DiffusionLoss", "scheduler": {"_target_": "uwudiff_amd.scheduler.EulerDiscreteScheduler"}}
    unet = {"unet": {"_target_": "duwu.modules.unet_patch.UNet2DFromScratch.from_config", "config": "tiny-unet"}}
    tr = DMTrainer(unet, lycoris_config=TOML, loss_config=loss, optimizer="torch.optim.AdamW", use_warm_up=False,
                   lr_scheduler=None)
    assert not tr.unet.flat.requires_grad
    params = list(tr.lycoris_model.parameters())  # (train_params: the generator configure_optimizers consumes)
    assert len(params) == 1 and params[0] is tr.lycoris_model.flat
    sd = tr.state_dict()
    assert any(k.startswith("lycoris_model.lycoris_") for k in sd)
    assert "unet.conv_in.weight" in sd and not any(k.startswith("unet.") and "lycoris" in k for k in sd)
    assert set(tr.unet.state_dict()) == set(tr.unet.P.registry)  # the UNet's own state dict: the base weights only
    opt = tr.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    tr.lycoris_model._dirty = False
    tr.lycoris_model.flat.grad = torch.zeros_like(tr.lycoris_model.flat)
    opt.step()
    assert tr.lycoris_model._dirty  # the step hook marks the adapters for merging
    cwd = os.getcwd()
    try:
        os.chdir(tmp_path)
        tr.on_train_epoch_end()  # no trainer attached: ./lycoris_weight relative to the working directory
    finally:
        os.chdir(cwd)
    saved = torch.load(os.path.join(tmp_path, "lycoris_weight", "epoch=0.pt"), weights_only=True)
    assert set(saved) == set(tr.lycoris_model.state_dict())
