"""CPU: LyCORIS convolution adapters (LoCon, Tucker, LoKr on the 3x3 convolutions) -- layer
matching over the SDXL UNet names (meta device), tensor names / public shapes / scales / parameter count, the state dict in
public shapes, the stored (tap-major) statement of dW against an independent fp64 einsum on the public tensors, the
refusals, and the Linear-only presets unchanged."""
import math
import os

import pytest
import torch

from tests.conftest import ROOT
from uwudiff_amd import adapters as A
from uwudiff_amd.unet import SDXL_UNET_CONFIG, UNet2DConditionModel

TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")
DORA = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers-dora.toml")
CONV = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers-conv.toml")
# a UNet with padded conv_in / conv_out (4 channels stored as 8) and ResNet, sampler convolutions at two widths
SMALL = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
             down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
             transformer_layers_per_block=(1, 1), attention_head_dim=(1, 1), cross_attention_dim=32,
             addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=64,
             norm_num_groups=8)
TARGETS = {"enable_conv": True, "target_module": ["ResnetBlock2D", "Downsample2D", "Upsample2D"],
           "target_name": ["conv_in", "conv_out"]}
FORMS = {
    "lora": {"config": {"algo": "lora", "conv_dim": 3, "conv_alpha": 1.5}, "preset": TARGETS},
    "tucker": {"config": {"algo": "lora", "conv_dim": 3, "conv_alpha": 1.5, "use_tucker": True}, "preset": TARGETS},
    "lokr": {"config": {"algo": "lokr", "conv_dim": 3, "conv_alpha": 1.5, "factor": 4, "full_matrix": True}, "preset": TARGETS},
    "lokr_lowrank": {"config": {"algo": "lokr", "conv_dim": 2, "conv_alpha": 3, "factor": 4}, "preset": TARGETS},
}


@pytest.fixture(scope="module")
def sdxl():
    return UNet2DConditionModel(SDXL_UNET_CONFIG, init_weights=False, device="meta")


@pytest.fixture(scope="module")
def small():
    return UNet2DConditionModel(SMALL, init_weights=False, device="meta")


def _conv_channels(unet, name):
    """(Cout, Cin) of a 3x3 convolution from the registry and the configuration alone (conv_in / conv_out: padded to 8)"""
    co, k = unet.P.registry[name + ".weight"][1]
    cout, cin = co, k // 9
    if name == "conv_in":
        cin = unet.cfg_dict["in_channels"]
    if name == "conv_out":
        cout = unet.cfg_dict["out_channels"]
    return cout, cin


def test_sdxl_conv_preset_assignment(sdxl):
    specs = A.match_layers(sdxl, CONV)
    got = {s.name: s for s in specs}
    convs = [n for n, k in sdxl.module_kinds.items() if k == "Conv2d"]
    # every 3x3 convolution of the UNet: conv1 / conv2 of every ResNet block, the samplers, conv_in, conv_out
    res = [n for n in sdxl.module_kinds if n.endswith(".time_emb_proj")]
    want = {"conv_in", "conv_out"} | {r[:-len("time_emb_proj")] + c for r in res for c in ("conv1", "conv2")}
    want |= {f"down_blocks.{i}.downsamplers.0.conv" for i in (0, 1)} | {f"up_blocks.{i}.upsamplers.0.conv" for i in (0, 1)}
    assert set(convs) == want and len(res) == 17 and len(convs) == 40
    total = 0
    for n in convs:
        s = got[n]
        cout, cin = _conv_channels(sdxl, n)
        assert s.algo == "lora" and s.tucker and s.conv is not None and s.shape == (cout, cin), n
        assert s.tensors == [("lora_down.weight", (4, cin, 1, 1)), ("lora_mid.weight", (4, 4, 3, 3)),
                             ("lora_up.weight", (cout, 4, 1, 1))], n
        assert s.dim == 4 and s.alpha == 1.0 and s.scale == 0.25 and not s.dora, n
        assert s.key == "lycoris_" + n.replace(".", "_")
        total += 4 * cin + 144 + cout * 4
    assert got["conv_in"].shape == (320, 4) and got["conv_out"].shape == (4, 320)
    assert got["down_blocks.2.resnets.0.conv1"].tensors[0] == ("lora_down.weight", (4, 640, 1, 1))
    assert got["up_blocks.0.resnets.0.conv1"].shape == (1280, 2560)
    # the Linears of a ResNet block stay Linears on linear_dim (the 1x1 conv_shortcut among them), its GroupNorms get
    # norm adapters; the transformer stacks are what the shipped preset gives
    for n, s in got.items():
        kind = sdxl.module_kinds[n]
        if kind == "Linear" and ".attentions." not in n:
            out, inn = sdxl.P.registry[n + ".weight"][1]
            assert n.endswith((".time_emb_proj", ".conv_shortcut")) and s.conv is None and not s.tucker
            assert s.tensors == [("lora_down.weight", (4, inn)), ("lora_up.weight", (out, 4))], n
            total += 4 * (inn + out)
        elif kind == "GroupNorm" and ".attentions." not in n:
            assert ".resnets." in n and s.algo == "norm"
            total += 2 * s.shape[0]
    assert "conv_norm_out" not in got  # (inside no target)
    stacks = {n: s for n, s in got.items() if ".attentions." in n}
    base = {s.name: s for s in A.match_layers(sdxl, TOML)}
    assert set(stacks) == set(base) and all(stacks[n].tensors == base[n].tensors for n in base)
    total += 52_377_500  # tests/test_lycoris_cpu.py: the shipped preset
    assert sum(s.numel for s in specs) == total == 52_952_892
    # registry order: conv_in first, conv_out last
    assert specs[0].name == "conv_in" and specs[-1].name == "conv_out"


@pytest.mark.parametrize("form", sorted(FORMS))
def test_state_dict_public_shapes_and_round_trip(small, form):
    torch.manual_seed(0)
    net = A.LycorisNetwork(small, FORMS[form])
    sd = net.state_dict()
    k = "lycoris_down_blocks_1_resnets_0_conv1"  # Cout 64, Cin 32
    if form == "lora":
        want = {"lora_down.weight": (3, 32, 3, 3), "lora_up.weight": (64, 3, 1, 1)}
    elif form == "tucker":
        want = {"lora_down.weight": (3, 32, 1, 1), "lora_mid.weight": (3, 3, 3, 3), "lora_up.weight": (64, 3, 1, 1)}
    elif form == "lokr":  # factorization(64, 4) = (4, 16), factorization(32, 4) = (4, 8)
        want = {"lokr_w1": (4, 4), "lokr_w2": (16, 8, 3, 3)}
    else:  # 2 < max(16, 8) / 2
        want = {"lokr_w1": (4, 4), "lokr_w2_a": (16, 2), "lokr_w2_b": (2, 72)}
    assert {t: tuple(v.shape) for t, v in ((q[len(k) + 1:], v) for q, v in sd.items() if q.startswith(k + "."))
            if t != "alpha"} == want
    assert float(sd[k + ".alpha"]) == FORMS[form]["config"]["conv_alpha"]
    # no padded channels in the public shapes: conv_in has 4 input channels, conv_out 4 output channels
    cin_key = {"lora": "lora_down.weight", "tucker": "lora_down.weight", "lokr": "lokr_w1", "lokr_lowrank": "lokr_w1"}[form]
    if form in ("lora", "tucker"):
        assert sd["lycoris_conv_in." + cin_key].shape[1] == 4 and sd["lycoris_conv_out.lora_up.weight"].shape[0] == 4
    # zero delta at the start: the zero factor is zero, the others are drawn within the kaiming bound of the PUBLIC shape
    zero = {"lora": "lora_up.weight", "tucker": "lora_up.weight", "lokr": "lokr_w2", "lokr_lowrank": "lokr_w2_b"}[form]
    for q, v in sd.items():
        if q.endswith(".alpha") or "norm" in q:
            continue
        if q.endswith("." + zero):
            assert float(v.abs().max()) == 0, q
        else:
            bound = 1 / math.sqrt(v[0].numel())  # kaiming_uniform(a = sqrt 5): 1 / sqrt(fan_in)
            assert 0 < float(v.abs().max()) <= bound, q
    for s in net.specs:
        if s.conv is not None:
            assert float(net.conv_delta(s.name).abs().max()) == 0
    # round trip through the flat buffer, entries contiguous
    sd2 = {q: torch.randn_like(v) if not q.endswith(".alpha") else v for q, v in sd.items()}
    net2 = A.LycorisNetwork(small, FORMS[form])
    net2.load_state_dict(sd2)
    back = net2.state_dict()
    assert all(torch.equal(back[q], sd2[q]) and back[q].is_contiguous() for q in sd2)
    for s in net2.specs:  # view(): the public shape
        for t, shape in s.tensors:
            assert torch.equal(net2.view(s.name, t), sd2[f"{s.key}.{t}"]) and tuple(net2.view(s.name, t).shape) == shape
    with pytest.raises(RuntimeError, match="size mismatch"):
        net2.load_state_dict({**sd2, k + "." + zero: torch.zeros(1)})


def _public_delta(s, sd):
    """dW [Cout, Cin, 3, 3] of one convolution from the PUBLIC tensors in fp64: the issue's formulas as einsums"""
    T = lambda t: sd[f"{s.key}.{t}"].double()
    if s.algo == "lora" and not s.tucker:
        return s.alpha / s.dim * torch.einsum("pi,ichw->pchw", T("lora_up.weight")[:, :, 0, 0], T("lora_down.weight"))
    if s.algo == "lora":
        return s.alpha / s.dim * torch.einsum("pi,ijhw,jc->pchw", T("lora_up.weight")[:, :, 0, 0], T("lora_mid.weight"),
                                              T("lora_down.weight")[:, :, 0, 0])
    w1 = T("lokr_w1")
    if s.lowrank:
        ok, dim = T("lokr_w2_a").shape
        w2 = (T("lokr_w2_a") @ T("lokr_w2_b")).view(ok, -1, 3, 3) * (s.alpha / s.dim)
    else:
        w2 = T("lokr_w2")
    cout, cin = w1.shape[0] * w2.shape[0], w1.shape[1] * w2.shape[1]
    return torch.einsum("ab,cdhw->acbdhw", w1, w2).reshape(cout, cin, 3, 3)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_stored_delta_matches_public_einsum(small, form):
    net = A.LycorisNetwork(small, FORMS[form])
    g = torch.Generator().manual_seed(5)
    net.flat.data.copy_(torch.randn(net.n, generator=g))
    sd = net.state_dict()
    seen_padded = 0
    for s in net.specs:
        if s.conv is None:
            continue
        cin, cout, ci, co = s.conv
        want = torch.zeros(co, 3, 3, ci, dtype=torch.float64)
        want[:cout, :, :, :cin] = _public_delta(s, sd).permute(0, 2, 3, 1)
        got = net.conv_delta(s.name)
        assert got.shape == (co, 9, ci)
        assert float((got.view(co, 3, 3, ci) - want).abs().max()) <= 1e-12 * float(want.abs().max()), s.name
        if (ci, co) != (cin, cout):
            seen_padded += 1
            assert float(got[cout:].abs().max() if co > cout else 0) == 0
            assert float(got[:, :, cin:].abs().max() if ci > cin else 0) == 0
    assert seen_padded == 2  # conv_in (4 of 8 input channels) and conv_out (4 of 8 output channels)


def test_conv_refusals(sdxl, small):
    with pytest.raises(NotImplementedError, match="dora_wd"):
        A.match_layers(small, {"config": {"conv_dim": 4, "dora_wd": True}, "preset": TARGETS})
    # a decomposed preset that reaches a convolution through module_algo_map says so too
    with pytest.raises(NotImplementedError, match="dora_wd"):
        A.match_layers(small, {"config": {"conv_dim": 4}, "preset": {**TARGETS, "module_algo_map": {"ResnetBlock2D": {"dora_wd": True}}}})
    with pytest.raises(NotImplementedError, match="conv_dim"):
        A.match_layers(sdxl, {"config": {}, "preset": {"target_module": ["ResnetBlock2D"], "enable_conv": True}})
    with pytest.raises(NotImplementedError, match="conv_dim"):
        A.match_layers(small, {"config": {"conv_dim": 129}, "preset": TARGETS})
    with pytest.raises(NotImplementedError, match="conv_dim"):
        # [1280, 2560, 3, 3] with factor 1: w2 is the whole weight, 129 < 2560 / 2 asks for the low-rank pair
        A.match_layers(sdxl, {"config": {"algo": "lokr", "factor": 1, "conv_dim": 129}, "preset":
                              {"enable_conv": True, "target_name": ["up_blocks.0.resnets.0.conv1"]}})
    with pytest.raises(NotImplementedError, match="lokr_t2"):
        A.match_layers(small, {"config": {"algo": "lokr", "conv_dim": 2, "factor": 4, "use_tucker": True}, "preset": TARGETS})
    # a full w2 has no low-rank pair to take through a Tucker core: use_tucker changes nothing there; Linears ignore it
    a = A.match_layers(small, FORMS["lokr"])
    b = A.match_layers(small, {"config": {**FORMS["lokr"]["config"], "use_tucker": True}, "preset": TARGETS})
    assert [s.tensors for s in a] == [s.tensors for s in b]
    lin = [s for s in A.match_layers(small, FORMS["tucker"]) if s.conv is None and s.algo == "lora"]
    assert lin and all(not s.tucker and len(s.tensors) == 2 for s in lin)


def _linear_only(unet, dora):
    """the adapted tensors of a shipped Linear-only preset, [(layer, tensor, shape)] in registry order, from the contract of
    DESIGN.md 4.21 / 4.39 alone: the Transformer2DModel stacks -- LoRA(4) on proj_in / proj_out, full LoKr with factor 64 on
    the attention projections and factor 6 on the feed-forward layers, norm adapters; one dora_scale per output row"""
    out = []
    for name, kind in unet.module_kinds.items():
        if ".attentions." not in name:
            continue
        shape = unet.P.registry[name + ".weight"][1]
        if kind in ("LayerNorm", "GroupNorm"):
            out += [(name, "w_norm", shape), (name, "b_norm", shape)]
            continue
        o, i = shape
        if ".attn1." in name or ".attn2." in name or ".ff." in name:
            f = 6 if ".ff." in name else 64
            (ol, ok), (im, inn) = A.factorization(o, f), A.factorization(i, f)
            out += [(name, "lokr_w1", (ol, im)), (name, "lokr_w2", (ok, inn))]
        else:
            out += [(name, "lora_down.weight", (4, i)), (name, "lora_up.weight", (o, 4))]
        if dora:
            out.append((name, "dora_scale", (o, 1)))
    order = {n: k for k, n in enumerate(unet.P.registry)}
    return sorted(out, key=lambda e: order[e[0] + ".weight"])  # (stable: the tensors of a layer keep their order)


@pytest.mark.parametrize("toml,dora", [(TOML, False), (DORA, True)], ids=["plain", "dora"])
def test_linear_presets_unchanged(sdxl, toml, dora):
    assert A.load_config(toml)[1]["enable_conv"] is False
    net = A.LycorisNetwork(sdxl, toml)
    want, off = {}, 0
    for name, t, shape in _linear_only(sdxl, dora):
        want[(name, t)] = (off, tuple(shape))
        off += (math.prod(shape) + 63) // 64 * 64
    assert list(net.offsets) == list(want)
    assert net.offsets == want and net.n == off
    assert all(s.conv is None and not s.tucker and not s.internal for s in net.specs)
    for s in net.specs:  # the public view of a Linear's tensor is the stored one
        t = s.tensors[0][0]
        assert net.view(s.name, t).data_ptr() == net.stored(s.name, t).data_ptr()
