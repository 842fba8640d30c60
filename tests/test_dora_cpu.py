"""CPU: weight decomposition (DoRA, ``dora_wd``) of the LyCORIS adapters -- configuration, specs and parameter count over
the SDXL UNet names, initialisation of ``dora_scale`` and the refusal of an uninitialised network, the state dict, and the
fp64 restatement of the rule that the GPU tests (tests/test_dora_gpu.py) compare the kernels with."""
import math
import os

import pytest
import torch

from tests.conftest import ROOT
from uwudiff_amd import adapters as A
from uwudiff_amd.unet import SDXL_UNET_CONFIG, TINY_UNET_CONFIG, UNet2DConditionModel

TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")
DORA_TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers-dora.toml")
DORA_YAML = os.path.join(ROOT, "configs", "demo_training_dora.yaml")
EPS = torch.finfo(torch.float32).eps


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def dora_weight(base, kind, leaves, scale, dora_scale, wd_on_out):
    """W' of DESIGN.md section 4.39 from leaf tensors with torch ops (differentiable; fp64 when the leaves are).

    ``kind``: 'lora' (leaves up [N, r], down [r, K]), 'lokr' (w1, w2) or 'lokr_lowrank' (w1, w2_a, w2_b); ``dora_scale``
    [N, 1] (wd_on_out) or [1, K]; ``dora_scale`` None: no decomposition, W + dW.  eps is added to the norm."""
    if kind == "lora":
        d = leaves[0] @ leaves[1]
    elif kind == "lokr":
        d = torch.kron(leaves[0], leaves[1])
    else:
        d = torch.kron(leaves[0], leaves[1] @ leaves[2])
    V = base + scale * d.view(base.shape)
    if dora_scale is None:
        return V
    ss = V.pow(2).sum(dim=1 if wd_on_out else 0, keepdim=True)
    # u = ||V||; where it is 0 its derivative is taken as 0 (the rule: the second term of dV vanishes there), not sqrt's inf
    u = torch.where(ss > 0, torch.where(ss > 0, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(ss))
    return dora_scale * (V / (u + EPS))


def _leaves(kind, N, K, g, r=2, out_k=0, in_n=0):
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if kind == "lora":
        return [rnd(N, r), rnd(r, K)]
    if kind == "lokr":
        return [rnd(N // out_k, K // in_n), rnd(out_k, in_n)]
    return [rnd(N // out_k, K // in_n), rnd(out_k, r), rnd(r, in_n)]


@pytest.mark.parametrize("kind,N,K,out_k,in_n", [("lora", 12, 20, 0, 0), ("lokr", 12, 20, 4, 5), ("lokr_lowrank", 39, 77, 13, 11)])
@pytest.mark.parametrize("wd_on_out", [True, False])
def test_restatement_properties(kind, N, K, out_k, in_n, wd_on_out):
    g = torch.Generator().manual_seed(5)
    base = torch.randn(N, K, generator=g, dtype=torch.float64)
    leaves = _leaves(kind, N, K, g, out_k=out_k, in_n=in_n)
    dim = 1 if wd_on_out else 0
    # zero delta (the last factor zero) and the initial dora_scale: W' = W to 1e-6 relative
    zero = leaves[:-1] + [torch.zeros_like(leaves[-1])]
    m0 = base.norm(dim=dim, keepdim=True)
    W0 = dora_weight(base, kind, zero, 0.5, m0, wd_on_out)
    assert float((W0 - base).abs().max() / base.abs().max()) < 1e-6
    assert not torch.equal(W0, base)  # u / (u + eps): equal within rounding, not bit for bit
    # every row (column) of W' has the norm m u / (u + eps)
    m = m0 * (1 + 0.1 * torch.randn(m0.shape, generator=g, dtype=torch.float64))
    Wd = dora_weight(base, kind, leaves, 0.5, m, wd_on_out)
    u = dora_weight(base, kind, leaves, 0.5, None, wd_on_out).norm(dim=dim, keepdim=True)
    assert torch.allclose(Wd.norm(dim=dim, keepdim=True), m.abs() * u / (u + EPS), rtol=1e-12, atol=0)
    assert tuple(m.shape) == ((N, 1) if wd_on_out else (1, K))


def test_restatement_gradients_are_the_stated_ones():
    """autograd of the restatement against the closed form of the rule (norm not detached; second term 0 where u = 0)"""
    g = torch.Generator().manual_seed(6)
    N, K = 7, 9
    for wd_on_out in (True, False):
        V = torch.randn(N, K, generator=g, dtype=torch.float64)
        V[2] = 0
        V[:, 3] = 0
        V.requires_grad_(True)
        m = torch.randn((N, 1) if wd_on_out else (1, K), generator=g, dtype=torch.float64).requires_grad_(True)
        G = torch.randn(N, K, generator=g, dtype=torch.float64)
        dim = 1 if wd_on_out else 0
        # (sqrt of a sum of squares has no finite autograd derivative at 0: the rule states the limit, 0)
        ss = V.pow(2).sum(dim=dim, keepdim=True)
        u = torch.where(ss > 0, ss.clamp_min(1e-300).sqrt(), torch.zeros_like(ss))
        n = u + EPS
        (G * (m * V / n)).sum().backward()
        with torch.no_grad():
            t = (G * V).sum(dim=dim, keepdim=True)
            dm = t / n
            second = torch.where(u > 0, V * t / (n * u.clamp_min(1e-300)), torch.zeros_like(V))
            dV = (m / n) * (G - second)
        assert torch.allclose(m.grad, dm, rtol=1e-12, atol=1e-14)
        assert torch.allclose(V.grad, dV, rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------- configuration
def _cfg(config=None, amap=None):
    return {"config": dict(config or {}), "preset": {"target_module": ["Transformer2DModel"],
                                                      "module_algo_map": dict(amap or {})}}


def test_config_keys_parse_and_override():
    assert A.CONFIG_DEFAULTS["dora_wd"] is False and A.CONFIG_DEFAULTS["wd_on_out"] is True
    config, preset = A.load_config(_cfg())
    assert config["dora_wd"] is False and config["wd_on_out"] is True
    config, preset = A.load_config(_cfg({"dora_wd": True, "wd_on_out": False},
                                        {"Attention": {"algo": "lokr", "dora_wd": False},
                                         "FeedForward": {"wd_on_out": True}}))
    assert config["dora_wd"] is True and config["wd_on_out"] is False
    assert preset["module_algo_map"]["Attention"] == {"algo": "lokr", "dora_wd": False}
    unet = UNet2DConditionModel(TINY_UNET_CONFIG, init_weights=False, device="meta")
    specs = {s.name: s for s in A.match_layers(unet, (config, preset))}
    blk = "down_blocks.1.attentions.0.transformer_blocks.0."
    assert not specs[blk + "attn1.to_q"].dora and specs[blk + "attn1.to_q"].tensors[-1][0] != "dora_scale"  # the table wins
    ff = specs[blk + "ff.net.2"]
    assert ff.dora and ff.wd_on_out and ff.tensors[-1] == ("dora_scale", (ff.shape[0], 1))
    pin = specs["down_blocks.1.attentions.0.proj_in"]
    assert pin.dora and not pin.wd_on_out and pin.tensors[-1] == ("dora_scale", (1, pin.shape[1]))


@pytest.mark.parametrize("key", ["dora_wd", "wd_on_out"])
@pytest.mark.parametrize("bad", [1, 0, "true", None, 1.0])
def test_non_bool_is_refused_by_name(key, bad):
    with pytest.raises(ValueError, match=key):
        A.load_config(_cfg({key: bad}))
    with pytest.raises(ValueError, match=key):
        A.load_config(_cfg({}, {"Attention": {key: bad}}))


def test_shipped_dora_configs_load():
    import yaml

    config, preset = A.load_config(DORA_TOML)
    plain, plain_preset = A.load_config(TOML)
    assert config["dora_wd"] is True and config["wd_on_out"] is True
    assert {k: v for k, v in config.items() if k not in ("dora_wd", "wd_on_out")} == \
        {k: v for k, v in plain.items() if k not in ("dora_wd", "wd_on_out")}
    assert preset == plain_preset
    y = yaml.safe_load(open(DORA_YAML))
    assert os.path.samefile(os.path.join(ROOT, y["trainer"]["lycoris_config"]), DORA_TOML)
    p = yaml.safe_load(open(os.path.join(ROOT, "configs", "demo_training_prodigy.yaml")))
    p["trainer"]["lycoris_config"] = y["trainer"]["lycoris_config"]
    assert y == p  # demo_training_prodigy.yaml pointing at the DoRA TOML, nothing else


# ------------------------------------------------------------------------------------------------------------------ specs
@pytest.fixture(scope="module")
def sdxl():
    return UNet2DConditionModel(SDXL_UNET_CONFIG, init_weights=False, device="meta")


@pytest.mark.parametrize("wd_on_out", [True, False])
def test_sdxl_specs_gain_one_trailing_dora_scale(sdxl, wd_on_out):
    config, preset = A.load_config(DORA_TOML)
    config["wd_on_out"] = wd_on_out
    plain = A.match_layers(sdxl, TOML)
    dora = A.match_layers(sdxl, (config, preset))
    assert [s.name for s in plain] == [s.name for s in dora]
    extra = 0
    for a, b in zip(plain, dora):
        assert (a.algo, a.shape, a.r, a.out_k, a.in_n, a.lowrank, a.scale) == (b.algo, b.shape, b.r, b.out_k, b.in_n,
                                                                               b.lowrank, b.scale)
        if a.algo == "norm":
            assert b.tensors == a.tensors and not b.dora  # norm adapters are never decomposed
            continue
        N, K = a.shape
        assert b.dora and b.tensors == a.tensors + [("dora_scale", (N, 1) if wd_on_out else (1, K))]
        extra += N if wd_on_out else K
    assert extra > 0
    net_plain = A.LycorisNetwork(sdxl, TOML)
    net = A.LycorisNetwork(sdxl, (config, preset))
    assert net.num_adapter_params() == net_plain.num_adapter_params() + extra
    assert net_plain.num_adapter_params() == sum(s.numel for s in plain)
    assert net.dora_uninitialised and not net_plain.dora_uninitialised


def test_off_is_identical_to_a_config_without_the_keys():
    unet = UNet2DConditionModel(TINY_UNET_CONFIG, init_weights=False, device="meta")
    config, preset = A.load_config(TOML)
    off = ({**config, "dora_wd": False, "wd_on_out": False}, preset)
    a, b = A.LycorisNetwork(unet, TOML), A.LycorisNetwork(unet, off)
    assert a.n == b.n and a.offsets == b.offsets
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert not any(k.endswith("dora_scale") for k in b.state_dict())
    assert not b.dora_uninitialised


# ---------------------------------------------------------------------------------------------- initialisation, refusals
@pytest.fixture(scope="module")
def tiny_cpu():
    torch.manual_seed(3)
    unet = UNet2DConditionModel(TINY_UNET_CONFIG, device="cpu")
    unet.requires_grad_(False)
    return unet


@pytest.mark.parametrize("wd_on_out", [True, False])
def test_dora_scale_starts_at_the_base_norm(tiny_cpu, wd_on_out):
    config, preset = A.load_config(DORA_TOML)
    config["wd_on_out"] = wd_on_out
    net = A.LycorisNetwork(tiny_cpu, (config, preset))
    assert not net.dora_uninitialised
    seen = 0
    for s in net.specs:
        if s.algo == "norm":
            assert ("dora_scale" not in dict(s.tensors))
            continue
        base = tiny_cpu.P.base32(s.name + ".weight").double()
        want = base.norm(dim=1 if wd_on_out else 0, keepdim=True)
        got = net.view(s.name, "dora_scale")
        assert got.shape == want.shape and got.dtype == torch.float32
        assert float(((got.double() - want).abs() / want).max()) < 4 * EPS
        seen += 1
    assert seen > 0
    # every other tensor starts as without decomposition: zero delta
    assert all(float(net.view(s.name, t).abs().max()) == 0 for s in net.specs for t, _ in s.tensors
               if t in ("lora_up.weight", "lokr_w2", "lokr_w2_b", "w_norm", "b_norm"))


class _Attach:
    """stands in for the UNet in apply_to (attaching to a real one needs the device)"""

    def __init__(self):
        self.attached = None

    def attach_adapters(self, net):
        self.attached = net


def test_meta_network_is_refused_until_loaded(tiny_cpu):
    meta = UNet2DConditionModel(TINY_UNET_CONFIG, init_weights=False, device="meta")
    net = A.LycorisNetwork(meta, DORA_TOML)
    assert net.dora_uninitialised
    for s in net.specs:
        if s.dora:
            assert float(net.view(s.name, "dora_scale").abs().max()) == 0
    with pytest.raises(RuntimeError, match="dora_scale"):
        net.apply_to(_Attach())
    full = A.LycorisNetwork(tiny_cpu, DORA_TOML).state_dict()
    # a state dict that lacks one dora_scale does not initialise the network
    one = next(k for k in full if k.endswith(".dora_scale"))
    net.load_state_dict({k: v for k, v in full.items() if k != one}, strict=False)
    assert net.dora_uninitialised
    with pytest.raises(RuntimeError, match="dora_scale"):
        net.apply_to(_Attach())
    net.load_state_dict(full)
    assert not net.dora_uninitialised
    target = _Attach()
    net.apply_to(target)
    assert target.attached is net
    # a plain network on meta is attached as before
    plain = A.LycorisNetwork(meta, TOML)
    plain.apply_to(target)
    assert target.attached is plain


def test_state_dict_round_trip(tiny_cpu):
    net = A.LycorisNetwork(tiny_cpu, DORA_TOML)
    sd = net.state_dict()
    n_lin = 0
    for s in net.specs:
        k = f"{s.key}.dora_scale"
        if s.algo == "norm":
            assert k not in sd
            continue
        n_lin += 1
        assert sd[k].shape == (s.shape[0], 1) and sd[k].dtype == torch.float32
        assert list(sd).index(k) == list(sd).index(f"{s.key}.alpha") - 1  # the last tensor of its layer
    assert n_lin == sum(k.endswith(".dora_scale") for k in sd) > 0
    g = torch.Generator().manual_seed(1)
    sd2 = {k: torch.randn(v.shape, generator=g) if not k.endswith(".alpha") else v for k, v in sd.items()}
    net2 = A.LycorisNetwork(tiny_cpu, DORA_TOML)
    net2.load_state_dict(sd2)
    back = net2.state_dict()
    assert list(back) == list(sd2) and all(torch.equal(back[k], sd2[k]) for k in sd2)
    one = next(k for k in sd2 if k.endswith(".dora_scale"))
    with pytest.raises(RuntimeError, match=one.replace(".", r"\.")):
        net2.load_state_dict({k: v for k, v in sd2.items() if k != one}, strict=True)
    # a checkpoint of the plain preset does not fit: every dora_scale is reported
    with pytest.raises(RuntimeError, match="dora_scale"):
        net2.load_state_dict(A.LycorisNetwork(tiny_cpu, TOML).state_dict(), strict=True)


def test_workspace_size_mirrors_the_kernel():
    s = A.Spec("x", "lora", (2050, 33), dim=2, dora_wd=True, wd_on_out=False)
    assert A.dora_grad_ws_elems(s, 2050, 33) == 4 * 9 * 33
    s = A.Spec("x", "lora", (2050, 33), dim=2, dora_wd=True, wd_on_out=True)
    assert A.dora_grad_ws_elems(s, 2050, 33) == 0
    assert math.prod(s.tensors[-1][1]) == 2050
