"""CPU: tests/clip_oracle.py against ``transformers`` itself in fp64, and the host side of uwudiff_amd.text_model -- the
transformers key set in both layouts, local-directory loading, the built-in SDXL configurations, target resolution of the YAMLs,
and the refusals that need no device."""
import json
import os

import pytest
import torch

from tests import clip_oracle
from tests.conftest import ROOT

LENGTHS = [5, 40, 77]


def _hf(cfg, projection):
    transformers = pytest.importorskip("transformers")
    hf_cfg = transformers.CLIPTextConfig(
        hidden_size=cfg["hidden_size"], num_attention_heads=cfg["num_attention_heads"], num_hidden_layers=cfg["num_hidden_layers"],
        intermediate_size=cfg["intermediate_size"], max_position_embeddings=cfg["max_position_embeddings"],
        vocab_size=cfg["vocab_size"], hidden_act=cfg["hidden_act"], eos_token_id=cfg["eos_token_id"], bos_token_id=cfg["vocab_size"] - 2,
        pad_token_id=1, layer_norm_eps=cfg["layer_norm_eps"], projection_dim=cfg["projection_dim"])
    torch.manual_seed(7)
    cls = transformers.CLIPTextModelWithProjection if projection else transformers.CLIPTextModel
    m = cls(hf_cfg).eval().double()
    with torch.no_grad():  # transformers initialises biases to 0 and norms to 1 / 0: randomise them so every term is live
        for n, p in m.named_parameters():
            if n.endswith(".bias"):
                p.normal_(0.0, 0.1)
            elif "layer_norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    return m


@pytest.mark.parametrize("cfg", [clip_oracle.TINY_QUICK, clip_oracle.TINY_GELU], ids=["quick_gelu-argmax", "gelu-eos_eq"])
@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
def test_oracle_equals_transformers_fp64(cfg, projection):
    """last hidden state, pooled, every hidden state (and text_embeds) to 1e-10 at ALL positions, padded ones included: the key
    mask changes those rows (a padded query sees only the unpadded keys), the causal bound alone would not"""
    m = _hf(cfg, projection)
    ids, mask = clip_oracle.tokens(cfg, LENGTHS, seed=3)
    with torch.no_grad():
        out = m(ids, attention_mask=mask, output_hidden_states=True, return_dict=True)
        nomask = m(ids, output_hidden_states=True, return_dict=True)
    ref = clip_oracle.forward(m.state_dict(), cfg, ids, mask)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0, atol=1e-10)  # noqa: E731
    close(ref["last_hidden_state"], out.last_hidden_state)
    assert len(out.hidden_states) == cfg["num_hidden_layers"] + 1 == len(ref["hidden_states"])
    for a, b in zip(ref["hidden_states"], out.hidden_states):
        close(a, b)
    if projection:
        close(ref["text_embeds"], out.text_embeds)
    else:
        close(ref["pooled"], out.pooler_output)
        assert ref["text_embeds"] is None
    # the mask matters, and only where it should: rows of the padded sequence past its length differ from the unmasked run
    assert float((out.last_hidden_state[0, 5:] - nomask.last_hidden_state[0, 5:]).abs().max()) > 1e-3
    close(out.last_hidden_state[0, :5], nomask.last_hidden_state[0, :5])
    close(clip_oracle.forward(m.state_dict(), cfg, ids, None)["last_hidden_state"], nomask.last_hidden_state)
    # pooling position: row 0 has its eos at 4 under both rules
    assert clip_oracle.pool_position(ids, cfg["eos_token_id"]).tolist() == [4, 39, 76]


def test_pool_position_rules():
    ids = torch.tensor([[998, 5, 999, 7, 999], [998, 5, 6, 7, 8]])
    assert clip_oracle.pool_position(ids, 2).tolist() == [2, 0]      # first occurrence of the largest id
    assert clip_oracle.pool_position(ids, 999).tolist() == [2, 0]    # first id equal to eos; none -> 0
    assert clip_oracle.pool_position(ids, 7).tolist() == [3, 3]


def _native(cfg, projection=False, **kw):
    from uwudiff_amd import text_model

    cls = text_model.CLIPTextModelWithProjection if projection else text_model.CLIPTextModel
    return cls.from_config(cfg, **kw)


@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
def test_transformers_state_dict_loads_in_both_layouts(projection):
    cfg = clip_oracle.TINY_GELU
    hf = _hf(cfg, projection)
    sd = {k: v.float() for k, v in hf.state_dict().items()}
    flat = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in sd.items()}
    prefixed = {(k if k.startswith("text_projection.") else "text_model." + k): v for k, v in flat.items()}
    prefixed["text_model.embeddings.position_ids"] = torch.arange(77)[None]  # the buffer older checkpoints carry
    for layout in (flat, prefixed):
        m = _native(cfg, projection, init_weights=False, compute_dtype="fp32")
        assert not m.flat.any()
        res = m.load_state_dict(layout)
        assert not res.missing_keys and not res.unexpected_keys
        got = m.state_dict()
        assert sorted(got) == sorted(sd)  # the key set of the installed transformers, for each class
        for k, v in sd.items():
            assert got[k].dtype == torch.float32 and torch.equal(got[k], v), k
    # q, k, v sit back to back as one [3 D, D] operand
    D = cfg["hidden_size"]
    w = m.w32("encoder.layers.1.self_attn.qkv_proj.weight")
    assert tuple(w.shape) == (3 * D, D)
    for j, c in enumerate("qkv"):
        assert torch.equal(w[j * D:(j + 1) * D], flat[f"encoder.layers.1.self_attn.{c}_proj.weight"])
    assert torch.equal(m.w32("encoder.layers.1.self_attn.qkv_proj.bias")[D:2 * D], flat["encoder.layers.1.self_attn.k_proj.bias"])


def test_load_state_dict_refusals_write_nothing():
    cfg = clip_oracle.TINY_QUICK
    m = _native(cfg, seed=1)
    ref = clip_oracle.random_state_dict(cfg, seed=2)
    before = m.state_dict()
    bad = dict(ref)
    del bad["encoder.layers.2.mlp.fc2.bias"]
    with pytest.raises(RuntimeError, match="mlp.fc2.bias"):
        m.load_state_dict(bad)
    bad = dict(ref)
    bad["encoder.layers.0.self_attn.q_proj.weight"] = torch.zeros(128, 64)
    with pytest.raises(RuntimeError, match="q_proj.weight"):
        m.load_state_dict(bad)
    bad = dict(ref)
    bad["text_projection.weight"] = torch.zeros(64, 128)  # a plain CLIPTextModel has no projection
    with pytest.raises(RuntimeError, match="text_projection"):
        m.load_state_dict(bad)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    m.load_state_dict(ref)
    assert all(torch.equal(v, ref[k]) for k, v in m.state_dict().items())


def test_parent_module_state_dict_round_trips():
    """inside a parent (the trainer's checkpoint): entries under the parent's prefix, restored by the parent's load_state_dict"""
    import torch.nn as nn

    cfg = clip_oracle.TINY_QUICK

    class Holder(nn.Module):
        def __init__(self, seed):
            super().__init__()
            self.te = nn.ModuleList([_native(cfg, seed=seed), _native(cfg, projection=True, seed=seed + 1)])
            self.register_buffer("ema", torch.tensor(float(seed)))

    a, b = Holder(1), Holder(5)
    sd = a.state_dict()
    assert "te.0.encoder.layers.2.mlp.fc1.weight" in sd and "te.1.text_projection.weight" in sd and "te.0.flat" not in sd
    assert not torch.equal(b.te[0].flat, a.te[0].flat)
    res = b.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(b.te[0].flat, a.te[0].flat) and torch.equal(b.te[1].flat, a.te[1].flat) and float(b.ema) == 1.0
    del sd["te.1.text_model.final_layer_norm.bias"]
    sd["te.0.nonsense"] = torch.zeros(1)
    res = b.load_state_dict(sd, strict=False)
    assert res.missing_keys == ["te.1.text_model.final_layer_norm.bias"] and res.unexpected_keys == ["te.0.nonsense"]
    with pytest.raises(RuntimeError, match="nonsense"):
        b.load_state_dict(sd)


def test_local_directory_round_trips(tmp_path, monkeypatch):
    """a save_pretrained-style directory: config.json (with keys this build ignores) + model.safetensors in the prefixed layout"""
    from safetensors.torch import save_file
    from uwudiff_amd.text_model import CLIPTextModel, CLIPTextModelWithProjection
    from uwudiff_amd.flat import FlatModule

    calls, inner = [], FlatModule._from_local_dir.__func__  # every local directory goes through the one loader in flat.py
    monkeypatch.setattr(FlatModule, "_from_local_dir", classmethod(lambda c, *a, **kw: calls.append(c) or inner(c, *a, **kw)))

    cfg = clip_oracle.TINY_GELU
    sd = clip_oracle.random_state_dict(cfg, seed=5, projection=True)
    d = tmp_path / "repo" / "text_encoder_2"
    os.makedirs(d)
    (d / "config.json").write_text(json.dumps(dict(cfg, architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model",
                                                   attention_dropout=0.0, initializer_factor=1.0, torch_dtype="float16")))
    save_file({("text_model." + k if not k.startswith("text_projection") else k): v.half().contiguous() for k, v in sd.items()},
              str(d / "model.safetensors"))
    for m in (CLIPTextModelWithProjection.from_pretrained(str(d)),
              CLIPTextModelWithProjection.from_pretrained(str(tmp_path / "repo"), subfolder="text_encoder_2")):
        assert m.config.hidden_act == "gelu" and m.config.eos_token_id == 999 and m.config.num_hidden_layers == 3
        assert "architectures" not in m.config and "torch_dtype" not in m.config
        got = m.state_dict()
        assert sorted(got) == sorted("text_model." + k if not k.startswith("text_projection") else k for k in sd)
        assert all(torch.equal(got["text_model." + k if not k.startswith("text_projection") else k], v.half().float()) for k, v in sd.items())
    assert calls == [CLIPTextModelWithProjection] * 2
    with pytest.raises(RuntimeError, match="text_projection"):  # the plain class refuses the extra tensor
        CLIPTextModel.from_pretrained(str(d))


def test_any_other_name_gives_the_same_weights_twice():
    from uwudiff_amd.text_model import CLIPTextModel

    over = dict(num_hidden_layers=1, vocab_size=1000)
    name = "stabilityai/stable-diffusion-xl-base-1.0"
    torch.manual_seed(1)
    a = CLIPTextModel.from_pretrained(name, subfolder="text_encoder", config=over).state_dict()
    torch.manual_seed(2)  # the global seed plays no part
    b = CLIPTextModel.from_pretrained(name, subfolder="text_encoder", config=over).state_dict()
    c = CLIPTextModel.from_pretrained("someone/else", subfolder="text_encoder", config=over).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["encoder.layers.0.mlp.fc1.weight"], c["encoder.layers.0.mlp.fc1.weight"])
    assert float(a["embeddings.token_embedding.weight"].std()) == pytest.approx(0.02, rel=0.05)
    assert torch.equal(a["final_layer_norm.weight"], torch.ones(768)) and not a["encoder.layers.0.mlp.fc1.bias"].any()
    with pytest.raises(ValueError, match="text_encoder_2"):
        CLIPTextModel.from_pretrained(name, subfolder="unet")


@pytest.mark.parametrize("subfolder,D,H,Lyr,F,act", [("text_encoder", 768, 12, 12, 3072, "quick_gelu"),
                                                      ("text_encoder_2", 1280, 20, 32, 5120, "gelu")])
def test_built_in_sdxl_configs(subfolder, D, H, Lyr, F, act):
    """the configuration as built in, and the buffer shapes of a 1-layer override (32 layers of 1280 are never allocated here)"""
    from uwudiff_amd.text_model import SDXL_TEXT_CONFIGS, CLIPTextModelWithProjection

    c = SDXL_TEXT_CONFIGS[subfolder]
    assert (c["hidden_size"], c["num_attention_heads"], c["num_hidden_layers"], c["intermediate_size"], c["hidden_act"]) == (D, H, Lyr, F, act)
    assert (c["max_position_embeddings"], c["vocab_size"], c["layer_norm_eps"], c["eos_token_id"]) == (77, 49408, 1e-5, 2)
    m = CLIPTextModelWithProjection.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder=subfolder,
                                                    config=dict(num_hidden_layers=1), init_weights=False)
    assert m.config.num_hidden_layers == 1 and m.config.hidden_size == D and m.compute_dtype == "bf16"
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    p = "text_model.encoder.layers.0."
    assert shapes["text_model.embeddings.token_embedding.weight"] == (49408, D)
    assert shapes["text_model.embeddings.position_embedding.weight"] == (77, D)
    assert shapes[p + "self_attn.q_proj.weight"] == shapes[p + "self_attn.out_proj.weight"] == (D, D)
    assert shapes[p + "mlp.fc1.weight"] == (F, D) and shapes[p + "mlp.fc2.weight"] == (D, F) and shapes[p + "mlp.fc1.bias"] == (F,)
    assert shapes["text_projection.weight"] == (c["projection_dim"], D) and c["projection_dim"] == D
    per_layer = 4 * (D * D + D) + 2 * D * F + F + D + 4 * D
    assert sum(v.numel() for _, v in m.named_tensors()) == (49408 + 77) * D + per_layer + 2 * D + D * D
    assert next(m.buffers()) is m.flat and m.flat.dtype == torch.float32 and not list(m.parameters()) and not m.training


def test_precision_casts_leave_the_fp32_master():
    """`_load_config_.precision: torch.float16` on the enclosing ConcatTextEncoders reaches the model as `.to(torch.float16)`: the
    flat fp32 master stays as it is (the compute dtype is the constructor's `compute_dtype`), as AutoencoderKL keeps its own"""
    m = _native(clip_oracle.TINY_QUICK, seed=3)
    before = m.flat.clone()
    m = m.to(torch.float16)
    assert m.flat.dtype == torch.float32 and torch.equal(m.flat, before) and m.ones.dtype == torch.float32
    assert m._uwu_keep_fp32_master is True and m.kind == "clip_sd1" and callable(m.final_layer_norm)


def test_refusals_without_a_device():
    from uwudiff_amd.lib import UwuError
    from uwudiff_amd.text_model import CLIPTextModel

    m = _native(clip_oracle.TINY_QUICK, seed=3)
    ids, mask = clip_oracle.tokens(clip_oracle.TINY_QUICK, [5], seed=0)
    with pytest.raises(UwuError, match="no CPU fallback"):
        m(ids, attention_mask=mask)
    with pytest.raises(UwuError, match="no CPU fallback"):
        m.final_layer_norm(torch.zeros(1, 77, 128))
    for bad in (dict(hidden_act="relu"), dict(num_attention_heads=4), dict(max_position_embeddings=256)):
        with pytest.raises(ValueError):
            CLIPTextModel.from_config(dict(clip_oracle.TINY_QUICK, **bad), init_weights=False)
    with pytest.raises(ValueError):
        CLIPTextModel.from_config(clip_oracle.TINY_QUICK, compute_dtype="fp16", init_weights=False)


def _text_targets(name):
    from uwudiff_amd.config import get_obj_from_str, load_yaml

    cfg = load_yaml(os.path.join(ROOT, "configs", name))
    nodes = [pair[0] for pair in cfg.trainer.model_config.te.text_model_and_configs]
    return nodes, [get_obj_from_str(n["_target_"]) for n in nodes]


def test_clip_yaml_names_the_native_classes_and_the_others_stay_synthetic():
    from uwudiff_amd.conditioning import SyntheticCLIPTextModel
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.text_model import CLIPTextModel

    nodes, fns = _text_targets("demo_training_clip.yaml")
    assert [n["subfolder"] for n in nodes] == ["text_encoder", "text_encoder_2"]
    assert all(n["pretrained_model_name_or_path"] == "stabilityai/stable-diffusion-xl-base-1.0" for n in nodes)
    assert all(f.__self__ is CLIPTextModel and f.__func__ is CLIPTextModel.from_pretrained.__func__ for f in fns)
    for name in ("demo_training.yaml", "demo_training_pixels.yaml"):
        _, fns = _text_targets(name)
        assert len(fns) == 2 and all(f.__self__ is SyntheticCLIPTextModel for f in fns)
    # apart from the two targets, the new file is demo_training_pixels.yaml
    a = load_yaml(os.path.join(ROOT, "configs", "demo_training_clip.yaml"))
    b = load_yaml(os.path.join(ROOT, "configs", "demo_training_pixels.yaml"))
    for pair in a.trainer.model_config.te.text_model_and_configs:
        pair[0]["_target_"] = "transformers.CLIPTextModel.from_pretrained"
    assert a == b
