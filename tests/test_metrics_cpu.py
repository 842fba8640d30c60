"""CPU: what duwu.metrics and the native CLIP image tower promise without a device -- the oracle of the GPU tests pinned to
``transformers.CLIPModel``, the preprocessing rule pinned to ``transformers.CLIPImageProcessor``, the presets' sizes, the state-dict
names, the reference's control flow, the folder datasets, the aliases and the refusals."""
import numpy as np
import pytest
import torch

from tests import clip_oracle, clip_vision_oracle as vo


def _clip_model_state_dict(vcfg, tcfg, seed):
    """a CLIPModel-layout state dict: text_model.*, vision_model.*, the two projections, logit_scale"""
    sd = vo.random_state_dict(vcfg, seed)
    text = clip_oracle.random_state_dict(tcfg, seed + 1, projection=True)
    sd.update({(k if k.startswith("text_projection.") else "text_model." + k): v for k, v in text.items()})
    sd["logit_scale"] = torch.tensor(2.6592)
    return sd


# ---------------------------------------------------------------------------------------------- the oracle against transformers
@pytest.mark.parametrize("vcfg", [vo.TINY_A, vo.TINY_B], ids=["tiny_a", "tiny_b"])
def test_oracle_matches_transformers_clip_model(vcfg):
    transformers = pytest.importorskip("transformers")
    tcfg = dict(clip_oracle.TINY_QUICK, bos_token_id=998)
    config = transformers.CLIPConfig(text_config=dict(tcfg), vision_config=dict(vcfg), projection_dim=64)
    model = transformers.CLIPModel(config).eval().double()
    sd = _clip_model_state_dict(vcfg, tcfg, 11)
    model.load_state_dict(sd, strict=True)  # every name is transformers' name, none is missing
    pv = vo.pixel_values(vcfg, 2, 12)
    ids, mask = clip_oracle.tokens(tcfg, [5, 9], 13)
    with torch.no_grad():
        vis = model.vision_model(pixel_values=pv.double(), output_hidden_states=True)
        image_embeds = model.visual_projection(vis.pooler_output)
        text_embeds = model.text_projection(model.text_model(input_ids=ids, attention_mask=mask).pooler_output)
    ref = vo.forward(sd, vcfg, pv)
    assert ref["last_hidden_state"].shape == (2, (vcfg["image_size"] // vcfg["patch_size"]) ** 2 + 1, 128)
    torch.testing.assert_close(ref["last_hidden_state"], vis.last_hidden_state, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ref["pooled"], vis.pooler_output, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ref["image_embeds"], image_embeds, rtol=1e-10, atol=1e-10)
    assert len(ref["hidden_states"]) == len(vis.hidden_states) == vcfg["num_hidden_layers"] + 1
    for a, b in zip(ref["hidden_states"], vis.hidden_states):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)
    # the score: transformers' embeddings, normalised and multiplied as torchmetrics does
    ie, te = (e / e.norm(dim=-1, keepdim=True) for e in (image_embeds, text_embeds))
    torch.testing.assert_close(vo.scores(ref["image_embeds"], text_embeds), 100 * (ie * te).sum(-1), rtol=1e-10, atol=1e-10)


def test_preprocessing_matches_transformers_image_processor():
    """(clamp(x, 0, 255) / 255 - mean) / std in fp32 is what CLIPImageProcessor() computes for an image that already has the model's
    size (its resize and centre crop are then the identity).  Measured: maximum difference exactly 0.0; the bound is two fp32 ulps at
    the largest normalised value (|x| < 4: ulp 2.4e-7), room for a processor that multiplies by 1 / 255 instead of dividing."""
    transformers = pytest.importorskip("transformers")
    try:
        proc = transformers.CLIPImageProcessor()
    except (ImportError, ModuleNotFoundError) as e:
        pytest.skip(f"CLIPImageProcessor needs a missing package: {e}")
    cfg = dict(vo.TINY_A, image_size=224)
    images = vo.images_u8(cfg, 2, 21)
    got = proc(images=[im.permute(1, 2, 0).numpy().astype(np.uint8) for im in images], return_tensors="pt")["pixel_values"]
    ref = vo.preprocess(images, torch.float32)
    assert got.shape == ref.shape
    diff = float((got - ref).abs().max())
    print(f"[preprocess] max |CLIPImageProcessor - rule| = {diff:.3e}")
    assert diff <= 2 * 2.0 ** -22
    assert tuple(proc.image_mean) == pytest.approx(vo.CLIP_MEAN) and tuple(proc.image_std) == pytest.approx(vo.CLIP_STD)
    # values outside [0, 255] are clamped by the rule
    wild = torch.tensor([-3.0, 0.0, 255.0, 300.0]).view(1, 1, 2, 2).expand(1, 3, 2, 2)
    torch.testing.assert_close(vo.preprocess(wild), vo.preprocess(wild.clamp(0, 255)))


# ---------------------------------------------------------------------------------------------- presets, names
PRESETS = {  # name: (tokens, vision + projection parameters, the whole CLIPModel's parameters)
    "openai/clip-vit-base-patch32": (50, 87_849_216, 151_277_313),
    "openai/clip-vit-base-patch16": (197, 86_192_640, 149_620_737),
    "openai/clip-vit-large-patch14": (257, 303_966_208, 427_616_513),
    "openai/clip-vit-large-patch14-336": (577, 304_293_888, 427_944_193),
}


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_preset_parameter_counts(name):
    from uwudiff_amd.text_model import CLIPTextModelWithProjection
    from uwudiff_amd.vision_model import CLIP_CONFIGS, CLIPVisionModelWithProjection

    assert sorted(CLIP_CONFIGS) == sorted(PRESETS)
    vcfg, tcfg = CLIP_CONFIGS[name]
    vision = CLIPVisionModelWithProjection(vcfg, device="meta", init_weights=False)
    text = CLIPTextModelWithProjection(tcfg, device="meta", init_weights=False)
    nv = sum(v.numel() for _, v in vision.named_tensors())
    nt = sum(v.numel() for _, v in text.named_tensors())
    T, want_v, want_all = PRESETS[name]
    assert vision.T == T
    assert vision.config["hidden_size"] == 64 * vision.config["num_attention_heads"]
    assert nv == want_v
    assert nv + nt + 1 == want_all  # + logit_scale


def test_state_dict_names_round_trip():
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection

    cfg = vo.TINY_A
    sd = vo.random_state_dict(cfg, 31)
    model = CLIPVisionModelWithProjection(cfg, compute_dtype="fp32", init_weights=False)
    model.load_state_dict(sd)
    out = model.state_dict()
    assert list(out) != [] and sorted(out) == sorted(sd)
    for k, v in sd.items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    assert out["vision_model.embeddings.patch_embedding.weight"].shape == (128, 3, 14, 14)
    assert "vision_model.pre_layrnorm.weight" in out  # transformers' spelling
    # q / k / v are views of one stored operand, in the order the GEMM reads them
    p = "vision_model.encoder.layers.1.self_attn."
    qkv = model.view(p + "qkv_proj.weight")
    assert torch.equal(qkv, torch.cat([sd[p + f"{c}_proj.weight"] for c in "qkv"]))
    assert torch.equal(model.view(p + "qkv_proj.bias"), torch.cat([sd[p + f"{c}_proj.bias"] for c in "qkv"]))
    # the columns that pad 3 p p = 588 to 592 stay zero
    w = model.view("vision_model.embeddings.patch_embedding.weight")
    assert w.shape == (128, 592) and not w[:, 588:].any()
    # a wrong shape and an unknown name are refused before anything is written
    before = model.flat.clone()
    bad = dict(sd)
    bad["visual_projection.weight"] = torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="unexpected"):
        model.load_state_dict(dict(sd, **{"vision_model.nonsense": torch.zeros(1)}))
    assert torch.equal(model.flat, before)


def test_clip_model_checkpoint_loads_into_both_towers(tmp_path):
    import json

    from safetensors.torch import save_file

    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection, load_clip_pair

    vcfg, tcfg = vo.TINY_B, clip_oracle.TINY_GELU
    sd = _clip_model_state_dict(vcfg, tcfg, 41)
    (tmp_path / "config.json").write_text(json.dumps(dict(vision_config=vcfg, text_config=tcfg, projection_dim=64, model_type="clip")))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    text, vision = load_clip_pair(str(tmp_path), compute_dtype="fp32")
    assert vision.config["hidden_act"] == "gelu" and vision.T == 82 and text.config["eos_token_id"] == 999
    for k, v in vision.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for k, v in text.state_dict().items():
        assert torch.equal(v, sd[k]), k
    alone = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), compute_dtype="fp32")
    assert torch.equal(alone.flat, vision.flat)


def test_from_pretrained_presets_and_refusals():
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection as V

    small = dict(num_hidden_layers=1)
    a = V.from_pretrained("openai/clip-vit-base-patch32", config=small, compute_dtype="fp32")
    b = V.from_pretrained("openai/clip-vit-base-patch32", config=small, compute_dtype="fp32")
    assert a.T == 50 and torch.equal(a.flat, b.flat)  # seeded by the name, not by the global seed
    with pytest.raises(ValueError, match="ViT-H/14"):
        V.from_pretrained("apple/DFN5B-CLIP-ViT-H-14-378")
    with pytest.raises(ValueError, match="heads of width 64"):
        V(dict(hidden_size=1280, num_attention_heads=16, num_hidden_layers=1, intermediate_size=5120, patch_size=14, image_size=378),
          device="meta", init_weights=False)
    with pytest.raises(ValueError, match="multiple of patch_size"):
        V(dict(vo.TINY_A, image_size=71), device="meta", init_weights=False)
    with pytest.raises(ValueError, match="compute_dtype"):
        V(vo.TINY_A, compute_dtype="fp16")


def test_cpu_tensors_and_unbuilt_keywords_are_refused():
    from uwudiff_amd import lib as L
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection

    model = CLIPVisionModelWithProjection(vo.TINY_A, compute_dtype="fp32", seed=1)
    pv = vo.pixel_values(vo.TINY_A, 1, 2)
    with pytest.raises(L.UwuError, match="HIP device only"):
        model(pv)
    with pytest.raises(L.UwuError, match="HIP device only"):
        model.embed_images(vo.images_u8(vo.TINY_A, 1, 3))
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding"):
        model(pv, interpolate_pos_encoding=True)
    with pytest.raises(NotImplementedError, match="return_dict"):
        model(pv, return_dict=True)


# ---------------------------------------------------------------------------------------------- duwu.metrics, datasets, aliases
def test_compute_metrics_control_flow():
    from duwu.metrics import MetricConfig, compute_metrics

    calls = []

    def dataset_func(paths):
        calls.append(("dataset", tuple(paths)))
        return [p.upper() for p in paths]

    def no_ref(generated):
        calls.append(("no_ref", tuple(generated)))
        return 1.5

    def with_ref(generated, reference):
        calls.append(("with_ref", tuple(generated), tuple(reference)))
        return 2.5

    configs = [MetricConfig(name="A", metric_func=no_ref, generated_dataset_func=dataset_func),
               MetricConfig(name="B", metric_func=with_ref, generated_dataset_func=dataset_func, ref_dataset=["r0", "r1"])]
    assert configs[0].ref_dataset is None
    out = compute_metrics(configs, ["x.png", "y.png"])
    assert out == {"A": 1.5, "B": 2.5} and list(out) == ["A", "B"]
    assert calls == [("dataset", ("x.png", "y.png")), ("no_ref", ("X.PNG", "Y.PNG")),
                     ("dataset", ("x.png", "y.png")), ("with_ref", ("X.PNG", "Y.PNG"), ("r0", "r1"))]
    # a metric without a reference dataset is never handed the keyword
    with pytest.raises(TypeError):
        compute_metrics([MetricConfig("C", with_ref, dataset_func)], ["x.png"])


def test_compute_fid_raises():
    from duwu.metrics import compute_fid

    with pytest.raises(NotImplementedError, match="InceptionV3"):
        compute_fid([torch.zeros(3, 8, 8)], [torch.zeros(3, 8, 8)])


def _write_folder(root, n, size=(12, 10)):
    from PIL import Image

    g = torch.Generator().manual_seed(5)
    arrays = []
    for i in range(n):
        a = torch.randint(0, 256, (size[1], size[0], 3), generator=g, dtype=torch.uint8).numpy()
        sub = root / ("a" if i % 2 else "b")
        sub.mkdir(exist_ok=True)
        Image.fromarray(a).save(sub / f"{i}.png")
        (sub / f"{i}.txt").write_text(f"  caption number {i}\n")
        arrays.append(a)
    return arrays


def test_local_datasets(tmp_path):
    from duwu.data.text_image_local import LocalImageDataset, LocalImageDatasetFromFolder, LocalTextImageDataset
    from duwu.utils import get_images_recursively
    from uwudiff_amd.transforms import Compose, Resize, ToTensor

    arrays = _write_folder(tmp_path, 4)
    paths = get_images_recursively(str(tmp_path))
    assert len(paths) == 4
    index = [int(p.rsplit("/", 1)[1].split(".")[0]) for p in paths]
    ds = LocalImageDataset(paths)
    assert len(ds) == 4
    for j, i in enumerate(index):  # the default transform: CHW float in [0, 1], exactly uint8 / 255
        x = ds[j]
        assert x.dtype == torch.float32 and x.shape == (3, 10, 12)
        assert torch.equal(x, torch.from_numpy(arrays[i]).permute(2, 0, 1).float() / 255)
    folder = LocalImageDatasetFromFolder(str(tmp_path), Compose([Resize([6, 8]), ToTensor()]))
    assert len(folder) == 4 and folder[0].shape == (3, 6, 8) and 0 <= float(folder[0].min()) and float(folder[0].max()) <= 1
    pairs = LocalTextImageDataset(paths, Compose([Resize(size=[10, 12]), ToTensor()]))  # a resize to the same size is the identity
    for j, i in enumerate(index):
        image, text = pairs[j]
        assert text == f"caption number {i}"
        assert torch.equal(image, ds[j])
    with pytest.raises(TypeError):
        Resize([4, 4])(torch.zeros(3, 8, 8))


def test_aliases_resolve_the_metric_nodes():
    from uwudiff_amd import config as C
    from uwudiff_amd import metrics, transforms, vision_model

    assert C.get_obj_from_str("torchvision.transforms.Compose") is transforms.Compose
    assert C.get_obj_from_str("torchvision.transforms.Resize") is transforms.Resize
    assert C.get_obj_from_str("torchvision.transforms.ToTensor") is transforms.ToTensor
    assert C.get_obj_from_str("torchmetrics.multimodal.CLIPScore") is metrics.CLIPScore
    assert C.get_obj_from_str("transformers.CLIPVisionModelWithProjection") is vision_model.CLIPVisionModelWithProjection
    # the two CLIP text aliases that were there before are not shadowed by the new one
    assert C.get_obj_from_str("transformers.CLIPTextModelWithProjection").__name__ == "SyntheticTextModel"
    # the metric node of the demo config, as the launcher instantiates it
    import os

    from tests.conftest import ROOT

    import importlib.util

    spec = importlib.util.spec_from_file_location("launcher_test_metrics", os.path.join(ROOT, "test_scripts", "test_metrics.py"))
    launcher = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launcher)
    node = C.load_yaml(os.path.join(ROOT, "configs", "demo_metrics.yaml")).metrics[0]
    mc = launcher.metric_config(node)
    import duwu.metrics
    from duwu.data.text_image_local import LocalTextImageDataset

    assert isinstance(mc, duwu.metrics.MetricConfig) and mc.name == "CLIP score" and mc.ref_dataset is None
    assert mc.metric_func.func is duwu.metrics.compute_clip_score
    assert mc.metric_func.keywords["model_name_or_path"] == "openai/clip-vit-large-patch14"
    assert mc.generated_dataset_func.func is LocalTextImageDataset
    transform = mc.generated_dataset_func.keywords["image_transform"]
    assert isinstance(transform, transforms.Compose) and transform.transforms[0].size == (224, 224)


def test_clip_score_refuses_cpu_and_wrong_sizes(monkeypatch):
    """the metric on a tiny pair of towers (the preset is swapped for it: the checks under test do not depend on the model's size)"""
    from uwudiff_amd import lib as L
    from uwudiff_amd import metrics
    from uwudiff_amd.text_model import CLIPTextModelWithProjection
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection

    def tiny_pair(name, compute_dtype="bf16", device=None):
        return (CLIPTextModelWithProjection(clip_oracle.TINY_QUICK, compute_dtype=compute_dtype, seed=1),
                CLIPVisionModelWithProjection(vo.TINY_A, compute_dtype=compute_dtype, seed=2))

    monkeypatch.setattr(metrics, "load_clip_pair", tiny_pair)
    m = metrics.CLIPScore("openai/clip-vit-large-patch14")
    with pytest.raises(L.UwuError, match="HIP device only"):
        m.update(vo.images_u8(vo.TINY_A, 2, 1), ["a", "b"])
    with pytest.raises(ValueError, match=r"torchvision.transforms.Resize with size: \[70, 70\]"):
        m.update(torch.zeros(2, 3, 64, 64), ["a", "b"])
    with pytest.raises(ValueError, match="2 images and 1 texts"):
        m.update(vo.images_u8(vo.TINY_A, 2, 1), ["a"])
    with pytest.raises(RuntimeError, match="before any update"):
        m.compute()
    with pytest.raises(NotImplementedError):
        metrics.CLIPScore("openai/clip-vit-large-patch14", dist_sync_on_step=True)


def test_clip_score_refuses_the_vit_h_model_of_the_reference_config():
    from uwudiff_amd import metrics

    with pytest.raises(ValueError, match="ViT-H/14"):
        metrics.CLIPScore("apple/DFN5B-CLIP-ViT-H-14-378")
