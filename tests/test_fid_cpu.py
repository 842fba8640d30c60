"""CPU: what the FID metric and the native InceptionV3 promise without a device -- the oracle of the GPU tests pinned to the published
layer table and parameter counts, the state-dict names, the FID formula on hand-made statistics, the input rule, ``CenterCrop``, the
aliases, the launcher's node, the datasets, the seeded initialisation's range and the refusals."""
import os

import numpy as np
import pytest
import torch

from tests import inception_oracle as io
from tests.conftest import ROOT


# ---------------------------------------------------------------------------------------------- the layer table
def test_oracle_parameter_counts_and_output_shape():
    sd = io.random_state_dict(1)
    n = sum(v.numel() for k, v in sd.items() if k.endswith(("conv.weight", "bn.weight", "bn.bias")))
    assert n == 21_785_568
    assert n + 2048 * 1000 + 1000 == 23_834_568  # torchvision's inception_v3 without its auxiliary head
    assert len(io.LAYERS) == 94 and sum(k.endswith("conv.weight") for k in sd) == 94
    out = io.forward(sd, io.preprocess(io.pictures(1, 2)), "bf16")
    assert out.shape == (1, 2048) and bool(torch.isfinite(out).all())


def test_model_layer_table_is_the_oracles():
    from uwudiff_amd.inception import FIDInceptionV3, layer_table

    assert {n: tuple(s) for n, *s in layer_table()} == {n: tuple(s) for n, s in io.LAYERS.items()}
    model = FIDInceptionV3(device="meta", init_weights=False)
    assert sum(v.numel() for k, v in model.named_tensors() if k.endswith(("conv.weight", "bn.weight", "bn.bias"))) == 21_785_568


def test_state_dict_names_round_trip():
    from uwudiff_amd.inception import FIDInceptionV3

    sd = io.random_state_dict(3, with_fc=True)
    model = FIDInceptionV3(compute_dtype="fp32", init_weights=False)
    res = model.load_state_dict(sd)  # fc.* and num_batches_tracked are accepted and passed over
    assert not res.missing_keys and not res.unexpected_keys
    out = model.state_dict()
    kept = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
    assert sorted(out) == sorted(kept) and len(out) == 94 * 5
    for k, v in kept.items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    assert out["Conv2d_3b_1x1.conv.weight"].shape == (80, 64, 1, 1)  # no padding shows
    assert out["Mixed_5b.branch5x5_2.conv.weight"].shape == (64, 48, 5, 5)
    # the folded operands: tap-major, the stem padded to 32 columns, the stacked 1x1 pair in one matrix
    ow, ob, rows, cols, names = model._ops["Mixed_6b.branch7x7_1"]
    assert (rows, cols) == (256, 768) and names == ("Mixed_6b.branch7x7_1", "Mixed_6b.branch7x7dbl_1")
    name = "Mixed_6b.branch7x7_2"
    ow, ob, rows, cols, _ = model._ops[name]
    scale = sd[name + ".bn.weight"].double() / (sd[name + ".bn.running_var"].double() + 1e-3).sqrt()
    want = (sd[name + ".conv.weight"].double() * scale[:, None, None, None]).permute(0, 2, 3, 1).flatten(1)
    torch.testing.assert_close(model.wf[ow:ow + rows * cols].view(rows, cols).double(), want, rtol=2.0 ** -23, atol=0)
    torch.testing.assert_close(model.bf[ob:ob + rows].double(), sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * scale,
                               rtol=2.0 ** -23, atol=2.0 ** -30)
    ow, _, rows, cols, _ = model._ops["Conv2d_1a_3x3"]
    assert (rows, cols) == (32, 32) and not model.wf[ow:ow + 1024].view(32, 32)[:, 27:].any()
    # missing and unexpected keys are reported; a refused load writes nothing
    before = model.flat.clone()
    short = dict(kept)
    del short["Mixed_7c.branch_pool.bn.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        model.load_state_dict(short)
    with pytest.raises(RuntimeError, match="unexpected"):
        model.load_state_dict(dict(kept, **{"AuxLogits.conv0.conv.weight": torch.zeros(1)}))
    res = model.load_state_dict(short, strict=False)
    assert res.missing_keys == ["Mixed_7c.branch_pool.bn.bias"]
    bad = dict(kept)
    bad["Conv2d_1a_3x3.conv.weight"] = torch.zeros(32, 3, 5, 5)
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(bad)
    assert torch.equal(model.flat, before)


def test_seeded_initialisation_keeps_every_layer_in_range():
    """the checkpoint cannot be fetched: the seeded weights must keep every layer's output rms within [0.1, 10] on structured
    pictures, or the bf16 comparisons of the GPU tests would compare noise"""
    from uwudiff_amd.inception import FIDInceptionV3

    a, b = FIDInceptionV3(compute_dtype="fp32"), FIDInceptionV3(compute_dtype="fp32")
    assert torch.equal(a.flat, b.flat)  # seeded by the checkpoint's name, not by the global seed
    rms = {}
    io.forward(a.state_dict(), io.preprocess(io.pictures(2, 5)), "bf16", rms=rms)
    print({k: round(v, 3) for k, v in rms.items()})
    assert len(rms) == 16 and all(0.1 <= v <= 10 for v in rms.values()), rms
    rms = {}
    io.forward(io.random_state_dict(1), io.preprocess(io.pictures(2, 5)), "bf16", rms=rms)  # the state dict the GPU tests load
    assert all(0.1 <= v <= 10 for v in rms.values()), rms


# ---------------------------------------------------------------------------------------------- the formula and the input rule
def test_fid_formula_on_hand_made_statistics():
    from uwudiff_amd.metrics import frechet_distance, moments_from_sums

    g = torch.Generator().manual_seed(0)
    D = 6
    a = torch.randn(D, D, generator=g, dtype=torch.float64)
    s = a @ a.T + torch.eye(D, dtype=torch.float64)
    mu1, mu2 = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    for f in (frechet_distance, io.fid):  # equal covariances: |dmu|^2
        assert float(f(mu1, s, mu2, s)) == pytest.approx(float((mu1 - mu2).square().sum()), rel=1e-10, abs=1e-10)
    v1, v2 = torch.rand(D, generator=g, dtype=torch.float64) + 0.1, torch.rand(D, generator=g, dtype=torch.float64) + 0.1
    want = float((v1.sqrt() - v2.sqrt()).square().sum() + (mu1 - mu2).square().sum())  # diagonal: sum (sigma1 - sigma2)^2 + |dmu|^2
    for f in (frechet_distance, io.fid):
        assert float(f(mu1, torch.diag(v1), mu2, torch.diag(v2))) == pytest.approx(want, rel=1e-10)
    # the sums the device keeps -> the moments
    x = torch.randn(9, D, generator=g, dtype=torch.float64) + 1
    mean, cov = moments_from_sums(9, x.sum(0), x.T @ x)
    torch.testing.assert_close(mean, x.mean(0))
    torch.testing.assert_close(cov, torch.cov(x.T), rtol=1e-10, atol=1e-12)
    # the oracle's short cut for n << D (the nuclear norm of the cross matrix) is the same number
    r, f = torch.randn(5, 64, generator=g, dtype=torch.float64), torch.randn(7, 64, generator=g, dtype=torch.float64) * 1.5 + 0.2
    assert io.fid_of_features(r, f) == pytest.approx(io.fid(*io.moments(r), *io.moments(f)), rel=1e-6)
    assert float(frechet_distance(*io.moments(r), *io.moments(f))) == pytest.approx(io.fid_of_features(r, f), rel=1e-6)


def test_truncation_rule_at_k_over_255():
    """torchmetrics' ``(imgs * 255).byte()``: the fp32 product is truncated, not rounded.  ToTensor's k / 255 still comes back as k for
    every k (the fp32 product k / 255 * 255 rounds to k exactly), so a PNG read through ToTensor gives the pixel values it holds"""
    k = torch.arange(256)
    x = k.float() / 255
    v = (io.preprocess(x.view(1, 1, 16, 16), normalize=True) * 128 + 128).flatten()
    assert torch.equal(v, (x * 255).to(torch.uint8).double())
    assert torch.equal(v, k.double())
    between = (k[:255].float() + 0.9) / 255  # truncated, not rounded: k + 0.9 is k
    assert torch.equal(io.preprocess(between, normalize=True) * 128 + 128, k[:255].double())
    assert torch.equal(io.preprocess(k.to(torch.uint8)), (k.double() - 128) / 128)
    wild = torch.tensor([-0.5, 1.5, float("nan")])
    assert io.preprocess(wild[:2], normalize=True).tolist() == [-1.0, 127 / 128]
    with pytest.raises(AssertionError):
        io.preprocess(x)  # a float without normalize has no meaning


# ---------------------------------------------------------------------------------------------- transforms, datasets, aliases, launcher
def test_center_crop_matches_pil_crop():
    from PIL import Image

    from uwudiff_amd.transforms import CenterCrop

    g = np.random.default_rng(0)
    for (w, h), size in [((11, 8), 5), ((10, 7), (4, 6)), ((9, 9), 9), ((300, 299), 299)]:
        img = Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8))
        th, tw = (size, size) if isinstance(size, int) else size
        top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
        got = CenterCrop(size)(img)
        assert got.size == (tw, th) and np.array_equal(np.asarray(got), np.asarray(img.crop((left, top, left + tw, top + th))))
    small = Image.fromarray(np.full((4, 6, 3), 200, dtype=np.uint8))
    got = np.asarray(CenterCrop(8)(small))  # a smaller picture is padded with zeros all round
    assert got.shape == (8, 8, 3) and (got[2:6, 1:7] == 200).all() and got.sum() == 200 * 4 * 6 * 3
    with pytest.raises(TypeError):
        CenterCrop(4)(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError):
        CenterCrop((1, 2, 3))


def test_hf_datasets_over_a_list_of_dicts():
    from PIL import Image

    from duwu.data.hf_dataset import HfImageDataset, HfPromptDataset

    src = open(os.path.join(ROOT, "duwu", "data", "hf_dataset.py")).read()
    assert "import datasets" not in src and "from datasets" not in src  # the module itself must not need the package
    rows = [{"image": Image.fromarray(np.full((4, 5), 10 * i, dtype=np.uint8)), "caption": [f"first {i}", f"second {i}"], "pic": None}
            for i in range(3)]
    ds = HfImageDataset(rows)
    assert len(ds) == 3 and ds[2].shape == (3, 4, 5) and torch.equal(ds[2], torch.full((3, 4, 5), 20 / 255))  # an L image is made RGB
    assert HfImageDataset(rows, image_transform=lambda im: im.size)[0] == (5, 4)
    assert list(HfPromptDataset(rows)) == ["first 0", "first 1", "first 2"]
    assert len(HfPromptDataset(rows, all_captions=True)) == 6 and HfPromptDataset(rows, all_captions=True)[1] == "second 0"


def test_aliases_and_the_launchers_fid_node(tmp_path):
    import importlib.util

    import duwu.metrics
    from duwu.data.text_image_local import LocalImageDataset, LocalImageDatasetFromFolder
    from uwudiff_amd import config as C
    from uwudiff_amd import metrics, transforms

    assert C.get_obj_from_str("torchvision.transforms.CenterCrop") is transforms.CenterCrop
    assert C.get_obj_from_str("torchmetrics.image.fid.FrechetInceptionDistance") is metrics.FrechetInceptionDistance
    spec = importlib.util.spec_from_file_location("launcher_test_metrics_fid", os.path.join(ROOT, "test_scripts", "test_metrics.py"))
    launcher = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launcher)
    from PIL import Image

    Image.fromarray(np.zeros((320, 400, 3), dtype=np.uint8)).save(tmp_path / "r.png")
    cfg = C.load_yaml(os.path.join(ROOT, "configs", "demo_metrics_fid.yaml"))
    assert [m["name"] for m in cfg.metrics] == ["FID"]
    node = cfg.metrics[0]
    node["ref_dataset"]["image_dir"] = str(tmp_path)
    mc = launcher.metric_config(node)
    assert isinstance(mc, duwu.metrics.MetricConfig) and mc.name == "FID"
    assert mc.metric_func.func is duwu.metrics.compute_fid and mc.metric_func.keywords == {"batch_size": 1024, "normalize": True}
    assert mc.generated_dataset_func.func is LocalImageDataset
    assert isinstance(mc.ref_dataset, LocalImageDatasetFromFolder) and len(mc.ref_dataset) == 1  # the node is instantiated
    kinds = [type(t) for t in mc.ref_dataset.image_transform.transforms]
    assert kinds == [transforms.Resize, transforms.CenterCrop, transforms.ToTensor]
    assert mc.ref_dataset[0].shape == (3, 299, 299)  # Resize(299) on the shorter side, then the centre
    assert mc.generated_dataset_func([str(tmp_path / "r.png")])[0].shape == (3, 299, 299)


# ---------------------------------------------------------------------------------------------- refusals
def test_wrong_size_is_refused_before_anything_is_loaded(monkeypatch):
    import duwu.metrics.fid as fid_mod
    from uwudiff_amd import lib as L

    def boom(*a, **k):
        raise AssertionError("the refusal must come first")

    monkeypatch.setattr(fid_mod, "FrechetInceptionDistance", boom)
    monkeypatch.setattr(L, "load", boom)
    for gen, ref in [([torch.zeros(3, 8, 8)], [torch.zeros(3, 299, 299)]), ([torch.zeros(3, 299, 299)], [torch.zeros(3, 299, 298)]),
                     ([torch.zeros(1, 299, 299)], [torch.zeros(3, 299, 299)])]:
        with pytest.raises(NotImplementedError, match="InceptionV3 resize.*dataset transform"):
            fid_mod.compute_fid(gen, ref, device="cuda")


def test_metric_refusals():
    from uwudiff_amd import lib as L
    from uwudiff_amd.metrics import FrechetInceptionDistance as FID

    for feature in (64, 192, 768, 2047, "2048"):
        with pytest.raises(NotImplementedError, match="feature="):
            FID(feature=feature)
    with pytest.raises(NotImplementedError, match="module as `feature`"):
        FID(feature=torch.nn.Identity())
    with pytest.raises(NotImplementedError, match="dist_sync_on_step"):
        FID(dist_sync_on_step=True)
    with pytest.raises(NotImplementedError, match="InceptionV3 resize"):
        FID(input_img_size=(3, 256, 256))
    with pytest.raises(ValueError, match="compute_dtype"):
        FID(compute_dtype="fp16")
    m = FID(compute_dtype="fp32")
    u8 = torch.zeros(2, 3, 299, 299, dtype=torch.uint8)
    with pytest.raises(ValueError, match="normalize=True"):
        m.update(u8.float(), real=True)  # a float under normalize=False
    with pytest.raises(NotImplementedError, match="InceptionV3 resize"):
        m.update(torch.zeros(2, 3, 64, 64, dtype=torch.uint8), real=True)
    with pytest.raises(TypeError):
        m.update([u8[0]], real=True)
    with pytest.raises(L.UwuError, match="HIP device only"):
        m.update(u8, real=True)
    with pytest.raises(RuntimeError, match="more than one sample"):
        m.compute()
    n = FID(normalize=True, compute_dtype="fp32")
    with pytest.raises(L.UwuError, match="HIP device only"):
        n.update(u8.float(), real=False)
    assert sorted(m.state_dict()) == sorted("inception." + k for k in m.inception.state_dict())


def test_feature_extractor_weights_path(tmp_path):
    from uwudiff_amd.metrics import FrechetInceptionDistance as FID

    sd = io.random_state_dict(9, with_fc=True)
    torch.save(sd, tmp_path / "pt_inception.pth")
    m = FID(feature_extractor_weights_path=str(tmp_path / "pt_inception.pth"), compute_dtype="fp32")
    assert torch.equal(m.inception.state_dict()["Mixed_7c.branch1x1.conv.weight"], sd["Mixed_7c.branch1x1.conv.weight"])
