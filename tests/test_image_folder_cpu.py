"""CPU: the folder training set and everything under it that needs no GPU.

  tests/pil_resample_oracle.py  equals Image.resize byte for byte (three filters, eight shape pairs, a noise and a ramp picture)
  uwu_resample_coeffs           (host-only, through ctypes) gives exactly the oracle's coefficients, bounds and ksize
  resize_and_crop_image         equals a PIL + torch restatement written here; the order of its random draws; its 256 values
  LocalTextImageTrainDataset    items, add_time_ids, picture modes, the missing caption, both collates, one seed -> the same plans
  wiring                        the config's dataset node, the export, Resize's default
"""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_oracle as O
from tests.conftest import ROOT

PIL_FILTER = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
# (h, w) -> (h, w): downscale, mixed, one axis skipped, upscale, a large one, long tap loops, nothing to do, a pure upscale
SHAPES = [((37, 53), (16, 16)), ((300, 200), (64, 96)), ((64, 64), (64, 33)), ((20, 31), (64, 99)), ((513, 770), (256, 385)),
          ((1000, 17), (32, 32)), ((33, 33), (33, 33)), ((8, 8), (64, 64))]


def noise(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7 % 256)], axis=2).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the oracle against PIL
@pytest.mark.parametrize("filt", list(PIL_FILTER))
@pytest.mark.parametrize("src,dst", SHAPES)
def test_oracle_equals_pil(src, dst, filt):
    for img in (noise(*src), ramp(*src)):
        ref = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), PIL_FILTER[filt]))
        got = O.resize(img, (dst[1], dst[0]), filt)
        assert got.shape == ref.shape and np.array_equal(got, ref), int((got != ref).sum())


def test_oracle_window_equals_the_crop_of_the_full_resize():
    img = noise(300, 200)
    for filt in PIL_FILTER:
        full = O.resize(img, (96, 144), filt)
        for left, top in ((0, 0), (32, 80), (13, 41)):
            assert np.array_equal(O.resize_crop(img, (96, 144), (left, top), (64, 64), filt), full[top:top + 64, left:left + 64])


# ---------------------------------------------------------------------------------------------- host coefficients
@pytest.mark.parametrize("filt", list(PIL_FILTER))
@pytest.mark.parametrize("src,dst", SHAPES)
def test_host_coefficients_equal_the_oracle(src, dst, filt):
    from uwudiff_amd import preprocess as P

    for in_size, out_size in zip(src, dst):
        K, bounds, ksize = O.coeffs(in_size, out_size, filt)
        assert P.resample_ksize(in_size, out_size, filt) == ksize
        c, b = P.resample_coeffs(in_size, out_size, filt)
        assert c.dtype == np.int32 and c.shape == (out_size, ksize) and np.array_equal(c, K)
        assert b.dtype == np.int32 and np.array_equal(b, bounds)
        first, count = out_size // 3, max(1, out_size // 2)  # a strict sub-range
        assert 0 < first and first + count < out_size
        c, b = P.resample_coeffs(in_size, out_size, filt, first, count)
        assert np.array_equal(c, K[first:first + count]) and np.array_equal(b, bounds[first:first + count])


def test_host_coefficients_refuse_bad_arguments():
    from uwudiff_amd import lib as L
    from uwudiff_amd import preprocess as P

    for kw in (dict(in_size=0), dict(out_size=0), dict(first=-1), dict(first=10, count=7), dict(count=0)):
        args = {"in_size": 40, "out_size": 16, "first": 0, "count": 16, **kw}
        with pytest.raises(L.UwuError, match="resample"):
            P.resample_coeffs(args["in_size"], args["out_size"], "lanczos", args["first"], args["count"])
    with pytest.raises(L.UwuError, match="filter"):
        L.call("uwu_resample_ksize", 40, 16, 5)


# ---------------------------------------------------------------------------------------------- resize_and_crop_image
def _restated(image, target_size, top_left=None):
    """utils.py:25-58 with PIL and torch only; top_left None: the centre crop"""
    scale = max(target_size[0] / image.width, target_size[1] / image.height)
    new_size = (math.ceil(image.width * scale), math.ceil(image.height * scale))
    t = torch.from_numpy(np.asarray(image.resize(new_size, Image.LANCZOS)).copy()).permute(2, 0, 1).float().div(255)
    crop_y, crop_x = new_size[1] - target_size[1], new_size[0] - target_size[0]
    top, left = (crop_y // 2, crop_x // 2) if top_left is None else top_left
    t = t[:, top:top + target_size[1], left:left + target_size[0]]
    mean = std = torch.tensor([0.5, 0.5, 0.5]).view(3, 1, 1)
    return t.sub(mean).div(std), new_size, (left, top)


@pytest.mark.parametrize("wh,target", [((53, 37), (16, 16)), ((200, 300), (96, 64)), ((31, 20), (64, 64)), ((64, 64), (64, 64)),
                                       ((770, 513), (96, 64))])
def test_resize_and_crop_image_equals_its_restatement(wh, target):
    from duwu.data.utils import plan_resize_and_crop, resize_and_crop_image

    image = Image.fromarray(noise(wh[1], wh[0]))
    got, new_size, lt = resize_and_crop_image(image, target, random_crop=False)
    ref, ref_size, ref_lt = _restated(image, target)
    assert got.dtype == torch.float32 and got.shape == (3, target[1], target[0])
    assert new_size == ref_size and lt == ref_lt and torch.equal(got, ref)
    assert lt == ((new_size[0] - target[0]) // 2, (new_size[1] - target[1]) // 2)  # centred
    assert plan_resize_and_crop(wh[0], wh[1], target, random_crop=False) == (new_size, lt)
    # random: top is drawn first, then left
    for seed in (0, 7):
        np.random.seed(seed)
        top = np.random.randint(0, new_size[1] - target[1] + 1)
        left = np.random.randint(0, new_size[0] - target[0] + 1)
        after = np.random.randint(0, 1 << 30)
        np.random.seed(seed)
        got, _, lt = resize_and_crop_image(image, target, random_crop=True)
        assert lt == (left, top) and np.random.randint(0, 1 << 30) == after  # (two draws, no more)
        assert torch.equal(got, _restated(image, target, (top, left))[0])
        np.random.seed(seed)
        assert plan_resize_and_crop(wh[0], wh[1], target, random_crop=True) == (new_size, (left, top))


def test_the_256_normalised_values_equal_torchs_chain():
    from duwu.data.utils import resize_and_crop_image

    a = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got, new_size, lt = resize_and_crop_image(Image.fromarray(np.stack([a, a, a], axis=2)), (16, 16), random_crop=False)
    chain = (torch.arange(256, dtype=torch.uint8).float().div(255) - 0.5) / 0.5
    assert new_size == (16, 16) and lt == (0, 0)
    for c in range(3):
        assert torch.equal(got[c].reshape(-1), chain)
    naive = torch.arange(256).float() * (2 / 255) - 1
    assert int((naive != chain).sum()) > 0  # the shortcut is a different function: the kernels take the chain


# ---------------------------------------------------------------------------------------------- the dataset
FILES = [("land.png", "RGB", (80, 48)), ("port.png", "RGB", (40, 90)), ("small.png", "RGB", (20, 12)), ("grey.png", "L", (50, 50)),
         ("alpha.png", "RGBA", (33, 47)), ("pal.png", "P", (64, 40)), ("sub/deep.png", "RGB", (70, 70))]  # (w, h)


def write_folder(root, files=FILES):
    paths = []
    for i, (name, mode, (w, h)) in enumerate(files):
        img = Image.fromarray(noise(h, w, seed=i))
        if mode == "RGBA":
            img.putalpha(Image.fromarray(noise(h, w, seed=99)[:, :, 0]))
        elif mode == "P":
            img = img.quantize(32)
        else:
            img = img.convert(mode)
        p = os.path.join(str(root), name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        img.save(p)
        with open(os.path.splitext(p)[0] + ".txt", "w") as f:
            f.write(f"  caption of {name}\n\n")
        paths.append(p)
    return paths


class _Tok:
    def __call__(self, text, padding=None, truncation=None, return_tensors=None):
        ids = torch.tensor([[len(text), 1, 2, 0]])
        return {"input_ids": ids, "attention_mask": (ids != 0).long()}


@pytest.mark.parametrize("on_device", [False, True], ids=["cpu", "device"])
def test_dataset_items(tmp_path, on_device):
    from duwu.data import LocalTextImageTrainDataset, UwUBaseDataset
    from duwu.data.utils import resize_and_crop_image

    paths = write_folder(tmp_path)
    ds = LocalTextImageTrainDataset(image_dir=str(tmp_path), target_size=(32, 24), random_crop=False, resize_on_device=on_device,
                                    tokenizers=[_Tok()])
    assert isinstance(ds, UwUBaseDataset) and len(ds) == len(FILES) and sorted(ds.image_paths) == sorted(paths)
    by_path = LocalTextImageTrainDataset(image_paths=paths, target_size=(32, 24), random_crop=False, resize_on_device=on_device)
    assert by_path.image_paths == paths and by_path.tokenizers == []
    for i, (name, mode, (w, h)) in enumerate(FILES):
        item = by_path[i]
        assert sorted(item) == ["add_time_ids", "caption", "sample", "tokenizer_out"]  # DummyDataset's keys
        assert item["caption"] == f"caption of {name}" and item["tokenizer_out"] == []
        rgb = Image.open(paths[i]).convert("RGB")
        ref, new_size, (left, top) = resize_and_crop_image(rgb, (32, 24), random_crop=False)
        # the file's own size, the crop's offset in the resized picture, the target: (h, w) pairs
        assert item["add_time_ids"].tolist() == [h, w, top, left, 24, 32]
        if on_device:
            assert item["sample"]["plan"] == (new_size, (left, top))
            assert item["sample"]["image"].dtype == torch.uint8 and item["sample"]["image"].shape == (h, w, 3)
            assert np.array_equal(item["sample"]["image"].numpy(), np.asarray(rgb))
        else:
            assert item["sample"].shape == (3, 24, 32) and torch.equal(item["sample"], ref)
    assert len(ds[0]["tokenizer_out"]) == 1


def test_add_time_ids_of_landscape_portrait_and_small(tmp_path):
    from duwu.data import LocalTextImageTrainDataset

    paths = write_folder(tmp_path, FILES[:3])
    ds = LocalTextImageTrainDataset(image_paths=paths, target_size=(32, 32), random_crop=False)
    # 80 x 48 -> 54 x 32 (ceil(53.3)), centred: left 11; 40 x 90 -> 32 x 72: top 20; 20 x 12 -> 54 x 32 (upscaled): left 11
    assert [ds[i]["add_time_ids"].tolist() for i in range(3)] == [[48, 80, 0, 11, 32, 32], [90, 40, 20, 0, 32, 32], [12, 20, 0, 11, 32, 32]]


def test_missing_caption_names_the_path(tmp_path):
    from duwu.data import LocalTextImageTrainDataset

    paths = write_folder(tmp_path, FILES[:2])
    os.remove(os.path.splitext(paths[1])[0] + ".txt")
    ds = LocalTextImageTrainDataset(image_dir=str(tmp_path))
    i = ds.image_paths.index(paths[1])
    with pytest.raises(FileNotFoundError, match="port"):
        ds[i]
    with pytest.raises(ValueError):
        LocalTextImageTrainDataset()
    with pytest.raises(ValueError):
        LocalTextImageTrainDataset(image_dir=str(tmp_path), filter="box")


def test_both_collates_and_one_seed_gives_both_modes_the_same_plans(tmp_path):
    from duwu.data import LocalTextImageTrainDataset, UwUBaseDataset
    from uwudiff_amd.preprocess import RaggedImages

    paths = write_folder(tmp_path)
    kw = dict(image_paths=paths, target_size=(32, 24), random_crop=True, tokenizers=[_Tok(), _Tok()])
    cpu = LocalTextImageTrainDataset(resize_on_device=False, **kw)
    dev = LocalTextImageTrainDataset(resize_on_device=True, **kw)
    np.random.seed(5)
    a = cpu.collate([cpu[i] for i in range(len(paths))])
    np.random.seed(5)
    b = dev.collate([dev[i] for i in range(len(paths))])
    # the CPU mode is the inherited collate
    np.random.seed(5)
    again = UwUBaseDataset.collate([cpu[i] for i in range(len(paths))])
    assert torch.equal(a[0], again[0]) and a[0].shape == (len(paths), 3, 24, 32) and a[0].dtype == torch.float32
    # the other four slots are the same in both modes
    assert a[1] == b[1] == [f"caption of {name}" for name, _, _ in FILES]
    assert len(a[2]) == len(b[2]) == 2
    for ta, tb in zip(a[2], b[2]):
        assert ta["input_ids"].shape == (len(paths), 4) and torch.equal(ta["input_ids"], tb["input_ids"])
        assert torch.equal(ta["attention_mask"], tb["attention_mask"])
    assert a[3]["time_ids"].dtype == torch.float32 and torch.equal(a[3]["time_ids"], b[3]["time_ids"]) and a[4] == b[4] == {}
    # the ragged batch describes the files
    r = b[0]
    assert isinstance(r, RaggedImages) and len(r) == len(paths) and r.target_size == (32, 24) and r.filter == "lanczos" and r.normalize
    assert r.data.dtype == torch.uint8 and r.offsets.dtype == torch.int64 and r.meta.dtype == torch.int32 and r.meta.shape == (len(paths), 6)
    at = 0
    for i, (name, mode, (w, h)) in enumerate(FILES):
        assert int(r.offsets[i]) == at
        rgb = np.asarray(Image.open(paths[i]).convert("RGB"))
        assert np.array_equal(r.data[at:at + h * w * 3].numpy().reshape(h, w, 3), rgb)
        at += h * w * 3
        sh, sw, nh, nw, top, left = r.meta[i].tolist()
        scale = max(32 / w, 24 / h)
        assert (sh, sw, nh, nw) == (h, w, math.ceil(h * scale), math.ceil(w * scale))
        assert [h, w, top, left, 24, 32] == a[3]["time_ids"][i].tolist()  # the plan the CPU mode drew
    assert at == r.data.numel()
    assert any(int(r.meta[i, 4]) or int(r.meta[i, 5]) for i in range(len(paths)))  # (some crop is off the corner)


# ---------------------------------------------------------------------------------------------- wiring
def test_config_node_export_and_resize_default(tmp_path):
    import importlib.util

    import duwu.data
    from duwu.data.utils import BicubicResize
    from duwu.loader import load_any
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.transforms import Resize

    spec = importlib.util.spec_from_file_location("make_demo_folder", os.path.join(ROOT, "tools", "make_demo_folder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    paths = tool.make(str(tmp_path / "demo"), n=12, seed=3)
    assert len(paths) == 12 and {Image.open(p).mode for p in paths} >= {"RGB", "L", "RGBA", "P"}

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_folder.yaml"))
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_pixels.yaml"))
    node = dict(cfg.data.dataset_config)
    assert node["_target_"] == "duwu.data.LocalTextImageTrainDataset" and node["image_dir"] == "data/demo_folder"
    assert cfg.trainer == base.trainer and cfg.lightning_config == base.lightning_config  # only the dataset node differs
    assert cfg.data.dataloader_config == base.data.dataloader_config
    ds = load_any({**node, "image_dir": str(tmp_path / "demo")})
    assert isinstance(ds, duwu.data.LocalTextImageTrainDataset) and len(ds) == 12
    assert ds.target_size == (256, 256) and ds.random_crop and ds.resize_on_device and ds.filter == "lanczos"
    item = ds[0]
    assert item["sample"]["image"].dtype == torch.uint8 and item["add_time_ids"].tolist()[4:] == [256, 256]

    img = Image.fromarray(noise(40, 60))
    assert Resize((20, 30)).interpolation == Image.BILINEAR
    assert np.array_equal(np.asarray(Resize((20, 30))(img)), np.asarray(img.resize((30, 20), Image.BILINEAR)))
    assert np.array_equal(np.asarray(Resize((20, 30), interpolation="bicubic")(img)), np.asarray(img.resize((30, 20), Image.BICUBIC)))
    assert np.array_equal(np.asarray(BicubicResize(20)(img)), np.asarray(img.resize((30, 20), Image.BICUBIC)))
