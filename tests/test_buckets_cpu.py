"""CPU: aspect-ratio buckets -- the bucket list, the assignment, the batch sampler, the folder dataset and the data
module with buckets -- and the host-only query of the attention route (``uwu_attention_route``), which says where a ragged query
count runs."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.conftest import ROOT

# the head widths whose ragged-query (QTAIL) kernels are shipped: at 72 and 128 the guarded dK / dV kernel needs scratch memory
# and is not built, so ragged query counts of those widths stay off the MFMA route
QTAIL_WIDTHS = (40, 64, 80)
MFMA_WIDTHS = (40, 64, 72, 80, 128)


# ---------------------------------------------------------------------------------------------- the route query
def route(T, d, Tk=None, ld=None, dtype=torch.bfloat16, backward=False):
    from uwudiff_amd import ops

    ld = d if ld is None else ld
    return ops.attention_route(T, T if Tk is None else Tk, d, ld, ld, ld, ld, dtype=dtype, backward=backward)


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_attention_route(backward):
    from uwudiff_amd import lib as L

    assert hasattr(L.load(), "uwu_attention_route")
    for T in (320, 4096):
        for d in MFMA_WIDTHS:
            assert route(T, d, backward=backward) is True, (T, d)
            assert route(T, d, Tk=77, ld=3 * 8 * d, backward=backward) is True, (T, d)
    for d in MFMA_WIDTHS:
        assert route(100, d, backward=backward) is False and route(16, d, backward=backward) is False
    for T in (64, 256, 320, 300, 3952):
        assert route(T, 160, backward=backward) is False                       # no MFMA kernel of that width
        assert route(T, 64, dtype=torch.float32, backward=backward) is False   # fp32
        assert route(T, 64, ld=196, backward=backward) is False                # a stride that is no multiple of 8
    for T in (257, 300, 3952, 988):
        for d in MFMA_WIDTHS:
            assert route(T, d, backward=backward) is (d in QTAIL_WIDTHS), (T, d)
            assert route(T, d, Tk=77, backward=backward) is (d in QTAIL_WIDTHS), (T, d)
    # up to 256 queries nothing changes: whole 64-row tiles only
    for T in range(1, 257):
        for d in MFMA_WIDTHS:
            assert route(T, d, backward=backward) is (T % 64 == 0), (T, d)
    # the C entry point itself: pass, Tq, Tk, d, four strides, dtype
    lib = L.load()
    assert lib.uwu_attention_route(int(backward), 3952, 3952, 64, 1920, 1920, 1920, 640, L.BF16) == 1
    assert lib.uwu_attention_route(int(backward), 3952, 3952, 64, 1920, 1920, 1920, 640, L.F32) == 0
    assert lib.uwu_attention_route(int(backward), 0, 64, 64, 64, 64, 64, 64, L.BF16) == 0


# ---------------------------------------------------------------------------------------------- make_buckets / assign_bucket
def test_make_buckets_defaults():
    from duwu.data.utils import make_buckets

    b = make_buckets()
    for pair in ((1024, 1024), (832, 1216), (1216, 832), (512, 2048)):
        assert pair in b
    for kw in (dict(), dict(resolution=256, min_side=128, max_side=512, step=64), dict(resolution=128, min_side=64, max_side=256),
               dict(resolution=512, min_side=256, max_side=1024, step=128)):
        b = make_buckets(**kw)
        res, lo, hi, step = kw.get("resolution", 1024), kw.get("min_side", 512), kw.get("max_side", 2048), kw.get("step", 64)
        assert b and all(isinstance(p, tuple) and len(p) == 2 for p in b)
        for w, h in b:
            assert w % step == 0 and h % step == 0 and lo <= w <= hi and lo <= h <= hi and w * h <= res * res, (w, h)
            assert (h, w) in b
        assert len(set(b)) == len(b)
        assert b == sorted(b, key=lambda p: (p[0] / p[1], p[0]))
    assert make_buckets(256, 128, 512, 64) == [(128, 512), (128, 448), (128, 384), (192, 320), (256, 256), (320, 192), (384, 128),
                                               (448, 128), (512, 128)]
    for bad in (32, 96, 0, -64):
        with pytest.raises(ValueError, match="64"):
            make_buckets(step=bad)


def test_assign_bucket():
    from duwu.data.utils import assign_bucket, make_buckets

    b = make_buckets()
    land, port = b[assign_bucket(3000, 2000, b)], b[assign_bucket(2000, 3000, b)]
    assert land == (port[1], port[0]) and land[0] > land[1]
    assert land == (1216, 832)  # log(1216 / 832) = 0.379 is nearer to log(1.5) = 0.405 than 1280 / 768 (0.511) or 1152 / 896 (0.251)
    assert b[assign_bucket(640, 640, b)] == (1024, 1024)
    assert b[assign_bucket(10000, 100, b)] == (2048, 512) and b[assign_bucket(100, 10000, b)] == (512, 2048)
    # every bucket is its own nearest
    assert [assign_bucket(w, h, b) for w, h in b] == list(range(len(b)))
    # a tie: the lower index (a square picture between two mirrored buckets; duplicates)
    assert assign_bucket(100, 100, [(128, 256), (256, 128)]) == 0 and assign_bucket(100, 100, [(256, 128), (128, 256)]) == 0
    assert assign_bucket(50, 70, [(64, 64), (64, 64), (128, 128)]) == 0
    with pytest.raises(ValueError):
        assign_bucket(0, 10, b)
    with pytest.raises(ValueError):
        assign_bucket(10, 10, [])


# ---------------------------------------------------------------------------------------------- the sampler
BUCKET_OF = [2, 0, 0, 2, 1, 0, 2, 2, 0, 0, 2, 0, 2, 5]  # bucket 0: 6 indices, 1: 1, 2: 6, 5: 1 (3 and 4 are empty)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [1, 4, 6, 7])
def test_sampler_batches_hold_one_bucket(shuffle, drop_last, batch_size):
    from duwu.data.utils import BucketBatchSampler

    s = BucketBatchSampler(BUCKET_OF, batch_size, shuffle, drop_last)
    torch.manual_seed(3)
    batches = list(s)
    assert len(batches) == len(s)
    counts = {b: BUCKET_OF.count(b) for b in set(BUCKET_OF)}
    want = sum(n // batch_size if drop_last else math.ceil(n / batch_size) for n in counts.values())
    assert len(s) == want
    seen = [i for batch in batches for i in batch]
    assert len(seen) == len(set(seen))
    for batch in batches:
        assert 1 <= len(batch) <= batch_size and len({BUCKET_OF[i] for i in batch}) == 1
        if drop_last:
            assert len(batch) == batch_size
    if not drop_last:
        assert sorted(seen) == list(range(len(BUCKET_OF)))  # every index once per epoch
    else:
        assert len(seen) == sum(n // batch_size * batch_size for n in counts.values())


def test_sampler_order_and_seed():
    from duwu.data.utils import BucketBatchSampler

    s = BucketBatchSampler(BUCKET_OF, 4, shuffle=False, drop_last=False)
    want = [[1, 2, 5, 8], [9, 11], [4], [0, 3, 6, 7], [10, 12], [13]]  # buckets in index order, indices ascending
    assert list(s) == want and list(s) == want
    assert list(BucketBatchSampler(BUCKET_OF, 4, shuffle=False, drop_last=True)) == [[1, 2, 5, 8], [0, 3, 6, 7]]
    s = BucketBatchSampler(BUCKET_OF, 2, shuffle=True)
    torch.manual_seed(7)
    a, b = list(s), list(s)
    torch.manual_seed(7)
    a2, b2 = list(s), list(s)
    assert a == a2 and b == b2  # torch's global CPU generator governs it
    assert a != b               # two epochs differ
    with pytest.raises(ValueError):
        BucketBatchSampler(BUCKET_OF, 0)


# ---------------------------------------------------------------------------------------------- the dataset and the data module
FILES = [("wide.png", (90, 30)), ("land.png", (80, 52)), ("square.png", (40, 40)), ("port.png", (36, 70)), ("tall.png", (20, 66)),
         ("land2.png", (120, 81))]  # (w, h): five sizes in five buckets, and a second landscape
BUCKETS = dict(resolution=64, min_side=64, max_side=128, step=64)  # (64, 64) only ...
BUCKET_LIST = [[32, 96], [48, 80], [64, 64], [80, 48], [96, 32]]  # ... so the dataset tests give the list


def write_folder(root, files=FILES):
    paths = []
    for i, (name, (w, h)) in enumerate(files):
        rng = np.random.default_rng(100 + i)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(str(root), name))
        with open(os.path.join(str(root), os.path.splitext(name)[0] + ".txt"), "w") as f:
            f.write(f"caption of {name}\n")
        paths.append(os.path.join(str(root), name))
    return paths


EXPECTED_BUCKET = [4, 3, 2, 1, 0, 3]


@pytest.mark.parametrize("on_device", [False, True], ids=["cpu", "device"])
def test_dataset_with_buckets(tmp_path, on_device):
    from duwu.data import LocalTextImageTrainDataset
    from duwu.data.utils import resize_and_crop_image
    from uwudiff_amd.preprocess import RaggedImages

    paths = write_folder(tmp_path)
    ds = LocalTextImageTrainDataset(image_paths=paths, target_size=(64, 64), random_crop=False, resize_on_device=on_device,
                                    buckets=BUCKET_LIST)
    assert ds.buckets == [tuple(b) for b in BUCKET_LIST] and ds.bucket_of == EXPECTED_BUCKET
    for i, (name, (w, h)) in enumerate(FILES):
        bw, bh = BUCKET_LIST[EXPECTED_BUCKET[i]]
        item = ds[i]
        ref, new_size, (left, top) = resize_and_crop_image(Image.open(paths[i]).convert("RGB"), (bw, bh), random_crop=False)
        assert item["add_time_ids"].tolist() == [h, w, top, left, bh, bw]
        if on_device:
            assert item["sample"]["plan"] == (new_size, (left, top)) and item["sample"]["image"].shape == (h, w, 3)
        else:
            assert item["sample"].shape == (3, bh, bw) and torch.equal(item["sample"], ref)
    # a batch of one bucket collates to that bucket's shape; a mixed one is refused
    out = ds.collate([ds[1], ds[5]])
    if on_device:
        assert isinstance(out[0], RaggedImages) and out[0].target_size == (80, 48) and len(out[0]) == 2
    else:
        assert out[0].shape == (2, 3, 48, 80)
    assert out[3]["time_ids"][:, 4:].tolist() == [[48.0, 80.0]] * 2
    with pytest.raises(ValueError, match="bucket"):
        ds.collate([ds[0], ds[1]])
    # the mapping form is make_buckets' arguments
    by_map = LocalTextImageTrainDataset(image_paths=paths, resize_on_device=on_device, buckets=BUCKETS)
    assert by_map.buckets == [(64, 64)] and by_map.bucket_of == [0] * len(paths)
    s = ds.batch_sampler(2, shuffle=False, drop_last=False)
    assert list(s) == [[4], [3], [2], [1, 5], [0]] and len(s) == 5


@pytest.mark.parametrize("on_device", [False, True], ids=["cpu", "device"])
def test_data_module_yields_batches_of_per_bucket_shape(tmp_path, on_device):
    from duwu.data import TrainDataModule

    write_folder(tmp_path)
    node = {"_target_": "duwu.data.LocalTextImageTrainDataset", "image_dir": str(tmp_path), "target_size": [64, 64],
            "random_crop": True, "resize_on_device": on_device, "buckets": BUCKET_LIST}
    dm = TrainDataModule(node, {"batch_size": 2, "shuffle": True, "drop_last": False, "num_workers": 3}, val_dataset_config=node)
    dm.setup("fit")
    for loader, n_batches in ((dm.train_dataloader(), 5), (dm.val_dataloader(), 5)):
        assert len(loader) == n_batches
        torch.manual_seed(1)
        shapes, n = set(), 0
        for x, captions, tok, added, ca in loader:
            hw = added["time_ids"][:, 4:].tolist()
            assert all(v == hw[0] for v in hw)
            h, w = int(hw[0][0]), int(hw[0][1])
            if on_device:
                assert x.target_size == (w, h) and len(x) == len(captions)
            else:
                assert x.shape == (len(captions), 3, h, w)
            shapes.add((w, h))
            n += len(captions)
        assert n == len(FILES) and shapes == {tuple(b) for b in BUCKET_LIST}  # shapes stay target_size without the feature
    # the dataset without buckets goes through the loader as before
    plain = TrainDataModule({k: v for k, v in node.items() if k != "buckets"}, {"batch_size": 4})
    plain.setup("fit")
    sizes = [len(b[1]) for b in plain.train_dataloader()]
    assert sizes == [4, 2]


@pytest.mark.parametrize("on_device", [False, True], ids=["cpu", "device"])
def test_buckets_none_gives_the_items_of_before(tmp_path, on_device):
    from duwu.data import LocalTextImageTrainDataset

    paths = write_folder(tmp_path)
    kw = dict(image_paths=paths, target_size=(48, 32), random_crop=True, resize_on_device=on_device)
    a, b = LocalTextImageTrainDataset(**kw), LocalTextImageTrainDataset(buckets=None, **kw)
    assert b.buckets is None and b.bucket_of is None
    with pytest.raises(ValueError):
        b.batch_sampler(2)
    np.random.seed(9)
    ia = [a[i] for i in range(len(paths))]
    np.random.seed(9)
    ib = [b[i] for i in range(len(paths))]
    for x, y, (name, (w, h)) in zip(ia, ib, FILES):
        assert x["add_time_ids"].tolist() == y["add_time_ids"].tolist() and x["add_time_ids"].tolist()[4:] == [32, 48]
        assert x["add_time_ids"].tolist()[:2] == [h, w] and x["caption"] == y["caption"]
        if on_device:
            assert x["sample"]["plan"] == y["sample"]["plan"] and torch.equal(x["sample"]["image"], y["sample"]["image"])
        else:
            assert x["sample"].shape == (3, 32, 48) and torch.equal(x["sample"], y["sample"])
    ca, cb = a.collate(ia), b.collate(ib)
    assert torch.equal(ca[3]["time_ids"], cb[3]["time_ids"])
    if on_device:
        assert ca[0].target_size == cb[0].target_size == (48, 32) and torch.equal(ca[0].meta, cb[0].meta)
    else:
        assert torch.equal(ca[0], cb[0])


def test_demo_buckets_config_loads(tmp_path):
    import importlib.util

    from duwu.data.utils import make_buckets
    from duwu.loader import load_any
    from uwudiff_amd.config import load_yaml

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_buckets.yaml"))
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_folder.yaml"))
    node = dict(cfg.data.dataset_config)
    assert dict(node["buckets"]) == dict(resolution=256, min_side=128, max_side=512, step=64)
    assert {k: v for k, v in node.items() if k != "buckets"} == dict(base.data.dataset_config)  # only the buckets node differs
    assert cfg.trainer == base.trainer and cfg.lightning_config == base.lightning_config
    assert cfg.data.dataloader_config == base.data.dataloader_config
    spec = importlib.util.spec_from_file_location("make_demo_folder", os.path.join(ROOT, "tools", "make_demo_folder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.make(str(tmp_path / "demo"), n=12, seed=3)
    ds = load_any({**node, "image_dir": str(tmp_path / "demo")})
    assert ds.buckets == make_buckets(256, 128, 512, 64) and len(ds.bucket_of) == 12
    assert len(set(ds.bucket_of)) >= 2  # the demo folder holds mixed sizes
    i = ds.bucket_of.index(max(ds.bucket_of))
    bw, bh = ds.buckets[ds.bucket_of[i]]
    assert ds[i]["add_time_ids"].tolist()[4:] == [bh, bw]
