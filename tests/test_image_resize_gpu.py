"""GPU: uwu_image_resize_crop against tests/pil_resample_oracle.py (which tests/test_image_folder_cpu.py holds to Image.resize byte
for byte) -- every comparison is torch.equal, the kernels are integer arithmetic after the host-made tables -- and the folder
training set through Fitter._to_device and two training steps, device mode against CPU mode."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import pil_resample_oracle as O
from tests.conftest import ROOT
from tests.test_image_folder_cpu import noise, write_folder

pytestmark = pytest.mark.gpu
FILTERS = ["lanczos", "bicubic", "bilinear"]
F32_NAN = 0x7FC00001  # a sentinel bit pattern for memory no kernel may touch
TO_TENSOR = torch.arange(256, dtype=torch.uint8).float().div(255)  # torch's own chains for the 256 levels, on the CPU
NORMALIZED = (TO_TENSOR - 0.5) / 0.5
RAGGED = [(37, 53), (300, 200), (20, 31), (64, 64), (513, 770)]  # (h, w)


def plan(h, w, target, where):
    """resize_and_crop_image's sizes for target = (Wt, Ht); where: 'centre', 'origin' or 'far' (the largest offset)"""
    scale = max(target[0] / w, target[1] / h)
    nw, nh = math.ceil(w * scale), math.ceil(h * scale)
    cx, cy = nw - target[0], nh - target[1]
    left, top = {"centre": (cx // 2, cy // 2), "origin": (0, 0), "far": (cx, cy)}[where]
    return [h, w, nh, nw, top, left]


@functools.lru_cache(maxsize=None)
def expected_u8(h, w, meta, target, filt):
    """the window's bytes [Ht, Wt, 3], computed once per case and shared"""
    _, _, nh, nw, top, left = meta
    return torch.from_numpy(O.resize_crop(noise(h, w), (nw, nh), (left, top), target, filt))


def expected(metas, target, filt, table=NORMALIZED):
    return torch.stack([table[expected_u8(m[0], m[1], tuple(m), target, filt).long()].permute(2, 0, 1) for m in metas])


def pack(metas):
    imgs = [torch.from_numpy(noise(m[0], m[1])) for m in metas]
    sizes = [im.numel() for im in imgs]
    offsets = np.cumsum([0] + sizes[:-1]).astype(np.int64)
    return torch.cat([im.reshape(-1) for im in imgs]).cuda(), offsets


def run(metas, target, filt, **kw):
    from uwudiff_amd import preprocess as P

    data, offsets = pack(metas)
    out = P.resize_crop(data, offsets, np.asarray(metas, dtype=np.int32), target, filt, **kw)
    torch.cuda.synchronize()
    return out.cpu()


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("where", ["centre", "origin", "far"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("target", [(64, 64), (96, 64)], ids=["64x64", "96x64"])
def test_ragged_batch_equals_the_oracle(target, filt, where):
    metas = [plan(h, w, target, where) for h, w in RAGGED]
    got = run(metas, target, filt)
    assert got.dtype == torch.float32 and got.shape == (5, 3, target[1], target[0])
    ref = expected(metas, target, filt)
    for i, m in enumerate(metas):
        assert torch.equal(got[i], ref[i]), (m, int((got[i] != ref[i]).sum()))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("hw,new,target", [((1000, 17), (32, 32), (32, 32)), ((17, 1000), (32, 32), (32, 32)),
                                           ((1024, 1536), (256, 256), (256, 256))], ids=["1000x17-long-taps", "17x1000-long-taps", "1024x1536"])
def test_single_pictures_equal_the_oracle(hw, new, target, filt):
    """1000 x 17 -> 32 x 32: 31-fold vertical reduction (189 taps with Lanczos) beside a horizontal upscale; 17 x 1000: the same
    horizontally, where a table of more than 127 taps is read from global memory instead of LDS; 1024 x 1536 -> 256 x 256: the
    sizes of a real batch, several workgroups in every grid dimension"""
    metas = [[hw[0], hw[1], new[1], new[0], 0, 0]]
    got = run(metas, target, filt)
    assert torch.equal(got, expected(metas, target, filt))


# ---------------------------------------------------------------------------------------------- the 256 levels
def test_all_256_levels_in_both_modes_and_bf16():
    from uwudiff_amd import preprocess as P

    a = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = torch.from_numpy(np.stack([a, np.flipud(a), a.T], axis=2).copy())
    meta = np.asarray([[16, 16, 16, 16, 0, 0]], dtype=np.int32)  # unchanged size: both passes are skipped
    for normalize, table in ((True, NORMALIZED), (False, TO_TENSOR)):
        ref = table[img.long()].permute(2, 0, 1)[None]
        got = P.resize_crop(img.reshape(-1).cuda(), [0], meta, (16, 16), "lanczos", normalize=normalize)
        assert torch.equal(got.cpu(), ref), normalize
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32))  # (bits: -0.0 would differ from 0.0)
        got16 = P.resize_crop(img.reshape(-1).cuda(), [0], meta, (16, 16), "lanczos", normalize=normalize, dtype=torch.bfloat16)
        assert got16.dtype == torch.bfloat16 and torch.equal(got16.cpu().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
    # and through a real resize: bf16 is the rounding of the fp32 result
    metas = [plan(h, w, (64, 64), "centre") for h, w in RAGGED[:3]]
    assert torch.equal(run(metas, (64, 64), "bicubic", dtype=torch.bfloat16), expected(metas, (64, 64), "bicubic").to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------- hygiene
def test_sentinel_workspace_repeat_and_neighbours():
    from uwudiff_amd import lib as L
    from uwudiff_amd import preprocess as P

    target, filt = (96, 64), "lanczos"
    metas = [plan(h, w, target, "far") for h, w in RAGGED]
    meta = np.asarray(metas, dtype=np.int32)
    data, offsets = pack(metas)
    n = 5 * 3 * 64 * 96
    need = int(L.load().uwu_image_resize_crop_ws_bytes(5, meta.ctypes.data, 64, 96, L.FILTER[filt]))
    assert need > 0
    outs = []
    for fill in (0xFF, 0x00, 0xFF):
        buf = torch.empty(n + 4096, device="cuda")
        buf.view(torch.int32).fill_(F32_NAN)
        ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device="cuda")
        P.resize_crop(data, offsets, meta, target, filt, out=buf[:n].view(5, 3, 64, 96), ws=ws[:need])
        torch.cuda.synchronize()
        assert bool((buf[n:].view(torch.int32) == F32_NAN).all())  # nothing after the output
        assert bool((ws[need:] == fill).all())  # nothing after the workspace
        outs.append(buf[:n].view(5, 3, 64, 96).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])  # stale workspace bytes and a second run change nothing
    assert torch.equal(outs[0], expected(metas, target, filt))
    # a picture's output does not depend on its neighbours: alone, and in another order
    for i in (0, 2, 4):
        assert torch.equal(run([metas[i]], target, filt)[0], outs[0][i])
    assert torch.equal(run(metas[::-1], target, filt), outs[0].flip(0))
    # more pictures than one launch group takes
    many = [metas[i % 3] for i in range(19)]
    got = run(many, target, filt)
    for i in range(19):
        assert torch.equal(got[i], outs[0][i % 3])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched():
    """host-side argument checks: a UwuError that names the entry point, nothing launched (the output keeps its sentinel)"""
    from uwudiff_amd import lib as L
    from uwudiff_amd import preprocess as P

    Wt, Ht = 64, 48
    metas = [plan(300, 200, (Wt, Ht), "centre"), plan(37, 53, (Wt, Ht), "centre")]
    data, offsets = pack(metas)
    meta = np.asarray(metas, dtype=np.int32)
    tables, tab_off = P.window_tables(meta, (Wt, Ht), "lanczos")
    tab = torch.from_numpy(tables).cuda()
    out = torch.empty(2 * 3 * Ht * Wt + 64, device="cuda")
    out.view(torch.int32).fill_(F32_NAN)
    need = int(L.load().uwu_image_resize_crop_ws_bytes(2, meta.ctypes.data, Ht, Wt, L.FILTER["lanczos"]))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")

    def call(src=data.data_ptr(), src_bytes=data.numel(), off=offsets, m=meta, t=tab.data_ptr(), tlen=tab.numel(), toff=tab_off,
             y=out.data_ptr(), dtype=L.F32, B=2, ht=Ht, wt=Wt, filt=L.FILTER["lanczos"], normalize=1, w=ws.data_ptr(), wn=need):
        host = [None if a is None else np.ascontiguousarray(a) for a in (off, m, toff)]
        L.call("uwu_image_resize_crop", src, src_bytes, *(None if a is None else a.ctypes.data for a in host[:2]), t, tlen,
               None if host[2] is None else host[2].ctypes.data, y, dtype, B, ht, wt, filt, normalize, w, wn, L.stream())

    def meta_with(b, col, value):
        m = meta.copy()
        m[b, col] = value
        return m

    nh, nw, top, left = (int(v) for v in meta[1, 2:6])
    cases = [
        dict(m=meta_with(1, 4, nh - Ht + 1)), dict(m=meta_with(0, 5, int(meta[0, 3]) - Wt + 1)), dict(m=meta_with(1, 4, -1)),
        dict(m=meta_with(0, 5, -1)),                                                # a window that leaves the resized picture
        dict(m=meta_with(1, 2, Ht - 1)), dict(m=meta_with(0, 3, Wt - 1)),            # a resized size smaller than the target
        dict(m=meta_with(0, 0, 0)), dict(m=meta_with(1, 1, 0)),                      # an empty picture
        dict(B=0), dict(ht=0), dict(wt=0), dict(B=-1),
        dict(src=None), dict(y=None), dict(w=None), dict(t=None), dict(off=None), dict(m=None), dict(toff=None),
        dict(src=data.data_ptr() + 4), dict(y=out.data_ptr() + 4), dict(w=ws.data_ptr() + 8), dict(t=tab.data_ptr() + 4),
        dict(dtype=L.I64), dict(dtype=7), dict(filt=3), dict(filt=-1), dict(normalize=2),
        dict(wn=need - 1), dict(wn=0),
        dict(src_bytes=data.numel() - 1), dict(off=np.asarray([0, -3], dtype=np.int64)),  # a picture outside src
        dict(tlen=tab.numel() - 1), dict(toff=-tab_off - 1),                               # a table outside tables
    ]
    for kw in cases:
        with pytest.raises(L.UwuError, match="image_resize_crop"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == F32_NAN).all())
    call()  # the same buffers with nothing wrong: runs
    torch.cuda.synchronize()
    assert torch.equal(out[:2 * 3 * Ht * Wt].view(2, 3, Ht, Wt).cpu(), expected(metas, (Wt, Ht), "lanczos"))
    assert bool((out[2 * 3 * Ht * Wt:].view(torch.int32) == F32_NAN).all())


# ---------------------------------------------------------------------------------------------- end to end
E2E_FILES = [("a.png", "RGB", (200, 120)), ("b.png", "RGB", (90, 260)), ("c.png", "RGB", (40, 30)), ("d.png", "L", (150, 150)),
             ("e.png", "RGBA", (133, 97)), ("f.png", "P", (64, 64)), ("sub/g.png", "RGB", (301, 77))]  # (w, h)


def _dataset(root, on_device, **kw):
    from duwu.data import LocalTextImageTrainDataset

    return LocalTextImageTrainDataset(image_dir=str(root), target_size=(64, 64), random_crop=True, resize_on_device=on_device, **kw)


def test_device_mode_gives_the_cpu_modes_batches(tmp_path):
    from uwudiff_amd.engine import Fitter

    write_folder(tmp_path, E2E_FILES)
    fit = Fitter()
    batches = []
    for on_device in (False, True):
        ds = _dataset(tmp_path, on_device)
        np.random.seed(11)
        batches.append(fit._to_device(ds.collate([ds[i] for i in range(len(ds))])))
    (xa, ca, _, aa, _), (xb, cb, _, ab, _) = batches
    assert xa.is_cuda and xb.is_cuda and xb.dtype == torch.float32 and xb.shape == (7, 3, 64, 64)
    assert torch.equal(xa, xb), int((xa != xb).sum())
    assert ca == cb and torch.equal(aa["time_ids"], ab["time_ids"]) and ab["time_ids"].is_cuda


def _small_trainer():
    from duwu.trainer import DMTrainer

    cfg = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": {"depth": 1, "hidden": 128, "heads": 2, "sample_size": 8}},
           "te": None,
           "vae": {"_target_": "diffusers.AutoencoderKL.from_pretrained", "_load_config_": {"precision": "torch.float16", "to_freeze": True},
                   "pretrained_model_name_or_path": "madebyollin/sdxl-vae-fp16-fix"}}
    torch.manual_seed(1215)
    return DMTrainer(cfg, vae_std=1 / 0.13025, use_warm_up=False)


def test_two_training_steps_on_the_folder_are_bit_equal_between_the_modes(tmp_path):
    """the trainer of tests/test_vae_gpu.py::test_trainer_encodes_pixels_with_the_autoencoder (small denoiser, VAE node), fitted for
    two steps on the folder in either mode"""
    from duwu.data import TrainDataModule
    from uwudiff_amd.engine import Fitter, seed_everything

    write_folder(tmp_path, E2E_FILES)
    losses = []
    for on_device in (False, True):
        dm = TrainDataModule({"_target_": "duwu.data.LocalTextImageTrainDataset", "image_dir": str(tmp_path), "target_size": [64, 64],
                              "random_crop": True, "resize_on_device": on_device}, {"batch_size": 4, "shuffle": True})
        tr = _small_trainer()
        seed_everything(1215)
        np.random.seed(1215)
        fit = Fitter(max_steps=2, log_every_n_steps=1, default_root_dir=str(tmp_path))
        hist = fit.fit(tr, dm)
        assert fit.global_step == 2 and len(hist) == 2
        losses.append([h["loss"] for h in hist])
    print(f"[folder fit] CPU mode {losses[0]}, device mode {losses[1]}")
    assert all(math.isfinite(v) for v in losses[0] + losses[1])
    assert losses[0] == losses[1]


def test_demo_folder_config_runs_under_fast_dev_run(tmp_path):
    import importlib.util

    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    spec = importlib.util.spec_from_file_location("make_demo_folder", os.path.join(ROOT, "tools", "make_demo_folder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.make(str(tmp_path / "demo"), n=20)
    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_folder.yaml"))
    assert cfg.lightning_config.fast_dev_run is True
    cfg = merge(cfg, {"data": {"dataset_config": {"image_dir": str(tmp_path / "demo")}}})
    # the small denoiser of the test above in place of the SDXL UNet and its text encoders; the VAE node is the file's
    cfg.trainer.model_config["unet"] = {"_target_": "uwudiff_amd.dit.DiT.from_config",
                                        "config": {"depth": 1, "hidden": 128, "heads": 2, "sample_size": 32}}
    cfg.trainer.model_config["te"] = None
    lc = dict(cfg.lightning_config)
    lc["callbacks"] = []
    fit = Fitter(default_root_dir=str(tmp_path), **lc)
    dm, tr = load_all(cfg)
    seed_everything(cfg.seed)
    hist = fit.fit(tr, dm)
    assert fit.global_step == 1 and len(hist) == 1 and math.isfinite(hist[0]["loss"])
    assert dm.dataset.resize_on_device and len(dm.dataset) == 20
