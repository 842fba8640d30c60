"""GPU: training on aspect-ratio buckets -- the UNet at a non-square latent whose token count is no multiple of 64
(self-attention on the ragged-query MFMA kernels) against the fp32 oracle, and the fit loop on batches whose shape changes from one
to the next: training, both ``resize_on_device`` modes, validation, an accumulation window over two shapes, the demo config."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- the UNet at 20 x 28
# tests/test_unet_gpu.py's TINY (restated) with the transformer blocks at BOTH levels and 64 / 128 channels in heads of 64: at a
# 20 x 28 latent level 0 attends at T = 560 (bf16: the ragged-query MFMA kernels) and level 1 at T = 10 x 14 = 140 (generic kernels)
TINY = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
            down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
            transformer_layers_per_block=(1, 2), attention_head_dim=(1, 1), cross_attention_dim=32,
            addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48,
            norm_num_groups=8)
BOTH = dict(TINY, block_out_channels=(64, 128), attention_head_dim=(1, 2), transformer_layers_per_block=(1, 1),
            down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"))


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item(), ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def run_pair(cfg, dtype, B, S, W, Tk=7, seed=0):
    """tests/test_unet_gpu.py's run_pair: the oracle with random weights away from the near-zero init, the model with its weights,
    one forward and backward each"""
    from oracle.unet import UNetOracle
    from uwudiff_amd.unet import UNet2DConditionModel

    torch.manual_seed(seed)
    ora = UNetOracle(**cfg)
    with torch.no_grad():
        for n, p in ora.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (0.5 / p[0].numel() ** 0.5))
            elif n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.05)
            else:
                p.copy_(1 + torch.randn_like(p) * 0.1)
    model = UNet2DConditionModel(cfg, compute_dtype=dtype).cuda()
    model.load_state_dict(ora.state_dict())
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, cfg["in_channels"], S, W, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    ctx = torch.randn(B, Tk, cfg["cross_attention_dim"], generator=g)
    pooled = torch.randn(B, 16, generator=g)
    ids = torch.tensor([[1024.0, 1024, 0, 0, 8.0 * S, 8.0 * W]] * B)
    dout = torch.randn(B, cfg["out_channels"], S, W, generator=g) / (S * W)
    yo = ora(x, t, encoder_hidden_states=ctx, added_cond_kwargs={"text_embeds": pooled, "time_ids": ids})[0]
    yo.backward(dout)
    y = model(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda(), added_cond_kwargs={"text_embeds": pooled.cuda(), "time_ids": ids.cuda()})[0]
    y.backward(dout.cuda())
    torch.cuda.synchronize()
    og = dict(ora.named_parameters())
    return y, yo, {n: (model.grad_tensor(n), og[n].grad) for n in model.P.registry}


def test_routes_of_the_20x28_latent():
    from uwudiff_amd import ops

    for bwd in (False, True):
        assert ops.attention_route(560, 560, 64, 192, 192, 192, 64, backward=bwd)           # packed q|k|v of one head of 64
        assert ops.attention_route(560, 7, 64, 64, 128, 128, 64, backward=bwd)              # its cross-attention
        assert not ops.attention_route(140, 140, 64, 384, 384, 384, 128, backward=bwd)      # level 1 stays generic
        assert not ops.attention_route(560, 560, 64, 192, 192, 192, 64, dtype=torch.float32, backward=bwd)


def test_unet_bf16_at_a_ragged_token_count_close_to_oracle():
    """test_unet_gpu.py::test_unet_bf16_close_to_oracle's bounds (B = 3) at a 20 x 28 latent"""
    y, yo, grads = run_pair(BOTH, "bf16", B=3, S=20, W=28)
    l2, _ = rel(y, yo)
    print(f"bf16 20 x 28: output rel l2 {l2:.3e}; worst gradient rel l2 {max(rel(g, go)[0] for g, go in grads.values()):.3e}")
    assert l2 < 4e-2, l2
    bad = {n: rel(g, go)[0] for n, (g, go) in grads.items() if rel(g, go)[0] > 0.12}
    assert not bad, bad


def test_unet_fp32_at_a_ragged_token_count_matches_oracle():
    """test_unet_gpu.py::test_unet_fp32_matches_oracle's bounds (B = 2) at the same shape: the generic kernels, as before"""
    y, yo, grads = run_pair(BOTH, "fp32", B=2, S=20, W=28)
    l2, mx = rel(y, yo)
    assert l2 < 1e-3 and mx < 1e-3, (l2, mx)
    for name, (g, go) in grads.items():
        l2, mx = rel(g, go)
        assert l2 < 2e-3, (name, l2, mx)


# ---------------------------------------------------------------------------------------------- the fit loop on a bucketed folder
SIZES = [(100, 50), (60, 60), (48, 90)]  # (w, h): 2 : 1, 1 : 1 and about 1 : 2 -- four pictures of each
BUCKETS = dict(resolution=128, min_side=64, max_side=256, step=64)  # (64, 256) (64, 192) (128, 128) (192, 64) (256, 64)
SHAPE_OF = {(100, 50): (192, 64), (60, 60): (128, 128), (48, 90): (64, 192)}  # nearest log aspect: 2 -> 3, 1 -> 1, 0.533 -> 1 / 3


def write_folder(root, n=12):
    os.makedirs(str(root), exist_ok=True)
    paths = []
    for i in range(n):
        w, h = SIZES[i % 3]
        rng = np.random.default_rng(500 + i)
        p = os.path.join(str(root), f"p{i:02d}.png")
        Image.fromarray(rng.integers(0, 256, (h + i // 3, w + i // 3, 3), dtype=np.uint8)).save(p)  # (a few pixels apart: no two alike)
        with open(os.path.splitext(p)[0] + ".txt", "w") as f:
            f.write(f"picture {i}\n")
        paths.append(p)
    return paths


def _node(root, on_device, **kw):
    return {"_target_": "duwu.data.LocalTextImageTrainDataset", "image_dir": str(root), "target_size": [64, 64], "random_crop": True,
            "resize_on_device": on_device, "buckets": BUCKETS, **kw}


def test_to_device_gives_each_batch_its_buckets_shape(tmp_path):
    from duwu.data import TrainDataModule
    from duwu.data.utils import make_buckets, resize_and_crop_image
    from uwudiff_amd.engine import Fitter

    write_folder(tmp_path)
    dm = TrainDataModule(_node(tmp_path, True, random_crop=False), {"batch_size": 3, "shuffle": True})
    dm.setup("fit")
    ds = dm.dataset
    assert ds.buckets == make_buckets(**BUCKETS)
    number = lambda p: int(os.path.basename(p)[1:3])
    assert [ds.buckets[b] for b in ds.bucket_of] == [SHAPE_OF[SIZES[number(p) % 3]] for p in ds.image_paths]
    fit = Fitter()
    torch.manual_seed(2)
    seen = []
    for batch in dm.train_dataloader():
        x, captions, _, added, _ = fit._to_device(batch)
        idx = [int(c.split()[1]) for c in captions]
        w, h = SHAPE_OF[SIZES[idx[0] % 3]]
        assert x.is_cuda and x.dtype == torch.float32 and x.shape == (len(idx), 3, h, w)
        assert added["time_ids"][:, 4:].tolist() == [[float(h), float(w)]] * len(idx)
        for row, i in zip(x.cpu(), idx):
            ref, _, _ = resize_and_crop_image(Image.open(os.path.join(str(tmp_path), f"p{i:02d}.png")).convert("RGB"), (w, h), random_crop=False)
            assert torch.equal(row, ref), (i, int((row != ref).sum()))
        seen.append((w, h))
    assert len(seen) == 6 and set(seen) == set(SHAPE_OF.values())


def _trainer_class():
    from duwu.trainer import DMTrainer

    class BucketTrainer(DMTrainer):
        """no text encoder: a fixed context and pooled embedding per sample slot, so that the UNet (which takes any latent shape, as
        the fixed-size DiT of the other folder tests does not) can be the denoiser"""

        def get_latent_and_conditioning(self, batch):
            x, _, attn_mask, added, ca = super().get_latent_and_conditioning(batch)
            if not hasattr(self, "_ctx"):
                g = torch.Generator().manual_seed(77)
                self._ctx, self._pooled = torch.randn(16, 7, 32, generator=g).to(x.device), torch.randn(16, 16, generator=g).to(x.device)
            added["text_embeds"] = self._pooled[:x.shape[0]]
            return x, self._ctx[:x.shape[0]], attn_mask, added, ca

    return BucketTrainer


def _trainer():
    cfg = {"unet": {"_target_": "uwudiff_amd.unet.UNet2DConditionModel.from_config", "config": dict(TINY), "compute_dtype": "bf16",
                    "device": "cuda"},
           "te": None,
           "vae": {"_target_": "diffusers.AutoencoderKL.from_pretrained", "_load_config_": {"precision": "torch.float16", "to_freeze": True},
                   "pretrained_model_name_or_path": "madebyollin/sdxl-vae-fp16-fix"}}
    torch.manual_seed(1215)
    return _trainer_class()(cfg, vae_std=1 / 0.13025, use_warm_up=False)


def _fit(tmp_path, on_device, loader=None, val=False, **fitter):
    from duwu.data import TrainDataModule
    from uwudiff_amd.engine import Fitter, seed_everything

    dm = TrainDataModule(_node(tmp_path, on_device), loader or {"batch_size": 2, "shuffle": True},
                         val_dataset_config=_node(tmp_path, on_device, random_crop=False) if val else None)
    tr = _trainer()
    seed_everything(1215)
    np.random.seed(1215)
    fit = Fitter(log_every_n_steps=1, default_root_dir=str(tmp_path), **fitter)
    shapes, inner = [], fit._to_device

    def spy(batch):
        out = inner(batch)
        shapes.append(tuple(out[0].shape))
        return out

    fit._to_device = spy
    hist = fit.fit(tr, dm)
    return fit, hist, shapes


def test_four_steps_over_changing_shapes_are_bit_equal_between_the_modes(tmp_path):
    write_folder(tmp_path)
    runs = [_fit(tmp_path, on_device, max_steps=4) for on_device in (False, True)]
    for fit, hist, shapes in runs:
        assert fit.global_step == 4 and len(hist) == 4 and all(math.isfinite(h["loss"]) for h in hist)
        assert len(shapes) == 4 and len(set(shapes)) >= 2, shapes  # (two batches per bucket: four batches visit two shapes at least)
        assert all(s[0] == 2 and (s[3], s[2]) in SHAPE_OF.values() for s in shapes)
    print(f"[bucket fit] shapes {runs[0][2]}; CPU mode {[h['loss'] for h in runs[0][1]]}, device mode {[h['loss'] for h in runs[1][1]]}")
    assert runs[0][2] == runs[1][2]
    assert [h["loss"] for h in runs[0][1]] == [h["loss"] for h in runs[1][1]]


def test_validation_over_a_bucketed_set(tmp_path):
    write_folder(tmp_path)
    fit, hist, shapes = _fit(tmp_path, True, val=True, max_steps=3, val_check_interval=2, check_val_every_n_epoch=None,
                             num_sanity_val_steps=0)
    assert fit.global_step == 3 and len(fit.val_history) == 1
    rec = fit.val_history[0]
    assert rec["step"] == 2 and rec["val_samples"] == 12 and math.isfinite(rec["val/loss"])
    # two training batches, then the validation set in bucket order (4 pictures of each of the three shapes, in batches of 2), then
    # the third training batch
    assert len(shapes) == 2 + 6 + 1 and [(s[3], s[2]) for s in shapes[2:8]] == [(64, 192)] * 2 + [(128, 128)] * 2 + [(192, 64)] * 2


def test_an_accumulation_window_spans_two_shapes(tmp_path):
    write_folder(tmp_path)
    fit, hist, shapes = _fit(tmp_path, True, loader={"batch_size": 4, "shuffle": False}, max_steps=1, accumulate_grad_batches=2)
    assert fit.global_step == 1 and len(hist) == 1 and hist[0]["accum"] == 2 and math.isfinite(hist[0]["loss"])
    assert [(s[3], s[2]) for s in shapes] == [(64, 192), (128, 128)]  # buckets in index order: the window holds two shapes


def test_demo_buckets_config_runs_under_fast_dev_run(tmp_path):
    import importlib.util

    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    spec = importlib.util.spec_from_file_location("make_demo_folder", os.path.join(ROOT, "tools", "make_demo_folder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.make(str(tmp_path / "demo"), n=20)
    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_buckets.yaml"))
    assert cfg.lightning_config.fast_dev_run is True
    cfg = merge(cfg, {"data": {"dataset_config": {"image_dir": str(tmp_path / "demo")}}})
    # the small UNet in place of the SDXL UNet and its text encoders (a DiT has one fixed sample size); the VAE node is the file's
    assert cfg.trainer.model_config["vae"]["pretrained_model_name_or_path"] == "madebyollin/sdxl-vae-fp16-fix"
    dm, tr = load_all(cfg, trainer=_trainer())
    lc = dict(cfg.lightning_config)
    lc["callbacks"] = []
    fit = Fitter(default_root_dir=str(tmp_path), **lc)
    seed_everything(cfg.seed)
    hist = fit.fit(tr, dm)
    assert fit.global_step == 1 and len(hist) == 1 and math.isfinite(hist[0]["loss"])
    ds = dm.dataset
    assert ds.resize_on_device and len(ds) == 20 and ds.buckets is not None and len(set(ds.bucket_of)) >= 2
