"""GPU: ``bitsandbytes.optim.AdamW8bit`` (uwudiff_amd.optim.FusedAdamW8bit) through DMTrainer / Fitter on the tiny UNet: the fused
branch, the state's dtypes and sizes, checkpoint and resume (the uint8 codes survive ``load_state_dict``), and
configs/demo_training_adamw8bit.yaml.  The pattern of tests/test_optimizers_gpu.py."""
import math
import os

import pytest
import torch

from tests.conftest import ROOT
from tests.test_optimizers_gpu import ElementwiseDenoiser

pytestmark = pytest.mark.gpu

TARGET = "bitsandbytes.optim.AdamW8bit"
CODES, SCALES = ("state1", "state2"), ("absmax1", "absmax2")


def _fit_cfg(tmp_path, steps, clip=None, unet=None):
    from uwudiff_amd.config import load_yaml, merge

    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1, "gradient_clip_val": clip,
                                 "default_root_dir": str(tmp_path)},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8},
                     "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": 1e-3, "optimizer": TARGET, "opt_config": {"weight_decay": 0.01, "betas": [0.9, 0.999]},
                        "lycoris_config": None}}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over)
    if unet is not None:
        cfg = merge(cfg, {"trainer": {"model_config": {"unet": {"_target_": unet}}}})
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    return cfg, lc


def _fresh(tmp_path, steps, clip=None, unet=None):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, steps, clip, unet)
    seed_everything(cfg.seed)
    fit = Fitter(**lc)
    dm, tr = load_all(cfg)
    return fit, dm, tr


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
def test_fitter_takes_the_fused_branch(tmp_path, clip):
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamW8bit

    fit, dm, tr = _fresh(tmp_path, 3, clip)
    flat0 = tr.unet.flat.detach().clone()

    def after_step(f):
        assert not tr.unet.flat.grad.any()  # left zeroed by the update kernel

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert isinstance(optim, FlatFusedOptimizer) and type(optim) is FusedAdamW8bit
    assert fit.global_step == 3 and len(hist) == 3 and all(math.isfinite(h["loss"]) for h in hist)
    flat = tr.unet.flat.detach()
    assert torch.isfinite(flat).all() and float((flat - flat0.to(flat.device)).abs().max()) > 0
    assert torch.equal(tr.unet.shadow, flat.bfloat16())  # written by the kernel
    st = optim.state[tr.unet.flat]
    n = flat.numel()
    blocks = -(-n // 256)
    assert set(st) == {"step", "state1", "state2", "absmax1", "absmax2", "qmap1", "qmap2"} and st["step"] == 3
    for k in CODES:
        assert st[k].dtype == torch.uint8 and st[k].shape == (n,) and st[k].is_cuda
    for k in SCALES:
        assert st[k].dtype == torch.float32 and st[k].shape == (blocks,) and torch.isfinite(st[k]).all() and st[k].max() > 0
    for k in ("qmap1", "qmap2"):
        assert st[k].dtype == torch.float32 and st[k].shape == (256,)
    held = sum(t.numel() * t.element_size() for t in st.values() if torch.is_tensor(t))
    assert held == 2 * n + 8 * blocks + 2 * 256 * 4


def _same_bits(a, b):
    view = {1: torch.uint8, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.cpu().view(view), b.cpu().view(view))


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after step 3, resume in fresh objects, steps 4-5: parameters, codes (uint8 in the file and after the load) and
    block scales equal the uninterrupted run's bit for bit (on the denoiser whose gradient is bit-reproducible)."""
    from uwudiff_amd.engine import seed_everything

    path = str(tmp_path / "step3.ckpt")
    unet = f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser"

    def save_at_3(f):
        if f.global_step == 3:
            f.save_checkpoint(path)
            seed_everything(777)

    fit, dm, tr = _fresh(tmp_path, 5, unet=unet)
    fit.step_hooks.append(save_at_3)
    fit.fit(tr, dm)
    fit2, dm2, tr2 = _fresh(tmp_path, 5, unet=unet)
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        st = fit2._fit_state[1].state[tr2.unet.flat]
        loaded.update({k: v.clone() if torch.is_tensor(v) else v for k, v in st.items()})
        loaded["flat"] = tr2.unet.flat.detach().clone()
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert fit.global_step == 5 and fit2.global_step == 5 and len(hist_b) == 2
    assert isinstance(tr.unet, ElementwiseDenoiser) and isinstance(tr2.unet, ElementwiseDenoiser)
    ck_st = torch.load(path, map_location="cpu", weights_only=True)["optimizer_states"][0]["state"][0]
    for k in CODES + SCALES + ("qmap1", "qmap2"):  # what the resumed run starts from is the file's content, in its dtype
        assert ck_st[k].dtype == (torch.uint8 if k in CODES else torch.float32)
        assert _same_bits(loaded[k], ck_st[k]), k
    assert ck_st["step"] == loaded["step"] == 3
    st_a, st_b = fit._fit_state[1].state[tr.unet.flat], fit2._fit_state[1].state[tr2.unet.flat]
    assert float((loaded["flat"] - tr2.unet.flat.detach()).abs().max()) > 0  # steps 4-5 did move them
    assert _same_bits(tr2.unet.flat.detach(), tr.unet.flat.detach())
    for k in CODES + SCALES:
        assert _same_bits(st_b[k], st_a[k]), k
        assert not _same_bits(st_b[k], loaded[k]), k
    assert st_b["step"] == st_a["step"] == 5
    assert torch.equal(tr2.unet.shadow, tr2.unet.flat.detach().bfloat16())


def test_the_adamw8bit_config_loads_and_trains():
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything
    from uwudiff_amd.optim import FusedAdamW8bit

    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_adamw8bit.yaml")),
                {"lightning_config": {"fast_dev_run": False, "max_steps": 2, "log_every_n_steps": 1},
                 "data": {"dataloader_config": {"num_workers": 0}}})
    fit = Fitter(**cfg["lightning_config"])
    dm, tr = load_all(cfg)
    seed_everything(cfg.seed)
    hist = fit.fit(tr, dm)
    assert type(fit._fit_state[1]) is FusedAdamW8bit
    assert fit.global_step == 2 and all(math.isfinite(h["loss"]) for h in hist)
