"""GPU tests of gradient accumulation (``Fitter(accumulate_grad_batches=N)``): the fit loop on the fused
optimizer path, the audit of the gradient writers -- every named tensor of ``flat.grad`` after a window of two batches against the sum
of the two batches' gradients taken one at a time --, the clip coefficient on the accumulated, scaled gradient, and the launcher.

The audit's yardstick is measured in the test itself: the by-hand sum ``g0 + g1`` taken twice at the same seed differs by the
run-to-run spread of the fp32 atomics; a writer that overwrote instead of adding would be off by the whole of ``g0``."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 1215
TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")
# the SDXL-width UNet of tests/test_configs_gpu.py (its smallest UNet configuration), run at its smallest latent (32 x 32)
SDXL_CUT = dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
                down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                transformer_layers_per_block=(1, 2, 2), attention_head_dim=(5, 10, 20), cross_attention_dim=2048,
                addition_embed_type="text_time", addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816,
                norm_num_groups=32)


class _ListDM:
    """a fixed list of batches: both the by-hand passes and the Fitter see the same tensors in the same order"""

    def __init__(self, batches):
        self.batches = batches

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return self.batches


def _spy(tr, on_step=None, on_clip=None):
    """wrap the optimizer `tr.configure_optimizers` hands to the next fit: `on_step(opt)` on entry to opt.step,
    `on_clip(opt, out)` around opt.grad_norm_clip"""
    inner = type(tr).configure_optimizers

    def configure():
        owner = tr.lycoris_model if tr.lycoris_model is not None else tr.unet
        tr.train_params = owner.parameters()  # (the trainer keeps a generator, which its first fit used up)
        cfg = inner(tr)
        opt = cfg["optimizer"] if isinstance(cfg, dict) else cfg
        step, norm = opt.step, opt.grad_norm_clip

        @functools.wraps(step)  # (keeps the mark an LR scheduler left on the method it wrapped)
        def spied_step(*a, **kw):
            if on_step is not None:
                on_step(opt, kw)
            return step(*a, **kw)

        def spied_clip(max_norm, pre_scale=1.0):
            g = opt.param_groups[0]["params"][0].grad.detach().clone()
            out = norm(max_norm, pre_scale=pre_scale)
            on_clip(g, float(pre_scale), out.detach().clone())
            return out

        opt.step = spied_step
        if on_clip is not None:
            opt.grad_norm_clip = spied_clip
        tr._spied_opt = opt
        return cfg

    tr.configure_optimizers = configure


def _fitter(**kw):
    from uwudiff_amd.engine import Fitter

    kw = {"precision": "bf16-mixed", "log_every_n_steps": 1, "fast_dev_run": False, **kw}
    return Fitter(**kw)


# ---------------------------------------------------------------------- the DiT of configs/demo_training_latent.yaml
@pytest.fixture(scope="module")
def dit():
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.engine import seed_everything

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    seed_everything(cfg.seed)
    dm, tr = load_all(cfg)
    tr.unet.reset_parameters("random")  # (the adaLN-zero start leaves the blocks' gradients exactly zero: nothing to compare)
    tr.cuda()
    dm.setup("fit")
    batches = list(dm.train_dataloader())
    assert [b[0].shape[0] for b in batches] == [16, 16, 16, 2]
    return {"cfg": cfg, "dm": dm, "tr": tr, "batches": batches, "flat0": tr.unet.flat.detach().clone()}


def _restore(env):
    tr = env["tr"]
    with torch.no_grad():
        tr.unet.flat.copy_(env["flat0"])
    tr.unet.refresh_shadow()
    tr.ema_loss.zero_()


def test_fitter_takes_two_steps_from_four_batches(dit):
    """(a) N = 2 on batches of 16, 16, 16, 2: two optimizer steps, the second on the window that holds the ragged batch"""
    from uwudiff_amd.engine import seed_everything
    from uwudiff_amd.optim import FusedAdamW

    _restore(dit)
    tr = dit["tr"]
    sizes, zero_after, handed = [], [], []
    inner = tr.training_step

    def training_step(batch, idx):
        sizes.append(int(batch[0].shape[0]))
        return inner(batch, idx)

    tr.training_step = training_step
    _spy(tr, on_step=lambda opt, kw: handed.append((len(sizes), kw.get("pre_scale"), tr.unet.flat.grad.abs().max())))
    try:
        seed_everything(SEED)
        fit = _fitter(accumulate_grad_batches=2, max_steps=2)
        fit.step_hooks.append(lambda f: zero_after.append(tr.unet.flat.grad.abs().max()))
        hist = fit.fit(tr, dit["dm"])
    finally:
        del tr.training_step, tr.configure_optimizers
    opt = tr._spied_opt
    assert isinstance(opt, FusedAdamW) and opt.state[tr.unet.flat]["step"] == 2
    assert fit.global_step == 2 and fit.train_batches == 4 and sizes == [16, 16, 16, 2]
    assert [h["step"] for h in hist] == [1, 2] and [h["accum"] for h in hist] == [2, 2]
    assert [n for n, _, _ in handed] == [2, 4] and [ps for _, ps, _ in handed] == [0.5, 0.5]  # 1/N rides on pre_scale
    assert all(float(m) > 0 for _, _, m in handed)
    assert [float(z) for z in zero_after] == [0.0, 0.0]  # the fused step leaves the consumed gradient zeroed
    assert fit.accum_pending == 0 and all(torch.isfinite(torch.tensor(h["loss"])) for h in hist)
    assert not torch.equal(tr.unet.flat.detach(), dit["flat0"])


# ---------------------------------------------------------------------- (b) the audit: every writer adds
def _segments(owner):
    """{name: (offset, length)} of the tensors a flat-buffer module keeps in `flat`"""
    import math

    layout = owner.offsets if hasattr(owner, "offsets") else owner.P.registry
    return {(k if isinstance(k, str) else ".".join(map(str, k))): (off, math.prod(shape)) for k, (off, shape) in layout.items()}


def _per_tensor(a, b, segs):
    """relative L2 distance of `a` from `b` per named tensor (float64), and the tensors' norms in `b`"""
    d = torch.stack([(a[o:o + n].double() - b[o:o + n].double()).norm() for o, n in segs.values()])
    r = torch.stack([b[o:o + n].double().norm() for o, n in segs.values()])
    return (d / r.clamp_min(1e-300)).cpu(), d.cpu(), r.cpu()


def _audit(tr, owner, batches, label):
    """`owner.flat.grad` as the optimizer sees it after a window of `batches` (two of them) against g0 + g1 taken by hand"""
    from uwudiff_amd.engine import seed_everything

    fit = _fitter(accumulate_grad_batches=2, max_steps=1)
    flat = owner.flat

    def by_hand():
        seed_everything(SEED)
        if flat.grad is not None:
            flat.grad.zero_()
        parts = []
        for b in batches:
            tr.training_step(fit._to_device(b), 0)["loss"].backward()
            parts.append(flat.grad.detach().clone())
            flat.grad.zero_()
        return parts

    g0, g1 = by_hand()
    ref = g0 + g1
    h0, h1 = by_hand()
    ref2 = h0 + h1
    del h0, h1
    spied = []
    _spy(tr, on_step=lambda opt, kw: spied.append(flat.grad.detach().clone()))
    try:
        seed_everything(SEED)
        hist = fit.fit(tr, _ListDM(batches))
    finally:
        del tr.configure_optimizers
    assert len(spied) == 1 and fit.global_step == 1 and hist[0]["accum"] == 2
    segs = _segments(owner)
    assert sum(n for _, n in segs.values()) <= flat.numel() and len(segs) > 4
    yard, _, norms = _per_tensor(ref2, ref, segs)
    dist, diff, _ = _per_tensor(spied[0], ref, segs)
    live = norms > 0
    # a writer that overwrote would leave g1 alone: its distance from g0 + g1 would be |g0| / |g0 + g1|, of order one
    one_batch, _, _ = _per_tensor(g1, ref, segs)
    names = list(segs)
    worst = names[int(torch.where(live, yard, torch.zeros_like(yard)).argmax())]
    print(f"{label}: {int(live.sum())} of {len(segs)} tensors carry a gradient; largest yardstick {float(yard[live].max()):.3e} "
          f"({worst}), median {float(yard[live].median()):.3e}; largest distance {float(dist[live].max()):.3e}, median "
          f"{float(dist[live].median()):.3e}; smallest distance of g1 alone {float(one_batch[live].min()):.3e}")
    assert int(live.sum()) >= 0.9 * len(segs), [n for n, ok in zip(segs, live) if not ok][:8]
    if bool((~live).any()):  # (a tensor no batch reaches, such as the unconditional DiT's unused y_embedder, stays exactly zero)
        assert float(diff[~live].max()) == 0.0
    bound = torch.clamp(10 * yard, min=1e-5)
    bad = {n: (float(d), float(b)) for n, d, b, ok in zip(segs, dist, bound, live) if ok and not d <= b}
    assert not bad, (len(bad), dict(list(bad.items())[:8]))
    # (and the bound can tell the two apart in every tensor: g0 is nowhere small enough to hide inside it)
    assert bool((one_batch[live] > bound[live]).all())


@pytest.mark.parametrize("ckpt", [False, True], ids=["bf16", "bf16_checkpoint"])
def test_dit_window_gradient_equals_the_sum_per_tensor(dit, ckpt):
    _restore(dit)
    tr = dit["tr"]
    tr.unet.enable_gradient_checkpointing(ckpt)
    try:
        _audit(tr, tr.unet, dit["batches"][:2], f"DiT-S/2 bf16{' + recomputation' if ckpt else ''}")
        _restore(dit)
        _audit(tr, tr.unet, dit["batches"][2:], f"DiT-S/2 bf16{' + recomputation' if ckpt else ''}, batches of 16 and 2")
    finally:
        tr.unet.enable_gradient_checkpointing(False)


def test_dit_rope_window_gradient_equals_the_sum_per_tensor():
    """the learnable axial-RoPE log-frequencies (atomics from the attention backward) next to the Linear and LayerNorm writers"""
    from duwu.trainer.trainer import DMTrainer

    torch.manual_seed(3)
    mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "init": "random",
                   "config": dict(depth=2, hidden=128, heads=2, patch=2, sample_size=16, in_channels=4, out_channels=4, cond_dim=0,
                                  rope=True)}}
    tr = DMTrainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-6).cuda()
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(n, 4, 16, 16, generator=g), [""] * n, [], {}, {}) for n in (16, 5)]
    assert "rope.freqs_h" in tr.unet.registry
    _audit(tr, tr.unet, batches, "DiT (depth 2, D 128) with RoPE")


def _unet_trainer(lycoris):
    from duwu.trainer.trainer import DMTrainer

    class _CondTrainer(DMTrainer):
        """no text encoder: the context and the pooled embedding travel in the batch's `added` dict"""

        def get_latent_and_conditioning(self, batch):
            x, _, _, added, ca = batch
            added = dict(added)
            return x, added.pop("ctx"), None, added, ca

    torch.manual_seed(5)
    mc = {"unet": {"_target_": "uwudiff_amd.unet.UNet2DConditionModel.from_config", "config": dict(SDXL_CUT),
                   "compute_dtype": "bf16", "device": "cuda"}}
    tr = _CondTrainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-6, lycoris_config=TOML if lycoris else None).cuda()
    gen = torch.Generator(device="cuda").manual_seed(6)
    with torch.no_grad():  # away from the near-zero residual outputs and the zero halves of fresh adapters: every branch carries signal
        flat = tr.unet.flat
        flat.add_(torch.randn(flat.shape, generator=gen, device="cuda") * 0.01)
        tr.unet.refresh_shadow()
        if lycoris:
            af = tr.lycoris_model.flat
            af.add_(torch.randn(af.shape, generator=gen, device="cuda") * 0.02)
            tr.lycoris_model.mark_dirty()
    g = torch.Generator().manual_seed(7)
    B, S = 2, 32
    batches = [(torch.randn(B, 4, S, S, generator=g), [""] * B, [],
                {"ctx": torch.randn(B, 77, 2048, generator=g), "text_embeds": torch.randn(B, 1280, generator=g),
                 "time_ids": torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B)}, {}) for _ in range(2)]
    return tr, batches


@pytest.mark.parametrize("lycoris", [False, True], ids=["full", "lycoris"])
def test_unet_window_gradient_equals_the_sum_per_tensor(lycoris):
    """the SDXL-width UNet at 32 x 32 latents, batch 2, bf16: GroupNorm dgamma / dbeta, the convolution and Linear weight gradients,
    the timestep / added-cond MLPs; with the shipped LyCORIS preset the views of the adapter buffer (LoRA, LoKr, norms)"""
    tr, batches = _unet_trainer(lycoris)
    try:
        owner = tr.lycoris_model if lycoris else tr.unet
        _audit(tr, owner, batches, "SDXL-width UNet bf16" + (", LyCORIS adapters" if lycoris else ""))
        if lycoris:
            assert tr.unet.flat.grad is None  # the base stayed frozen
    finally:
        del tr, batches
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------- (c) the clip coefficient
def test_clip_coefficient_is_taken_on_the_accumulated_scaled_gradient(dit):
    from uwudiff_amd.engine import seed_everything

    _restore(dit)
    tr = dit["tr"]
    max_norm, seen, handed = 1e-4, [], []
    _spy(tr, on_step=lambda opt, kw: handed.append((kw.get("pre_scale"), kw["clip"].detach().clone())),
         on_clip=lambda g, pre, out: seen.append((g, pre, out)))
    try:
        seed_everything(SEED)
        fit = _fitter(accumulate_grad_batches=2, max_steps=2, gradient_clip_val=max_norm)
        hist = fit.fit(tr, _ListDM(dit["batches"]))
    finally:
        del tr.configure_optimizers
    assert fit.global_step == 2 and len(seen) == 2 and [h["accum"] for h in hist] == [2, 2]  # once per optimizer step
    for (g, pre, out), (step_pre, step_clip) in zip(seen, handed):
        assert pre == 0.5 and step_pre == 0.5 and torch.equal(step_clip, out)
        norm = float((g.double() * 0.5).norm())  # the spied gradient times 1/N, on the host in float64
        want = min(1.0, max_norm / (norm + 1e-6))
        sq, coef = (float(v) for v in out.cpu())
        print(f"norm of the window's gradient / N: {norm:.6e}; clip coefficient {coef:.8e}, host {want:.8e}")
        assert want < 1.0  # the bound bites
        assert coef == pytest.approx(want, rel=1e-5) and sq == pytest.approx(norm * norm, rel=1e-5)


# ---------------------------------------------------------------------- (d) the launcher
def test_launcher_steps_once_per_four_batches(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_train.py"), "--configs",
                        os.path.join(ROOT, "configs", "demo_training_accum.yaml")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"step"')]
    # an epoch has 4 batches (16, 16, 16, 2) and N = 4: every record closes a window of four, max_steps = 3 optimizer steps
    assert [h["step"] for h in recs] == [1, 2, 3] and [h["accum"] for h in recs] == [4, 4, 4]
    assert all(h["loss"] == h["loss"] for h in recs)
