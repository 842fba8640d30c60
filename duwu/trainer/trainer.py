"""reference src/duwu/trainer/trainer.py: ``DMTrainer`` (constructor signature, ``training_step`` contract,
``configure_optimizers``, LyCORIS adapter training) without Lightning.  Lightning checkpoint fix-ups are out of scope.
"""
import os
from typing import Any

import torch
import torch.nn as nn
import torch.optim as optim
import torch.optim.lr_scheduler as lr_sch

from duwu.loader import load_any
from duwu.utils import instantiate_any
from uwudiff_amd.engine import GradualWarmupScheduler
from uwudiff_amd.optim import FusedAdafactor, FusedAdamW, FusedAdamWFP16, flat_segments, flat_tensors


class BaseTrainer(nn.Module):
    def __init__(self, *args, name="", lr=1e-5, optimizer=optim.AdamW,
                 opt_config={"weight_decay": 0.01, "betas": (0.9, 0.999)},
                 lr_scheduler=lr_sch.CosineAnnealingLR, lr_scheduler_config={"T_max": 100_000, "eta_min": 1e-7},
                 use_warm_up=True, warm_up_period=1000, **kwargs):
        super().__init__()
        self.name = name
        self.train_params = None
        self.optimizer = instantiate_any(optimizer)
        self.opt_config = dict(opt_config)
        if "betas" in self.opt_config:
            self.opt_config["betas"] = tuple(self.opt_config["betas"])
        self.lr = lr
        self.lr_sch = instantiate_any(lr_scheduler)
        self.lr_sch_config = dict(lr_scheduler_config)
        self.use_warm_up = use_warm_up
        self.warm_up_period = warm_up_period
        self.global_step = 0
        self._trainer = None

    # trainer.py:52-74
    def configure_optimizers(self):
        assert self.train_params is not None
        params = list(self.train_params)
        opt_cls = self.optimizer
        if opt_cls is optim.AdamW and all(p.is_cuda for p in params):
            opt_cls = FusedAdamW  # same update rule, one HIP launch over the flat buffer
        opt_config = dict(self.opt_config)
        lyc = getattr(self, "lycoris_model", None)
        if isinstance(opt_cls, type) and issubclass(opt_cls, FusedAdamWFP16) and "segments" not in opt_config:
            # optimizers.py:64-76 keeps one decay phase per parameter tensor: the tensors of the flat buffer that trains
            owner = lyc if lyc is not None else getattr(self, "unet", None)
            if owner is not None and (hasattr(owner, "offsets") or hasattr(owner, "P")):
                opt_config["segments"] = flat_segments(owner)
        if isinstance(opt_cls, type) and issubclass(opt_cls, FusedAdafactor):
            # Adafactor's rule is per tensor: the tensors of the flat buffer that trains, with their shapes as stored
            owner = lyc if lyc is not None else getattr(self, "unet", None)
            if "tensors" not in opt_config and owner is not None and (hasattr(owner, "offsets") or hasattr(owner, "P")):
                opt_config["tensors"] = flat_tensors(owner)
            if self.lr is None and (self.lr_sch is not None or self.use_warm_up):
                raise ValueError("Adafactor with relative_step computes its own step size (lr: null): set lr_scheduler: null and "
                                 "use_warm_up: false (AdafactorSchedule is not built)")
        optimizer = opt_cls(params, lr=self.lr, **opt_config)
        if lyc is not None:  # every step changes the adapters: the UNet merges them again before its next forward
            optimizer.register_step_post_hook(lambda opt, args, kwargs: lyc.mark_dirty())
        sched = self.lr_sch(optimizer, **self.lr_sch_config) if self.lr_sch is not None else None
        if self.use_warm_up:
            sched = GradualWarmupScheduler(optimizer, 1, self.warm_up_period, sched)
        if sched is None:
            return optimizer
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": sched, "interval": "step"}}


class DMTrainer(BaseTrainer):
    def __init__(self, model_config, te_use_normed_ctx=False, vae_std=None, vae_mean=None, lycoris_config=None, *args,
                 name="", lr=1e-5, optimizer=optim.AdamW, opt_config={"weight_decay": 0.01, "betas": (0.9, 0.999)},
                 lr_scheduler=lr_sch.CosineAnnealingLR, lr_scheduler_config={"T_max": 100_000, "eta_min": 1e-7},
                 use_warm_up=True, warm_up_period=1000, loss_config=None):
        super().__init__(*args, name=name, lr=lr, optimizer=optimizer, opt_config=opt_config,
                         lr_scheduler=lr_scheduler, lr_scheduler_config=lr_scheduler_config, use_warm_up=use_warm_up,
                         warm_up_period=warm_up_period)
        self.unet = load_any(model_config["unet"])
        self.te = load_any(model_config["te"]) if model_config.get("te") is not None else None
        # trainer.py:136,241-244: any frozen module with `.encode(x).latent_dist.sample()`: `diffusers.AutoencoderKL` resolves to
        # `uwudiff_amd.vae.AutoencoderKL` (the SDXL VAE on the HIP kernels; hub names give seeded random weights), and
        # `uwudiff_amd.conditioning.SyntheticVAE` is the 8x-pooling stand-in.  The (x - mean) / std step that follows the
        # encoder is folded into the loss's q-sample kernel.
        self.vae = load_any(model_config["vae"]) if model_config.get("vae") is not None else None
        if self.vae is not None:
            self.vae.requires_grad_(False).eval()
        self.te_use_normed_ctx = te_use_normed_ctx
        self.vae_std, self.vae_mean = vae_std, vae_mean or 0
        self.register_buffer("ema_loss", torch.tensor(0.0))
        self.ema_decay = 0.99
        # trainer.py:148-169: LyCORIS adapters (uwudiff_amd/adapters.py) on a frozen UNet; only the adapters train
        if lycoris_config is not None:
            from uwudiff_amd.adapters import LycorisNetwork

            if not hasattr(self.unet, "attach_adapters"):
                raise NotImplementedError(f"lycoris_config: adapters are implemented for the UNet, not for "
                                          f"{type(self.unet).__name__}")
            self.lycoris_model = LycorisNetwork(self.unet, lycoris_config)
            self.lycoris_model.apply_to(self.unet)
            self.lycoris_model.train()
            self.unet.requires_grad_(False)
            self.train_params = self.lycoris_model.parameters()
        else:
            self.lycoris_model = None
            self.unet.requires_grad_(True).train()
            self.train_params = self.unet.parameters()
        if loss_config is None:  # trainer.py:171-178: default = SDXL scheduler, epsilon objective
            from duwu.loss import DiffusionLoss
            from uwudiff_amd.scheduler import EulerDiscreteScheduler

            self.loss = DiffusionLoss(EulerDiscreteScheduler.from_pretrained(
                "stabilityai/stable-diffusion-xl-base-1.0", subfolder="scheduler"))
        else:
            self.loss = instantiate_any(loss_config)
        self.n_diffusion_time_steps = self.loss.n_diffusion_time_steps
        if self.vae is not None and self.vae_std is not None:
            if not hasattr(self.loss, "set_latent_normalisation"):
                raise NotImplementedError("vae_mean / vae_std need a loss with set_latent_normalisation (duwu.loss.*)")
            self.loss.set_latent_normalisation(self.vae_mean, self.vae_std)

    # trainer.py:233-261
    def get_latent_and_conditioning(self, batch):
        x, captions, tokenizer_outputs, added_cond, cross_attn_kwargs = batch
        ctx = attn_mask = pooled = None
        with torch.no_grad():
            if self.vae is not None:  # trainer.py:241-243 (the normalisation of :244 happens inside the loss kernel)
                x = self.vae.encode(x).latent_dist.sample()
            if self.te is not None:
                embedding, normed, pooled, attn_mask = self.te(tokenizer_outputs)
                ctx = normed if self.te_use_normed_ctx else embedding
        added_cond = dict(added_cond)
        added_cond["text_embeds"] = pooled
        return x, ctx, attn_mask, added_cond, cross_attn_kwargs

    # trainer.py:263-294 (the two .item() host syncs per step are left to the driver's periodic logging)
    def training_step(self, batch, idx):
        x, ctx, attn_mask, added_cond, cross_attn_kwargs = self.get_latent_and_conditioning(batch)
        loss, aux_output = self.loss(x, self.unet, encoder_hidden_states=ctx, encoder_attention_mask=attn_mask,
                                     added_cond_kwargs=added_cond, cross_attention_kwargs=cross_attn_kwargs)
        ema_decay = min(self.global_step / (10 + self.global_step), self.ema_decay)
        self.ema_loss = ema_decay * self.ema_loss + (1 - ema_decay) * loss.detach()
        return {"loss": loss, "aux_output": aux_output}

    def validation_step(self, batch, idx):
        x, ctx, attn_mask, added_cond, cross_attn_kwargs = self.get_latent_and_conditioning(batch)
        with torch.no_grad():
            return self.loss(x, self.unet, encoder_hidden_states=ctx, encoder_attention_mask=attn_mask,
                             added_cond_kwargs=added_cond, cross_attention_kwargs=cross_attn_kwargs)

    # trainer.py:184-187
    def merge_lycoris(self):
        """Fold the adapters into the UNet's base weights and detach them: a plain UNet remains (for sampling)."""
        self.lycoris_model.restore()
        self.lycoris_model.merge_to(self.unet)

    # trainer.py:189-215 (no loggers here: <default_root_dir>/lycoris_weight/epoch=N.pt)
    def on_train_epoch_end(self):
        if self.lycoris_model is None:
            return
        trainer = self._trainer
        epoch = trainer.current_epoch if trainer is not None else 0
        if trainer is not None and getattr(trainer, "global_rank", 0) != 0:
            return
        root = getattr(trainer, "default_root_dir", None) or "."
        d = os.path.join(root, "lycoris_weight")
        os.makedirs(d, exist_ok=True)
        torch.save(self.lycoris_model.state_dict(), os.path.join(d, f"epoch={epoch}.pt"))
