"""Step driver that replaces the subset of ``lightning.Trainer`` the reference's launcher uses
(test_scripts/test_train.py:43-77): device placement, the fit loop, backward, data-parallel gradient exchange,
global-norm clipping, optimizer + per-step LR schedule, rank-aware seeding, periodic logging, and the validation schedule
(``val_check_interval`` and its companions; a pass is :meth:`Fitter.validate`), and gradient accumulation
(``accumulate_grad_batches``: an optimizer step every N-th batch on the summed gradient / N), and the callback
hooks a weight average needs (``setup``, ``on_train_batch_end``, ``on_train_epoch_end``, ``on_train_end``, ``on_save_checkpoint``,
``on_load_checkpoint``, ``on_exception``, a callback's own ``state_dict``: uwudiff_amd/averaging.py).  The same
hooks carry the two modes of the schedule-free optimizer (``ScheduleFreeMode``, installed by ``fit`` itself: DESIGN.md section 4.42).

Lightning's loop is third-party control plane; the hot path it drives (loss -> denoiser fwd/bwd -> all-reduce ->
clip -> AdamW) is the part this build implements natively.  Checkpoint / resume follow Lightning's file layout
(``Fitter.save_checkpoint`` / ``fit(ckpt_path=...)``; the ``ModelCheckpoint`` callback of the YAMLs writes them).
"""
import json
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from .averaging import ScheduleFreeMode, WeightAveraging
from .gradsync import FlatGradSync
from .optim import FlatFusedOptimizer, FusedAdamWScheduleFree
from .preprocess import RaggedImages, ragged_to_device


def seed_everything(seed: int):
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)
    return seed


class ModelCheckpoint:
    """``lightning.pytorch.callbacks.ModelCheckpoint`` subset the reference configs use (configs/demo_training.yaml:14-19):
    ``dirpath``, ``filename``, ``every_n_train_steps`` (or ``every_n_epochs``), ``save_last``.  Registered by
    :meth:`Fitter.fit` as a step hook that calls :meth:`Fitter.save_checkpoint` (Lightning checkpoint layout).

    ``monitor`` naming a key of the validation record (``val/loss``) switches to "the best k by that value": one file at the end of
    every validation pass that is no sanity pass, the best ``save_top_k`` (default 1, Lightning's) by ``mode`` kept, the others removed;
    the periodic triggers are then off (``save_last`` still writes).  ``monitor: step`` or none: the newest k files, as before."""

    def __init__(self, dirpath=None, filename=None, every_n_train_steps=None, every_n_epochs=None, save_last=False,
                 save_top_k=None, monitor=None, mode="min", **kw):
        self.dirpath = dirpath or "checkpoints"
        self.filename = filename or "epoch={epoch}-step={step}"  # Lightning's default name
        self.every_n_train_steps = int(every_n_train_steps) if every_n_train_steps else None
        self.every_n_epochs = int(every_n_epochs) if every_n_epochs else None
        self.save_last = bool(save_last)
        self.save_top_k = save_top_k  # monitor: step / mode: max (the reference YAML) == keep the newest k files
        self.kw = kw
        self.saved = []
        self.monitor = None if monitor in (None, "step") else str(monitor)
        if mode not in ("min", "max"):
            raise ValueError(f"ModelCheckpoint: mode must be 'min' or 'max', got {mode!r}")
        self.mode = mode
        self.best = []  # (path, score) of the files kept for `monitor`, best first

    def _rank(self, score):
        """sort key, best first; a NaN score is the worst in either mode"""
        if score != score:
            return float("inf")
        return score if self.mode == "min" else -score

    def on_validation_end(self, fitter, module=None):
        if self.monitor is None or fitter.sanity_checking or fitter.fast_dev_run or not fitter.val_history:
            return  # (Lightning's fast_dev_run disables checkpoint callbacks)
        rec = fitter.val_history[-1]
        if self.monitor not in rec:
            raise KeyError(f"ModelCheckpoint: monitor {self.monitor!r} is no key of the validation record {sorted(rec)}")
        k = 1 if self.save_top_k is None else int(self.save_top_k)
        if k == 0:
            return
        path, score = self._path(fitter), float(rec[self.monitor])
        ranked = sorted([(p, s) for p, s in self.best if p != path] + [(path, score)], key=lambda e: self._rank(e[1]))
        keep = ranked if k < 0 else ranked[:k]
        if (path, score) not in keep:  # (not among the best k: nothing is written)
            return
        fitter.save_checkpoint(path, callbacks={"ModelCheckpoint": {"saved": list(self.saved), "best": [[p, s] for p, s in keep]}})
        if fitter.global_rank == 0:
            for old, _ in ranked[len(keep):]:
                if os.path.exists(old):
                    os.remove(old)
        self.best = keep

    def _save(self, fitter, path):
        k = self.save_top_k
        if k == 0:  # Lightning: save_top_k = 0 keeps no periodic file (save_last still writes "last"), -1 keeps all
            return
        fitter.save_checkpoint(path, callbacks={"ModelCheckpoint": {"saved": self.saved + [path]}})
        self.saved.append(path)
        if k is not None and k > 0 and fitter.global_rank == 0:
            while len(self.saved) > k:
                old = self.saved.pop(0)
                if os.path.exists(old):
                    os.remove(old)

    def _path(self, fitter, name=None):
        name = name or self.filename.format(step=fitter.global_step, epoch=fitter.current_epoch)
        return os.path.join(self.dirpath, name + ".ckpt")

    def on_step(self, fitter):
        if self.monitor is None and self.every_n_train_steps and fitter.global_step % self.every_n_train_steps == 0:
            self._save(fitter, self._path(fitter))

    def on_epoch_end(self, fitter):
        if self.monitor is None and self.every_n_epochs and (fitter.current_epoch + 1) % self.every_n_epochs == 0:
            self._save(fitter, self._path(fitter))

    def on_fit_end(self, fitter):
        if self.save_last:
            fitter.save_checkpoint(self._path(fitter, "last"), callbacks={"ModelCheckpoint": {
                "saved": list(self.saved), "best": [[p, s] for p, s in self.best]}} if self.monitor is not None else None)


class LearningRateMonitor:
    """Lightning's callback of that name: `lr` is in every logged record already; with this callback present, an optimizer that
    estimates its own step size (``FusedProdigy.d``: a device scalar, a host synchronisation to read) has it logged next to `lr`,
    at the logging interval only."""

    def __init__(self, **kw):
        self.kw = kw

    def extra(self, opt):
        out = {"d": float(opt.d)} if hasattr(opt, "d") else {}
        if getattr(opt, "lr_t", None) is not None:  # Adafactor: the step size of the last step (with relative_step `lr` is None)
            out["lr_t"] = float(opt.lr_t)
        if "scheduled_lr" in opt.param_groups[0]:  # schedule-free AdamW: `lr` times its own warm-up (a host float, no sync)
            out["scheduled_lr"] = float(opt.param_groups[0]["scheduled_lr"])
        return out


class GradualWarmupScheduler:
    """``warmup_scheduler.GradualWarmupScheduler(optimizer, 1, warm_up_period, after)`` semantics
    (reference trainer.py:61-64): lr = base_lr * step / period during warm-up, then ``after``."""

    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        assert multiplier == 1
        self.optimizer, self.total, self.after = optimizer, total_epoch, after_scheduler
        self.base = [g["lr"] for g in optimizer.param_groups]
        self.n = 0
        self._apply()

    def _apply(self):
        if self.n <= self.total:
            for g, b in zip(self.optimizer.param_groups, self.base):
                g["lr"] = b * (float(self.n) / self.total)

    def step(self):
        self.n += 1
        if self.n > self.total and self.after is not None:
            self.after.step()
        else:
            self._apply()

    # resume (reference trainer.py:76-92 re-links the wrapped scheduler's optimizer on load; here both live in one state)
    def state_dict(self):
        after = self.after.state_dict() if self.after is not None and hasattr(self.after, "state_dict") else None
        return {"n": self.n, "base": list(self.base), "total": self.total, "after": after,
                "lr": [g["lr"] for g in self.optimizer.param_groups]}

    def load_state_dict(self, sd):
        self.n, self.base, self.total = int(sd["n"]), list(sd["base"]), sd["total"]
        if sd.get("after") is not None and self.after is not None:
            self.after.load_state_dict(sd["after"])
        for g, lr in zip(self.optimizer.param_groups, sd["lr"]):  # the LR in force when the checkpoint was written
            g["lr"] = lr


def _dist_env():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return rank, world, local


class Fitter:
    def __init__(self, max_steps=-1, precision="bf16-mixed", gradient_clip_val=None, fast_dev_run=False,
                 log_every_n_steps=10, accelerator="gpu", devices=1, strategy=None, callbacks=(), logger=(),
                 max_epochs=None, default_root_dir=None, val_check_interval=1.0, check_val_every_n_epoch=1, limit_val_batches=1.0,
                 num_sanity_val_steps=2, val_seed=0, accumulate_grad_batches=1, **ignored):
        self.max_steps = max_steps
        n_acc = accumulate_grad_batches
        if isinstance(n_acc, dict):
            raise TypeError(f"accumulate_grad_batches must be an int >= 1, got the dict {n_acc!r}: a per-epoch schedule is Lightning's "
                            f"GradientAccumulationScheduler callback, which is not built")
        if isinstance(n_acc, bool) or not isinstance(n_acc, int) or n_acc < 1:
            raise TypeError(f"accumulate_grad_batches must be an int >= 1, got {n_acc!r}")
        self.accumulate_grad_batches = n_acc
        self.accum_pending = 0  # micro-batches summed into the gradient and not yet applied (0 at every optimizer step)
        self.train_batches = 0  # training batches consumed over all epochs (== global_step when accumulate_grad_batches is 1)
        self.default_root_dir = os.fspath(default_root_dir) if default_root_dir is not None else os.getcwd()
        self.precision = str(precision)
        self.gradient_clip_val = gradient_clip_val
        self.fast_dev_run = fast_dev_run
        self.log_every_n_steps = max(1, int(log_every_n_steps))
        self.max_epochs = max_epochs
        self.global_rank, self.world_size, self.local_rank = _dist_env()
        self.global_step = 0
        self.current_epoch = 0
        self.history = []
        self.val_history = []  # one record per validation pass (the sanity pass leaves none)
        for name, v in (("val_check_interval", val_check_interval), ("limit_val_batches", limit_val_batches)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v < 0 or (isinstance(v, float) and v > 1.0):
                raise ValueError(f"{name} must be a float in [0, 1] or a non-negative int, got {v!r}")
        if isinstance(val_check_interval, float) and val_check_interval == 0.0:
            raise ValueError("val_check_interval must be a float in (0, 1] or a positive int, got 0.0")
        if check_val_every_n_epoch is not None and (isinstance(check_val_every_n_epoch, bool) or int(check_val_every_n_epoch) < 1):
            raise ValueError(f"check_val_every_n_epoch must be a positive int or None, got {check_val_every_n_epoch!r}")
        self.val_check_interval = val_check_interval
        self.check_val_every_n_epoch = None if check_val_every_n_epoch is None else int(check_val_every_n_epoch)
        self.limit_val_batches = limit_val_batches
        self.num_sanity_val_steps = int(num_sanity_val_steps)
        self.val_seed = int(val_seed)
        self.sanity_checking = False
        self.val_stats = None
        self.step_hooks = []  # callables(fitter) run after every optimizer step (e.g. periodic save_checkpoint)
        self.callbacks = list(callbacks or [])
        if sum(isinstance(cb, WeightAveraging) for cb in self.callbacks) > 1:
            raise ValueError("more than one weight-averaging callback: one average is kept per fit (averaging.py)")
        use_gpu = torch.cuda.is_available() and str(accelerator) != "cpu"
        if self.world_size > 1 and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl" if use_gpu else "gloo")
        if use_gpu:
            torch.cuda.set_device(self.local_rank)
            self.device = torch.device("cuda", self.local_rank)
        else:
            self.device = torch.device("cpu")

    @property
    def compute_dtype(self):
        return "fp32" if self.precision.startswith("32") else "bf16"

    # ------------------------------------------------------------------ checkpoint / resume
    # Lightning's checkpoint layout (the keys `Trainer.fit(ckpt_path=...)` and the reference's loader read:
    # loader.py:24-46 extracts `state_dict` entries by prefix, e.g. "unet."): the module's state_dict carries the
    # denoiser as `unet.<diffusers-style names>`, optimizer / scheduler states are the torch ones.
    def save_checkpoint(self, path, callbacks=None):
        """Write the state of the current / last ``fit`` (rank 0 only).  Returns the dict that was saved."""
        module, opt, sched = self._fit_state

        def snap(o):  # detached CPU copy (torch's optimizer.state_dict() aliases the live state)
            if torch.is_tensor(o):
                return o.detach().cpu().clone()
            if isinstance(o, dict):
                return {k: snap(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return type(o)(snap(v) for v in o)
            return o

        # "batches_in_epoch": how far into epoch `epoch` the run was (not inferred from global_step % len(loader),
        # which is wrong once an epoch was cut short by max_steps or the loader length changes)
        ckpt = {"epoch": self.current_epoch, "global_step": self.global_step, "pytorch-lightning_version": "uwudiff_amd",
                "batches_in_epoch": int(getattr(self, "batches_in_epoch", 0)),
                # the batch counter of its own (val_check_interval counts batches, global_step optimizer steps) and how many of those
                # batches sit in the gradient unapplied: a resume replays them
                "train_batches": int(self.train_batches), "accum_pending": int(self.accum_pending),
                "callbacks": dict(callbacks or {}),
                "state_dict": snap(dict(module.state_dict())),
                "optimizer_states": [snap(opt.state_dict())],
                "lr_schedulers": [sched.state_dict()] if sched is not None and hasattr(sched, "state_dict") else []}
        for cb in self.callbacks:  # a callback with state of its own (Lightning's Callback.state_dict / state_key)
            if callable(getattr(cb, "state_dict", None)):
                ckpt["callbacks"][getattr(cb, "state_key", type(cb).__name__)] = cb.state_dict()
        self._hook("on_save_checkpoint", module, ckpt)
        if self.global_rank == 0:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            torch.save(ckpt, path)
        return ckpt

    def load_checkpoint(self, path):
        """Resume: parameters (+ bf16 shadow), optimizer moments / step count, scheduler, global_step."""
        module, opt, sched = self._fit_state
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        two_sets = (WeightAveraging, ScheduleFreeMode)  # who reads current_model_state
        if "current_model_state" in ckpt and not any(isinstance(cb, two_sets) for cb in self.callbacks) and self.global_rank == 0:
            print("resume: the checkpoint was written with weight averaging and this run has no such callback: the averaged weights "
                  "of state_dict are loaded, the trained weights under current_model_state were not used", flush=True)
        self._hook("on_load_checkpoint", module, ckpt)  # (may redirect ckpt["state_dict"])
        sd = ckpt["state_dict"]
        # the denoiser keeps ONE flat parameter and exposes named views: it restores itself from the `unet.*` entries;
        # everything else (buffers such as ema_loss, other sub-modules) goes through the generic loader
        module.unet.load_state_dict({k[len("unet."):]: v for k, v in sd.items() if k.startswith("unet.")})
        rest = {k: v for k, v in sd.items() if not k.startswith("unet.")}
        unexpected = module.load_state_dict(rest, strict=False).unexpected_keys
        if unexpected:
            raise RuntimeError(f"checkpoint has entries this trainer does not know: {unexpected[:5]}")
        if hasattr(module.unet, "refresh_shadow"):
            module.unet.refresh_shadow()
        opt.load_state_dict(ckpt["optimizer_states"][0])
        if sched is not None and ckpt.get("lr_schedulers") and hasattr(sched, "load_state_dict"):
            sched.load_state_dict(ckpt["lr_schedulers"][0])
        self.global_step = int(ckpt["global_step"])
        self.current_epoch = int(ckpt.get("epoch", 0))
        self._resume_batches = ckpt.get("batches_in_epoch")  # None: a checkpoint of an earlier version
        self._resume_pending = int(ckpt.get("accum_pending", 0))
        self.train_batches = int(ckpt.get("train_batches", self.global_step))  # (earlier versions: one step per batch)
        state = (ckpt.get("callbacks") or {}).get("ModelCheckpoint", {})
        saved, best = state.get("saved"), state.get("best")
        for cb in self.callbacks:  # top-k pruning continues over the files the interrupted run had written
            if isinstance(cb, ModelCheckpoint):
                if saved is not None:
                    cb.saved = list(saved)
                if best is not None:
                    cb.best = [(p, float(s)) for p, s in best]
            else:
                own = (ckpt.get("callbacks") or {}).get(getattr(cb, "state_key", type(cb).__name__))
                if own is not None and callable(getattr(cb, "load_state_dict", None)):
                    cb.load_state_dict(own)
        return ckpt

    def _to_device(self, batch):
        x, captions, tok, added, ca = batch
        if isinstance(x, RaggedImages):  # decoded pictures of a folder dataset: resized, cropped and normalised on the device
            x = ragged_to_device(x, self.device)
        else:
            x = x.to(self.device, non_blocking=True)
        tok = [{k: v.to(self.device, non_blocking=True) for k, v in t.items()} for t in tok]
        added = {k: v.to(self.device, non_blocking=True) for k, v in added.items()}
        return x, captions, tok, added, ca

    # ------------------------------------------------------------------ validation
    def _hook(self, name, *args):
        for cb in self.callbacks:
            fn = getattr(cb, name, None)
            if fn is not None:
                fn(self, *args)

    def _n_val_batches(self, loader):
        n = len(loader)
        if self.fast_dev_run:
            return min(1, n)
        lim = self.limit_val_batches
        return int(n * lim) if isinstance(lim, float) else min(int(lim), n)

    def _val_due(self, k, n_batches, epoch):
        """validate after training batch k (1-based) of `epoch`?  Lightning's rules, as its documentation states them."""
        if self.fast_dev_run:
            return True
        vci, every = self.val_check_interval, self.check_val_every_n_epoch
        if every is None:
            if isinstance(vci, float):
                raise ValueError("check_val_every_n_epoch: null needs an int val_check_interval (a number of training batches)")
            return self.train_batches % vci == 0
        if (epoch + 1) % every != 0:
            return False
        period = max(1, int(n_batches * vci)) if isinstance(vci, float) else vci
        return k % period == 0

    def validate(self, module, loader, limit=None, sanity=False):
        """One validation pass over (the first ``limit`` batches of) ``loader``: ``module.validation_step(batch, idx) -> (loss, aux)``
        under ``no_grad`` in eval mode, ``aux.losses`` / ``aux.timesteps`` / ``loss`` into a :class:`TimestepLossStats`, one all-reduce
        and ONE device-to-host read at the end.  Returns the record that is appended to ``val_history`` (a sanity pass appends nothing).

        The pass draws from its own random stream (``val_seed``: every pass sees the same timesteps and noise) and leaves training where
        it was: the device generator's (seed, offset), the CPU generator (a DataLoader iterator draws from it), every sub-module's
        train / eval flag and the DiT's fp8 step counters are saved before and put back after.  It takes no optimizer step, calls no
        backward and does not write ``ema_loss`` or ``global_step``."""
        from .validation import TimestepLossStats

        t_start = time.time()
        cuda_gen = None
        if self.device.type == "cuda":
            cuda_gen = torch.cuda.default_generators[self.device.index if self.device.index is not None else torch.cuda.current_device()]
            cuda_state = cuda_gen.get_state()
        cpu_state = torch.get_rng_state()
        modes = [(m, m.training) for m in module.modules()]
        unet = getattr(module, "unet", None)
        f8 = {k: getattr(unet, k) for k in ("_f8_steps", "_f8_mode") if hasattr(unet, k)}
        self.sanity_checking = bool(sanity)
        n_seen = 0
        try:
            if cuda_gen is not None:
                cuda_gen.manual_seed(self.val_seed)
            torch.default_generator.manual_seed(self.val_seed)
            module.eval()
            stats = None
            with torch.no_grad():
                self._hook("on_validation_epoch_start", module)
                for idx, batch in enumerate(loader):
                    if limit is not None and idx >= limit:
                        break
                    batch = self._to_device(batch)
                    out = module.validation_step(batch, idx)
                    loss, aux = out
                    if stats is None:
                        stats = self.val_stats
                        if stats is None or stats.n_steps != int(module.n_diffusion_time_steps) or stats.device != aux.losses.device:
                            stats = self.val_stats = TimestepLossStats(module.n_diffusion_time_steps, aux.losses.device)
                        stats.reset()
                    stats.update(aux.losses, aux.timesteps, loss)
                    self._hook("on_validation_batch_end", module, out, batch, idx)
                    n_seen += 1
                res = stats.reduce().compute() if stats is not None else {"loss": float("nan"), "n_samples": 0}
                rec = {"step": self.global_step, "epoch": self.current_epoch, "val/loss": res["loss"],
                       "val_samples": int(res["n_samples"]), "elapsed_s": round(time.time() - getattr(self, "_t0", t_start), 3)}
                if not sanity:
                    self.val_history.append(rec)
                    if self.global_rank == 0:
                        print(json.dumps(rec), flush=True)
                self._hook("on_validation_epoch_end", module)
        except BaseException as e:  # (a callback that changed something for the pass puts it back: the weight average does)
            self._hook("on_exception", module, e)
            raise
        finally:
            for m, was in modes:
                m.training = was
            for k, v in f8.items():
                setattr(unet, k, v)
            torch.set_rng_state(cpu_state)
            if cuda_gen is not None:
                cuda_gen.set_state(cuda_state)
        try:
            self._hook("on_validation_end", module)
        finally:
            self.sanity_checking = False
        return rec

    def fit(self, module, datamodule, ckpt_path=None):
        if hasattr(module.unet, "cfg"):
            module.unet.cfg.compute_dtype = self.compute_dtype
            if hasattr(module.unet, "P"):
                module.unet.P.bf16 = self.compute_dtype == "bf16"
        module.to(self.device)
        module._trainer = self
        datamodule.setup("fit")
        loader = datamodule.train_dataloader()
        val_loader = datamodule.val_dataloader() if hasattr(datamodule, "val_dataloader") else None
        n_val = 0
        if val_loader is not None and hasattr(module, "validation_step"):
            n_val = self._n_val_batches(val_loader)  # 0 (limit_val_batches = 0, an empty loader): validation is off
        cfg = module.configure_optimizers()
        opt = cfg["optimizer"] if isinstance(cfg, dict) else cfg
        sched = cfg["lr_scheduler"]["scheduler"] if isinstance(cfg, dict) and "lr_scheduler" in cfg else None
        fused = isinstance(opt, FlatFusedOptimizer)
        # the schedule-free optimizer trains y and evaluates x: its two modes ride on the callback hooks, ahead of the user's callbacks
        self.callbacks[:] = [cb for cb in self.callbacks if not isinstance(cb, ScheduleFreeMode)]  # (an earlier fit's)
        if isinstance(opt, FusedAdamWScheduleFree):
            averaging = [type(cb).__name__ for cb in self.callbacks if isinstance(cb, WeightAveraging)]
            if averaging:
                raise ValueError(f"{averaging[0]} together with {type(opt).__name__} (schedulefree.AdamWScheduleFree): the callback would "
                                 f"average y, the point the gradient is taken at, which is no model to evaluate; the optimizer keeps "
                                 f"its own average x and fit validates and saves that one.  Remove the callback")
            self.callbacks.insert(0, ScheduleFreeMode(opt))
        sync = FlatGradSync(self.world_size)
        lyc = getattr(module, "lycoris_model", None)  # adapter training: the UNet is frozen, the adapter buffer trains
        if fused and lyc is None:  # the early (inside-backward) reduction is consumed by the fused optimizers' per-chunk waits only; a foreign
            sync.attach(module.unet)  # optimizer takes the plain whole-buffer exchange below
        elif hasattr(module.unet, "set_grad_ready_hook"):
            module.unet.set_grad_ready_hook(None)
        self._fit_state = (module, opt, sched)
        if ckpt_path is not None:
            self.load_checkpoint(ckpt_path)
        if self.world_size > 1 and hasattr(module.unet, "flat"):
            # identical replicas (Lightning DDP broadcasts rank 0's module state): do not rely on per-rank seeding order
            dist.broadcast(module.unet.flat.data, src=0)
            if lyc is not None:  # (the adapter gradient is exchanged whole-buffer below: it is small)
                dist.broadcast(lyc.flat.data, src=0)
                lyc.mark_dirty()
            if hasattr(module.unet, "refresh_shadow"):
                module.unet.refresh_shadow()
        self._hook("setup", module, "fit")  # the weights are what training starts from (a weight average is created here)
        # Lightning's fast_dev_run disables checkpoint callbacks and loggers
        ckpt_cbs = [] if self.fast_dev_run else [cb for cb in self.callbacks if isinstance(cb, ModelCheckpoint)]
        params = [p for g in opt.param_groups for p in g["params"]]
        max_steps = 1 if self.fast_dev_run else self.max_steps
        t0 = self._t0 = time.time()
        epoch = self.current_epoch if ckpt_path is not None else 0  # a resumed run continues its epoch count (max_epochs, {epoch})
        done = False
        # resume mid-epoch like Lightning does: skip the batches the interrupted epoch had already consumed
        n_batches = max(len(loader), 1)
        if n_val and not self.fast_dev_run:
            vci = self.val_check_interval
            if self.check_val_every_n_epoch is None and isinstance(vci, float):
                raise ValueError("check_val_every_n_epoch: null needs an int val_check_interval (a number of training batches)")
            if self.check_val_every_n_epoch is not None and not isinstance(vci, float) and vci > n_batches:
                raise ValueError(f"val_check_interval ({vci}) is larger than the number of training batches of an epoch ({n_batches}); "
                                 f"set check_val_every_n_epoch: null to count batches across epochs")
            if isinstance(vci, int) and vci < 1:
                raise ValueError("val_check_interval must be a float in (0, 1] or a positive int, got 0")
        n_acc = self.accumulate_grad_batches
        resume_skip = 0
        if ckpt_path is not None:
            rb = getattr(self, "_resume_batches", None)
            if rb is None and n_acc > 1:
                raise ValueError("this checkpoint does not say how far into its epoch it was written, and global_step counts optimizer "
                                 "steps, not batches, when accumulate_grad_batches > 1: resume it with accumulate_grad_batches = 1")
            resume_skip = int(rb) if rb is not None else (self.global_step % n_batches)
            if rb is None and resume_skip == 0 and self.global_step > 0:
                resume_skip = n_batches  # (old checkpoints: written after the last batch of their epoch)
            if resume_skip >= n_batches:
                epoch += 1  # the checkpoint was written after the last batch of its epoch: that epoch is complete
                resume_skip = 0
            pending = min(getattr(self, "_resume_pending", 0), resume_skip)
            if pending:  # written inside a window (a validation-triggered save): the partial sum is not stored, the window starts again
                resume_skip -= pending
                self.train_batches -= pending
                if self.global_rank == 0:
                    print(f"resume: the checkpoint was written {pending} batch(es) into an accumulation window; replaying them "
                          f"from batch {resume_skip + 1} of epoch {epoch}", flush=True)
        self.current_epoch = epoch
        self.batches_in_epoch = resume_skip
        self.accum_pending = 0
        grads_zeroed = False
        one = None
        if n_val and ckpt_path is None and not self.fast_dev_run and self.num_sanity_val_steps != 0:
            # Lightning's sanity check: a few validation batches before the first training step (not on a resume: the interrupted run
            # had none at this point); its results reach the callbacks only
            ns = self.num_sanity_val_steps
            self.validate(module, val_loader, limit=n_val if ns < 0 else min(ns, n_val), sanity=True)
        while not done:
            finished_epoch, ran = True, 0
            for bi, batch in enumerate(loader):
                if bi < resume_skip:
                    continue
                if 0 <= max_steps <= self.global_step:  # nothing left to do (resumed at max_steps)
                    done, finished_epoch = True, False
                    break
                module.global_step = self.global_step
                # an optimizer step follows batch k (1-based) of the epoch when k % N == 0 or k is the epoch's last: windows never
                # span epochs.  Every other batch only adds into the gradient.
                boundary = n_acc == 1 or (bi + 1) % n_acc == 0 or bi + 1 >= n_batches or bool(self.fast_dev_run)
                # (a fused step leaves the gradients zeroed: FlatFusedOptimizer.step(zero_grad=True); inside a window nothing is zeroed)
                if not grads_zeroed and self.accum_pending == 0:
                    for p in params:
                        if p.grad is not None:
                            p.grad.zero_()
                sync.defer(not boundary)  # no exchange inside a window: the boundary's backward and all_reduce carry the whole sum
                batch = self._to_device(batch)
                out = module.training_step(batch, self.global_step)
                loss = out["loss"]
                if one is None or one.device != loss.device or one.dtype != loss.dtype:
                    one = torch.ones_like(loss)  # (kept: autograd's own ones_like(loss) is a fill launch per step)
                loss.backward(one)
                self.accum_pending += 1
                self.train_batches += 1
                ran += 1
                self.batches_in_epoch = bi + 1
                if not boundary:
                    grads_zeroed = False  # (what the last step zeroed now holds a partial sum)
                    self._hook("on_train_batch_end", module, out, batch, bi)
                    if n_val and self._val_due(bi + 1, n_batches, epoch):
                        self.validate(module, val_loader, limit=n_val)  # (writes no gradient: the partial sum survives the pass)
                    continue
                window, self.accum_pending = self.accum_pending, 0
                # the gradient used is (sum over the window) / N, also in a short last window (Lightning divides every loss by N);
                # 1/N rides on the factor that already carries 1/world into the norm and update kernels
                scale = sync.pre_scale / n_acc
                clip = None
                if isinstance(opt, FlatFusedOptimizer):
                    chunks = sync.all_reduce(params[0].grad)
                    if self.gradient_clip_val:
                        sync.wait_all()
                        clip = opt.grad_norm_clip(self.gradient_clip_val, pre_scale=scale)
                        opt.step(clip=clip, pre_scale=scale, zero_grad=True)
                    else:
                        opt.step(pre_scale=scale, chunks=chunks, before_chunk=sync.wait_chunk, zero_grad=True)
                    grads_zeroed = True
                else:  # foreign optimizer (e.g. lion): plain torch path on the flat buffer
                    for p in params:
                        if self.world_size > 1:
                            sync.all_reduce(p.grad)  # same chunked exchange; nothing was reduced early (no hook)
                            sync.wait_all()
                        if self.world_size > 1 or n_acc > 1:
                            p.grad.mul_(scale)
                    if self.gradient_clip_val:
                        torch.nn.utils.clip_grad_norm_(params, self.gradient_clip_val)
                    opt.step()
                    if lyc is not None:
                        lyc.mark_dirty()  # (the adapters are merged again by the next forward; the base shadow is unchanged)
                    elif hasattr(module.unet, "refresh_shadow"):
                        module.unet.refresh_shadow()
                if sched is not None:
                    sched.step()
                self.global_step += 1
                if 0 <= max_steps <= self.global_step:  # checked at the END of the step: no empty extra epoch afterwards
                    done = True
                    finished_epoch = bi + 1 >= n_batches
                self._hook("on_train_batch_end", module, out, batch, bi)
                for hook in self.step_hooks:
                    hook(self)
                for cb in ckpt_cbs:
                    cb.on_step(self)
                if self.global_step % self.log_every_n_steps == 0 or self.fast_dev_run or done:
                    rec = {"step": self.global_step, "loss": float(loss.detach()), "ema_loss": float(module.ema_loss),
                           "lr": opt.param_groups[0]["lr"], "elapsed_s": round(time.time() - t0, 3)}
                    for cb in self.callbacks:
                        if isinstance(cb, LearningRateMonitor):
                            rec.update(cb.extra(opt))
                    if n_acc > 1:
                        rec["accum"] = window  # micro-batches in this window (`loss` is the last one's, as Lightning's on_step log)
                    self.history.append(rec)
                    if self.global_rank == 0:
                        print(json.dumps(rec), flush=True)
                if n_val and self._val_due(bi + 1, n_batches, epoch):
                    self.validate(module, val_loader, limit=n_val)
                if done:
                    break
            if not finished_epoch or (ran == 0 and resume_skip == 0 and done):
                break  # cut short by max_steps: the epoch is partial -- no epoch-end hooks, no epoch count
            if hasattr(module, "on_train_epoch_end"):
                module.on_train_epoch_end()
            self._hook("on_train_epoch_end", module)
            for cb in ckpt_cbs:
                cb.on_epoch_end(self)
            epoch += 1
            self.current_epoch = epoch
            self.batches_in_epoch = 0
            resume_skip = 0
            if self.max_epochs is not None and epoch >= self.max_epochs:
                break
            if max_steps < 0 and self.max_epochs is None:
                break  # one pass when neither bound is given
        for cb in ckpt_cbs:
            cb.on_fit_end(self)
        self._hook("on_train_end", module)  # (after the `last` checkpoint: that file resumes; the module returned holds the average)
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return self.history
