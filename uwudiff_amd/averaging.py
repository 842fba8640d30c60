"""An average of the trained weights kept on the device: ``lightning.pytorch.callbacks.WeightAveraging`` and
``EMAWeightAveraging`` (built there on ``torch.optim.swa_utils.AveragedModel``) on the flat parameter buffer.

``FlatAverage`` is the average itself: one fp32 buffer as long as the trained flat buffer, updated by ``uwu_ema_update`` and put in place
of the weights -- and back -- by ``uwu_ema_swap``, which moves the numbers and no pointer (the DiT driver, the adapter merge and the
fused optimizers hold raw pointers into ``flat`` and ``shadow``).  The two callbacks drive it from the hooks of ``Fitter``: an update
after an optimizer step, the average in place of the weights round every validation pass, both sets of weights in a checkpoint, the
average in the module when ``fit`` returns.
"""
import torch

from . import lib as L
from .flat import FlatModule


class FlatAverage:
    """The average of ``owner.flat``: ``owner`` is the module that holds the trained flat buffer (a ``FlatModule``, or the adapter
    network when adapters train).  4 bytes per parameter next to the weights; there is no CPU path."""

    def __init__(self, owner):
        flat = getattr(owner, "flat", None)
        if not torch.is_tensor(flat):
            raise TypeError(f"FlatAverage needs a module with a flat parameter buffer, got {type(owner).__name__}")
        if not flat.is_cuda:
            raise L.UwuError("FlatAverage keeps the average on the HIP device next to the weights (got a CPU tensor); there is no CPU path")
        self.owner = owner
        self.avg = torch.empty_like(flat.data)
        self.n_averaged = 0
        self.reset()

    # ------------------------------------------------------------------ the buffers the kernels address
    def _flat(self):
        flat = self.owner.flat.data
        if flat.device != self.avg.device or flat.numel() != self.avg.numel() or flat.dtype != torch.float32:
            raise L.UwuError("FlatAverage: the flat buffer was moved or resized after the average was created")
        return flat

    def _shadow(self):
        """the bf16 shadow the swap kernel refreshes in the same pass (None: fp32 mode, no shadow yet, or the adapter network)"""
        o = self.owner
        if not isinstance(o, FlatModule) or not o._wants_shadow():
            return None
        sh = o.shadow
        return sh if sh.numel() == self.avg.numel() and sh.device == self.avg.device else None

    def _weights_written(self, shadow_done):
        o = self.owner
        if isinstance(o, FlatModule):
            if shadow_done:
                o._shadow_stale()  # (the shadow itself is fresh: the kernel wrote it)
            else:
                o.refresh_shadow()
        else:
            o.mark_dirty()  # the UNet merges the adapters again before its next forward

    # ------------------------------------------------------------------ the average
    @torch.no_grad()
    def reset(self):
        """the average becomes a device copy of the weights; the next ``update`` is a plain copy"""
        self.avg.copy_(self._flat())
        self.n_averaged = 0

    @torch.no_grad()
    def update(self, keep, take):
        """avg = keep * avg + take * weights (both coefficients rounded once to fp32); the first update after a ``reset`` is a plain copy,
        as ``AveragedModel.update_parameters`` does at ``n_averaged == 0``"""
        flat = self._flat()
        if self.n_averaged == 0:
            self.avg.copy_(flat)
        else:
            L.call("uwu_ema_update", L.ptr(self.avg), L.ptr(flat), flat.numel(), float(keep), float(take), L.stream())
        self.n_averaged += 1

    def _swap(self, mode):
        flat, sh = self._flat(), self._shadow()
        L.call("uwu_ema_swap", L.ptr(self.avg), L.ptr(flat), L.ptr(sh), flat.numel(), mode, L.stream())
        self._weights_written(sh is not None)

    @torch.no_grad()
    def swap(self):
        """exchange the average and the weights bit for bit (its own inverse); the shadow follows the weights"""
        self._swap(0)

    @torch.no_grad()
    def copy_to_current(self):
        """the weights (and their shadow) become the average; the average stays"""
        self._swap(1)

    # ------------------------------------------------------------------ state dict entries read from / written to the average
    def _views(self):
        o = self.owner
        if isinstance(o, FlatModule):
            return dict(o._public_views(self.avg))
        return {f"{s.key}.{t}": o.view(s.name, t, buf=self.avg) for s in o.specs for t, _ in s.tensors}

    def averaged_state(self):
        """the owner's public state-dict entries with the tensors read from the average"""
        o = self.owner
        if isinstance(o, FlatModule):
            return {k: v.detach().clone().contiguous() for k, v in self._views().items()}
        sd = {}
        for s in o.specs:  # (the order and the alpha entries of LycorisNetwork.state_dict)
            for t, _ in s.tensors:
                sd[f"{s.key}.{t}"] = o.view(s.name, t, buf=self.avg).detach().clone(memory_format=torch.contiguous_format)
            if s.alpha is not None:
                sd[f"{s.key}.alpha"] = torch.tensor(s.alpha)
        return sd

    @torch.no_grad()
    def load_averaged_state(self, sd):
        """the reverse of ``averaged_state``: every tensor of the average must be there with its shape; nothing else is written"""
        o = self.owner
        views = self._views()
        if isinstance(o, FlatModule):
            sd = o._prepare_load(dict(sd))
            sd = {o._load_key(k): v for k, v in sd.items() if o._load_key(k) is not None}
        else:
            sd = {k: v for k, v in sd.items() if not k.endswith(".alpha")}
        missing = [k for k in views if k not in sd]
        unexpected = [k for k in sd if k not in views]
        wrong = [k for k in views if k in sd and tuple(sd[k].shape) != tuple(views[k].shape)]
        if missing or unexpected or wrong:
            raise RuntimeError(f"averaged weights do not fit {type(o).__name__}: missing {missing[:5]}, unexpected {unexpected[:5]}, "
                               f"size mismatch {wrong[:5]}")
        if isinstance(o, FlatModule):
            for k, v in views.items():
                v.copy_(sd[k])
        else:  # (a convolution adapter's public shape is not always a view of the buffer: LycorisNetwork.write permutes)
            for s in o.specs:
                for t, _ in s.tensors:
                    o.write(s.name, t, sd[f"{s.key}.{t}"].to(self.avg.device), buf=self.avg)


class WeightAveraging:
    """``lightning.pytorch.callbacks.WeightAveraging``: the running mean of the weights over the optimizer steps for which
    ``should_update`` says yes (subclasses override it), on the device.

    Only the trained flat buffer is averaged (the denoiser's, or the adapter network's when adapters train).  ``use_buffers`` is accepted
    and has no effect: module buffers (``ema_loss``) and the frozen sub-modules are written to a checkpoint as they are.  ``device`` must
    be None or the model's device: the average lives next to the weights.  ``avg_fn`` / ``multi_avg_fn`` callables are not supported."""

    state_key = "WeightAveraging"  # the key of ``state_dict()`` under ``ckpt["callbacks"]``, for subclasses too

    def __init__(self, device=None, use_buffers=True, **kwargs):
        named = [k for k in ("avg_fn", "multi_avg_fn") if kwargs.pop(k, None) is not None]
        if named:
            raise TypeError(f"{type(self).__name__}: {' / '.join(named)} callables are not supported: the average is kept by a device "
                            f"kernel (subclass and override coefficients() instead)")
        if kwargs:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kwargs)}")
        if device is not None and torch.device(device).type == "cpu":
            raise ValueError(f"{type(self).__name__}: device={device!r}: the average lives next to the weights on the HIP device; "
                             f"an average on the host is not built (use device=None)")
        self.device = None if device is None else torch.device(device)
        self.use_buffers = use_buffers
        self.average = None
        self.latest_update_step = 0
        self._swapped = False
        self._resumed = None  # (averaged entries, n_averaged) of the checkpoint being resumed, until setup

    # ------------------------------------------------------------------ what subclasses decide
    def should_update(self, step_idx=None, epoch_idx=None):
        return step_idx is not None

    def coefficients(self, n_averaged):
        """(keep, take) of the update after `n_averaged` earlier ones, as python floats: the running mean"""
        return n_averaged / (n_averaged + 1), 1 / (n_averaged + 1)

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _owner(module):
        lyc = getattr(module, "lycoris_model", None)
        return (lyc, "lycoris_model.") if lyc is not None else (module.unet, "unet.")

    def _update(self):
        keep, take = self.coefficients(self.average.n_averaged)
        self.average.update(keep, take)

    def _swap(self):
        self.average.swap()
        self._swapped = not self._swapped

    # ------------------------------------------------------------------ hooks (Fitter._hook: the fitter comes first)
    def setup(self, fitter, module, stage=None):
        owner, _ = self._owner(module)
        flat = owner.flat
        if self.device is not None and flat.is_cuda:
            want = self.device if self.device.index is not None else torch.device(self.device.type, flat.device.index)
            if want != flat.device:
                raise ValueError(f"{type(self).__name__}: device={str(self.device)!r} is not the model's device {str(flat.device)!r}: "
                                 f"the average lives next to the weights")
        self.average = FlatAverage(owner)
        self._swapped = False
        if self._resumed is not None:
            sd, n = self._resumed
            self.average.load_averaged_state(sd)
            self.average.n_averaged = n
            self._resumed = None

    def on_train_batch_end(self, fitter, module, outputs=None, batch=None, batch_idx=None):
        g = fitter.global_step  # (a batch inside an accumulation window advances no global_step: nothing happens)
        if g > self.latest_update_step and self.should_update(step_idx=g - 1):
            self._update()
        self.latest_update_step = g

    def on_train_epoch_end(self, fitter, module):
        if self.should_update(epoch_idx=fitter.current_epoch):
            self._update()

    def on_validation_epoch_start(self, fitter, module):
        if self.average is not None:
            self._swap()

    def on_validation_epoch_end(self, fitter, module):
        if self.average is not None and self._swapped:
            self._swap()

    def on_exception(self, fitter, module, exception):
        if self.average is not None and self._swapped:  # a pass that raised: training goes on (or is examined) on its own weights
            self._swap()

    def on_train_end(self, fitter, module):
        if self.average is not None:
            self.average.copy_to_current()

    def on_save_checkpoint(self, fitter, module, ckpt):
        """``state_dict`` carries the averaged owner (what a loader of ``state_dict`` / ``unet.`` picks up), ``current_model_state`` the
        module as training has it.  Both are read from where they are: no weight is written while saving."""
        if self.average is None:
            return
        _, prefix = self._owner(module)
        held = {prefix + k: v.detach().cpu() for k, v in self.average.averaged_state().items()}
        current = dict(ckpt["state_dict"])
        averaged = {**current, **held}
        if self._swapped:  # saved from inside a validation pass: the module holds the average, the buffer the trained weights
            current, averaged = averaged, current
        ckpt["current_model_state"] = current
        ckpt["state_dict"] = averaged
        ckpt["averaging_state"] = {"n_averaged": int(self.average.n_averaged)}

    def on_load_checkpoint(self, fitter, module, ckpt):
        _, prefix = self._owner(module)
        if "current_model_state" not in ckpt:
            self._resumed = None
            if fitter.global_rank == 0:
                print(f"{type(self).__name__}: the checkpoint has no current_model_state (it was written without weight averaging): "
                      f"the average starts as a copy of the loaded weights", flush=True)
            return
        sd = ckpt["state_dict"]
        self._resumed = ({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)},
                         int((ckpt.get("averaging_state") or {}).get("n_averaged", 0)))
        ckpt["state_dict"] = ckpt["current_model_state"]  # the module resumes from the weights it was training

    def state_dict(self):
        return {"latest_update_step": int(self.latest_update_step)}

    def load_state_dict(self, sd):
        self.latest_update_step = int(sd["latest_update_step"])


class EMAWeightAveraging(WeightAveraging):
    """``lightning.pytorch.callbacks.EMAWeightAveraging``: avg = decay * avg + (1 - decay) * weights after every
    ``update_every_n_steps``-th optimizer step from ``update_starting_at_step`` on (and at the end of every epoch from
    ``update_starting_at_epoch`` on, when that is given).  The first update is a copy.  There is no decay warm-up."""

    def __init__(self, device=None, use_buffers=True, decay=0.999, update_every_n_steps=1, update_starting_at_step=None,
                 update_starting_at_epoch=None, **kwargs):
        super().__init__(device=device, use_buffers=use_buffers, **kwargs)
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMAWeightAveraging: decay must be a number in [0, 1], got {decay!r}")
        self.decay = float(decay)
        self.update_every_n_steps = int(update_every_n_steps)
        self.update_starting_at_step = None if update_starting_at_step is None else int(update_starting_at_step)
        self.update_starting_at_epoch = None if update_starting_at_epoch is None else int(update_starting_at_epoch)

    def should_update(self, step_idx=None, epoch_idx=None):
        if step_idx is not None:
            started = self.update_starting_at_step is None or step_idx >= self.update_starting_at_step
            return started and self.update_every_n_steps > 0 and step_idx % self.update_every_n_steps == 0
        if epoch_idx is not None:
            return self.update_starting_at_epoch is not None and epoch_idx >= self.update_starting_at_epoch
        return False

    def coefficients(self, n_averaged):
        return self.decay, 1.0 - self.decay  # (1 - decay in double: 1 - 0.999f is off by 1.3e-5 relative)


class ScheduleFreeMode:
    """The two modes of ``FusedAdamWScheduleFree`` (optim.py) driven from the hooks of ``Fitter``, which installs
    this by itself when the optimizer is one: training runs on ``y``, and every validation pass, every checkpoint's ``state_dict`` and
    the module ``fit`` returns hold the average ``x``.  The spare buffer of the optimizer is the buffer of a ``FlatAverage`` over the
    module that owns the trained flat buffer (``WeightAveraging._owner``'s rule), so ``x`` goes in place of ``y`` and back the way an
    average does: no pointer moved, the bf16 shadow refreshed, the adapters merged again, ``y`` back bit for bit."""

    def __init__(self, optimizer):
        self.opt = optimizer
        self.average = None

    def _training(self):
        return bool(self.opt.param_groups[0]["train_mode"])

    def setup(self, fitter, module, stage=None):
        owner, _ = WeightAveraging._owner(module)
        self.average = FlatAverage(owner)
        self.opt.use_average(self.average)
        self.opt.train()  # (after a resume too: the module was loaded from current_model_state, which is y)

    def on_validation_epoch_start(self, fitter, module):  # (the sanity check at step 0: x = y = z, nothing is exchanged)
        self.opt.eval()

    def on_validation_epoch_end(self, fitter, module):
        self.opt.train()

    def on_exception(self, fitter, module, exception):  # a pass that raised: training goes on (or is examined) on y
        self.opt.train()

    def on_train_end(self, fitter, module):
        self.opt.eval()  # the module is left holding x, as the averaging callbacks leave the average

    def on_save_checkpoint(self, fitter, module, ckpt):
        """``state_dict`` carries ``x`` (what a loader of ``state_dict`` / ``unet.`` picks up), ``current_model_state`` ``y``.  Both are
        read from where they are: while training ``x`` is written into the spare buffer, inside a validation pass ``y`` sits there.  No
        weight is written while saving."""
        if self.average is None:
            return
        owner, prefix = WeightAveraging._owner(module)
        p = owner.flat
        in_module = dict(ckpt["state_dict"])
        training = self._training()
        aside = self.opt.write_average(p) if training else self.opt.held_weights(p)
        if aside is None:  # before the first step: x = y = z
            ckpt["current_model_state"] = in_module
            return
        other = {**in_module, **{prefix + k: v.detach().cpu() for k, v in self.average.averaged_state().items()}}
        ckpt["current_model_state"], ckpt["state_dict"] = (in_module, other) if training else (other, in_module)

    def on_load_checkpoint(self, fitter, module, ckpt):
        if "current_model_state" not in ckpt:
            if fitter.global_rank == 0:
                print("ScheduleFreeMode: the checkpoint has no current_model_state (it was written under another optimizer): training "
                      "starts with y = the loaded weights", flush=True)
            return
        ckpt["state_dict"] = ckpt["current_model_state"]  # the module resumes from y; z, v and the scalars come with the optimizer state
