"""The flat parameter store every model here keeps its weights in.

One fp32 buffer holds all tensors of a model, each starting on a 64-element boundary; a bf16 shadow of the same layout feeds the
MFMA operands; gradients accumulate into ``flat.grad`` from inside the kernels.  One AdamW launch, one all-reduce and the C++ DiT
driver all address that buffer by offset, so the order of ``add`` calls is the layout.  ``FlatParams`` is the registry and its
views, ``FlatModule`` the ``nn.Module`` side: named views as ``state_dict()``, a loader that checks before it writes, the shadow,
and moves / casts that keep the master fp32.
"""
import json
import math
import os

import torch
import torch.nn as nn

from . import lib as L


def pad8(c):
    return (c + 7) // 8 * 8


def pad64(n):
    return (n + 63) // 64 * 64


class _Config(dict):
    """a model's transformers / diffusers configuration, attribute-accessible (``model.config.hidden_size``)"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class FlatParams:
    """name -> (offset, shape) over one flat fp32 buffer, its bf16 shadow and its gradient buffer; views alias them."""

    def __init__(self):
        self.registry = {}
        self.n = 0
        self.flat = None
        self.shadow = None
        self.bf16 = True

    def add(self, name, shape):
        self.registry[name] = (self.n, tuple(shape))
        self.n += pad64(math.prod(shape))

    def _view(self, buf, name):
        if isinstance(name, tuple):  # (first name, n): n equally shaped matrices stored back to back, seen as one
            first, n = name
            off, (rows, cols) = self.registry[first]
            return buf[off:off + n * rows * cols].view(n * rows, cols)
        off, shape = self.registry[name]
        return buf[off:off + math.prod(shape)].view(shape)

    def span(self, names):
        """(first, n) when `names` sit back to back with no padding between them (one stacked GEMM operand), else None"""
        off, shape = self.registry[names[0]]
        for i, nm in enumerate(names):
            o, sh = self.registry[nm]
            if sh != shape or len(sh) != 2 or o != off + i * math.prod(shape):
                return None
        return (names[0], len(names))

    def base32(self, name):  # the stored fp32 weights themselves
        return self._view(self.flat.data, name)

    w32 = base32  # what an operator reads in fp32 (biases, norm vectors); a subclass may put effective weights here

    def w(self, name):  # GEMM operand copy
        if self.bf16:
            return self._view(self.shadow, name)
        return self.w32(name)

    def g(self, name):
        if self.flat.grad is None:
            self.flat.grad = torch.zeros_like(self.flat.data)
        return self._view(self.flat.grad, name)

    @property
    def dtype(self):
        return torch.bfloat16 if self.bf16 else torch.float32


class FlatModule(nn.Module):
    """Base of the models: ``self.P`` (the store), ``self.flat`` (parameter or buffer) and the non-persistent ``shadow`` buffer.

    A model adds its tensors to ``self.P`` and calls ``_alloc``; its public (checkpoint) names and layouts come from two hooks,
    ``_public_names`` and ``_public_view``; ``_load_key``, ``_prepare_load``, ``_after_load``, ``_wants_shadow``, ``_shadow_stale``
    and ``_moved`` cover what else differs between them."""

    _uwu_keep_fp32_master = True  # duwu.loader.prepare_model: `precision: torch.float16` leaves this module's dtype alone

    def __init__(self, store=FlatParams):
        super().__init__()
        self.P = store()

    def _alloc(self, bf16, device=None, trainable=True, buffer=False):
        """once every tensor is added: ``flat`` (zeros: a parameter, or a non-persistent buffer) and the empty shadow"""
        flat = torch.zeros(self.P.n, dtype=torch.float32, device=device)
        if buffer:
            self.register_buffer("flat", flat, persistent=False)
        else:
            self.flat = nn.Parameter(flat, requires_grad=trainable)
        self.register_buffer("shadow", torch.zeros(0, dtype=torch.bfloat16, device=device), persistent=False)
        self.P.flat, self.P.shadow, self.P.bf16 = self.flat, self.shadow, bf16
        self.w, self.w32 = self.P.w, self.P.w32

    registry = property(lambda self: self.P.registry)
    n = property(lambda self: self.P.n)

    def view(self, name):
        return self.P.base32(name)

    def grad_view(self, name):
        return self.P._view(self.flat.grad, name)

    # ------------------------------------------------------------------ hooks
    def _public_names(self):
        """public name -> (registry name, first row, rows; None: the whole tensor), in ``state_dict()`` order"""
        return {name: (name, 0, None) for name in self.P.registry}

    def _public_view(self, v, name):
        """the stored tensor `v` of registry entry `name` in the public layout (a view: writes go to the flat buffer)"""
        return v

    @staticmethod
    def _conv_public(v, meta, taps, bias):
        """a stored convolution tensor in diffusers' layout: the weight ``[Cout][taps][Cin]`` (1x1: ``[Cout][Cin]``) as
        ``[Cout, Cin, k, k]``, the channels that pad Cin / Cout to 8 cut off; `meta` = (cin, cout, stored cin, stored cout)"""
        cin, cout, ci, co = meta
        if bias:
            return v[:cout]
        if taps == 9:
            return v.view(co, 3, 3, ci)[:cout, :, :, :cin].permute(0, 3, 1, 2)
        return v[:cout, :cin, None, None]

    def _load_key(self, key):
        """a key of a loaded state dict -> public name (None: an entry to pass over)"""
        return key

    def _prepare_load(self, state_dict):
        """the state dict as the loader should see it (a tensor stored once under two public names); raises to refuse the load"""
        return state_dict

    def _after_load(self):
        pass

    def _wants_shadow(self):
        return self.P.bf16

    def _shadow_stale(self):
        pass

    def _moved(self):
        pass

    # ------------------------------------------------------------------ named views
    def _public_views(self, buf):
        for public, (name, r0, rows) in self._public_names().items():
            v = self.P._view(buf, name)
            yield public, self._public_view(v if rows is None else v[r0:r0 + rows], name)

    def named_tensors(self):
        """(public name, view of the fp32 master in the public layout) pairs"""
        return self._public_views(self.flat.data)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = destination if destination is not None else {}
        for name, v in self.named_tensors():
            sd[prefix + name] = v if keep_vars else v.detach().clone().contiguous()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Every key is resolved and every shape checked against the public view first; a refused load has written nothing."""
        state_dict = self._prepare_load(state_dict)
        views = dict(self.named_tensors())
        todo, unexpected, errors = {}, [], []
        for key, src in state_dict.items():
            name = self._load_key(key)
            if name is None:
                continue
            if name not in views:
                unexpected.append(key)
            elif tuple(src.shape) != tuple(views[name].shape):
                errors.append(f"size mismatch for {key}: copying a param with shape {tuple(src.shape)}, the model has "
                              f"{tuple(views[name].shape)}")
            else:
                todo[name] = src
        missing = [name for name in views if name not in todo]
        if errors:
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: {'; '.join(errors[:5])}")
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing {missing[:5]}, unexpected "
                               f"{unexpected[:5]}")
        for name, src in todo.items():
            views[name].copy_(src)
        self._after_load()
        self.refresh_shadow()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """a parent's ``load_state_dict`` (a trainer checkpoint, whose entries ``state_dict()`` above wrote under the parent's
        prefix) reaches the model here: the same loader, reporting into the parent's lists"""
        own = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        try:
            res = self.load_state_dict(own, strict=False)
        except RuntimeError as e:
            error_msgs.append(str(e))
            return
        missing_keys.extend(prefix + k for k in res.missing_keys)
        unexpected_keys.extend(prefix + k for k in res.unexpected_keys)

    @staticmethod
    def _drop_hub_keywords(kw):
        """`kw` of a ``from_pretrained`` without the keywords that only steer a download or a cast: nothing is ever fetched, and
        no dtype is taken from the caller"""
        hub = ("torch_dtype", "variant", "use_safetensors", "cache_dir", "local_files_only", "revision")
        return {k: v for k, v in kw.items() if k not in hub}

    @classmethod
    def _from_local_dir(cls, path, subfolder, known, weights, **kw):
        """The local-directory branch of every ``from_pretrained``.  When ``<path>[/<subfolder>]`` is a directory with
        ``config.json``: the model built from that file's keys in `known` (the rest is not built) under a ``config=`` override,
        holding the tensors of the safetensors file `weights`.  Anything else (a hub name, a preset) -> None."""
        local = os.path.join(path, subfolder) if subfolder else path
        if not (os.path.isdir(local) and os.path.exists(os.path.join(local, "config.json"))):
            return None
        from safetensors.torch import load_file

        with open(os.path.join(local, "config.json")) as f:
            config = {k: v for k, v in json.load(f).items() if k in known}
        config.update(kw.pop("config", None) or {})
        model = cls(config, init_weights=False, **kw)
        model.load_state_dict(load_file(os.path.join(local, weights)))
        return model

    # ------------------------------------------------------------------ shadow, moves
    @torch.no_grad()
    def refresh_shadow(self):
        """bf16 copy of the flat parameters for the MFMA operands (kept fresh by the fused AdamW afterwards)."""
        self._shadow_stale()
        if not self._wants_shadow() or not self.flat.is_cuda:
            return
        n = self.P.n
        if self.shadow.numel() != n or self.shadow.device != self.flat.device:
            self.shadow = torch.empty(n, device=self.flat.device, dtype=torch.bfloat16)
        L.call("uwu_cast_f32_to_bf16", L.ptr(self.flat.data), L.ptr(self.shadow), n, L.stream())
        self.P.shadow = self.shadow
        self.flat._uwu_bf16_shadow = self.shadow  # the fused AdamW writes the updated weights here too (optim.py)

    def _apply(self, fn, recurse=True):
        held = {k: t.data for k, t in (*self._parameters.items(), *self._buffers.items()) if t is not None}
        grad = self.flat.grad.data if self.flat.grad is not None else None
        r = super()._apply(fn, recurse)
        # a dtype cast (`.half()`, `.to(torch.bfloat16)`) must not touch the fp32 master, the bf16 shadow or any table the
        # kernels read by pointer (they would read past a half-sized buffer): only the device moves
        for k, old in held.items():
            t = getattr(self, k)
            if t.dtype != old.dtype:
                t.data = old.to(t.device)
        if grad is not None and self.flat.grad.dtype != grad.dtype:
            self.flat.grad = grad.to(self.flat.device)
        self.P.flat, self.P.shadow = self.flat, self.shadow
        self._moved()
        self.refresh_shadow()
        return r
