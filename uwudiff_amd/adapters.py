"""LyCORIS adapters (LoRA, LoKr, norm; LoCon / Tucker / LoKr on the 3x3 convolutions) on the flat UNet: configuration, layer matching, one flat adapter parameter.

The reference trainer wraps the UNet with the ``lycoris`` library (reference src/duwu/trainer/trainer.py:148-169): a
``config`` table (algo, dims, alpha, ...) and a ``preset`` table (which module classes / names are adapted).  The library
is not a dependency of this build; the subset below is this project's contract:

  * LoRA   dW = alpha / dim * up @ down                     down [dim, in] kaiming-uniform(a=sqrt 5), up [out, dim] zeros
  * LoKr   dW = scale * kron(w1, w2)                         w1 [out_l, in_m] kaiming-uniform, w2 [out_k, in_n] zeros
           (out_l, out_k) = factorization(out, factor), (in_m, in_n) = factorization(in, factor); w2 = w2_a @ w2_b
           (w2_b the zero factor, scale alpha / dim) when not full_matrix and dim < max(out_k, in_n) / 2, else scale 1
  * norm   gamma + w_norm, beta + b_norm                     both zeros
  * dora_wd (on LoRA / LoKr): W' = m (W + dW) / (||W + dW|| + eps), one magnitude m (``dora_scale``) and one norm per
           output row (wd_on_out) or per input column, eps = 2^-23 added to the norm; m starts at the base weight's norm
           

  * 3x3 convolutions (``enable_conv``; ``conv_dim`` / ``conv_alpha``), W [Cout, Cin, 3, 3]:
           LoRA    down [dim, Cin, 3, 3], up [Cout, dim, 1, 1]: dW = alpha / dim * up @ down.view(dim, -1)
           Tucker  (``use_tucker``) down [dim, Cin, 1, 1], mid [dim, dim, 3, 3] kaiming-uniform, up [Cout, dim, 1, 1]:
                   dW[p, c, kh, kw] = alpha / dim * sum_ij up[p, i] mid[i, j, kh, kw] down[j, c]
           LoKr    w1 [out_l, in_m], w2 [out_k, in_n, 3, 3] (or w2_a [out_k, dim] @ w2_b [dim, in_n * 9]) on the
                   factorizations of Cout and Cin: dW[a out_k + c, b in_n + d, kh, kw] = scale * w1[a, b] w2[c, d, kh, kw]
           the buffer holds these tap-major (Spec.internal), the state dict in the shapes above

so a freshly attached network leaves the model's output unchanged (with dora_wd: to rounding).  Every adapter tensor is a named view of ONE flat
fp32 parameter (the fused AdamW and the gradient exchange work on it as on the UNet's flat buffer); the UNet merges them
into its effective weights with one kernel launch (csrc/adapter.hip) and computes their gradients from the weight
gradients of the adapted layers.  Matching runs on the UNet's name / shape registry only: a UNet built on the ``meta``
device (no storage) is enough.
"""
import fnmatch
import math
import re

import torch
import torch.nn as nn

from .flat import pad64

CONFIG_DEFAULTS = dict(algo="lora", linear_dim=4, linear_alpha=1.0, factor=-1, full_matrix=False, train_norm=False,
                       conv_dim=None, conv_alpha=None, use_tucker=False, dora_wd=False, wd_on_out=True)
BOOL_KEYS = ("dora_wd", "wd_on_out")
PRESET_KEYS = ("target_module", "target_name", "enable_conv", "module_algo_map")
ALGOS = ("lora", "lokr")
KIND_NORM, KIND_LORA, KIND_LOKR, KIND_LOKR_LOWRANK = 0, 1, 2, 3  # UWU_ADAPTER_* of include/uwu_hip.h
KIND_CONV_LORA, KIND_CONV_TUCKER, KIND_CONV_LOKR, KIND_CONV_LOKR_LOWRANK = 4, 5, 6, 7  # UWU_ADAPTER_CONV_*
MAX_RANK = 128


def factorization(dim, factor=-1):
    """(m, n), m <= n, m * n = dim: (factor, dim / factor) when factor divides dim, else the largest divisor pair whose
    smaller member does not exceed factor (factor < 0: no bound)."""
    dim, factor = int(dim), int(factor)
    if factor > 0 and dim % factor == 0:
        m, n = factor, dim // factor
        return (m, n) if m <= n else (n, m)
    if factor < 0:
        factor = dim
    m, n = 1, dim
    while m < n:
        new_m = m + 1
        while dim % new_m:
            new_m += 1
        if new_m > factor:
            break
        m, n = new_m, dim // new_m
    return (m, n) if m <= n else (n, m)


def load_config(cfg):
    """A ``lycoris_config``: dict, or path of a TOML file (read with tomli).  Returns (config, preset), validated."""
    if isinstance(cfg, (str, bytes)) or hasattr(cfg, "__fspath__"):
        try:
            import tomli as _toml
        except ImportError:  # (the standard library's copy of the same parser)
            import tomllib as _toml
        with open(cfg, "rb") as f:
            cfg = _toml.load(f)
    if not isinstance(cfg, dict):
        raise ValueError(f"lycoris_config must be a dict or a TOML path, got {type(cfg).__name__}")
    extra = set(cfg) - {"config", "preset"}
    if extra:
        raise ValueError(f"lycoris_config: unknown table(s) {sorted(extra)} (known: config, preset)")
    if "preset" not in cfg:
        raise ValueError("lycoris_config needs a [preset] table (target_module / target_name)")
    config = _check_algo_table(dict(cfg.get("config") or {}), "config")
    config = {**CONFIG_DEFAULTS, **config}
    preset = dict(cfg["preset"])
    extra = set(preset) - set(PRESET_KEYS)
    if extra:
        raise ValueError(f"lycoris_config.preset: unknown key(s) {sorted(extra)} (known: {', '.join(PRESET_KEYS)})")
    preset.setdefault("target_module", [])
    preset.setdefault("target_name", [])
    preset.setdefault("enable_conv", False)
    amap = {}
    for cls, table in dict(preset.get("module_algo_map") or {}).items():
        if not isinstance(table, dict):
            raise ValueError(f"lycoris_config.preset.module_algo_map.{cls} must be a table")
        amap[cls] = _check_algo_table(dict(table), f"preset.module_algo_map.{cls}")
    preset["module_algo_map"] = amap
    for k in ("target_module", "target_name"):
        if isinstance(preset[k], str) or not all(isinstance(v, str) for v in preset[k]):
            raise ValueError(f"lycoris_config.preset.{k} must be a list of strings")
    return config, preset


def _check_algo_table(t, where):
    extra = set(t) - set(CONFIG_DEFAULTS)
    if extra:
        raise ValueError(f"lycoris_config.{where}: unknown key(s) {sorted(extra)} (known: {', '.join(CONFIG_DEFAULTS)})")
    if "algo" in t and t["algo"] not in ALGOS:
        raise NotImplementedError(f"lycoris_config.{where}: algo {t['algo']!r} is not implemented (supported: "
                                  f"{', '.join(ALGOS)})")
    for k in BOOL_KEYS:
        if k in t and not isinstance(t[k], bool):
            raise ValueError(f"lycoris_config.{where}: {k} must be true or false, got {t[k]!r}")
    return t


# ------------------------------------------------------------------------------------------ class names of the UNet names
_CONTAINERS = [
    (re.compile(r"^(down_blocks|up_blocks)\.\d+\.attentions\.\d+$|^mid_block\.attentions\.\d+$"), "Transformer2DModel"),
    (re.compile(r"\.transformer_blocks\.\d+$"), "BasicTransformerBlock"),
    (re.compile(r"\.attn[12]$"), "Attention"),
    (re.compile(r"\.ff$"), "FeedForward"),
    (re.compile(r"\.ff\.net\.0$"), "GEGLU"),
    (re.compile(r"\.resnets\.\d+$"), "ResnetBlock2D"),
    (re.compile(r"\.downsamplers\.0$"), "Downsample2D"),
    (re.compile(r"\.upsamplers\.0$"), "Upsample2D"),
    (re.compile(r"^(time_embedding|add_embedding)$"), "TimestepEmbedding"),
    (re.compile(r"^mid_block$"), "UNetMidBlock2DCrossAttn"),
]


def module_classes(unet):
    """{module name: diffusers class name} for every layer of the flat UNet and every module containing one."""
    kinds = getattr(unet, "module_kinds", None)
    if kinds is None:
        raise NotImplementedError(f"LyCORIS adapters are implemented for the UNet only, not for {type(unet).__name__}")
    cfg = getattr(unet, "cfg_dict", {})
    out = {"": "UNet2DConditionModel"}
    for leaf, kind in kinds.items():
        parts = leaf.split(".")
        for i in range(1, len(parts)):
            name = ".".join(parts[:i])
            if name in out:
                continue
            cls = None
            for rx, c in _CONTAINERS:
                if rx.search(name):
                    cls = c
                    break
            m = re.match(r"^(down|up)_blocks\.(\d+)$", name)
            if m and cls is None:
                cls = cfg.get(f"{m.group(1)}_block_types", [None] * 99)[int(m.group(2))]
            out[name] = cls or "Module"
        out[leaf] = kind
    return out


class Spec:
    """One adapted layer: ``name`` (module), ``algo`` ('lora' / 'lokr' / 'norm'), ``shape`` ([out, in] or [C]), the
    adapter tensors [(tensor name, shape)], and the factors the kernels need.

    A 3x3 convolution (``conv``: its (cin, cout, stored cin, stored cout)) has ``shape`` = the true
    (Cout, Cin); ``tensors`` holds the PUBLIC shapes (the state dict's), ``internal`` the tap-major shapes the flat buffer
    and the kernels use ([A, B, 3, 3] is stored [A, 9, B], [A, B, 1, 1] as [A, B], lokr_w2_b [dim, in_n * 9] as
    [dim, 9, in_n]); ``to_internal`` / ``to_public`` permute between the two."""

    def __init__(self, name, algo, shape, dim=0, alpha=1.0, factor=-1, full_matrix=False, dora_wd=False, wd_on_out=True,
                 conv=None, use_tucker=False):
        self.name, self.algo, self.shape = name, algo, tuple(shape)
        self.dim, self.alpha, self.r, self.out_k, self.in_n, self.lowrank = 0, None, 0, 0, 0, False
        self.dora, self.wd_on_out = bool(dora_wd) and algo != "norm", bool(wd_on_out)
        self.conv, self.tucker, self.internal = conv, False, {}
        if conv is not None:
            self._conv_factors(dim, alpha, factor, full_matrix, use_tucker)
            return
        self._factors(dim, alpha, factor, full_matrix)
        if self.dora:  # one magnitude per output row or per input column, always the last tensor
            self.tensors.append(("dora_scale", (self.shape[0], 1) if self.wd_on_out else (1, self.shape[1])))

    def _conv_factors(self, dim, alpha, factor, full_matrix, use_tucker):
        name, algo = self.name, self.algo
        if self.dora:
            raise NotImplementedError(f"{name}: dora_wd on a convolution adapter is not implemented")
        out, inn = self.shape
        dim = int(dim)
        if dim < 1:
            raise ValueError(f"{name}: conv_dim must be >= 1")
        self.dim, self.alpha = dim, float(alpha)
        too_wide = NotImplementedError(f"{name}: conv_dim {dim} > {MAX_RANK} is not implemented")
        if algo == "lora":
            if dim > MAX_RANK:
                raise too_wide
            self.r, self.scale, self.tucker = dim, self.alpha / dim, bool(use_tucker)
            if self.tucker:
                self.kind = KIND_CONV_TUCKER
                self.tensors = [("lora_down.weight", (dim, inn, 1, 1)), ("lora_mid.weight", (dim, dim, 3, 3)),
                                ("lora_up.weight", (out, dim, 1, 1))]
            else:
                self.kind = KIND_CONV_LORA
                self.tensors = [("lora_down.weight", (dim, inn, 3, 3)), ("lora_up.weight", (out, dim, 1, 1))]
        else:
            out_l, out_k = factorization(out, factor)
            in_m, in_n = factorization(inn, factor)
            self.out_k, self.in_n = out_k, in_n
            self.tensors = [("lokr_w1", (out_l, in_m))]
            if not full_matrix and dim < max(out_k, in_n) / 2:
                if use_tucker:
                    raise NotImplementedError(f"{name}: low-rank LoKr with use_tucker (lokr_t2) is not implemented")
                if dim > MAX_RANK:
                    raise too_wide
                self.kind, self.lowrank, self.r, self.scale = KIND_CONV_LOKR_LOWRANK, True, dim, self.alpha / dim
                self.tensors += [("lokr_w2_a", (out_k, dim)), ("lokr_w2_b", (dim, in_n * 9))]
            else:
                self.kind, self.scale = KIND_CONV_LOKR, 1.0
                self.tensors += [("lokr_w2", (out_k, in_n, 3, 3))]
        for t, sh in self.tensors:
            if len(sh) == 4:
                self.internal[t] = (sh[0], 9, sh[1]) if sh[2] == 3 else (sh[0], sh[1])
            elif t == "lokr_w2_b":
                self.internal[t] = (sh[0], 9, sh[1] // 9)
            else:
                self.internal[t] = sh

    def to_internal(self, t, v):
        """a public tensor of this layer in the flat buffer's layout (a copy where the two differ)"""
        sh = dict(self.tensors)[t]
        if self.conv is None or self.internal[t] == sh:
            return v
        if len(sh) == 4:
            return v.permute(0, 2, 3, 1).reshape(self.internal[t])
        return v.reshape(sh[0], sh[1] // 9, 9).permute(0, 2, 1).contiguous()  # lokr_w2_b: columns (d, tap) -> (tap, d)

    def to_public(self, t, v):
        """the stored tensor `v` in the public shape: a view of `v`, except lokr_w2_b of a convolution (a copy)"""
        sh = dict(self.tensors)[t]
        if self.conv is None or self.internal[t] == sh:
            return v
        if len(sh) == 4:
            return v.view(sh[0], sh[2], sh[3], sh[1]).permute(0, 3, 1, 2)
        return v.permute(0, 2, 1).reshape(sh)

    def _factors(self, dim, alpha, factor, full_matrix):
        name, algo = self.name, self.algo
        if algo == "norm":
            self.tensors = [("w_norm", self.shape), ("b_norm", self.shape)]
            self.scale = 1.0
            return
        out, inn = self.shape
        dim = int(dim)
        if dim < 1:
            raise ValueError(f"{name}: linear_dim must be >= 1")
        self.dim, self.alpha = dim, float(alpha)
        if algo == "lora":
            if dim > MAX_RANK:
                raise ValueError(f"{name}: LoRA dim {dim} > {MAX_RANK}")
            self.r, self.scale = dim, self.alpha / dim
            self.tensors = [("lora_down.weight", (dim, inn)), ("lora_up.weight", (out, dim))]
            return
        out_l, out_k = factorization(out, factor)
        in_m, in_n = factorization(inn, factor)
        self.out_k, self.in_n = out_k, in_n
        self.tensors = [("lokr_w1", (out_l, in_m))]
        if not full_matrix and dim < max(out_k, in_n) / 2:
            if dim > MAX_RANK:
                raise ValueError(f"{name}: LoKr dim {dim} > {MAX_RANK}")
            self.lowrank, self.r, self.scale = True, dim, self.alpha / dim
            self.tensors += [("lokr_w2_a", (out_k, dim)), ("lokr_w2_b", (dim, in_n))]
        else:
            self.scale = 1.0
            self.tensors += [("lokr_w2", (out_k, in_n))]

    @property
    def key(self):
        return "lycoris_" + self.name.replace(".", "_")

    @property
    def numel(self):
        return sum(math.prod(s) for _, s in self.tensors)

    def __repr__(self):
        return f"Spec({self.name!r}, {self.algo!r}, {self.shape}, tensors={self.tensors})"


def match_layers(unet, lycoris_config):
    """The adapted layers of ``unet`` under ``lycoris_config`` (dict / TOML path / (config, preset)), in registry order.

    A Linear takes the algo (and settings) of its nearest ancestor listed in ``module_algo_map``; otherwise the
    ``config`` algo, if an ancestor's class is in ``target_module`` or its name matches ``target_name``.  With
    ``train_norm`` every LayerNorm / GroupNorm inside a target gets a norm adapter.  3x3 convolutions inside a target:
    skipped, or with ``enable_conv`` adapted on ``conv_dim`` / ``conv_alpha`` (``use_tucker``: the Tucker form of LoRA);
    1x1 convolutions are Linears here."""
    config, preset = lycoris_config if isinstance(lycoris_config, tuple) else load_config(lycoris_config)
    classes = module_classes(unet)
    tmod, tname, amap = set(preset["target_module"]), list(preset["target_name"]), preset["module_algo_map"]
    registry = unet.P.registry
    specs = []
    for leaf, kind in unet.module_kinds.items():
        parts = leaf.split(".")
        chain = [".".join(parts[:i]) for i in range(len(parts) + 1)]  # "", ..., leaf
        over = None
        for n in reversed(chain):
            if classes[n] in amap:
                over = amap[classes[n]]
                break
        targeted = over is not None or any(classes[n] in tmod for n in chain) or any(
            fnmatch.fnmatchcase(n, pat) for n in chain if n for pat in tname)
        if not targeted:
            continue
        cfg = {**config, **(over or {})}
        if kind == "Linear":
            specs.append(Spec(leaf, cfg["algo"], registry[leaf + ".weight"][1], dim=cfg["linear_dim"],
                              alpha=cfg["linear_alpha"], factor=cfg["factor"], full_matrix=cfg["full_matrix"],
                              dora_wd=cfg["dora_wd"], wd_on_out=cfg["wd_on_out"]))
        elif kind in ("LayerNorm", "GroupNorm"):
            if cfg["train_norm"]:
                specs.append(Spec(leaf, "norm", registry[leaf + ".weight"][1]))
        elif kind == "Conv2d" and preset["enable_conv"]:
            if cfg["conv_dim"] is None:
                raise NotImplementedError(f"lycoris_config: enable_conv reaches the 3x3 convolution {leaf!r} and conv_dim "
                                          "is not set; the fallback of conv_dim to linear_dim is not implemented")
            if cfg["dora_wd"]:
                raise NotImplementedError(f"lycoris_config: dora_wd reaches the 3x3 convolution {leaf!r}; weight "
                                          "decomposition of convolution adapters is not implemented")
            meta = unet._conv_meta[leaf]  # (cin, cout, stored cin, stored cout)
            specs.append(Spec(leaf, cfg["algo"], (meta[1], meta[0]), dim=cfg["conv_dim"],
                              alpha=cfg["linear_alpha"] if cfg["conv_alpha"] is None else cfg["conv_alpha"],
                              factor=cfg["factor"], full_matrix=cfg["full_matrix"], conv=meta,
                              use_tucker=cfg["use_tucker"]))
    if not specs:
        raise ValueError("lycoris_config matches no layer of the UNet")
    order = {n: i for i, n in enumerate(registry)}
    specs.sort(key=lambda s: order[s.name + ".weight"])
    return specs


def grad_ws_elems(spec, N, K):
    """floats of uwu_adapter_grad's workspace (include/uwu_hip.h)"""
    if spec.algo == "lora":
        return -(-K // 256) * N * spec.r + -(-N // 32) * spec.r * K
    out_l, in_m, W2 = N // spec.out_k, K // spec.in_n, spec.out_k * spec.in_n
    return out_l * -(-W2 // 2048) * in_m + out_l * W2 + 2 * W2


def conv_grad_ws_elems(spec):
    """floats of uwu_adapter_conv_grad's workspace (include/uwu_hip.h)"""
    cout, cin = spec.shape
    K = 9 * cin
    if spec.algo == "lora":
        return -(-K // 256) * cout * spec.r + -(-cout // 32) * spec.r * K + (2 * spec.r * K if spec.tucker else 0)
    out_l, in_m, W2 = cout // spec.out_k, cin // spec.in_n, 9 * spec.out_k * spec.in_n
    return out_l * -(-W2 // 2048) * in_m + out_l * W2 + 2 * W2


def dora_grad_ws_elems(spec, N, K):
    """floats of uwu_adapter_dora_grad's workspace (include/uwu_hip.h): the column sums go through row-tile partials"""
    return 0 if spec.wd_on_out else 4 * -(-N // 256) * K


class LycorisNetwork(nn.Module):
    """The adapters of one UNet: ``flat`` (one fp32 parameter) with every adapter tensor as a named view.

    ``apply_to(unet)`` makes the UNet run with W + dW (merged by the UNet before its next forward whenever the adapters
    changed), ``restore()`` detaches them again, ``merge_to()`` folds dW into the UNet's base weights."""

    def __init__(self, unet, lycoris_config, device=None):
        super().__init__()
        self.specs = match_layers(unet, lycoris_config)
        self._by_name = {s.name: s for s in self.specs}
        self.offsets = {}  # (spec name, tensor name) -> (offset, shape)
        n = 0
        for s in self.specs:
            for t, shape in s.tensors:
                self.offsets[(s.name, t)] = (n, shape)
                n += pad64(math.prod(shape))
        self.n = n
        if device is None:
            device = unet.flat.device if unet.flat.device.type != "meta" else "cpu"
        self.flat = nn.Parameter(torch.zeros(n, dtype=torch.float32, device=device))
        self._dirty = True
        # dora_scale starts at the norm of the BASE weight; a UNet without storage (meta) cannot supply it
        self.dora_uninitialised = False
        self.reset_parameters(unet)

    # ------------------------------------------------------------------ views / init
    def stored(self, spec_name, tensor, buf=None):
        """the tensor as the flat buffer holds it (a convolution adapter: tap-major, Spec.internal), always a view"""
        off, shape = self.offsets[(spec_name, tensor)]
        shape = self._by_name[spec_name].internal.get(tensor, shape)
        return (self.flat.data if buf is None else buf)[off:off + math.prod(shape)].view(shape)

    def view(self, spec_name, tensor, buf=None):
        """the tensor in its public shape: a view of the buffer, except lokr_w2_b of a convolution (a copy: ``write`` is
        the way in)"""
        return self._by_name[spec_name].to_public(tensor, self.stored(spec_name, tensor, buf))

    @torch.no_grad()
    def write(self, spec_name, tensor, value, buf=None):
        """`value` (public shape) into the buffer"""
        self.stored(spec_name, tensor, buf).copy_(self._by_name[spec_name].to_internal(tensor, value))

    @torch.no_grad()
    def conv_delta(self, spec_name, dtype=torch.float64):
        """dW of one adapted convolution in the STORED layout [Cout_store, 9, Cin_store] (zeros in the padding), computed
        by torch from the buffer: what uwu_adapter_conv_merge adds to the base weight (the host-side statement of it)"""
        s = self._by_name[spec_name]
        cin, cout, ci, co = s.conv
        T = lambda t: self.stored(spec_name, t).to(dtype)
        if s.algo == "lora":
            down = T("lora_down.weight")  # [dim, 9, Cin]; Tucker: [dim, Cin], taken through mid [dim, 9, dim] first
            if s.tucker:
                down = torch.einsum("itj,jc->itc", T("lora_mid.weight"), down)
            d = torch.einsum("oi,itc->otc", T("lora_up.weight"), down)
        else:
            w2 = torch.einsum("kr,rtl->ktl", T("lokr_w2_a"), T("lokr_w2_b")) if s.lowrank else T("lokr_w2")
            d = torch.einsum("ab,ktl->aktbl", T("lokr_w1"), w2).reshape(cout, 9, cin)
        out = torch.zeros(co, 9, ci, dtype=dtype, device=d.device)
        out[:cout, :, :cin] = d * s.scale
        return out

    @torch.no_grad()
    def reset_parameters(self, unet=None):
        """kaiming_uniform(a=sqrt 5) on lora_down / lora_mid / lokr_w1 / lokr_w2_a (torch's default generator, drawn in
        the public shape: a convolution's fan-in counts its taps), zeros elsewhere:
        dW = 0 and the adapted model computes what the bare one does.  dora_scale: the norms of the base weights of
        ``unet`` (default: the UNet the network is attached to)."""
        self.flat.data.zero_()
        for s in self.specs:
            for t, shape in s.tensors:
                if t in ("lora_down.weight", "lora_mid.weight", "lokr_w1", "lokr_w2_a"):
                    w = torch.empty(shape, dtype=torch.float32)
                    nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                    self.write(s.name, t, w)
        self._init_dora(unet if unet is not None else self.__dict__.get("_unet"))
        self.mark_dirty()

    def _init_dora(self, unet):
        dora = [s for s in self.specs if s.dora]
        if not dora:
            return
        if unet is None or unet.flat.device.type == "meta":
            self.dora_uninitialised = True  # zeros: apply_to refuses until a state dict supplies every dora_scale
            return
        for s in dora:
            w = unet.P.base32(s.name + ".weight").detach().double()  # (summed in fp64, rounded once)
            m = torch.linalg.vector_norm(w, dim=1 if s.wd_on_out else 0, keepdim=True).float()
            self.view(s.name, "dora_scale").copy_(m)
        self.dora_uninitialised = False

    def mark_dirty(self):
        """the adapter weights changed (optimizer step, load): the UNet merges again before its next forward"""
        self._dirty = True

    def num_adapter_params(self):
        return sum(s.numel for s in self.specs)

    # ------------------------------------------------------------------ state dict (lycoris_<name>.<tensor>)
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = destination if destination is not None else {}
        for s in self.specs:
            for t, _ in s.tensors:
                sd[f"{prefix}{s.key}.{t}"] = self.view(s.name, t).detach().clone(memory_format=torch.contiguous_format)
            if s.alpha is not None:
                sd[f"{prefix}{s.key}.alpha"] = torch.tensor(s.alpha)
        return sd

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        mine, dora_loaded = set(), True
        with torch.no_grad():
            for s in self.specs:
                for t, shape in s.tensors:
                    k = f"{prefix}{s.key}.{t}"
                    mine.add(k)
                    if k not in state_dict:
                        missing_keys.append(k)
                        dora_loaded &= t != "dora_scale"
                        continue
                    v = state_dict[k]
                    if tuple(v.shape) != tuple(shape):
                        error_msgs.append(f"size mismatch for {k}: checkpoint {tuple(v.shape)}, adapter {tuple(shape)}")
                        dora_loaded &= t != "dora_scale"
                        continue
                    self.write(s.name, t, v.float())
                if s.alpha is not None:
                    k = f"{prefix}{s.key}.alpha"
                    mine.add(k)
                    if k in state_dict and abs(float(state_dict[k]) - s.alpha) > 1e-6 * max(1.0, abs(s.alpha)):
                        error_msgs.append(f"{k}: checkpoint alpha {float(state_dict[k])} != configured {s.alpha}")
        for k in state_dict:
            if k.startswith(prefix) and k not in mine:
                unexpected_keys.append(k)
        if dora_loaded:
            self.dora_uninitialised = False
        self.mark_dirty()

    # ------------------------------------------------------------------ attach / detach / fold
    def apply_to(self, unet=None):
        unet = unet if unet is not None else self._unet
        if self.dora_uninitialised:
            raise RuntimeError("LycorisNetwork.apply_to: dora_scale is uninitialised (the network was built on a UNet "
                               "without storage); build it on a UNet with weights or load a state dict with every "
                               "dora_scale first")
        object.__setattr__(self, "_unet", unet)  # (not a sub-module: the UNet's state dict stays the base weights)
        unet.attach_adapters(self)
        return self

    def restore(self):
        unet = self.__dict__.get("_unet")
        if unet is not None:
            unet.detach_adapters()

    def merge_to(self, unet=None):
        """W += dW in the UNet's flat fp32 weights (one uwu_adapter_merge launch) and detach: a plain UNet remains."""
        unet = unet if unet is not None else self._unet
        unet.fold_adapters(self)
