"""The text encoders on the HIP kernels, frozen, forward only: the CLIP text transformer (SDXL's two; DESIGN.md section 4.23, described
here) and, at the end of the file, the T5 v1.1 encoder (section 4.25).

The reference wraps ``transformers.CLIPTextModel`` / ``CLIPTextModelWithProjection`` in ``ConcatTextEncoders`` and runs them
inside every training step under ``no_grad`` (reference src/duwu/modules/text_encoders.py:153-191, src/duwu/trainer/trainer.py:238).
This module restates that model from its public description -- token + position embedding; L pre-LN layers ``h += out_proj(
attn(LN1 h))``, ``h += fc2(act(fc1(LN2 h)))`` with causal self-attention that also hides the keys ``attention_mask`` marks as
padding; ``final_layer_norm``; the pooled row at the eos token -- keeps transformers' parameter names in ``state_dict()`` and
runs every operator through ``libuwu_hip.so``:

  * activations stay ``[B*T, D]`` in the compute dtype; q, k and v are ONE bias GEMM on weights stored back to back, read in
    place by ``uwu_attention_causal_fwd`` (which takes the 1/sqrt(d) scale); every LayerNorm is ``uwu_add_ln_modulate_fwd``
    (affine) with the previous sublayer's residual add fused in; fc1 is ``uwu_gemm(EPI_BIAS)`` followed by ``uwu_bias_act_fwd``
    in place with no bias; embedding and pooling are ``uwu_text_embed`` / ``uwu_text_pool`` (the eos position is found on the
    device: no host synchronisation anywhere in the forward);
  * all parameters live in one flat fp32 buffer (+ a bf16 shadow in bf16 mode), both registered as buffers;
  * there is no backward and no CPU path.
"""
import hashlib
import math

import torch

from . import lib as L
from . import ops
from .flat import FlatModule, _Config

_COMMON = dict(max_position_embeddings=77, vocab_size=49408, layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=49406,
               pad_token_id=1)
# stabilityai/stable-diffusion-xl-base-1.0: text_encoder (CLIP ViT-L/14) and text_encoder_2 (OpenCLIP ViT-bigG/14)
SDXL_TEXT_CONFIGS = {
    "text_encoder": dict(_COMMON, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                         hidden_act="quick_gelu", projection_dim=768),
    "text_encoder_2": dict(_COMMON, hidden_size=1280, num_attention_heads=20, num_hidden_layers=32, intermediate_size=5120,
                           hidden_act="gelu", projection_dim=1280),
}
_HEAD_DIM = 64   # the one head width uwu_attention_causal_fwd is built for
_MAX_T = 128     # and its longest sequence


class _FinalLayerNorm:
    """``model.final_layer_norm``: callable on any hidden state [B, T, D] (ConcatTextEncoders applies it to ``hidden_states[
    layer_idx]``, text_encoders.py:185-186); runs on uwu_add_ln_modulate_fwd."""

    def __init__(self, model):
        self._m = model

    def __call__(self, x):
        m = self._m
        m._require_device(x, "final_layer_norm")
        D = m.config["hidden_size"]
        if x.shape[-1] != D:
            raise ValueError(f"final_layer_norm: expected [..., {D}], got {tuple(x.shape)}")
        x2 = x.reshape(-1, D).to(m.dtype).contiguous()
        return m._ln(x2, "final_layer_norm")[1].view(x.shape)


class _TextEncoder(FlatModule):
    """What the two encoders share on the host side: the constructor preamble, the checks on what ``forward`` is given, and
    ``from_config``.  A subclass brings its parameter table, ``reset_parameters``, ``_encode`` and ``from_pretrained``."""

    def _setup(self, defaults, config, compute_dtype, kw):
        """the head of a constructor: `config` and the remaining keywords merged over `defaults` into ``self.config``, the compute
        dtype checked and set -> (init_weights, device, seed)"""
        init_weights = kw.pop("init_weights", True)
        device = kw.pop("device", None)
        seed = kw.pop("seed", None)
        cfg = dict(defaults)
        cfg.update({k: v for k, v in (config or {}).items() if not k.startswith("_")})
        cfg.update(kw)
        if compute_dtype not in ("bf16", "fp32"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        self.config = _Config(cfg)
        self.compute_dtype = compute_dtype
        self.dtype = torch.bfloat16 if compute_dtype == "bf16" else torch.float32
        self._names = {}  # transformers name -> (stored name, first row, rows)
        return init_weights, device, seed

    def _require_device(self, t, what):
        if not torch.is_tensor(t) or not t.is_cuda or not self.flat.is_cuda:
            raise L.UwuError(f"{type(self).__name__}.{what} runs on the HIP device only (no CPU fallback)")
        if self.dtype == torch.bfloat16 and self.shadow.numel() != self.n:
            self.refresh_shadow()

    def _ids_and_mask(self, input_ids, attention_mask, max_T):
        """-> (int64 ids [B, T], int64 key mask [B, T] or None), both contiguous on the device"""
        self._require_device(input_ids, "forward")
        if input_ids.dim() != 2 or not 1 <= input_ids.shape[1] <= max_T:
            raise ValueError(f"input_ids must be [B, T <= {max_T}], got {tuple(input_ids.shape)}")
        B, T = input_ids.shape
        mask = None
        if attention_mask is not None:
            if not attention_mask.is_cuda or tuple(attention_mask.shape) != (B, T):
                raise L.UwuError(f"attention_mask must be a device tensor [{B}, {T}], got {tuple(attention_mask.shape)}")
            mask = attention_mask.long().contiguous()
        return input_ids.long().contiguous(), mask

    def _check_call(self, return_dict, kw):
        if return_dict:
            raise NotImplementedError("return_dict=True is not built: ConcatTextEncoders calls with return_dict=False")
        extra = sorted(k for k, v in kw.items() if v is not None)
        if extra:  # position_ids, inputs_embeds, output_attentions, ...: nothing is silently ignored
            raise NotImplementedError(f"{type(self).__name__}.forward: {extra} not built")

    @classmethod
    def from_config(cls, config, **kw):
        return cls(dict(config), **kw)


class _CLIPTower(_TextEncoder):
    """What the CLIP text transformer and the CLIP image tower (uwudiff_amd/vision_model.py) share: the parameters of a pre-LN
    encoder layer with q, k, v stored back to back, and the layer stack itself.  The attention operator is the caller's."""

    def _add_param(self, name, shape, alias=None):
        self.P.add(name, shape)
        if alias is None:
            self._names[name] = (name, 0, None)

    def _add_layers(self, prefix, n_layers, D, F):
        """``<prefix>encoder.layers.N.*`` under transformers' names, in the order the flat buffer keeps them"""
        add = self._add_param
        for i in range(n_layers):
            p = f"{prefix}encoder.layers.{i}."
            for sfx, shape in ((".weight", (3 * D, D)), (".bias", (3 * D,))):  # q, k, v back to back: one GEMM operand
                add(p + "self_attn.qkv_proj" + sfx, shape, alias=True)
                for c, row in (("k", D), ("v", 2 * D), ("q", 0)):  # (transformers lists k, v, q)
                    self._names[f"{p}self_attn.{c}_proj{sfx}"] = (p + "self_attn.qkv_proj" + sfx, row, D)
            for name, shape in (("self_attn.out_proj", (D, D)), ("layer_norm1", None), ("mlp.fc1", (F, D)), ("mlp.fc2", (D, F)),
                                ("layer_norm2", None)):
                add(p + name + ".weight", shape or (D,))
                add(p + name + ".bias", (shape[0],) if shape else (D,))

    def _ln(self, x, name, y=None):
        """(x + y, LayerNorm(x + y)): the residual add of the sublayer that produced y happens here"""
        return ops.add_ln_modulate_fwd(x, 1, x.shape[0], y=y, gate=self.ones if y is not None else None, shift=self.w32(name + ".bias"),
                                       scale=self.w32(name + ".weight"), mod_ld=0, eps=float(self.config["layer_norm_eps"]),
                                       affine=True)[:2]

    def _lin(self, x, name):
        return ops.gemm(x, self.w(name + ".weight"), bias=self.w32(name + ".bias"), epilogue=L.EPI_BIAS)

    def _run_layers(self, x, prefix, attn):
        """x [B*T, D] through every layer; ``attn(q, k, v)`` is the tower's attention on column slices of the packed projection ->
        (x, y, inputs): the stream before the last feed-forward's residual add, that feed-forward's output (the caller's next
        LayerNorm adds it), and the input of every layer"""
        cfg = self.config
        D = cfg["hidden_size"]
        inputs, y = [], None
        for i in range(cfg["num_hidden_layers"]):
            p = f"{prefix}encoder.layers.{i}."
            x, n = self._ln(x, p + "layer_norm1", y)  # x: the input of layer i = the output of layer i - 1
            inputs.append(x)
            qkv = self._lin(n, p + "self_attn.qkv_proj")
            o = attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:])
            x, n = self._ln(x, p + "layer_norm2", self._lin(o, p + "self_attn.out_proj"))
            u = self._lin(n, p + "mlp.fc1")
            ops.bias_act_fwd(u, cfg["hidden_act"], out=u)
            y = self._lin(u, p + "mlp.fc2")
        return x, y, inputs


class CLIPTextModel(_CLIPTower):
    """``transformers.CLIPTextModel``: ``forward(...) -> (last_hidden_state, pooled[, hidden_states])``."""

    kind = "clip_sd1"  # ConcatTextEncoders recomputes normed = final_layer_norm(hidden_states[layer_idx]) for this class
    _with_projection = False

    def __init__(self, config=None, compute_dtype="bf16", **kw):
        super().__init__()
        init_weights, device, seed = self._setup(SDXL_TEXT_CONFIGS["text_encoder"], config, compute_dtype, kw)
        cfg = self.config
        if cfg["hidden_act"] not in L.ACT:
            raise ValueError(f"CLIPTextModel: hidden_act {cfg['hidden_act']!r} is not built (known: {sorted(L.ACT)})")
        D, H = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
        if D != H * _HEAD_DIM:
            raise ValueError(f"CLIPTextModel: the attention kernel is built for heads of width {_HEAD_DIM}, got {D} / {H}")
        if cfg["max_position_embeddings"] > _MAX_T:
            raise ValueError(f"CLIPTextModel: at most {_MAX_T} positions, got {cfg['max_position_embeddings']}")
        if D % 8 or cfg["intermediate_size"] % 8 or (self._with_projection and cfg["projection_dim"] % 8):
            raise ValueError("CLIPTextModel: widths must be multiples of 8")

        add = self._add_param
        F = int(cfg["intermediate_size"])
        add("embeddings.token_embedding.weight", (cfg["vocab_size"], D))
        add("embeddings.position_embedding.weight", (cfg["max_position_embeddings"], D))
        self._add_layers("", cfg["num_hidden_layers"], D, F)
        add("final_layer_norm.weight", (D,))
        add("final_layer_norm.bias", (D,))
        if self._with_projection:
            add("text_projection.weight", (cfg["projection_dim"], D))
        self._alloc(compute_dtype == "bf16", device, buffer=True)
        self.register_buffer("ones", torch.ones(D, dtype=torch.float32, device=device), persistent=False)  # the residual's gate
        self.final_layer_norm = _FinalLayerNorm(self)
        if init_weights:
            self.reset_parameters(seed)
        self.eval().requires_grad_(False)

    # ------------------------------------------------------------------ parameters
    def _public(self, name):
        return name if not self._with_projection or name.startswith("text_projection.") else "text_model." + name

    def _public_names(self):
        return {self._public(name): ent for name, ent in self._names.items()}

    def _load_key(self, key):
        """transformers name, flat or in the ``text_model.``-prefixed layout of hub checkpoints; ``position_ids`` is a buffer older
        checkpoints carry, and a ``CLIPModel`` checkpoint holds the image tower and ``logit_scale`` next to the text model"""
        if key.endswith("position_ids") or key.startswith(("vision_model.", "visual_projection.")) or key == "logit_scale":
            return None
        return self._public(key.removeprefix("text_model."))

    @torch.no_grad()
    def reset_parameters(self, seed=None):
        """transformers' CLIP initialisation at initializer_factor 1 (embeddings N(0, 0.02), projections N(0, D^-1/2 (2L)^-1/2),
        fc1 N(0, (2D)^-1/2), norms 1 / 0, biases 0), drawn on the CPU from `seed` (default: torch.initial_seed(), as
        AutoencoderKL.reset_parameters) so the weights do not depend on the device the model is built on"""
        g = torch.Generator().manual_seed((torch.initial_seed() if seed is None else seed) % (2 ** 31))
        D, nl = self.config["hidden_size"], max(self.config["num_hidden_layers"], 1)
        in_std, out_std, fc_std = D ** -0.5 * (2 * nl) ** -0.5, D ** -0.5, (2 * D) ** -0.5
        for name, v in self.named_tensors():
            if name.endswith(".bias"):
                v.zero_()
            elif "layer_norm" in name:
                v.fill_(1.0)
            else:
                std = (0.02 if "embedding" in name else out_std if "out_proj" in name else fc_std if "fc1" in name
                       else D ** -0.5 if "text_projection" in name else in_std)
                v.copy_(torch.randn(v.shape, generator=g) * std)
        self.refresh_shadow()

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def _encode(self, input_ids, attention_mask):
        """-> (last_hidden_state [B, T, D], pooled [B, D], hidden_states: L + 1 tensors [B, T, D], embeddings first)"""
        cfg = self.config
        ids, mask = self._ids_and_mask(input_ids, attention_mask, cfg["max_position_embeddings"])
        B, T = ids.shape
        D, H = cfg["hidden_size"], cfg["num_attention_heads"]
        x = ops.text_embed(ids, self.w("embeddings.token_embedding.weight"), self.w("embeddings.position_embedding.weight"))
        x, y, hidden = self._run_layers(
            x, "", lambda q, k, v: ops.attention_causal_fwd(q, k, v, B, T, H, _HEAD_DIM, _HEAD_DIM ** -0.5, key_mask=mask))
        x, last = self._ln(x, "final_layer_norm", y)
        hidden.append(x)
        pooled = ops.text_pool(ids, last, cfg["eos_token_id"])
        return last.view(B, T, D), pooled, tuple(h.view(B, T, D) for h in hidden)

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=False, **kw):
        self._check_call(return_dict, kw)
        last, pooled, hidden = self._encode(input_ids, attention_mask)
        return (last, pooled, hidden) if output_hidden_states else (last, pooled)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, subfolder=None, **kw):
        """A local directory (``<path>[/<subfolder>]`` with ``config.json`` and ``model.safetensors``) is loaded.  Any other name ->
        deterministic random weights (seeded by the name and subfolder, not by the global seed) at the built-in SDXL configuration
        keyed by ``subfolder`` (``text_encoder`` when there is none): nothing is ever fetched."""
        kw = cls._drop_hub_keywords(kw)
        src = str(pretrained_model_name_or_path)
        model = cls._from_local_dir(src, subfolder, SDXL_TEXT_CONFIGS["text_encoder"], "model.safetensors", **kw)
        if model is not None:
            return model
        key = subfolder if subfolder is not None else "text_encoder"
        if key not in SDXL_TEXT_CONFIGS:
            raise ValueError(f"unknown text encoder {src!r} / subfolder {subfolder!r}: not a local directory with config.json; built-in "
                             f"configurations: {sorted(SDXL_TEXT_CONFIGS)}")
        config = dict(SDXL_TEXT_CONFIGS[key])
        config.update(kw.pop("config", None) or {})
        # the same name gives the same weights in every process, whatever the global seed
        return cls(config, seed=int.from_bytes(hashlib.md5(f"{src}/{key}".encode()).digest()[:4], "little"), **kw)


class CLIPTextModelWithProjection(CLIPTextModel):
    """``transformers.CLIPTextModelWithProjection``: ``forward(...) -> (text_embeds, last_hidden_state[, hidden_states])`` with
    ``text_embeds = text_projection(pooled)`` (no bias).  Not a plain ``CLIPTextModel`` for ConcatTextEncoders' normed-context rule
    (the reference's ``isinstance`` test, text_encoders.py:185), hence no ``kind``."""

    kind = "clip"
    _with_projection = True

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=False, **kw):
        self._check_call(return_dict, kw)
        last, pooled, hidden = self._encode(input_ids, attention_mask)
        embeds = ops.gemm(pooled, self.w("text_projection.weight"))
        return (embeds, last, hidden) if output_hidden_states else (embeds, last)


# ====================================================================================================== T5 v1.1 encoder
_T5_COMMON = dict(vocab_size=32128, d_kv=64, relative_attention_num_buckets=32, relative_attention_max_distance=128,
                  layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu", pad_token_id=0, eos_token_id=1)
# google/t5-v1_1-*: the published release (encoder stacks only are built here)
T5_CONFIGS = {
    "google/t5-v1_1-small": dict(_T5_COMMON, d_model=512, d_ff=1024, num_heads=6, num_layers=8),
    "google/t5-v1_1-base": dict(_T5_COMMON, d_model=768, d_ff=2048, num_heads=12, num_layers=12),
    "google/t5-v1_1-large": dict(_T5_COMMON, d_model=1024, d_ff=2816, num_heads=16, num_layers=24),
    "google/t5-v1_1-xl": dict(_T5_COMMON, d_model=2048, d_ff=5120, num_heads=32, num_layers=24),
    "google/t5-v1_1-xxl": dict(_T5_COMMON, d_model=4096, d_ff=10240, num_heads=64, num_layers=24),
}
_T5_MAX_T = 512  # the longest sequence uwu_attention_relbias_fwd is built for


def t5_offset_buckets(T, num_buckets=32, max_distance=128):
    """int32 [2T - 1]: the bucket of every offset ``key - query`` in ``-(T - 1) .. T - 1`` under T5's bidirectional rule -- half
    the buckets for each direction (keys after the query take the upper half); inside a half the distances below a quarter of
    ``num_buckets`` get a bucket each, the rest are spaced logarithmically up to ``max_distance`` and everything farther shares
    the last bucket.  The logarithm is taken in fp32, the precision the published checkpoints were trained with: a bucket edge
    that falls on an integer distance must land on the side it landed on then."""
    rel = torch.arange(-(T - 1), T, dtype=torch.long)
    half = num_buckets // 2
    exact = half // 2
    dist = rel.abs()
    far = dist.clamp_min(1).to(torch.float32) / exact
    log_bucket = exact + (torch.log(far) / math.log(max_distance / exact) * (half - exact)).to(torch.long)
    bucket = torch.where(dist < exact, dist, log_bucket.clamp_max(half - 1)) + (rel > 0).long() * half
    return bucket.to(torch.int32)


class T5EncoderModel(_TextEncoder):
    """``transformers.T5EncoderModel`` for the v1.1 (gated-GELU) checkpoints: ``forward(...) -> (last_hidden_state[, hidden_states])``
    (DESIGN.md section 4.25).  ``h = shared[ids]``; L blocks ``h += o(attn(RMS h))``, ``h += wo(gelu_new(wi_0 n) * wi_1 n)`` with
    ``n = RMS h``; ``final_layer_norm``.  No biases, no attention scale; the relative-position bias of block 0 is shared by all
    blocks and reaches the kernel as one fp32 row per head, gathered once per sequence length."""

    kind = "t5"

    def __init__(self, config=None, compute_dtype="bf16", **kw):
        super().__init__()
        init_weights, device, seed = self._setup(T5_CONFIGS["google/t5-v1_1-small"], config, compute_dtype, kw)
        cfg = self.config
        built = "built: the T5 v1.1 encoder -- d_kv = 64, feed_forward_proj = 'gated-gelu', widths that are multiples of 8"
        if cfg["feed_forward_proj"] not in L.GATE:
            raise ValueError(f"T5EncoderModel: feed_forward_proj {cfg['feed_forward_proj']!r} is not built ({built})")
        if int(cfg["d_kv"]) != _HEAD_DIM:
            raise ValueError(f"T5EncoderModel: d_kv = {cfg['d_kv']} is not built ({built})")
        D, H, F = int(cfg["d_model"]), int(cfg["num_heads"]), int(cfg["d_ff"])
        if D % 8 or F % 8 or D < 8 or F < 8 or H < 1 or cfg["relative_attention_num_buckets"] < 4:
            raise ValueError(f"T5EncoderModel: d_model = {D}, d_ff = {F}, num_heads = {H} ({built})")
        self._buckets, self._bias = {}, {}  # per T: the bucket of every offset (int32, device), the gathered bias [H, 2T - 1]
        HD = H * _HEAD_DIM

        def add(name, shape, public=True):
            self.P.add(name, shape)
            if public:
                self._names[name] = (name, 0, None)

        add("shared.weight", (cfg["vocab_size"], D))
        self._names["encoder.embed_tokens.weight"] = ("shared.weight", 0, None)  # one storage under both names
        for i in range(cfg["num_layers"]):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            add(a + "SelfAttention.qkv.weight", (3 * HD, D), public=False)  # q, k, v back to back: one GEMM operand
            for j, c in enumerate("qkv"):
                self._names[f"{a}SelfAttention.{c}.weight"] = (a + "SelfAttention.qkv.weight", j * HD, HD)
            add(a + "SelfAttention.o.weight", (D, HD))
            if i == 0:
                add(a + "SelfAttention.relative_attention_bias.weight", (cfg["relative_attention_num_buckets"], H))
            add(a + "layer_norm.weight", (D,))
            add(f + "DenseReluDense.wi.weight", (2 * F, D), public=False)  # wi_0 | wi_1: one GEMM, gated by uwu_gated_act_fwd
            for j in range(2):
                self._names[f"{f}DenseReluDense.wi_{j}.weight"] = (f + "DenseReluDense.wi.weight", j * F, F)
            add(f + "DenseReluDense.wo.weight", (D, F))
            add(f + "layer_norm.weight", (D,))
        add("encoder.final_layer_norm.weight", (D,))
        self._alloc(compute_dtype == "bf16", device, buffer=True)
        if init_weights and self.flat.device.type != "meta":
            self.reset_parameters(seed)
        self.eval().requires_grad_(False)

    # ------------------------------------------------------------------ parameters
    def _public_names(self):
        return self._names

    _TIED = ("shared.weight", "encoder.embed_tokens.weight")

    def _prepare_load(self, state_dict):
        """the embedding table may come under either of its two names or both; two tables that differ are refused before anything
        is written"""
        sd = dict(state_dict)
        a, b = (sd.get(k) for k in self._TIED)
        if a is not None and b is not None:
            if a.shape != b.shape or not torch.equal(a, b):
                raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: {self._TIED[0]} and {self._TIED[1]} are "
                                   "one tensor in this model, the state dict holds two that differ")
        elif a is not None or b is not None:  # one name given: the other is the same tensor, not a missing key
            sd[self._TIED[0]] = sd[self._TIED[1]] = a if a is not None else b
        return sd

    @torch.no_grad()
    def reset_parameters(self, seed=None):
        """transformers' T5 initialisation at initializer_factor 1 (embedding N(0, 1); q N(0, (d_model d_kv)^-1/2); k, v, wi_0, wi_1
        and the bias table N(0, d_model^-1/2); o N(0, (H d_kv)^-1/2); wo N(0, d_ff^-1/2); norms 1), drawn tensor by tensor on the
        CPU from `seed` (default: torch.initial_seed()): the weights do not depend on the device, and the host never holds more
        than one tensor"""
        g = torch.Generator().manual_seed((torch.initial_seed() if seed is None else seed) % (2 ** 31))
        c = self.config
        D, F, HD = c["d_model"], c["d_ff"], c["num_heads"] * _HEAD_DIM
        for name, v in self.named_tensors():
            if name == self._TIED[1]:
                continue
            if "layer_norm" in name:
                v.fill_(1.0)
                continue
            std = (1.0 if name == "shared.weight" else (D * _HEAD_DIM) ** -0.5 if name.endswith(".q.weight") else HD ** -0.5
                   if name.endswith(".o.weight") else F ** -0.5 if name.endswith(".wo.weight") else D ** -0.5)
            v.copy_(torch.randn(v.shape, generator=g) * std)
        self.refresh_shadow()

    def _shadow_stale(self):  # weights loaded, reset, or the model moved: the gathered bias is rebuilt on the next call
        self._bias = {}

    def _moved(self):
        self._buckets = {}

    # ------------------------------------------------------------------ forward
    def _rel_bias(self, T):
        """fp32 [H, 2T - 1] on the device; in steady state a dictionary lookup"""
        if T not in self._bias:
            c = self.config
            if T not in self._buckets:
                self._buckets[T] = t5_offset_buckets(T, c["relative_attention_num_buckets"], c["relative_attention_max_distance"]).to(
                    self.flat.device)
            self._bias[T] = ops.t5_rel_bias(self.w32("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), self._buckets[T])
        return self._bias[T]

    def _rms(self, x, name, y=None):
        """(x + y, RMSNorm(x + y)): the residual add of the sublayer that produced y happens here"""
        return ops.add_rmsnorm_fwd(x, self.w32(name), float(self.config["layer_norm_epsilon"]), y=y)

    @torch.no_grad()
    def _encode(self, input_ids, attention_mask):
        """-> (last_hidden_state [B, T, D], hidden_states: L + 1 tensors [B, T, D] -- the embeddings, the output of every block but
        the last, and last_hidden_state itself: transformers' encoder stack appends its final state after final_layer_norm)"""
        cfg = self.config
        ids, mask = self._ids_and_mask(input_ids, attention_mask, _T5_MAX_T)
        B, T = ids.shape
        D, H = cfg["d_model"], cfg["num_heads"]
        HD = H * _HEAD_DIM
        bias = self._rel_bias(T)
        x = ops.token_embed(ids, self.w("shared.weight"))
        hidden, y = [], None
        for i in range(cfg["num_layers"]):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            x, n = self._rms(x, a + "layer_norm.weight", y)  # x: the input of block i = the output of block i - 1
            hidden.append(x)
            qkv = ops.gemm(n, self.w(a + "SelfAttention.qkv.weight"))
            o = ops.attention_relbias_fwd(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], bias, B, T, H, _HEAD_DIM, 1.0, key_mask=mask)
            x, n = self._rms(x, f + "layer_norm.weight", ops.gemm(o, self.w(a + "SelfAttention.o.weight")))
            u = ops.gemm(n, self.w(f + "DenseReluDense.wi.weight"))
            y = ops.gemm(ops.gated_act_fwd(u, cfg["feed_forward_proj"]), self.w(f + "DenseReluDense.wo.weight"))
        _, last = self._rms(x, "encoder.final_layer_norm.weight", y)
        hidden.append(last)
        return last.view(B, T, D), tuple(h.view(B, T, D) for h in hidden)

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=False, **kw):
        self._check_call(return_dict, kw)
        last, hidden = self._encode(input_ids, attention_mask)
        return (last, hidden) if output_hidden_states else (last,)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, subfolder=None, **kw):
        """A local directory (``<path>[/<subfolder>]`` with ``config.json`` and ``model.safetensors``) is loaded.  Any other name ->
        deterministic random weights (seeded by the name, not by the global seed) at the built-in configuration of that name
        (``T5_CONFIGS``): nothing is ever fetched.  Without a ``device=`` the random model is built on the HIP device when there
        is one -- google/t5-v1_1-xxl is 19 GB of fp32, which the host never holds: the weights are drawn tensor by tensor.
        The local-directory path does not share that property yet: it builds the model where ``device=`` says (the CPU by
        default, as CLIP's does) and reads the whole safetensors file into host memory before copying it, 19 GB for xxl."""
        kw = cls._drop_hub_keywords(kw)
        src = str(pretrained_model_name_or_path)
        model = cls._from_local_dir(src, subfolder, T5_CONFIGS["google/t5-v1_1-small"], "model.safetensors", **kw)
        if model is not None:
            return model
        if src not in T5_CONFIGS:
            raise ValueError(f"unknown T5 encoder {src!r}: not a local directory with config.json; built-in configurations: "
                             f"{sorted(T5_CONFIGS)}")
        config = dict(T5_CONFIGS[src])
        config.update(kw.pop("config", None) or {})
        if "device" not in kw and torch.cuda.is_available():
            kw["device"] = "cuda"
        # the same name gives the same weights in every process, whatever the global seed
        return cls(config, seed=int.from_bytes(hashlib.md5(src.encode()).digest()[:4], "little"), **kw)
