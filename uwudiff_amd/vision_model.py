"""The CLIP image tower on the HIP kernels, frozen, forward only: ``transformers.CLIPVisionModelWithProjection``
restated from its public description --

    patches = conv(pixel_values, patch_embedding, stride p)         no bias: one GEMM on uwu_clip_patches' operand
    h = pre_layrnorm([class_embedding; patches] + position_embedding)
    L pre-LN layers, the ones of the CLIP text transformer (text_model._CLIPTower) under bidirectional attention with no mask
    image_embeds = visual_projection(post_layernorm(h[:, 0]))       no bias

-- with transformers' parameter names in ``state_dict()`` (their misspelt ``pre_layrnorm`` included) and every operator in
``libuwu_hip.so``: activations stay ``[B*T, D]`` in the compute dtype, q / k / v are one bias GEMM read in place by
``uwu_attention_bidir_fwd`` (T = (S/p)^2 + 1 = 50, 197, 257 or 577: none is a multiple of the MFMA tile, the kernel pads inside), every
LayerNorm is ``uwu_add_ln_modulate_fwd`` with the previous residual add fused in.  There is no backward and no CPU path.

Head width 64 only: ViT-H/14 (heads of 80, ``apple/DFN5B-CLIP-ViT-H-14-378`` among them) is not built.
"""
import hashlib
import json
import os

import torch

from . import lib as L
from . import ops
from .flat import pad8
from .text_model import _HEAD_DIM, CLIPTextModelWithProjection, _CLIPTower

CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)  # transformers OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
_MAX_T = 1024  # the longest sequence uwu_attention_bidir_fwd takes

_VISION_COMMON = dict(num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5, image_mean=CLIP_IMAGE_MEAN, image_std=CLIP_IMAGE_STD)
_VIT_B = dict(_VISION_COMMON, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, projection_dim=512)
_VIT_L = dict(_VISION_COMMON, hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, intermediate_size=4096, projection_dim=768)
_TEXT_COMMON = dict(max_position_embeddings=77, vocab_size=49408, layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=49406, pad_token_id=1,
                    hidden_act="quick_gelu")
_TEXT_B = dict(_TEXT_COMMON, hidden_size=512, num_attention_heads=8, num_hidden_layers=12, intermediate_size=2048, projection_dim=512)
_TEXT_L = dict(_TEXT_COMMON, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, projection_dim=768)
# the four published OpenAI CLIP releases: name -> (vision tower, text tower)
CLIP_CONFIGS = {
    "openai/clip-vit-base-patch32": (dict(_VIT_B, patch_size=32, image_size=224), _TEXT_B),
    "openai/clip-vit-base-patch16": (dict(_VIT_B, patch_size=16, image_size=224), _TEXT_B),
    "openai/clip-vit-large-patch14": (dict(_VIT_L, patch_size=14, image_size=224), _TEXT_L),
    "openai/clip-vit-large-patch14-336": (dict(_VIT_L, patch_size=14, image_size=336), _TEXT_L),
}
_PATCH_W = "vision_model.embeddings.patch_embedding.weight"


def _name_seed(name):
    return int.from_bytes(hashlib.md5(name.encode()).digest()[:4], "little")


class CLIPVisionModelWithProjection(_CLIPTower):
    """``forward(pixel_values) -> (image_embeds, last_hidden_state[, hidden_states])``; ``embed_images`` takes [0, 255] images and
    fuses CLIP's preprocessing into the patch kernel."""

    kind = "clip_vision"

    def __init__(self, config=None, compute_dtype="bf16", **kw):
        super().__init__()
        init_weights, device, seed = self._setup(CLIP_CONFIGS["openai/clip-vit-large-patch14"][0], config, compute_dtype, kw)
        cfg = self.config
        if cfg["hidden_act"] not in L.ACT:
            raise ValueError(f"CLIPVisionModelWithProjection: hidden_act {cfg['hidden_act']!r} is not built (known: {sorted(L.ACT)})")
        D, H, F = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
        p, S, proj = int(cfg["patch_size"]), int(cfg["image_size"]), int(cfg["projection_dim"])
        if D != H * _HEAD_DIM:
            raise ValueError(f"CLIPVisionModelWithProjection: the attention kernel is built for heads of width {_HEAD_DIM}, got {D} / {H} = "
                             f"{D / H:g} (ViT-H/14 has heads of 80 -- apple/DFN5B-CLIP-ViT-H-14-378 included -- and is not built)")
        if int(cfg["num_channels"]) != 3 or p < 1 or S < p or S % p:
            raise ValueError(f"CLIPVisionModelWithProjection: 3 channels and image_size a multiple of patch_size, got {cfg['num_channels']} "
                             f"channels, {S} / {p}")
        self.T = (S // p) ** 2 + 1
        if self.T > _MAX_T:
            raise ValueError(f"CLIPVisionModelWithProjection: at most {_MAX_T} tokens, image_size {S} / patch_size {p} gives {self.T}")
        if D % 8 or F % 8 or proj % 8:
            raise ValueError("CLIPVisionModelWithProjection: widths must be multiples of 8")
        self._K = 3 * p * p  # the patch GEMM's K, stored padded to a multiple of 8 (3 * 14 * 14 = 588 is none)
        add = self._add_param
        add("vision_model.embeddings.class_embedding", (D,))
        add(_PATCH_W, (D, pad8(self._K)))
        add("vision_model.embeddings.position_embedding.weight", (self.T, D))
        for n in ("weight", "bias"):
            add("vision_model.pre_layrnorm." + n, (D,))
        self._add_layers("vision_model.", cfg["num_hidden_layers"], D, F)
        for n in ("weight", "bias"):
            add("vision_model.post_layernorm." + n, (D,))
        add("visual_projection.weight", (proj, D))
        self._alloc(compute_dtype == "bf16", device, buffer=True)
        self.register_buffer("ones", torch.ones(D, dtype=torch.float32, device=device), persistent=False)  # the residual's gate
        if init_weights and self.flat.device.type != "meta":
            self.reset_parameters(seed)
        self.eval().requires_grad_(False)

    # ------------------------------------------------------------------ parameters
    def _public_names(self):
        return self._names

    def _public_view(self, v, name):
        if name == _PATCH_W:  # [D, pad8(3 p p)] -> transformers' [D, 3, p, p]; the padding columns stay zero
            p = int(self.config["patch_size"])
            return v[:, :self._K].unflatten(1, (3, p, p))
        return v

    def _load_key(self, key):
        """transformers names; a ``CLIPModel`` checkpoint holds the text tower and ``logit_scale`` next to the image tower"""
        if key.endswith("position_ids") or key.startswith(("text_model.", "text_projection.")) or key == "logit_scale":
            return None
        return key

    @torch.no_grad()
    def reset_parameters(self, seed=None):
        """transformers' CLIP initialisation at initializer_factor 1 (class embedding N(0, D^-1/2), patch and position embeddings
        N(0, 0.02), projections N(0, D^-1/2 (2L)^-1/2), out_proj N(0, D^-1/2), fc1 N(0, (2D)^-1/2), visual_projection N(0, D^-1/2),
        norms 1 / 0, biases 0), drawn tensor by tensor on the CPU from `seed` (default: torch.initial_seed())"""
        g = torch.Generator().manual_seed((torch.initial_seed() if seed is None else seed) % (2 ** 31))
        D, nl = self.config["hidden_size"], max(self.config["num_hidden_layers"], 1)
        in_std, out_std, fc_std = D ** -0.5 * (2 * nl) ** -0.5, D ** -0.5, (2 * D) ** -0.5
        for name, v in self.named_tensors():
            if name.endswith(".bias"):
                v.zero_()
            elif "layer_norm" in name or "layernorm" in name or "layrnorm" in name:
                v.fill_(1.0)
            else:
                std = (0.02 if "_embedding." in name else out_std if "out_proj" in name or "class_embedding" in name or
                       "visual_projection" in name else fc_std if "fc1" in name else in_std)
                v.copy_(torch.randn(v.shape, generator=g) * std)
        self.refresh_shadow()

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def _encode(self, images, normalize):
        """images [B, 3, S, S] -> (image_embeds [B, P], last_hidden_state [B, T, D], hidden_states: L + 1 tensors [B, T, D] -- the
        output of pre_layrnorm, then of every layer)"""
        cfg = self.config
        self._require_device(images, "forward")
        S = int(cfg["image_size"])
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B, 3, {S}, {S}] (interpolate_pos_encoding is not built), got {tuple(images.shape)}")
        if images.dtype != torch.uint8:
            images = images.float()
        B, T, D, H = images.shape[0], self.T, cfg["hidden_size"], cfg["num_attention_heads"]
        a = ops.clip_patches(images.contiguous(), int(cfg["patch_size"]), self.dtype,
                             mean=tuple(cfg["image_mean"]) if normalize else None, std=tuple(cfg["image_std"]) if normalize else None)
        x = ops.vit_embed(ops.gemm(a, self.w(_PATCH_W)), self.w("vision_model.embeddings.class_embedding"),
                          self.w("vision_model.embeddings.position_embedding.weight"), B)
        _, x = self._ln(x, "vision_model.pre_layrnorm")  # the residual stream starts at the normalised embeddings
        x, y, hidden = self._run_layers(x, "vision_model.", lambda q, k, v: ops.attention_bidir_fwd(q, k, v, B, T, H, _HEAD_DIM,
                                                                                                     _HEAD_DIM ** -0.5))
        last = ops.add(x, y) if y is not None else x  # the last feed-forward's residual add (no layers: nothing to add)
        hidden.append(last)
        _, pooled = self._ln(last.view(B, T, D)[:, 0].contiguous(), "vision_model.post_layernorm")  # the class token's rows only
        embeds = ops.gemm(pooled, self.w("visual_projection.weight"))
        return embeds, last.view(B, T, D), tuple(h.view(B, T, D) for h in hidden)

    def forward(self, pixel_values, output_hidden_states=False, return_dict=False, **kw):
        """pixel_values: fp32 [B, 3, S, S], already normalised (what ``CLIPImageProcessor`` returns)"""
        self._check_call(return_dict, kw)
        if torch.is_tensor(pixel_values) and pixel_values.dtype == torch.uint8:
            raise ValueError("pixel_values are normalised floats; a uint8 image goes through embed_images")
        embeds, last, hidden = self._encode(pixel_values, False)
        return (embeds, last, hidden) if output_hidden_states else (embeds, last)

    def embed_images(self, images):
        """images: [B, 3, S, S] with values in [0, 255], fp32 or uint8, already at the model's size -> image_embeds [B, P].  CLIP's
        preprocessing, ``(clamp(x, 0, 255) / 255 - mean) / std``, happens inside uwu_clip_patches."""
        return self._encode(images, True)[0]

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, subfolder=None, **kw):
        """A local directory (``<path>[/<subfolder>]`` with ``config.json`` and ``model.safetensors``) is loaded: a saved
        ``CLIPVisionModelWithProjection``, or a whole ``CLIPModel`` (``vision_config`` inside ``config.json``; the text tower's
        tensors and ``logit_scale`` are passed over).  One of the names in ``CLIP_CONFIGS`` -> deterministic random weights seeded by
        the name.  Anything else raises; nothing is ever fetched."""
        kw = cls._drop_hub_keywords(kw)
        src = str(pretrained_model_name_or_path)
        local = os.path.join(src, subfolder) if subfolder else src
        if os.path.isdir(local) and os.path.exists(os.path.join(local, "config.json")):
            from safetensors.torch import load_file

            config = clip_configs_from_json(os.path.join(local, "config.json"))[0]
            config.update(kw.pop("config", None) or {})
            model = cls(config, init_weights=False, **kw)
            model.load_state_dict(load_file(os.path.join(local, "model.safetensors")))
            return model
        if src not in CLIP_CONFIGS:
            raise ValueError(f"unknown CLIP model {src!r}: not a local directory with config.json; built-in configurations: "
                             f"{sorted(CLIP_CONFIGS)} (heads of width 64 only: ViT-H/14 models such as apple/DFN5B-CLIP-ViT-H-14-378 "
                             "are not built)")
        config = dict(CLIP_CONFIGS[src][0])
        config.update(kw.pop("config", None) or {})
        return cls(config, seed=_name_seed(src + "/vision"), **kw)


def clip_configs_from_json(path):
    """``config.json`` of a ``CLIPModel`` (``vision_config`` / ``text_config`` / ``projection_dim``) or of one tower saved alone ->
    (vision config, text config) restricted to the keys that are built; a tower the file does not describe comes back as None"""
    with open(path) as f:
        raw = json.load(f)
    known_v, known_t = CLIP_CONFIGS["openai/clip-vit-large-patch14"]

    def pick(sub, known):
        if sub is None:
            return None
        out = {k: v for k, v in sub.items() if k in known}
        if "projection_dim" in raw:  # CLIPModel keeps it at the top level, and that one is what sizes both projections
            out["projection_dim"] = raw["projection_dim"]
        return out

    if "vision_config" in raw or "text_config" in raw:
        return pick(raw.get("vision_config"), known_v), pick(raw.get("text_config"), known_t)
    if "patch_size" in raw:
        return pick(raw, known_v), None
    return None, pick(raw, known_t)


def load_clip_pair(model_name_or_path, compute_dtype="bf16", device=None):
    """(CLIPTextModelWithProjection, CLIPVisionModelWithProjection) of one CLIP model: a local ``CLIPModel`` directory (both towers
    read from its one ``model.safetensors``) or a name in ``CLIP_CONFIGS`` (random weights seeded by the name)."""
    src = str(model_name_or_path)
    kw = dict(compute_dtype=compute_dtype, device=device)
    if os.path.isdir(src) and os.path.exists(os.path.join(src, "config.json")):
        from safetensors.torch import load_file

        vcfg, tcfg = clip_configs_from_json(os.path.join(src, "config.json"))
        if vcfg is None or tcfg is None:
            raise ValueError(f"{src}: config.json must describe both towers (vision_config and text_config of a CLIPModel)")
        sd = load_file(os.path.join(src, "model.safetensors"))
        text = CLIPTextModelWithProjection(tcfg, init_weights=False, **kw)
        vision = CLIPVisionModelWithProjection(vcfg, init_weights=False, **kw)
        text.load_state_dict(sd)
        vision.load_state_dict(sd)
        return text, vision
    vision = CLIPVisionModelWithProjection.from_pretrained(src, **kw)  # raises for a name that is not built
    return CLIPTextModelWithProjection(dict(CLIP_CONFIGS[src][1]), seed=_name_seed(src + "/text"), **kw), vision
