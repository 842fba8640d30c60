"""A plain-torch restatement of the CLIP image tower (transformers' CLIPVisionModelWithProjection) and of the CLIP score: the reference
the GPU tests of uwudiff_amd/vision_model.py and uwudiff_amd/metrics.py compare against, in the role tests/clip_oracle.py has for the
text transformer.  It takes a state dict under transformers' names and a config dict, runs in the dtype asked for (float64 for the
reference, bfloat16 to measure what that precision costs) and needs nothing but torch.  tests/test_metrics_cpu.py pins it to
``transformers.CLIPModel`` where that package is installed."""
import torch
import torch.nn.functional as F

from tests import clip_oracle

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def preprocess(images, dtype=torch.float64):
    """images [B, 3, S, S] with values in [0, 255] -> pixel_values: (clamp(x, 0, 255) / 255 - mean) / std"""
    x = images.to(dtype).clamp(0, 255) / 255
    mean, std = (torch.tensor(t, dtype=dtype).view(1, 3, 1, 1) for t in (CLIP_MEAN, CLIP_STD))
    return (x - mean) / std


@torch.no_grad()
def forward(state_dict, config, pixel_values, dtype=torch.float64):
    """-> dict(image_embeds [B, P], last_hidden_state [B, T, D], pooled [B, D] = post_layernorm(last[:, 0]), hidden_states (L + 1
    tensors: the output of pre_layrnorm, then of every layer))"""
    sd = {k: v.to(dtype) for k, v in state_dict.items() if k.startswith(("vision_model.", "visual_projection."))}
    D, H, eps, p = config["hidden_size"], config["num_attention_heads"], config.get("layer_norm_eps", 1e-5), config["patch_size"]
    d = D // H
    x = pixel_values.to(dtype)
    B = x.shape[0]
    patches = F.conv2d(x, sd["vision_model.embeddings.patch_embedding.weight"], stride=p).flatten(2).transpose(1, 2)  # [B, Np, D]
    cls = sd["vision_model.embeddings.class_embedding"].expand(B, 1, D)
    x = torch.cat([cls, patches], dim=1) + sd["vision_model.embeddings.position_embedding.weight"][None]
    T = x.shape[1]
    x = F.layer_norm(x, (D,), sd["vision_model.pre_layrnorm.weight"], sd["vision_model.pre_layrnorm.bias"], eps)
    hidden = [x]
    for i in range(config["num_hidden_layers"]):
        pre = f"vision_model.encoder.layers.{i}."
        lin = lambda t, n: F.linear(t, sd[pre + n + ".weight"], sd[pre + n + ".bias"])  # noqa: E731
        h = F.layer_norm(x, (D,), sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"], eps)
        q, k, v = (lin(h, f"self_attn.{c}_proj").view(B, T, H, d).transpose(1, 2) for c in "qkv")
        a = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2), dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, D), "self_attn.out_proj")
        h = F.layer_norm(x, (D,), sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"], eps)
        x = x + lin(clip_oracle._act(lin(h, "mlp.fc1"), config["hidden_act"]), "mlp.fc2")
        hidden.append(x)
    pooled = F.layer_norm(x[:, 0], (D,), sd["vision_model.post_layernorm.weight"], sd["vision_model.post_layernorm.bias"], eps)
    return dict(image_embeds=F.linear(pooled, sd["visual_projection.weight"]), last_hidden_state=x, pooled=pooled,
                hidden_states=tuple(hidden))


def scores(image_embeds, text_embeds):
    """100 cos(image_b, text_b), in the dtype of the embeddings"""
    a = image_embeds / image_embeds.norm(dim=-1, keepdim=True)
    b = text_embeds / text_embeds.norm(dim=-1, keepdim=True)
    return 100 * (a * b).sum(-1)


@torch.no_grad()
def clip_score(state_dict, vision_config, text_config, images, input_ids, attention_mask, dtype=torch.float64):
    """max(mean(100 cos), 0) of [0, 255] images and tokenised captions under a CLIPModel-layout state dict -> (score, per-pair scores)"""
    img = forward(state_dict, vision_config, preprocess(images, dtype), dtype)["image_embeds"]
    text_sd = {k: v for k, v in state_dict.items() if k.startswith(("text_model.", "text_projection."))}
    txt = clip_oracle.forward(text_sd, text_config, input_ids, attention_mask, dtype)["text_embeds"]
    s = scores(img.double(), txt.double())
    return max(float(s.mean()), 0.0), s


def random_state_dict(config, seed, scale=1.0):
    """the image tower's state dict with every tensor random -- biases, LayerNorm parameters and the class embedding too, so no
    term of the model is switched off -- at magnitudes that keep activations O(1) through the layers"""
    g = torch.Generator().manual_seed(seed)
    D, Fd, p = config["hidden_size"], config["intermediate_size"], config["patch_size"]
    T = (config["image_size"] // p) ** 2 + 1
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std * scale  # noqa: E731
    v = "vision_model."
    sd = {v + "embeddings.class_embedding": r(D, std=0.5),
          v + "embeddings.patch_embedding.weight": r(D, 3, p, p, std=0.5 * (3 * p * p) ** -0.5),
          v + "embeddings.position_embedding.weight": r(T, D, std=0.2),
          v + "pre_layrnorm.weight": 1.0 + r(D, std=0.2), v + "pre_layrnorm.bias": r(D, std=0.1)}
    for i in range(config["num_hidden_layers"]):
        pre = f"{v}encoder.layers.{i}."
        for c in "kvq":
            sd[pre + f"self_attn.{c}_proj.weight"] = r(D, D, std=1.5 * D ** -0.5)
            sd[pre + f"self_attn.{c}_proj.bias"] = r(D, std=0.1)
        sd[pre + "self_attn.out_proj.weight"], sd[pre + "self_attn.out_proj.bias"] = r(D, D, std=D ** -0.5), r(D, std=0.1)
        sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
        sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"] = r(Fd, D, std=D ** -0.5), r(Fd, std=0.1)
        sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"] = r(D, Fd, std=Fd ** -0.5), r(D, std=0.1)
        sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
    sd[v + "post_layernorm.weight"], sd[v + "post_layernorm.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
    sd["visual_projection.weight"] = r(config["projection_dim"], D, std=D ** -0.5)
    return sd


_TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512, projection_dim=64, num_channels=3,
             layer_norm_eps=1e-5, hidden_act="quick_gelu")
TINY_A = dict(_TINY, patch_size=14, image_size=70)                      # T = 26: inside one 64-query block; 3 p p = 588 is padded to 592
TINY_B = dict(_TINY, patch_size=8, image_size=72, hidden_act="gelu")   # T = 82: crosses one 64-query block and leaves a tail


def pixel_values(config, B, seed):
    """normalised pixel values of the size a real image gives: N(0, 1), roughly what (x / 255 - mean) / std spans"""
    S = config["image_size"]
    return torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed))


def images_u8(config, B, seed):
    """integer-valued float images [B, 3, S, S] in [0, 255]"""
    S = config["image_size"]
    return torch.randint(0, 256, (B, 3, S, S), generator=torch.Generator().manual_seed(seed)).float()
