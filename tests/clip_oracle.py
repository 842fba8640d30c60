"""A plain-torch restatement of the CLIP text transformer (transformers' CLIPTextModel / CLIPTextModelWithProjection): the
reference the GPU tests of uwudiff_amd/text_model.py compare against, in the role tests/vae_oracle.py has for the VAE.  It takes a
state dict (transformers' names, with or without the ``text_model.`` prefix) and a config dict, runs in the dtype asked for
(float64 for the reference, bfloat16 to measure what that precision costs), and needs nothing but torch.
tests/test_text_model_cpu.py pins it to ``transformers`` itself where that package is installed."""
import torch
import torch.nn.functional as F


def _act(x, kind):
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if kind == "gelu":
        return F.gelu(x)
    raise ValueError(kind)


def pool_position(input_ids, eos_token_id):
    """the eos position of each row: the legacy largest-id rule at eos_token_id == 2, else the first id equal to it (0 if none)"""
    if eos_token_id == 2:
        return input_ids.argmax(dim=-1)
    return (input_ids == eos_token_id).int().argmax(dim=-1)


def visible(attention_mask, B, T):
    """bool [B, T, T]: key j is visible to query i iff j <= i and attention_mask[b, j] != 0"""
    vis = torch.ones(T, T, dtype=torch.bool).tril()[None].expand(B, T, T)
    if attention_mask is not None:
        vis = vis & (attention_mask != 0)[:, None, :]
    return vis


@torch.no_grad()
def forward(state_dict, config, input_ids, attention_mask=None, dtype=torch.float64):
    """-> dict(last_hidden_state [B, T, D], pooled [B, D], hidden_states (L + 1 tensors, embeddings first), text_embeds [B, P] or
    None when the state dict has no ``text_projection.weight``)"""
    sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.to(dtype) for k, v in state_dict.items()
          if not k.endswith("position_ids")}
    B, T = input_ids.shape
    D, H, eps = config["hidden_size"], config["num_attention_heads"], config.get("layer_norm_eps", 1e-5)
    d = D // H
    x = sd["embeddings.token_embedding.weight"][input_ids] + sd["embeddings.position_embedding.weight"][:T][None]
    bias = torch.zeros(B, 1, T, T, dtype=dtype).masked_fill(~visible(attention_mask, B, T)[:, None], float("-inf"))
    hidden = [x]
    for i in range(config["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        lin = lambda t, n: F.linear(t, sd[p + n + ".weight"], sd[p + n + ".bias"])  # noqa: E731
        h = F.layer_norm(x, (D,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
        q, k, v = (lin(h, f"self_attn.{c}_proj").view(B, T, H, d).transpose(1, 2) for c in "qkv")
        a = torch.softmax((q * d ** -0.5) @ k.transpose(-1, -2) + bias, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, D), "self_attn.out_proj")
        h = F.layer_norm(x, (D,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps)
        x = x + lin(_act(lin(h, "mlp.fc1"), config["hidden_act"]), "mlp.fc2")
        hidden.append(x)
    last = F.layer_norm(x, (D,), sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps)
    pooled = last[torch.arange(B), pool_position(input_ids, config.get("eos_token_id", 2))]
    proj = sd.get("text_projection.weight")
    return dict(last_hidden_state=last, pooled=pooled, hidden_states=tuple(hidden),
                text_embeds=None if proj is None else F.linear(pooled, proj))


def final_layer_norm(state_dict, config, x, dtype=torch.float64):
    sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}
    return F.layer_norm(x.to(dtype), (config["hidden_size"],), sd["final_layer_norm.weight"].to(dtype),
                        sd["final_layer_norm.bias"].to(dtype), config.get("layer_norm_eps", 1e-5))


def random_state_dict(config, seed, projection=False, scale=1.0):
    """a state dict with every tensor random -- biases and LayerNorm parameters too, so no term of the model is switched off --
    at magnitudes that keep activations O(1) through the layers"""
    g = torch.Generator().manual_seed(seed)
    D, Fd, V, P = config["hidden_size"], config["intermediate_size"], config["vocab_size"], config["max_position_embeddings"]
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std * scale  # noqa: E731
    sd = {"embeddings.token_embedding.weight": r(V, D, std=0.5), "embeddings.position_embedding.weight": r(P, D, std=0.2)}
    for i in range(config["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for c in "kvq":
            sd[p + f"self_attn.{c}_proj.weight"] = r(D, D, std=1.5 * D ** -0.5)
            sd[p + f"self_attn.{c}_proj.bias"] = r(D, std=0.1)
        sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"] = r(D, D, std=D ** -0.5), r(D, std=0.1)
        sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = r(Fd, D, std=D ** -0.5), r(Fd, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = r(D, Fd, std=Fd ** -0.5), r(D, std=0.1)
        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
    sd["final_layer_norm.weight"], sd["final_layer_norm.bias"] = 1.0 + r(D, std=0.2), r(D, std=0.1)
    if projection:
        sd["text_projection.weight"] = r(config["projection_dim"], D, std=D ** -0.5)
    return sd


TINY_QUICK = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512, max_position_embeddings=77,
                  vocab_size=1000, hidden_act="quick_gelu", eos_token_id=2, layer_norm_eps=1e-5, projection_dim=64)
TINY_GELU = dict(TINY_QUICK, hidden_act="gelu", eos_token_id=999)


def tokens(config, lengths, seed, T=77):
    """right-padded ids / attention_mask int64 [len(lengths), T]: bos (vocab - 2), `length - 2` words, eos (vocab - 1, the largest id
    and the eos of TINY_GELU), then pad = eos as CLIP tokenizers pad; a length-1 row is bos alone"""
    g = torch.Generator().manual_seed(seed)
    V = config["vocab_size"]
    ids = torch.full((len(lengths), T), V - 1, dtype=torch.long)
    mask = torch.zeros(len(lengths), T, dtype=torch.long)
    for b, n in enumerate(lengths):
        ids[b, 0] = V - 2
        if n > 2:
            ids[b, 1:n - 1] = torch.randint(3, V - 2, (n - 2,), generator=g)
        mask[b, :n] = 1
    return ids, mask
