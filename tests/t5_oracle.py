"""A plain-torch restatement of the T5 v1.1 encoder (transformers' T5EncoderModel with ``feed_forward_proj="gated-gelu"``): the
reference the GPU tests of uwudiff_amd.text_model.T5EncoderModel compare against, in the role tests/clip_oracle.py has for CLIP.
It takes a state dict (transformers' names) and a config dict, runs in the dtype asked for (float64 for the reference, bfloat16
to measure what that precision costs), and needs nothing but torch.  tests/test_t5_model_cpu.py pins it to ``transformers`` itself
where that package is installed."""
import math

import torch
import torch.nn.functional as F


def bucket_of(rel, num_buckets=32, max_distance=128):
    """T5's bidirectional bucket of the offsets ``rel = key - query`` (an integer tensor): keys after the query take the upper half
    of the buckets; in each half the distances below ``num_buckets / 4`` have a bucket each, then logarithmic steps up to
    ``max_distance``, everything farther in the last bucket.  fp32 logarithm, as the model was trained.
    The model's own t5_offset_buckets states the same published rule, so a whole-model comparison cannot tell a mistake the two
    share.  What makes them independent: tests/test_t5_model_cpu.py compares both with transformers' table where that package is
    installed, and its test_offset_buckets_rule pins the exact range, the first logarithmic edges and the clamps without it."""
    half = num_buckets // 2
    exact = half // 2
    dist = rel.abs()
    ratio = torch.log(dist.clamp_min(1).float() / exact) / math.log(max_distance / exact)
    far = (exact + (ratio * (half - exact)).long()).clamp_max(half - 1)
    return torch.where(dist < exact, dist, far) + (rel > 0).long() * half


def position_bias(table, T, num_buckets=32, max_distance=128, reverse=False):
    """[H, T, T]: bias[h, i, j] = table[bucket(j - i), h] for query i and key j (`reverse`: the mistake of indexing it by i - j)"""
    pos = torch.arange(T)
    rel = pos[None, :] - pos[:, None]
    return table[bucket_of(-rel if reverse else rel, num_buckets, max_distance)].permute(2, 0, 1)


def rms_norm(x, weight, eps):
    """T5LayerNorm: no mean, no bias.  The variance is taken in fp32 whatever the dtype of x -- also for float64, where it is
    the one step of transformers' model that is not carried out in the tensor's own precision (1e-7 relative, far below every
    bar of the GPU tests); restated so because the oracle is pinned to transformers at 1e-10."""
    var = x.float().pow(2).mean(-1, keepdim=True)
    return weight * (x * torch.rsqrt(var + eps)).to(x.dtype)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def attention(q, k, v, bias, attention_mask, scale=1.0):
    """q / k / v [B, H, T, 64], bias [H, T, T], attention_mask [B, T] or None -> [B, H, T, 64]; a row with no visible key gives zeros"""
    s = scale * (q @ k.transpose(-1, -2)) + bias[None]
    if attention_mask is not None:
        s = s.masked_fill((attention_mask == 0)[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.nan_to_num(p, nan=0.0) @ v


@torch.no_grad()
def forward(state_dict, config, input_ids, attention_mask=None, dtype=torch.float64, reverse_bias=False):
    """-> dict(last_hidden_state [B, T, D], hidden_states: L + 1 tensors -- the embeddings, the output of each block but the last,
    and last_hidden_state (transformers appends the final state after final_layer_norm))"""
    sd = {k: v.to(dtype) for k, v in state_dict.items()}
    B, T = input_ids.shape
    H, eps, d = config["num_heads"], config.get("layer_norm_epsilon", 1e-6), 64
    emb = sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"]
    x = emb[input_ids]
    bias = position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], T,
                         config.get("relative_attention_num_buckets", 32), config.get("relative_attention_max_distance", 128),
                         reverse=reverse_bias)
    hidden = []
    for i in range(config["num_layers"]):
        hidden.append(x)
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1.DenseReluDense."
        n = rms_norm(x, sd[a + "layer_norm.weight"], eps)
        q, k, v = (F.linear(n, sd[f"{a}SelfAttention.{c}.weight"]).view(B, T, H, d).transpose(1, 2) for c in "qkv")
        o = attention(q, k, v, bias, attention_mask).transpose(1, 2).reshape(B, T, H * d)
        x = x + F.linear(o, sd[a + "SelfAttention.o.weight"])
        n = rms_norm(x, sd[f"encoder.block.{i}.layer.1.layer_norm.weight"], eps)
        x = x + F.linear(gelu_new(F.linear(n, sd[f + "wi_0.weight"])) * F.linear(n, sd[f + "wi_1.weight"]), sd[f + "wo.weight"])
    last = rms_norm(x, sd["encoder.final_layer_norm.weight"], eps)
    hidden.append(last)
    return dict(last_hidden_state=last, hidden_states=tuple(hidden))


def random_state_dict(config, seed, bias_std=1.0):
    """a state dict with every tensor random (the norm weights too) at magnitudes that keep activations O(1).  The bias table is
    drawn at std 1.0, not the initialiser's d_model^-1/2: on the tiny configuration, indexing the bias by i - j instead of j - i
    then moves the last hidden state by 0.39 relative L2 (fp64), far above the bf16 bar of about 0.017; at the default
    initialisation the same mistake moves it by 0.064, and far less at width 4096, where a test could pass it."""
    g = torch.Generator().manual_seed(seed)
    D, Fd, H, V = config["d_model"], config["d_ff"], config["num_heads"], config["vocab_size"]
    HD = 64 * H
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std  # noqa: E731
    sd = {"shared.weight": r(V, D)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for i in range(config["num_layers"]):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        sd[a + "SelfAttention.q.weight"] = r(HD, D, std=(D * 8.0) ** -0.5)  # scores of a few units: neither flat nor one-hot
        sd[a + "SelfAttention.k.weight"] = r(HD, D, std=D ** -0.5)
        sd[a + "SelfAttention.v.weight"] = r(HD, D, std=D ** -0.5)
        sd[a + "SelfAttention.o.weight"] = r(D, HD, std=HD ** -0.5)
        if i == 0:
            sd[a + "SelfAttention.relative_attention_bias.weight"] = r(config.get("relative_attention_num_buckets", 32), H, std=bias_std)
        sd[a + "layer_norm.weight"] = 1.0 + r(D, std=0.2)
        sd[f + "DenseReluDense.wi_0.weight"] = r(Fd, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wi_1.weight"] = r(Fd, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wo.weight"] = r(D, Fd, std=Fd ** -0.5)
        sd[f + "layer_norm.weight"] = 1.0 + r(D, std=0.2)
    sd["encoder.final_layer_norm.weight"] = 1.0 + r(D, std=0.2)
    return sd


TINY = dict(d_model=128, num_heads=2, d_ff=256, num_layers=3, vocab_size=1000, d_kv=64, relative_attention_num_buckets=32,
            relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")


def tokens(config, lengths, seed, T=77):
    """right-padded ids / attention_mask int64 [len(lengths), T]: `length - 1` words, eos (1), then pad (0)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lengths), T, dtype=torch.long)
    mask = torch.zeros(len(lengths), T, dtype=torch.long)
    for b, n in enumerate(lengths):
        ids[b, :n - 1] = torch.randint(3, config["vocab_size"], (n - 1,), generator=g)
        ids[b, n - 1] = 1
        mask[b, :n] = 1
    return ids, mask
