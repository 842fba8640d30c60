"""CPU: tests/t5_oracle.py against ``transformers`` itself in fp64, and the host side of uwudiff_amd.text_model.T5EncoderModel -- the
bucket-per-offset table, the transformers key set with the embedding under both of its names, local-directory loading, the
built-in configurations, target resolution of the alias and of configs/demo_training_sd3te.yaml, the tokenizer stand-in, and the
refusals that need no device."""
import json
import os

import pytest
import torch

from tests import t5_oracle
from tests.conftest import ROOT

LENGTHS = [77, 40, 5]  # two padded rows
SMALL = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, vocab_size=500)


def _hf(cfg):
    transformers = pytest.importorskip("transformers")
    hf_cfg = transformers.T5Config(
        d_model=cfg["d_model"], d_kv=64, d_ff=cfg["d_ff"], num_layers=cfg["num_layers"], num_heads=cfg["num_heads"],
        vocab_size=cfg["vocab_size"], relative_attention_num_buckets=cfg["relative_attention_num_buckets"],
        relative_attention_max_distance=cfg["relative_attention_max_distance"], layer_norm_epsilon=cfg["layer_norm_epsilon"],
        feed_forward_proj="gated-gelu", dropout_rate=0.0)
    torch.manual_seed(7)
    m = transformers.T5EncoderModel(hf_cfg).eval().double()
    with torch.no_grad():  # norms are initialised to 1 and the bias table small: make every term live
        for n, p in m.named_parameters():
            if "layer_norm" in n:
                p.add_(0.2 * torch.randn_like(p))
            elif "relative_attention_bias" in n:
                p.normal_(0.0, 1.0)
            elif n.endswith((".q.weight", ".k.weight")):
                p.mul_(0.5)
    return m


def test_oracle_equals_transformers_fp64():
    """last hidden state and every hidden state to 1e-10 at all positions, with and without a mask; L + 1 hidden states, the
    embeddings first, the last one equal to last_hidden_state (after final_layer_norm)"""
    cfg = t5_oracle.TINY
    m = _hf(cfg)
    ids, mask = t5_oracle.tokens(cfg, LENGTHS, seed=3)
    with torch.no_grad():
        out = m(ids, attention_mask=mask, output_hidden_states=True, return_dict=True)
        nomask = m(ids, output_hidden_states=True, return_dict=True)
    sd = m.state_dict()
    ref = t5_oracle.forward(sd, cfg, ids, mask)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0, atol=1e-10)  # noqa: E731
    close(ref["last_hidden_state"], out.last_hidden_state)
    assert len(out.hidden_states) == cfg["num_layers"] + 1 == len(ref["hidden_states"])
    for a, b in zip(ref["hidden_states"], out.hidden_states):
        close(a, b)
    assert torch.equal(out.hidden_states[0], sd["shared.weight"][ids])
    assert torch.equal(out.hidden_states[-1], out.last_hidden_state)
    close(t5_oracle.forward(sd, cfg, ids, None)["last_hidden_state"], nomask.last_hidden_state)
    assert float((out.last_hidden_state[2] - nomask.last_hidden_state[2]).abs().max()) > 1e-3  # the mask matters
    # the direction of the bias matters far more than the bf16 bar (2e-2): what random_state_dict's std 1.0 is for
    rev = t5_oracle.forward(sd, cfg, ids, mask, reverse_bias=True)["last_hidden_state"]
    moved = float((rev - ref["last_hidden_state"]).norm() / ref["last_hidden_state"].norm())
    print(f"[t5 oracle] reversed bias moves the last hidden state by {moved:.3f} relative L2")
    assert moved > 0.2


@pytest.mark.parametrize("T", [77, 128, 512])
@pytest.mark.parametrize("num_buckets,max_distance", [(32, 128), (16, 64)])
def test_offset_buckets_equal_transformers(T, num_buckets, max_distance):
    """the host's table over offsets -(T - 1) .. T - 1 against transformers' bucket of every (query, key) pair"""
    pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention

    from uwudiff_amd.text_model import t5_offset_buckets

    table = t5_offset_buckets(T, num_buckets, max_distance)
    assert table.dtype == torch.int32 and tuple(table.shape) == (2 * T - 1,)
    pos = torch.arange(T)
    rel = pos[None, :] - pos[:, None]  # key - query
    want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
    assert torch.equal(table.long()[rel + T - 1], want)
    assert torch.equal(t5_oracle.bucket_of(rel, num_buckets, max_distance), want)
    if (num_buckets, max_distance) == (32, 128):  # T = 77 stops short of the last bucket of each direction (first reached at 91)
        assert table.unique().numel() == (29 if T == 77 else 31)


def test_offset_buckets_rule():
    """without transformers: exact below num_buckets / 4, the upper half for keys after the query, clamped to the last bucket"""
    from uwudiff_amd.text_model import t5_offset_buckets

    T = 200
    t = t5_offset_buckets(T, 32, 128).tolist()
    at = lambda rel: t[rel + T - 1]  # noqa: E731
    assert [at(-r) for r in range(8)] == list(range(8)) and [at(r) for r in range(1, 8)] == [16 + r for r in range(1, 8)]
    assert at(-8) == 8 and at(8) == 24 and at(-127) == 15 and at(-199) == 15 and at(199) == 31 and at(128) == 31
    assert all(at(-r) <= at(-r - 1) for r in range(T - 1))  # monotone in the distance
    assert min(r for r in range(T) if at(-r) == 15) == 91


def _native(cfg=None, **kw):
    from uwudiff_amd.text_model import T5EncoderModel

    return T5EncoderModel.from_config(cfg or SMALL, **kw)


def test_key_set_and_both_embedding_spellings():
    """state_dict() has transformers' keys (both names of the embedding); a load accepts either name or both, packs q / k / v and
    wi_0 / wi_1 back to back, and refuses two embeddings that differ without writing anything"""
    ref = t5_oracle.random_state_dict(dict(t5_oracle.TINY, **SMALL), seed=2)
    for drop in (None, "shared.weight", "encoder.embed_tokens.weight"):
        m = _native(init_weights=False, compute_dtype="fp32")
        assert not m.flat.any()
        res = m.load_state_dict({k: v for k, v in ref.items() if k != drop})
        assert not res.missing_keys and not res.unexpected_keys
        got = m.state_dict()
        assert sorted(got) == sorted(ref)
        for k, v in ref.items():
            assert got[k].dtype == torch.float32 and torch.equal(got[k], v), (drop, k)
    try:
        import transformers
        hf = transformers.T5EncoderModel(transformers.T5Config(d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2, vocab_size=500,
                                                                feed_forward_proj="gated-gelu"))
        assert sorted(hf.state_dict()) == sorted(got)  # the key set of the installed transformers
        assert all(tuple(hf.state_dict()[k].shape) == tuple(got[k].shape) for k in got)
    except ImportError:
        pass
    HD, F = 128, 256
    w = m.w32("encoder.block.1.layer.0.SelfAttention.qkv.weight")
    assert tuple(w.shape) == (3 * HD, 128)
    for j, c in enumerate("qkv"):
        assert torch.equal(w[j * HD:(j + 1) * HD], ref[f"encoder.block.1.layer.0.SelfAttention.{c}.weight"])
    w = m.w32("encoder.block.1.layer.1.DenseReluDense.wi.weight")
    assert torch.equal(w[:F], ref["encoder.block.1.layer.1.DenseReluDense.wi_0.weight"])
    assert torch.equal(w[F:], ref["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"])
    assert tuple(m.w32("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").shape) == (32, 2)
    assert "encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight" not in got


def test_load_state_dict_refusals_write_nothing():
    m = _native(seed=1)
    ref = t5_oracle.random_state_dict(dict(t5_oracle.TINY, **SMALL), seed=2)
    before = m.state_dict()
    bad = dict(ref)
    bad["encoder.embed_tokens.weight"] = ref["shared.weight"] + 1.0
    with pytest.raises(RuntimeError, match="embed_tokens"):
        m.load_state_dict(bad)
    bad = dict(ref)
    del bad["encoder.block.1.layer.1.DenseReluDense.wi_1.weight"]
    with pytest.raises(RuntimeError, match="wi_1.weight"):
        m.load_state_dict(bad)
    bad = dict(ref)
    bad["encoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(64, 128)
    with pytest.raises(RuntimeError, match="q.weight"):
        m.load_state_dict(bad)
    bad = dict(ref)
    bad["encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight"] = torch.zeros(32, 2)  # block 0 owns the only table
    with pytest.raises(RuntimeError, match="relative_attention_bias"):
        m.load_state_dict(bad)
    bad = {k: v for k, v in ref.items() if "embed_tokens" not in k and k != "shared.weight"}
    with pytest.raises(RuntimeError, match="shared.weight"):
        m.load_state_dict(bad)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_local_directory_round_trip(tmp_path, monkeypatch):
    from safetensors.torch import save_file

    from uwudiff_amd.text_model import T5EncoderModel
    from uwudiff_amd.flat import FlatModule

    calls, inner = [], FlatModule._from_local_dir.__func__  # every local directory goes through the one loader in flat.py
    monkeypatch.setattr(FlatModule, "_from_local_dir", classmethod(lambda c, *a, **kw: calls.append(c) or inner(c, *a, **kw)))

    cfg = dict(t5_oracle.TINY, **SMALL)
    ref = t5_oracle.random_state_dict(cfg, seed=5)
    d = tmp_path / "enc"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(cfg, architectures=["T5EncoderModel"], model_type="t5", is_gated_act=True)))
    save_file({k: v.clone().contiguous() for k, v in ref.items() if k != "encoder.embed_tokens.weight"}, str(d / "model.safetensors"))
    for m in (T5EncoderModel.from_pretrained(str(d), torch_dtype=torch.float16), T5EncoderModel.from_pretrained(str(tmp_path), subfolder="enc")):
        assert m.config.d_model == 128 and m.config.num_layers == 2 and m.kind == "t5" and "is_gated_act" not in m.config
        got = m.state_dict()
        assert all(torch.equal(got[k], v) for k, v in ref.items())
    assert calls == [T5EncoderModel] * 2


def test_same_name_same_weights_and_builtin_configs():
    from uwudiff_amd.text_model import T5_CONFIGS, T5EncoderModel

    rows = {"small": (512, 1024, 6, 8), "base": (768, 2048, 12, 12), "large": (1024, 2816, 16, 24), "xl": (2048, 5120, 32, 24),
            "xxl": (4096, 10240, 64, 24)}
    for name, (D, F, H, nl) in rows.items():
        c = T5_CONFIGS[f"google/t5-v1_1-{name}"]
        assert (c["d_model"], c["d_ff"], c["num_heads"], c["num_layers"]) == (D, F, H, nl)
        assert (c["vocab_size"], c["relative_attention_num_buckets"], c["relative_attention_max_distance"], c["layer_norm_epsilon"],
                c["d_kv"], c["feed_forward_proj"]) == (32128, 32, 128, 1e-6, 64, "gated-gelu")
    # the xxl layout on the meta device: 24 (4 * 4096^2 + 3 * 4096 * 10240) + 32128 * 4096 + norms + the bias table
    m = T5EncoderModel.from_pretrained("google/t5-v1_1-xxl", device="meta")
    params = sum(v.numel() for k, v in m.named_tensors() if k != "encoder.embed_tokens.weight")
    assert params == 24 * (4 * 4096 ** 2 + 3 * 4096 * 10240 + 2 * 4096) + 32128 * 4096 + 4096 + 32 * 64 and m.flat.device.type == "meta"
    small = dict(num_layers=1, vocab_size=64)
    a, b = (T5EncoderModel.from_pretrained("google/t5-v1_1-small", config=small, device="cpu") for _ in range(2))
    torch.manual_seed(99)  # the global seed plays no part
    c = T5EncoderModel.from_pretrained("google/t5-v1_1-small", config=small, device="cpu")
    d = T5EncoderModel.from_pretrained("google/t5-v1_1-base", config=dict(small, d_model=512, d_ff=1024, num_heads=6), device="cpu")
    assert torch.equal(a.flat, b.flat) and torch.equal(a.flat, c.flat) and not torch.equal(a.flat, d.flat)
    assert a.config.d_model == 512 and a.config.num_heads == 6  # H * 64 = 384 != d_model
    sd = a.state_dict()
    std = lambda k: float(sd[k].std())  # noqa: E731
    p = "encoder.block.0.layer."
    assert abs(std("shared.weight") - 1.0) < 0.05 and abs(std(p + "0.SelfAttention.q.weight") / (512 * 64) ** -0.5 - 1) < 0.05
    assert abs(std(p + "0.SelfAttention.k.weight") / 512 ** -0.5 - 1) < 0.05 and abs(std(p + "0.SelfAttention.o.weight") / 384 ** -0.5 - 1) < 0.05
    assert abs(std(p + "1.DenseReluDense.wi_1.weight") / 512 ** -0.5 - 1) < 0.05 and abs(std(p + "1.DenseReluDense.wo.weight") / 1024 ** -0.5 - 1) < 0.05
    assert bool((sd[p + "0.layer_norm.weight"] == 1).all()) and bool((sd["encoder.final_layer_norm.weight"] == 1).all())
    with pytest.raises(ValueError, match="built-in configurations"):
        T5EncoderModel.from_pretrained("google/flan-t5-huge")


def test_configuration_refusals_say_what_is_built():
    for bad in (dict(d_kv=32), dict(feed_forward_proj="relu"), dict(feed_forward_proj="gelu"), dict(d_model=132), dict(d_ff=1001)):
        with pytest.raises(ValueError, match="gated-gelu"):
            _native(dict(SMALL, **bad), device="meta")
    with pytest.raises(ValueError, match="compute_dtype"):
        _native(compute_dtype="fp16", device="meta")


def test_forward_refuses_cpu_tensors_and_unbuilt_arguments():
    from uwudiff_amd import lib as L

    m = _native(seed=0)
    ids = torch.ones(1, 8, dtype=torch.long)
    with pytest.raises(L.UwuError, match="HIP device only"):
        m(ids)
    with pytest.raises(NotImplementedError, match="return_dict"):
        m(ids, return_dict=True)
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        m(ids, inputs_embeds=torch.zeros(1, 8, 128))


def test_alias_and_yaml_resolve_to_the_native_class():
    from uwudiff_amd import config as C
    from uwudiff_amd.text_model import CLIPTextModel, T5EncoderModel

    assert C.get_obj_from_str("transformers.T5EncoderModel") is T5EncoderModel
    assert C.get_obj_from_str("transformers.T5EncoderModel.from_pretrained") == T5EncoderModel.from_pretrained
    assert C.ALIASES["transformers.CLIPTextModel"] == "uwudiff_amd.conditioning.SyntheticCLIPTextModel"  # untouched
    cfg = C.load_yaml(os.path.join(ROOT, "configs", "demo_training_sd3te.yaml"))
    te = cfg.trainer.model_config.te
    assert te.tokenizers[2] == "google/t5-v1_1-xxl" and len(te.text_model_and_configs) == 3
    node, extra = te.text_model_and_configs[2]
    assert node["_target_"] == "transformers.T5EncoderModel.from_pretrained" and extra["concat_bucket"] == 1 and extra["need_mask"] is True
    m = C.instantiate(dict(node, device="meta"))
    assert type(m) is T5EncoderModel and m.config.d_model == 4096 == cfg.trainer.model_config.unet.cross_attention_dim
    assert [C.get_obj_from_str(p[0]["_target_"]).__self__ for p in te.text_model_and_configs[:2]] == [CLIPTextModel, CLIPTextModel]
    assert [p[1]["concat_bucket"] for p in te.text_model_and_configs] == [0, 0, 1]


def test_t5_tokenizer_stand_in_stays_inside_the_vocabulary():
    from uwudiff_amd.conditioning import ConcatTextEncoders, SyntheticTokenizer

    clip = SyntheticTokenizer("openai/clip-vit-large-patch14")
    assert clip.model_max_length == 77 and clip("a cat")["input_ids"][0, 0].item() == 49406  # names without t5: as before
    for name in ("google/t5-v1_1-xxl", "T5Tokenizer"):
        tok = SyntheticTokenizer(name)
        assert tok.model_max_length == 512
        out = tok(["a photo of a cat", " ".join(f"w{i}" for i in range(600)), ""])
        ids, mask = out["input_ids"], out["attention_mask"]
        assert tuple(ids.shape) == (3, 512) and int(ids.max()) < 32100 and int(ids.min()) >= 0
        assert mask.sum(1).tolist() == [6, 512, 1]
        assert ids[0, 5].item() == 1 and not ids[0, 6:].any() and bool((ids[0, :5] >= 3).all())  # words, eos, pad; no bos
        assert ids[1, 511].item() == 1 and ids[2, 0].item() == 1
    te = ConcatTextEncoders(tokenizers=["openai/clip-vit-large-patch14", "google/t5-v1_1-xxl"], max_length=256)
    assert [t.model_max_length for t in te.tokenizers] == [77, 256]
