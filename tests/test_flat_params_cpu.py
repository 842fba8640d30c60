"""CPU: the shared flat-parameter store (uwudiff_amd/flat.py) and what the four models inherit from it.

  * the layout pin: ``tests/golden/flat_layouts.json`` holds, per model, ``n`` and a sha256 over the ordered (name, offset, shape)
    list and the ordered ``state_dict()`` keys, plus the sha256 of ``flat`` after ``torch.manual_seed(0)`` + construction at a tiny
    configuration.  The C++ DiT driver, the fused AdamW, the gradient-sync slices and the optimizer moments of saved checkpoints all
    index the flat buffer by offset, so neither may move.  The fixture was written by running ``layout_digest`` / ``flat_digest``
    of this file over ``LAYOUT_CASES`` / ``INIT_CASES`` on the commit before the store was shared (each model still had its own
    registry then: ``model.P`` on UNet and VAE, ``model.registry`` / ``model.n`` / ``model.n_flat`` on CLIP and DiT);
  * the store on a toy registry: padding, aliasing views, stacked matrices, ``span``;
  * per model: the round trip under a parent module, the two-phase load (a refused load writes nothing), missing / unexpected keys,
    and dtype casts that leave the fp32 master alone.
"""
import hashlib
import json
import os
import re

import pytest
import torch
import torch.nn as nn

from tests import clip_oracle
from tests.conftest import GOLDEN, ROOT

TINY_UNET = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
                 down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
                 transformer_layers_per_block=(1, 2), attention_head_dim=(1, 1), cross_attention_dim=32,
                 addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48,
                 norm_num_groups=8)
TINY_VAE = dict(block_out_channels=(32, 64), layers_per_block=1, mid_block_add_attention=False)
TINY_DIT = dict(depth=2, hidden=64, heads=1, patch=2, sample_size=8, in_channels=4, out_channels=4, cond_dim=16)


def _unet(cfg, **kw):
    from uwudiff_amd.unet import UNet2DConditionModel

    return UNet2DConditionModel(cfg, **kw)


def _vae(cfg, **kw):
    from uwudiff_amd.vae import AutoencoderKL

    return AutoencoderKL(cfg, **kw)


def _clip(cfg, projection=True, **kw):
    from uwudiff_amd.text_model import CLIPTextModel, CLIPTextModelWithProjection

    return (CLIPTextModelWithProjection if projection else CLIPTextModel)(cfg, **kw)


def _dit(**cfg):
    from uwudiff_amd.dit import DiT, DiTConfig

    return DiT(DiTConfig(**cfg))


def _sdxl(which):
    from uwudiff_amd import text_model, unet, vae

    return {"unet": unet.SDXL_UNET_CONFIG, "tiny_unet": unet.TINY_UNET_CONFIG, "vae": vae.SDXL_VAE_CONFIG,
            "te1": text_model.SDXL_TEXT_CONFIGS["text_encoder"], "te2": text_model.SDXL_TEXT_CONFIGS["text_encoder_2"]}[which]


_META = dict(init_weights=False, device="meta")
LAYOUT_CASES = {
    "unet_sdxl": lambda: _unet(_sdxl("unet"), **_META),
    "unet_tiny_config": lambda: _unet(_sdxl("tiny_unet"), **_META),
    "vae_sdxl": lambda: _vae(_sdxl("vae"), **_META),
    "clip_sdxl_text_encoder": lambda: _clip(_sdxl("te1"), projection=False, **_META),
    "clip_sdxl_text_encoder_proj": lambda: _clip(_sdxl("te1"), **_META),
    "clip_sdxl_text_encoder_2_proj": lambda: _clip(_sdxl("te2"), **_META),
    "dit_s2_rope": lambda: _dit(depth=12, hidden=384, heads=6, patch=2, rope=True, cond_dim=1280),
    "dit_s2_uncond": lambda: _dit(depth=12, hidden=384, heads=6, patch=2, cond_dim=0),
}
INIT_CASES = {
    "unet": lambda: _unet(TINY_UNET),
    "unet_rope": lambda: _unet(dict(TINY_UNET, rope=True)),
    "vae": lambda: _vae(TINY_VAE),
    "clip": lambda: _clip(clip_oracle.TINY_QUICK, projection=False),
    "clip_proj": lambda: _clip(clip_oracle.TINY_GELU),
    "dit": lambda: _dit(**TINY_DIT),
    "dit_rope_uncond": lambda: _dit(**dict(TINY_DIT, rope=True, cond_dim=0)),
}
MODELS = ["unet", "vae", "clip", "clip_proj", "dit"]


def layout_digest(registry, keys):
    """sha256 over the ordered (name, offset, shape) list and the ordered state_dict keys"""
    doc = [[[name, int(off), [int(s) for s in shape]] for name, (off, shape) in registry.items()], list(keys)]
    return hashlib.sha256(json.dumps(doc).encode()).hexdigest()


def flat_digest(flat):
    return hashlib.sha256(flat.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "flat_layouts.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------- the pin
@pytest.mark.parametrize("case", sorted(LAYOUT_CASES))
def test_flat_layout_is_pinned(case, golden):
    m = LAYOUT_CASES[case]()
    assert m.P.n == golden["layout"][case]["n"] == m.flat.numel()
    assert layout_digest(m.P.registry, m.state_dict()) == golden["layout"][case]["sha256"]
    assert m.registry is m.P.registry and m.n == m.P.n  # the names tests and tools read


@pytest.mark.parametrize("case", sorted(INIT_CASES))
def test_seeded_initialisation_is_pinned(case, golden):
    torch.manual_seed(0)
    m = INIT_CASES[case]()
    assert flat_digest(m.flat) == golden["init"][case]


# ---------------------------------------------------------------------- the store on a toy registry
def _toy():
    from uwudiff_amd.flat import FlatParams

    P = FlatParams()
    for name, shape in (("a.weight", (3, 5)), ("q", (4, 16)), ("k", (4, 16)), ("v", (4, 16)), ("o", (2, 16)), ("odd0", (3, 7)),
                        ("odd1", (3, 7)), ("vec0", (64,)), ("vec1", (64,))):
        P.add(name, shape)
    P.flat = torch.arange(P.n, dtype=torch.float32)
    P.shadow = P.flat.to(torch.bfloat16)
    return P


def test_store_pads_every_tensor_to_64_elements():
    from uwudiff_amd.flat import pad8, pad64

    assert [pad64(n) for n in (0, 1, 63, 64, 65, 128)] == [0, 64, 64, 64, 128, 128]
    assert [pad8(n) for n in (1, 3, 8, 9)] == [8, 8, 8, 16]
    P = _toy()
    assert P.registry["a.weight"] == (0, (3, 5)) and P.registry["q"] == (64, (4, 16))
    assert [P.registry[k][0] for k in ("k", "v", "o", "odd0", "odd1", "vec0", "vec1")] == [128, 192, 256, 320, 384, 448, 512]
    assert P.n == 576 and all(off % 64 == 0 for off, _ in P.registry.values())


def test_store_views_alias_the_buffers():
    P = _toy()
    P.bf16 = False
    w = P.w("a.weight")
    assert w.dtype == torch.float32 and P.dtype == torch.float32 and tuple(w.shape) == (3, 5)
    assert torch.equal(w, torch.arange(15.0).view(3, 5))
    w[1, 2] = -7.0
    assert P.flat[7] == -7.0 and P.w32("a.weight")[1, 2] == -7.0 and P.base32("a.weight").data_ptr() == P.flat.data_ptr()
    P.bf16 = True
    assert P.dtype == torch.bfloat16 and P.w("q").dtype == torch.bfloat16 and P.w("q").data_ptr() == P.shadow[64:].data_ptr()
    assert P.w32("q").dtype == torch.float32  # biases and norm vectors are read in fp32 in bf16 mode too
    P.flat = P.flat.requires_grad_()
    g = P.g("k")  # the gradient buffer appears on first use and is viewed the same way
    g += 1.0
    assert P.flat.grad.sum() == 64 and P.flat.grad[128:192].sum() == 64


def test_store_stacks_back_to_back_matrices():
    P = _toy()
    P.bf16 = False
    assert P.span(["q", "k", "v"]) == ("q", 3)
    qkv = P.w(("q", 3))
    assert tuple(qkv.shape) == (12, 16) and torch.equal(qkv[4:8], P.w("k")) and qkv.data_ptr() == P.w("q").data_ptr()
    assert P.span(["k", "v"]) == ("k", 2) and P.span(["q"]) == ("q", 1)


def test_store_span_refuses_gaps_and_shape_changes():
    P = _toy()
    assert P.span(["v", "o"]) is None          # another shape
    assert P.span(["odd0", "odd1"]) is None    # 21 elements each: padding sits between them
    assert P.span(["q", "v"]) is None          # not adjacent
    assert P.span(["vec0", "vec1"]) is None    # vectors are no GEMM operand


# ---------------------------------------------------------------------- the four models
class _Holder(nn.Module):
    """a trainer-like parent: the model as a sub-module beside a buffer of its own"""

    def __init__(self, m):
        super().__init__()
        self.m = m
        self.register_buffer("steps", torch.zeros(1))


def _build(name, seed):
    torch.manual_seed(seed)
    return INIT_CASES[name]()


@pytest.fixture(scope="module", params=MODELS)
def pair(request):
    """(model name, the state dict of a seed-2 model, that model's flat buffer) -- left as they are by every test, which load them
    into seed-5 models of their own"""
    twin = _build(request.param, 2)
    return request.param, twin.state_dict(), twin.flat.detach().clone()


def _matrix_key(sd, skip=0):
    """a key whose tensor is a non-square matrix (conv kernels count: their leading two dims)"""
    keys = [k for k, v in sd.items() if v.dim() >= 2 and v.shape[0] != v.shape[1]]
    return keys[len(keys) // 2 + skip]


def test_round_trip_under_a_parent_module(pair):
    name, sd, twin_flat = pair
    fresh = _build(name, 5)
    src = _Holder(fresh)
    fresh.load_state_dict(sd)
    psd = src.state_dict()
    assert "m.flat" not in psd and "steps" in psd and [k[2:] for k in psd if k.startswith("m.")] == list(sd)
    dst = _Holder(_build(name, 5))
    assert not torch.equal(dst.m.flat, twin_flat)
    res = dst.load_state_dict(psd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.m.flat, twin_flat)  # bit exact, padding included
    got = dst.m.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) and got[k].is_contiguous() for k in sd)
    # and the parent reports what its child reports
    bad = dict(psd)
    del bad["m." + list(sd)[3]]
    bad["m.nonsense.weight"] = torch.zeros(1)
    res = dst.load_state_dict(bad, strict=False)
    assert res.missing_keys == ["m." + list(sd)[3]] and res.unexpected_keys == ["m.nonsense.weight"]
    with pytest.raises(RuntimeError, match="nonsense"):
        dst.load_state_dict(bad, strict=True)


@pytest.mark.parametrize("how", ["transposed", "one_row", "one_more_row"])
def test_wrong_shape_is_refused_with_nothing_written(pair, how):
    name, sd, _ = pair
    m = _build(name, 5)
    before = m.flat.detach().clone()
    bad = dict(sd)  # every other entry is valid and differs from the model's: a one-pass loader would have written them
    k = _matrix_key(sd)
    v = sd[k]
    bad[k] = {"transposed": v.transpose(0, 1).contiguous(),  # as many elements (a reshape would take it)
              "one_row": v[:1].contiguous(),                  # broadcastable (a bare copy_ would take it)
              "one_more_row": torch.cat([v, v[:1]])}[how]
    assert list(bad).index(k) > 0 and not torch.equal(m.state_dict()[list(sd)[0]], sd[list(sd)[0]])
    with pytest.raises(RuntimeError, match=re.escape(k)):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError, match=re.escape(k)):
        m.load_state_dict(bad, strict=False)
    assert torch.equal(m.flat, before)
    holder = _Holder(m)
    with pytest.raises(RuntimeError, match=re.escape(k)):
        holder.load_state_dict({"steps": torch.zeros(1), **{"m." + n: t for n, t in bad.items()}})
    assert torch.equal(m.flat, before)


def test_missing_and_unexpected_keys(pair):
    name, sd, twin_flat = pair
    m = _build(name, 5)
    before = m.flat.detach().clone()
    gone = _matrix_key(sd, skip=1)
    short = {k: v for k, v in sd.items() if k != gone}
    extra = {**sd, "no.such.tensor": torch.zeros(3)}
    for bad, word in ((short, gone), (extra, "no.such.tensor")):
        with pytest.raises(RuntimeError, match=re.escape(word)):
            m.load_state_dict(bad)
        assert torch.equal(m.flat, before)  # strict: refused before anything is written
    res = m.load_state_dict({**short, "no.such.tensor": torch.zeros(3)}, strict=False)
    assert res.missing_keys == [gone] and res.unexpected_keys == ["no.such.tensor"]
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in short) and not torch.equal(got[gone], sd[gone])
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(m.flat, twin_flat)


def test_dtype_casts_leave_the_fp32_master_alone(pair):
    m = _build(pair[0], 5)
    assert m._uwu_keep_fp32_master is True
    kind = (type(m.flat), m.flat.requires_grad, "flat" in dict(m.named_buffers()))
    if m.flat.requires_grad:
        m.flat.grad = torch.full_like(m.flat.data, 0.25)
    before = m.flat.detach().clone()
    for cast in (lambda x: x.half(), lambda x: x.to(torch.bfloat16), lambda x: x.to("cpu", torch.float16), lambda x: x.double()):
        assert cast(m) is m
        assert m.flat.dtype == torch.float32 and torch.equal(m.flat, before)
        assert m.shadow.dtype == torch.bfloat16 and m.P.flat is m.flat and m.P.shadow is m.shadow
        assert (type(m.flat), m.flat.requires_grad, "flat" in dict(m.named_buffers())) == kind
        if m.flat.requires_grad:
            assert m.flat.grad.dtype == torch.float32 and bool((m.flat.grad == 0.25).all())
    m.P.w32(next(iter(m.P.registry))).fill_(3.0)  # the store still views the module's buffer
    assert float(m.flat.detach()[0]) == 3.0


def test_flat_stays_the_kind_of_object_it_was():
    unet, vae, clip, dit = (_build(n, 0) for n in ("unet", "vae", "clip", "dit"))
    for m in (unet, dit):
        assert isinstance(m.flat, nn.Parameter) and m.flat.requires_grad and list(m.parameters()) == [m.flat]
    assert isinstance(vae.flat, nn.Parameter) and not vae.flat.requires_grad
    assert not isinstance(clip.flat, nn.Parameter) and not list(clip.parameters()) and "flat" in dict(clip.named_buffers())
    for m in (unet, vae, clip, dit):
        assert "shadow" in dict(m.named_buffers()) and "shadow" not in m.state_dict() and "flat" not in m.state_dict()
    assert dit.n_flat == dit.P.n and torch.equal(dit.view("final.bias"), dit.P.base32("final.bias"))
    live = dit.state_dict(keep_vars=True)["final.bias"]
    assert live.data_ptr() == dit.view("final.bias").data_ptr()  # keep_vars: the views themselves
    assert "y_embedder.weight" not in _build("dit_rope_uncond", 0).state_dict() and "y_embedder.weight" in dit.state_dict()


@pytest.mark.parametrize("name", ["clip", "clip_proj"])
def test_clip_takes_both_key_layouts_and_passes_over_position_ids(name):
    twin = _build(name, 2)
    sd, twin_flat = twin.state_dict(), twin.flat
    m = _build(name, 5)
    strip = lambda k: k[len("text_model."):] if k.startswith("text_model.") else k  # noqa: E731
    res = m.load_state_dict({**{"text_model." + strip(k): v for k, v in sd.items() if not k.startswith("text_projection")},
                             **{k: v for k, v in sd.items() if k.startswith("text_projection")},
                             "text_model.embeddings.position_ids": torch.arange(77)[None]})
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(m.flat, twin_flat)
    m = _build(name, 5)
    m.load_state_dict({strip(k): v for k, v in sd.items()})
    assert torch.equal(m.flat, twin_flat)


# ---------------------------------------------------------------------- one copy of each
def test_the_store_is_written_once():
    src = {}
    pkg = os.path.join(ROOT, "uwudiff_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            with open(os.path.join(pkg, f)) as fh:
                src[f] = fh.read()
    count = lambda pat, skip=(): {f: len(re.findall(pat, s)) for f, s in src.items() if f not in skip and re.search(pat, s)}  # noqa: E731
    assert count(r"def _?pad64\b") == {"flat.py": 1} and count(r"def _?pad8\b") == {"flat.py": 1}
    assert count(r"def refresh_shadow\b") == {"flat.py": 1}
    # (the adapter network keeps a loader of its own kind; engine.py's warm-up scheduler is no module)
    assert count(r"def load_state_dict\(self, state_dict", skip=("adapters.py",)) == {"flat.py": 1}
    assert count(r"def _apply\(self, fn") == {"flat.py": 1}
    assert "from .unet import" not in src["vae.py"] and "import unet" not in src["vae.py"]
