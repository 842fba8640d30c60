"""GPU: the CLIP text transformer (uwudiff_amd/text_model.py) and its four kernels against references computed on the CPU.

  uwu_attention_causal_fwd  fp64 softmax with -inf masking (on the bf16-rounded operands for bf16), the tolerances
                            tests/test_kernels_gpu.py applies to uwu_attention_fwd
  uwu_text_embed / _pool    one-line torch references, exact
  uwu_bias_act_fwd          the fp64 activation: fp32 within 2 ulp, bf16 within one rounding of the fp32 result
  the whole model           tests/clip_oracle.py in fp64 with the same weights: fp32 mode to 1e-3, bf16 mode to twice the error of
                            the oracle itself run in bfloat16 on the CPU
  ConcatTextEncoders        the reference's assembly rule (text_encoders.py:139-264) applied to the oracle's outputs
"""
import os

import pytest
import torch

from tests import clip_oracle
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BF16_NAN, F32_NAN = 0x7FC1, 0x7FC00001  # sentinel bit patterns for memory no kernel may touch
D_HEAD = 64


def _fill_sentinel(t):
    (t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)).fill_(BF16_NAN if t.dtype == BF else F32_NAN)


def _is_sentinel(t):
    return bool(((t.view(torch.int16) == BF16_NAN) if t.dtype == BF else (t.view(torch.int32) == F32_NAN)).all())


def _tol(dtype):  # tests/test_kernels_gpu.py tol()
    return dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)


# ---------------------------------------------------------------------------------------------- causal attention
def _ref_attn(q, k, v, mask):
    """q / k / v [B, T, H, 64] (already rounded to the kernel's dtype) -> fp64 [B*T, H*64]"""
    B, T, H, d = q.shape
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    s = s.masked_fill(~clip_oracle.visible(mask, B, T)[:, None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * T, H * d)


def _run_attn(q, k, v, mask, packed, guard=8):
    """q / k / v [B, T, H, 64] on the CPU in the kernel's dtype -> (o [B*T, H*64] on the CPU, the output buffer's guard rows).  The
    output goes into the middle of a buffer of sentinels."""
    from uwudiff_amd import lib as L

    B, T, H, d = q.shape
    HD = H * d
    if packed:
        qkv = torch.cat([t.reshape(B * T, HD) for t in (q, k, v)], dim=1).cuda()
        qd, kd, vd = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    else:
        qd, kd, vd = (t.reshape(B * T, HD).cuda() for t in (q, k, v))
    buf = torch.empty(B * T + 2 * guard, HD, dtype=q.dtype, device="cuda")
    _fill_sentinel(buf)
    o = buf[guard:guard + B * T]
    md = None if mask is None else mask.cuda()
    L.call("uwu_attention_causal_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None if md is None else md.data_ptr(),
           o.data_ptr(), B, T, H, d, qd.stride(0), kd.stride(0), vd.stride(0), HD, d ** -0.5, L.dt(qd), L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(buf[:guard]) and _is_sentinel(buf[guard + B * T:]), "guard rows overwritten"
    return o.cpu()


def _masks(B, T):
    """None, right-padded lengths {1, 5, 16, 17, T} (those that fit, spread over the batch), one mask per call"""
    out = [None]
    for n in sorted({min(n, T) for n in (1, 5, 16, 17, T)}):
        m = torch.zeros(B, T, dtype=torch.long)
        m[:, :n] = 1
        if B > 1:
            m[1, :] = 0
            m[1, :max(1, n // 2)] = 1  # a second length in the same launch
        out.append(m)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 5)])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 64, 65, 77, 128])
def test_attention_causal_matches_fp64(T, B, H, dtype):
    g = torch.Generator().manual_seed(100 * T + 10 * B + H)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    q = q * 1.5  # scores with a spread of a few units: a softmax that is neither flat nor one-hot
    worst = 0.0
    for mask in _masks(B, T):
        ref = _ref_attn(q, k, v, mask)
        for packed in (True, False):
            o = _run_attn(q, k, v, mask, packed)
            assert o.dtype == dtype and bool(torch.isfinite(o).all())
            worst = max(worst, float((o.double() - ref).abs().max()))
            torch.testing.assert_close(o.double(), ref, **_tol(dtype))
    print(f"[attention_causal] T={T} B={B} H={H} {dtype}: max |got - ref| over masks and layouts = {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_causal_reads_the_mask_per_key(dtype):
    """ones at 0, 2, 3, 9 only: a kernel that took the mask for a length would see keys 1, 4 .. 8 (or none past 0)"""
    B, T, H = 2, 17, 3
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    mask = torch.zeros(B, T, dtype=torch.long)
    mask[:, [0, 2, 3, 9]] = 1
    ref = _ref_attn(q, k, v, mask)
    as_length = torch.zeros_like(mask)
    as_length[:, :4] = 1
    assert float((ref - _ref_attn(q, k, v, as_length)).abs().max()) > 0.1
    for packed in (True, False):
        torch.testing.assert_close(_run_attn(q, k, v, mask, packed).double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_causal_hidden_keys_never_contribute(dtype):
    """T = 77, H = 3.  NaNs are planted where no visible key lives, the reference is computed on the clean tensors:
      batch 0, no key mask, query row 20 (its horizon, 21 keys, is the interior of key tile 1): K and V rows 21 .. 76 are NaN -- the
        rest of its own tile, where keys 21 .. 31 are visible to OTHER queries of the tile, and every skipped tile; output rows
        0 .. 20 are compared (a product that multiplied those V rows by a probability of exactly 0 would give NaN);
      batch 1, key mask of length 37 (again a tile interior): K and V rows 37 .. 76 are NaN; all 77 output rows are compared;
      32 rows of NaN follow the last sequence in the K and V buffers: the kernel pads T to its tile without reading them."""
    B, T, H, row, n1 = 2, 77, 3, 20, 37
    g = torch.Generator().manual_seed(20)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, n1:] = 0
    ref = _ref_attn(q, k, v, mask)
    kp, vp = k.clone(), v.clone()
    kp[0, row + 1:] = float("nan")
    vp[0, row + 1:] = float("nan")
    kp[1, n1:] = float("nan")
    vp[1, n1:] = float("nan")
    pad = torch.full((1, 32, H, D_HEAD), float("nan"), dtype=dtype)
    from uwudiff_amd import lib as L

    qd = q.reshape(B * T, -1).cuda()
    kd, vd = (torch.cat([t.reshape(1, B * T, H, D_HEAD), pad], dim=1).reshape(B * T + 32, -1).cuda() for t in (kp, vp))
    o = torch.empty(B * T, H * D_HEAD, dtype=dtype, device="cuda")
    _fill_sentinel(o)
    md = mask.cuda()
    L.call("uwu_attention_causal_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), md.data_ptr(), o.data_ptr(), B, T, H, D_HEAD,
           H * D_HEAD, H * D_HEAD, H * D_HEAD, H * D_HEAD, D_HEAD ** -0.5, L.dt(qd), L.stream())
    got = o.cpu().double()
    keep = torch.cat([torch.arange(row + 1), torch.arange(T, 2 * T)])
    assert bool(torch.isfinite(got[keep]).all())
    torch.testing.assert_close(got[keep], ref[keep], **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_causal_fully_masked_sequence_gives_zeros(dtype):
    """the precondition (key 0 visible) broken for sequence 1 of 2, whose key mask is all zeros and whose K and V rows are NaN: its
    rows are exactly zero, not NaN; sequence 0 is unaffected"""
    B, T, H = 2, 17, 2
    g = torch.Generator().manual_seed(31)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1] = 0
    ref = _ref_attn(q, k, v, mask)[:T]
    k[1] = float("nan")
    v[1] = float("nan")
    for packed in (True, False):
        got = _run_attn(q, k, v, mask, packed)
        assert not bool(got[T:].any())  # (NaN != 0 counts as set)
        torch.testing.assert_close(got[:T].double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_causal_first_key_tile_hidden(dtype):
    """T = 77 (two 64-row query blocks), sequence 0 hides keys 0 .. 39 -- the whole first 32-key tile of the fp32 path and part of the
    next, so its running maximum is still -inf when the first visible key arrives -- and sequence 1 sees every key.  Rows 0 .. 39
    of sequence 0 see nothing and are exactly zero; every other row matches fp64.  Scores as in test_attention_causal_matches_fp64:
    a spread of a few units, no exponent near underflow whatever the maximum is carried as."""
    B, T, H, n0 = 2, 77, 2, 40
    g = torch.Generator().manual_seed(32)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    q = q * 1.5
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, :n0] = 0
    ref = _ref_attn(q, k, v, mask)
    assert bool(torch.isnan(ref[:n0]).all()) and bool(torch.isfinite(ref[n0:]).all())  # the rows the reference has nothing for
    for packed in (True, False):
        got = _run_attn(q, k, v, mask, packed)
        assert not bool(got[:n0].any())
        torch.testing.assert_close(got[n0:].double(), ref[n0:], **_tol(dtype))


def test_attention_causal_refusals():
    """null pointers, d = 72, T = 0, T = 129, a misaligned base, ld not a multiple of 8: a UwuError that names the entry point, and
    nothing is launched (the output keeps its sentinel)"""
    from uwudiff_amd import lib as L

    H, T = 2, 16
    a = torch.zeros(256 * 3 * H * D_HEAD + 64, dtype=BF, device="cuda")
    m = torch.ones(256, dtype=torch.long, device="cuda")
    out = torch.empty(256 * H * D_HEAD, dtype=BF, device="cuda")
    _fill_sentinel(out)
    p, o = a.data_ptr(), out.data_ptr()
    hd = H * D_HEAD

    def call(q=p, k=p + 2 * hd, v=p + 4 * hd, mask=m.data_ptr(), y=o, B=1, T=T, H=H, d=D_HEAD, ld=(3 * hd, 3 * hd, 3 * hd, hd),
             scale=0.125, dtype=L.BF16):
        L.call("uwu_attention_causal_fwd", q, k, v, mask, y, B, T, H, d, *ld, scale, dtype, L.stream())

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(y=None), dict(d=72), dict(T=0), dict(T=129), dict(q=p + 8), dict(y=o + 2),
               dict(mask=m.data_ptr() + 4), dict(ld=(3 * hd + 4, 3 * hd, 3 * hd, hd)), dict(ld=(3 * hd, 3 * hd, 3 * hd, hd + 4)),
               dict(ld=(3 * hd, 3 * hd, hd - 8, hd)), dict(B=0), dict(H=0), dict(scale=0.0), dict(dtype=3)):
        with pytest.raises(L.UwuError, match="attention_causal_fwd"):
            call(**kw)
    torch.cuda.synchronize()
    assert _is_sentinel(out)
    call()  # the same buffers with nothing wrong: runs (zeros in, zeros out)
    call(mask=None)
    torch.cuda.synchronize()
    assert bool((out[:T * hd] == 0).all()) and _is_sentinel(out[T * hd:])


# ---------------------------------------------------------------------------------------------- embed, bias + activation, pool
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_text_embed_is_exact_and_clamps(dtype):
    from uwudiff_amd import ops

    B, T, D, V = 3, 77, 136, 1000
    g = torch.Generator().manual_seed(1)
    tok = (torch.randn(V, D, generator=g)).to(dtype)
    pos = (torch.randn(T + 3, D, generator=g) * 0.25).to(dtype)
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[0, 0], ids[0, 1], ids[1, 5], ids[2, 76] = V - 1, 0, V + 17, -4  # the last row; the first; out of range on both sides
    out = ops.text_embed(ids.cuda(), tok.cuda(), pos.cuda())
    ref = (tok[ids.clamp(0, V - 1)].float() + pos[:T].float()[None]).to(dtype).reshape(B * T, D)  # one rounding of the exact sum
    assert out.dtype == dtype and torch.equal(out.cpu(), ref)


def _ulp(ref, bits):
    """the spacing of a format with `bits` significand bits at |ref| (fp64 tensor)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - bits)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_bias_act_matches_fp64(kind, with_bias, dtype):
    """fp32: |got - ref| <= 2 ulp of fp32 at ref.  bf16: one rounding of the fp32 result -- half a bf16 ulp -- plus 2^-19 |ref| for
    the fp32 arithmetic before it (a few fp32 ulp times the left tail's condition number |x f'(x) / f(x)| <= 1.702 * 9 here).
    ld = 272 > N = 264: the 8 columns past N keep their sentinel; out of place and in place."""
    from uwudiff_amd import ops

    M, N, ld = 37, 264, 272
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, ld, generator=g) * 3.0
    x[0, :8] = torch.tensor([-9.0, -7.5, -5.0, -3.0, 0.0, 1e-3, 6.0, 9.0])
    x = x.to(dtype)
    bias = (torch.randn(N, generator=g) * 0.5) if with_bias else None
    z = x[:, :N].double() + (bias.double() if with_bias else 0.0)
    ref = z * torch.sigmoid(1.702 * z) if kind == "quick_gelu" else 0.5 * z * torch.erfc(-z * 0.5 ** 0.5)
    bound = 2.0 * _ulp(ref, 24) if dtype == torch.float32 else 0.5 * _ulp(ref, 8) + 2.0 ** -19 * ref.abs()
    xd = x.cuda()
    bd = bias.cuda() if with_bias else None
    y = torch.empty_like(xd)
    _fill_sentinel(y)
    ops.bias_act_fwd(xd, kind, bias=bd, out=y, N=N)
    inplace = xd.clone()
    ops.bias_act_fwd(inplace, kind, bias=bd, out=inplace, N=N)
    for what, got in (("out of place", y), ("in place", inplace)):
        err = (got[:, :N].cpu().double() - ref).abs()
        print(f"[bias_act {kind} {dtype} {what}] worst |got - ref| / bound = {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), (what, int((err > bound).sum()))
    assert _is_sentinel(y[:, N:]) and torch.equal(inplace[:, N:], xd[:, N:])


def test_bias_act_refusals():
    from uwudiff_amd import lib as L

    x = torch.zeros(64 * 64, dtype=BF, device="cuda")
    y = torch.empty_like(x)
    _fill_sentinel(y)
    b = torch.zeros(64, device="cuda")
    for args in ((None, b.data_ptr(), y.data_ptr(), 8, 64, 64, 0, L.BF16), (x.data_ptr(), None, None, 8, 64, 64, 0, L.BF16),
                 (x.data_ptr(), None, y.data_ptr(), 8, 60, 64, 0, L.BF16), (x.data_ptr(), None, y.data_ptr(), 8, 64, 56, 0, L.BF16),
                 (x.data_ptr(), None, y.data_ptr(), 8, 64, 64, 2, L.BF16), (x.data_ptr(), None, y.data_ptr(), 8, 64, 64, 0, 5),
                 (x.data_ptr() + 2, None, y.data_ptr(), 8, 64, 64, 0, L.BF16), (x.data_ptr(), b.data_ptr() + 4, y.data_ptr(), 8, 64, 64, 1, L.BF16),
                 (x.data_ptr(), None, y.data_ptr(), 0, 64, 64, 0, L.BF16)):
        with pytest.raises(L.UwuError, match="bias_act_fwd"):
            L.call("uwu_bias_act_fwd", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(y)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_text_pool_both_rules(dtype):
    """eos_id == 2: first position of the largest id; otherwise the first id equal to eos_id, position 0 when there is none"""
    from uwudiff_amd import ops

    B, T, D = 5, 77, 136
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(10, 900, (B, T), generator=g)
    ids[0, 4:] = 999                      # eos at 4, padded with eos: the FIRST of the largest
    ids[1, 76] = 999                      # the last position
    ids[2, 70], ids[2, 33] = 950, 950     # no 999: largest-id rule -> 33 (first 950), equality rule -> 0
    ids[3, 0] = 999                       # position 0
    ids[4, 65], ids[4, 10] = 999, 7       # beyond one 64-lane pass; the equality rule with eos_id = 7 -> 10
    h = torch.randn(B * T, D, generator=g).to(dtype)
    for eos, want in ((2, [4, 76, 33, 0, 65]), (999, [4, 76, 0, 0, 65]), (7, None)):
        pos = clip_oracle.pool_position(ids, eos)
        if want is not None:
            assert pos.tolist() == want
        else:
            assert pos[4].item() == 10
        got = ops.text_pool(ids.cuda(), h.cuda(), eos)
        assert got.dtype == dtype and torch.equal(got.cpu(), h.view(B, T, D)[torch.arange(B), pos])


def test_embed_and_pool_refusals():
    from uwudiff_amd import lib as L

    ids = torch.zeros(4, 16, dtype=torch.long, device="cuda")
    t = torch.zeros(64 * 64, dtype=BF, device="cuda")
    out = torch.empty(64 * 64, dtype=BF, device="cuda")
    _fill_sentinel(out)
    i, p, o = ids.data_ptr(), t.data_ptr(), out.data_ptr()
    for args in ((None, p, p, o, 4, 16, 64, 32, L.BF16), (i, p, None, o, 4, 16, 64, 32, L.BF16), (i, p, p, o, 4, 16, 60, 32, L.BF16),
                 (i, p, p, o, 4, 16, 64, 0, L.BF16), (i, p + 2, p, o, 4, 16, 64, 32, L.BF16), (i, p, p, o, 4, 16, 64, 32, 9)):
        with pytest.raises(L.UwuError, match="text_embed"):
            L.call("uwu_text_embed", *args, L.stream())
    for args in ((None, p, o, 4, 16, 64, 2, L.BF16), (i, p, None, 4, 16, 64, 2, L.BF16), (i, p, o, 4, 0, 64, 2, L.BF16),
                 (i, p, o, 4, 16, 12, 2, L.BF16), (i, p, o + 2, 4, 16, 64, 2, L.BF16)):
        with pytest.raises(L.UwuError, match="text_pool"):
            L.call("uwu_text_pool", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(out)


# ---------------------------------------------------------------------------------------------- the whole model
REAL_WIDTH = dict(hidden_size=1280, num_attention_heads=20, num_hidden_layers=2, intermediate_size=5120, max_position_embeddings=77,
                  vocab_size=1000, hidden_act="gelu", eos_token_id=2, layer_norm_eps=1e-5, projection_dim=1280)
CASES = {"tiny-quick_gelu": (clip_oracle.TINY_QUICK, [5, 40, 77]), "tiny-gelu": (clip_oracle.TINY_GELU, [5, 40, 77]),
         "width-1280": (REAL_WIDTH, [23, 77])}
_cache = {}


def _case(name):
    """(config, state dict with a projection, ids, mask, fp64 oracle outputs, bf16 CPU oracle outputs), computed once per module run"""
    if name not in _cache:
        cfg, lengths = CASES[name]
        sd = clip_oracle.random_state_dict(cfg, seed=len(name), projection=True)
        ids, mask = clip_oracle.tokens(cfg, lengths, seed=11)
        ref = clip_oracle.forward(sd, cfg, ids, mask)
        low = clip_oracle.forward(sd, cfg, ids, mask, dtype=BF)
        _cache[name] = (cfg, sd, ids, mask, ref, low)
    return _cache[name]


def _native(cfg, sd, compute_dtype, projection):
    from uwudiff_amd import text_model

    cls = text_model.CLIPTextModelWithProjection if projection else text_model.CLIPTextModel
    m = cls.from_config(cfg, compute_dtype=compute_dtype, init_weights=False)
    m.load_state_dict(sd if projection else {k: v for k, v in sd.items() if not k.startswith("text_projection")})
    return m.cuda()


def _errs(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


def _outputs(model, ids, mask, projection):
    """name -> tensor for everything forward returns, in the order transformers returns it"""
    out = model(ids.cuda(), attention_mask=mask.cuda(), output_hidden_states=True, return_dict=False)
    short = model(ids.cuda(), attention_mask=mask.cuda())
    assert len(out) == 3 and len(short) == 2 and torch.equal(short[0], out[0]) and torch.equal(short[1], out[1])
    first, second, hidden = out
    named = {"text_embeds": first, "last_hidden_state": second} if projection else {"last_hidden_state": first, "pooled": second}
    assert len(hidden) == model.config.num_hidden_layers + 1
    named.update({f"hidden_states[{i}]": h for i, h in enumerate(hidden)})
    return named


def _ref_of(ref, name):
    return ref["hidden_states"][int(name[14:-1])] if name.startswith("hidden_states") else ref[name]


@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_fp32_matches_fp64_oracle(name, projection):
    """every returned tensor: relative L2 and max-abs / max-abs <= 1e-3 (the project's fp32 parity bar)"""
    cfg, sd, ids, mask, ref, _ = _case(name)
    m = _native(cfg, sd, "fp32", projection)
    for what, got in _outputs(m, ids, mask, projection).items():
        want = _ref_of(ref, what)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
        l2, mx = _errs(got, want)
        print(f"[clip fp32 {name}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)


@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_bf16_within_twice_the_cpu_bf16_oracle(name, projection):
    """The bound is measured in the test (tests/test_vae_gpu.py's rule): the oracle run once in torch.bfloat16 on the CPU, its
    relative-L2 and max-abs / max-abs errors against the fp64 oracle, per returned tensor; the HIP result stays within 2x each.
    Both pipelines round every tensor to bf16 and differ in summation order and in where the norms and the softmax round."""
    cfg, sd, ids, mask, ref, low = _case(name)
    m = _native(cfg, sd, "bf16", projection)
    rows = []
    for what, got in _outputs(m, ids, mask, projection).items():
        want = _ref_of(ref, what)
        assert got.dtype == BF and tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all()), what
        hip, cpu = _errs(got, want), _errs(_ref_of(low, what), want)
        rows.append((what, hip, cpu))
        print(f"[clip bf16 {name}] {what}: rel L2 HIP {hip[0]:.3e} / CPU bf16 oracle {cpu[0]:.3e} = {hip[0] / max(cpu[0], 1e-30):.2f}; "
              f"max-abs HIP {hip[1]:.3e} / CPU {cpu[1]:.3e} = {hip[1] / max(cpu[1], 1e-30):.2f}")
    for what, hip, cpu in rows:
        assert hip[0] <= 2.0 * cpu[0] and hip[1] <= 2.0 * cpu[1], (what, hip, cpu)


# ---------------------------------------------------------------------------------------------- ConcatTextEncoders
@pytest.mark.parametrize("zero_for_padding", [True, False], ids=["zero_pad", "keep_pad"])
def test_concat_text_encoders_assembles_the_native_models(zero_for_padding):
    """two native CLIPTextModels (fp32 mode), buckets [0, 0], layer_idx [-1, -2], use_pooled [False, True]: (emb, normed, pooled,
    mask) against text_encoders.py:139-264 applied to the oracle's outputs -- emb = hidden_states[layer_idx], normed =
    final_layer_norm(emb) for a plain CLIPTextModel (:185-186), both times the attention mask when zero_for_padding, features
    concatenated, pooled from the second model, the mask of the first `need_mask` encoder"""
    from uwudiff_amd.conditioning import ConcatTextEncoders

    names, layer_idx, use_pooled = ["tiny-quick_gelu", "tiny-gelu"], [-1, -2], [False, True]
    models, toks, embs, normeds, pooleds = [], [], [], [], []
    for name, li, up in zip(names, layer_idx, use_pooled):
        cfg, sd, ids, mask, ref, _ = _case(name)
        plain = {k: v for k, v in sd.items() if not k.startswith("text_projection")}
        models.append((_native(cfg, sd, "fp32", False), dict(concat_bucket=0, layer_idx=li, use_pooled=up, need_mask=not up)))
        toks.append({"input_ids": ids, "attention_mask": mask})
        emb = ref["hidden_states"][li]
        normed = clip_oracle.final_layer_norm(plain, cfg, emb)
        w = mask[..., None].double() if zero_for_padding else 1.0
        embs.append(emb * w)
        normeds.append(normed * w)
        if up:
            pooleds.append(ref["pooled"])
    te = ConcatTextEncoders(tokenizers=["a", "b"], text_model_and_configs=models, zero_for_padding=zero_for_padding).cuda()
    assert te.device.type == "cuda"
    emb, normed, pooled, attn = te(toks)
    want_emb, want_normed, want_pooled = torch.cat(embs, -1), torch.cat(normeds, -1), torch.cat(pooleds, -1)
    assert tuple(emb.shape) == (3, 77, 256) and tuple(pooled.shape) == (3, 128) and emb.dtype == torch.float32
    assert torch.equal(attn.cpu(), toks[0]["attention_mask"])
    for what, got, want in (("emb", emb, want_emb), ("normed", normed, want_normed), ("pooled", pooled, want_pooled)):
        l2, mx = _errs(got, want)
        print(f"[concat native zero_for_padding={zero_for_padding}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)
    if zero_for_padding:
        assert not bool(emb[0, 5:].any()) and not bool(normed[0, 5:].any())
    # normed is final_layer_norm(hidden_states[layer_idx]) for BOTH models -- also for layer_idx = -2, where it is not last_hidden_state
    for (m, c), t, f0 in zip(models, toks, (0, 128)):
        _, _, hs = m(t["input_ids"].cuda(), attention_mask=t["attention_mask"].cuda(), output_hidden_states=True)
        ln = m.final_layer_norm(hs[c["layer_idx"]]).float()
        if zero_for_padding:
            ln = ln * t["attention_mask"].cuda()[..., None]
        assert torch.equal(normed[..., f0:f0 + 128], ln)


# ---------------------------------------------------------------------------------------------- trainer
def test_trainer_encodes_captions_with_the_native_text_encoders():
    """two steps of DMTrainer from configs/demo_training_clip.yaml, cut down to a small UNet and small text configurations (the
    nodes' `config=` override; the classes, hub names and subfolders are the YAML's): finite losses, and the context handed to the
    denoiser is [B, 77, sum of the two widths] with the pooled vector of the second encoder"""
    from duwu.trainer import DMTrainer
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.text_model import CLIPTextModel
    from uwudiff_amd.unet import TINY_UNET_CONFIG

    mc = load_yaml(os.path.join(ROOT, "configs", "demo_training_clip.yaml")).trainer.model_config
    small = [dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512),
             dict(hidden_size=192, num_attention_heads=3, num_hidden_layers=2, intermediate_size=768)]
    for pair, cfg in zip(mc.te.text_model_and_configs, small):
        pair[0]["config"] = cfg
    mc["unet"] = {"_target_": "duwu.modules.unet_patch.UNet2DFromScratch.from_config", "_load_config_": {"precision": "torch.float32"},
                  "config": dict(TINY_UNET_CONFIG, in_channels=4, out_channels=4, cross_attention_dim=320, sample_size=8,
                                 projection_class_embeddings_input_dim=192 + 6 * 256)}
    torch.manual_seed(1215)
    tr = DMTrainer(mc, use_warm_up=False).cuda()
    assert [type(m) for m in tr.te.text_models] == [CLIPTextModel, CLIPTextModel]
    assert [m.config.hidden_act for m in tr.te.text_models] == ["quick_gelu", "gelu"]
    assert all(m.flat.dtype == torch.float32 and m.flat.is_cuda and m.compute_dtype == "bf16" for m in tr.te.text_models)
    seen = []
    tr.unet.register_forward_pre_hook(lambda mod, args, kwargs: seen.append((tuple(kwargs["encoder_hidden_states"].shape),
                                                                             tuple(kwargs["added_cond_kwargs"]["text_embeds"].shape))),
                                      with_kwargs=True)
    opt = tr.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    captions = ["a photo of a cat", "DUMMY TEST with a few more words in it"]
    batch = (torch.randn(2, 3, 64, 64).cuda(), captions, tr.te.tokenize(captions), {"time_ids": torch.tensor([[1024, 1024, 0, 0, 1024, 1024.0]] * 2)}, {})
    for step in range(2):
        out = tr.training_step(batch, step)
        assert bool(torch.isfinite(out["loss"])), step
        out["loss"].backward()
        opt.step()
        opt.zero_grad()
    assert seen == [((2, 77, 320), (2, 192))] * 2
