"""GPU: the T5 v1.1 encoder (uwudiff_amd.text_model.T5EncoderModel) and its five kernels against references computed on the CPU.

  uwu_attention_relbias_fwd  fp64 softmax with -inf masking (on the bf16-rounded operands for bf16), the tolerances
                             tests/test_kernels_gpu.py applies to uwu_attention_fwd; the same reference with the bias indexed
                             backwards must miss those tolerances tenfold, or the comparison says nothing about the direction
  uwu_add_rmsnorm_fwd        fp64 on the stored sum; the sum itself exact in fp32
  uwu_gated_act_fwd          the fp64 gate: fp32 within 2 ulp, bf16 within one rounding of the fp32 result
  uwu_t5_rel_bias / uwu_token_embed   one-line torch references, exact
  the whole model            tests/t5_oracle.py in fp64 with the same weights: fp32 mode to 1e-3, bf16 mode to twice the error of the
                             oracle itself run in bfloat16 on the CPU
  ConcatTextEncoders         the reference's assembly rule (text_encoders.py:139-264) applied to the oracles' outputs
"""
import os

import pytest
import torch

from tests import clip_oracle, t5_oracle
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


# ---------------------------------------------------------------------------------------------- attention
def _ref_attn(q, k, v, bias, mask, scale=1.0, reverse=False):
    """q / k / v [B, T, H, 64] (already rounded to the kernel's dtype), bias fp32 [H, 2T - 1] -> fp64 [B*T, H*64]"""
    B, T, H, d = q.shape
    pos = torch.arange(T)
    off = pos[None, :] - pos[:, None]  # key - query
    full = bias.double()[:, (-off if reverse else off) + T - 1]  # [H, T, T]
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    return t5_oracle.attention(q, k, v, full, mask, scale).transpose(1, 2).reshape(B * T, H * d)


def _run_attn(q, k, v, bias, mask, packed, scale=1.0, guard=8):
    """q / k / v [B, T, H, 64] on the CPU in the kernel's dtype -> o [B*T, H*64] on the CPU; the output sits in the middle of a
    buffer of sentinels"""
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
    bd = bias.cuda()
    L.call("uwu_attention_relbias_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), bd.data_ptr(), None if md is None else md.data_ptr(),
           o.data_ptr(), B, T, H, d, qd.stride(0), kd.stride(0), vd.stride(0), HD, scale, L.dt(qd), L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(buf[:guard]) and _is_sentinel(buf[guard + B * T:]), "guard rows overwritten"
    return o.cpu()


def _attn_inputs(T, B, H, dtype):
    g = torch.Generator().manual_seed(100 * T + 10 * B + H)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    q = q * 0.25  # unscaled scores with a spread of a few units, like the bias (std 1): a softmax neither flat nor one-hot
    bias = torch.randn(H, 2 * T - 1, generator=g)
    masks = [None]
    right = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        right[b, :max(1, (T * (b + 2)) // (B + 2))] = 1  # a length per sequence, none of them T
    scattered = (torch.rand(B, T, generator=g) < 0.6).long()
    scattered[:, T // 2] = 1  # at least one visible key; key 0 is hidden in some sequences
    return q, k, v, bias, masks + [right, scattered]


def _miss(got, ref, dtype):
    """the largest |got - ref| in units of the tolerance atol + rtol |ref| (<= 1 passes assert_close)"""
    t = _tol(dtype)
    return float(((got - ref).abs() / (t["atol"] + t["rtol"] * ref.abs())).max())


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 5)])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 77, 93, 128, 129, 256, 511, 512])
def test_attention_relbias_matches_fp64(T, B, H, dtype):
    """NULL, right-padded and scattered masks, packed and separate operands.  Before anything runs on the device: the same fp64
    reference with the bias indexed by query - key misses the tolerance by at least 10x for every mask (T > 1), so a kernel that
    reads the bias backwards cannot pass."""
    q, k, v, bias, masks = _attn_inputs(T, B, H, dtype)
    worst = 0.0
    for mask in masks:
        ref = _ref_attn(q, k, v, bias, mask)
        if T > 1:
            blind = _miss(_ref_attn(q, k, v, bias, mask, reverse=True), ref, dtype)
            assert blind >= 10.0, f"the reversed bias is only {blind:.1f}x the tolerance away: the test would not see it"
        for packed in (True, False):
            o = _run_attn(q, k, v, bias, mask, packed)
            assert o.dtype == dtype and bool(torch.isfinite(o).all())
            worst = max(worst, float((o.double() - ref).abs().max()))
            torch.testing.assert_close(o.double(), ref, **_tol(dtype))
    print(f"[attention_relbias] T={T} B={B} H={H} {dtype}: max |got - ref| over masks and layouts = {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_relbias_applies_the_scale(dtype):
    B, T, H = 2, 77, 3
    q, k, v, bias, masks = _attn_inputs(T, B, H, dtype)
    ref = _ref_attn(q, k, v, bias, masks[1], scale=0.5)
    assert _miss(_ref_attn(q, k, v, bias, masks[1]), ref, dtype) >= 10.0
    torch.testing.assert_close(_run_attn(q, k, v, bias, masks[1], True, scale=0.5).double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_relbias_hidden_keys_never_contribute(dtype):
    """T = 150, H = 3: batch 0 right-padded to 37 keys (a tile interior), batch 1 with scattered hidden keys, among them key 0 and a
    whole 64-key chunk.  The K and V rows of every hidden key are NaN, the reference is computed on the clean tensors; 32 rows of
    NaN follow the last sequence in the K and V buffers: the kernel pads T to its tile without reading them."""
    B, T, H = 2, 150, 3
    g = torch.Generator().manual_seed(20)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    q = q * 0.25
    bias = torch.randn(H, 2 * T - 1, generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, 37:] = 0
    mask[1, (torch.rand(T, generator=g) < 0.4)] = 0
    mask[1, 0] = 0
    mask[1, 64:128] = 0
    mask[1, 140] = 1
    ref = _ref_attn(q, k, v, bias, mask)
    kp, vp = k.clone(), v.clone()
    kp[mask == 0] = float("nan")
    vp[mask == 0] = float("nan")
    pad = torch.full((1, 32, H, D_HEAD), float("nan"), dtype=dtype)
    from uwudiff_amd import lib as L

    qd = q.reshape(B * T, -1).cuda()
    kd, vd = (torch.cat([t.reshape(1, B * T, H, D_HEAD), pad], dim=1).reshape(B * T + 32, -1).cuda() for t in (kp, vp))
    o = torch.empty(B * T, H * D_HEAD, dtype=dtype, device="cuda")
    _fill_sentinel(o)
    md, bd = mask.cuda(), bias.cuda()
    L.call("uwu_attention_relbias_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), bd.data_ptr(), md.data_ptr(), o.data_ptr(), B, T, H,
           D_HEAD, H * D_HEAD, H * D_HEAD, H * D_HEAD, H * D_HEAD, 1.0, L.dt(qd), L.stream())
    got = o.cpu().double()
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got, ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_relbias_fully_masked_sequence_gives_zeros(dtype):
    """the precondition (a visible key per sequence) broken for batch 1 of 3: its rows are zeros, not NaN; the others are unaffected"""
    B, T, H = 3, 77, 2
    q, k, v, bias, _ = _attn_inputs(T, B, H, dtype)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1] = 0
    mask[2, 50:] = 0
    ref = _ref_attn(q, k, v, bias, mask)
    assert not bool(ref[T:2 * T].any())
    for packed in (True, False):
        got = _run_attn(q, k, v, bias, mask, packed)
        assert not bool(got[T:2 * T].any())
        torch.testing.assert_close(got.double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_relbias_first_key_tile_hidden(dtype):
    """T = 77 (two 64-row query blocks), sequence 0 hides keys 0 .. 39 -- the whole first 32-key tile of the fp32 path and part of the
    next, so the running maximum is still -inf when the first visible key arrives -- and sequence 1 sees every key.  Every row sees
    a key and matches fp64.  Scores as in test_attention_relbias_matches_fp64: no exponent near underflow."""
    B, T, H = 2, 77, 2
    q, k, v, bias, _ = _attn_inputs(T, B, H, dtype)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, :40] = 0
    ref = _ref_attn(q, k, v, bias, mask)
    for packed in (True, False):
        got = _run_attn(q, k, v, bias, mask, packed)
        assert bool(torch.isfinite(got).all())
        torch.testing.assert_close(got.double(), ref, **_tol(dtype))


def test_attention_relbias_refusals():
    """null pointers, d = 72, T = 0, T = 513, misaligned bases, strides too short or not a multiple of 8: a UwuError that names the
    entry point, and nothing is launched (the output keeps its sentinel)"""
    from uwudiff_amd import lib as L

    H, T = 2, 16
    a = torch.zeros(600 * 3 * H * D_HEAD + 64, dtype=BF, device="cuda")
    m = torch.ones(600, dtype=torch.long, device="cuda")
    rb = torch.zeros(H * 1023 + 8, device="cuda")
    out = torch.empty(600 * H * D_HEAD, dtype=BF, device="cuda")
    _fill_sentinel(out)
    p, o = a.data_ptr(), out.data_ptr()
    hd = H * D_HEAD

    def call(q=p, k=p + 2 * hd, v=p + 4 * hd, bias=rb.data_ptr(), mask=m.data_ptr(), y=o, B=1, T=T, H=H, d=D_HEAD,
             ld=(3 * hd, 3 * hd, 3 * hd, hd), scale=1.0, dtype=L.BF16):
        L.call("uwu_attention_relbias_fwd", q, k, v, bias, mask, y, B, T, H, d, *ld, scale, dtype, L.stream())

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(y=None), dict(bias=None), dict(d=72), dict(d=128), dict(T=0), dict(T=513),
               dict(q=p + 8), dict(y=o + 2), dict(mask=m.data_ptr() + 4), dict(bias=rb.data_ptr() + 2),
               dict(ld=(3 * hd + 4, 3 * hd, 3 * hd, hd)), dict(ld=(3 * hd, 3 * hd, 3 * hd, hd + 4)), dict(ld=(3 * hd, 3 * hd, hd - 8, hd)),
               dict(B=0), dict(H=0), dict(scale=0.0), dict(scale=float("nan")), dict(dtype=3)):
        with pytest.raises(L.UwuError, match="attention_relbias_fwd"):
            call(**kw)
    torch.cuda.synchronize()
    assert _is_sentinel(out)
    call()  # the same buffers with nothing wrong: runs (zeros in, zeros out)
    call(mask=None)
    call(T=512)
    torch.cuda.synchronize()
    assert bool((out[:512 * hd] == 0).all()) and _is_sentinel(out[512 * hd:])


# ---------------------------------------------------------------------------------------------- RMS norm, gate, gather, embedding
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("residual", [True, False], ids=["add", "plain"])
@pytest.mark.parametrize("D", [8, 128, 4096])
def test_add_rmsnorm_matches_fp64(D, residual, dtype):
    """x_out is the one rounding of the exact sum (exact in fp32: two fp32 numbers add with one rounding either way); n_out against
    fp64 on x_out as stored.  Rows of very different magnitude; M = 37 rows, more than one workgroup."""
    from uwudiff_amd import ops

    M, eps = 37, 1e-6
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g) * torch.logspace(-3, 2, M)[:, None]).to(dtype)
    y = (torch.randn(M, D, generator=g) * 0.5).to(dtype) if residual else None
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    xs = (x.float() + y.float()).to(dtype) if residual else x
    ref = xs.double() * torch.rsqrt(xs.double().pow(2).mean(-1, keepdim=True) + eps) * w.double()
    xd = x.cuda()
    keep = xd.clone()
    x_out, n = ops.add_rmsnorm_fwd(xd, w.cuda(), eps, y=None if y is None else y.cuda())
    assert torch.equal(xd, keep) and x_out.dtype == n.dtype == dtype
    assert torch.equal(x_out.cpu(), xs) and (residual or x_out.data_ptr() == xd.data_ptr())
    err = float(((n.cpu().double() - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max(-1, keepdim=True).values)).max())
    print(f"[add_rmsnorm D={D} residual={residual} {dtype}] worst relative error {err:.3e}")
    assert err <= (1e-5 if dtype == torch.float32 else 2.0 ** -8)  # fp32: the project's norm bar; bf16: one rounding (2^-9) + fp32 noise


def test_add_rmsnorm_refusals():
    from uwudiff_amd import lib as L

    x = torch.zeros(16 * 64, dtype=BF, device="cuda")
    n = torch.empty(16 * 64, dtype=BF, device="cuda")
    xo = torch.empty(16 * 64, dtype=BF, device="cuda")
    _fill_sentinel(n)
    _fill_sentinel(xo)
    w = torch.ones(64 + 8, device="cuda")
    X, N, O, W = x.data_ptr(), n.data_ptr(), xo.data_ptr(), w.data_ptr()
    for args in ((None, None, W, None, N, 16, 64, 1e-6, L.BF16), (X, None, None, None, N, 16, 64, 1e-6, L.BF16), (X, None, W, None, None, 16, 64, 1e-6, L.BF16),
                 (X, X, W, None, N, 16, 64, 1e-6, L.BF16), (X, None, W, None, N, 16, 60, 1e-6, L.BF16), (X, None, W, None, N, 0, 64, 1e-6, L.BF16),
                 (X, None, W, None, N, 16, 64, -1.0, L.BF16), (X, None, W, None, N, 16, 64, 1e-6, 7), (X + 2, None, W, None, N, 16, 64, 1e-6, L.BF16),
                 (X, None, W + 4, None, N, 16, 64, 1e-6, L.BF16), (X, None, W, None, X, 16, 64, 1e-6, L.BF16), (X, X, W, O, O, 16, 64, 1e-6, L.BF16)):
        with pytest.raises(L.UwuError, match="add_rmsnorm_fwd"):
            L.call("uwu_add_rmsnorm_fwd", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(n) and _is_sentinel(xo)


def _ulp(ref, bits):
    """the spacing of a format with `bits` significand bits at |ref| (fp64 tensor)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - bits)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_gated_act_matches_fp64(dtype):
    """out = gelu_new(u[:, :F]) * u[:, F:2F] on a grid of x up to |x| = 12 plus random rows, against fp64 in the form x sigmoid(2 z),
    z = sqrt(2 / pi)(x + 0.044715 x^3), which equals 0.5 x (1 + tanh z) and keeps its digits in the left tail (1 + tanh cancels
    there in any precision).  Bounds as test_bias_act_matches_fp64: fp32 tensors within 2 ulp of fp32 at the reference; bf16 tensors
    within one rounding of the fp32 result -- half a bf16 ulp -- plus 2^-19 |ref| for the fp32 arithmetic before it.
    ldu = 2F + 8 and ldo = F + 8: the columns past the tensors keep what they held."""
    from uwudiff_amd import lib as L

    M, F = 41, 264
    ldu, ldo = 2 * F + 8, F + 8
    g = torch.Generator().manual_seed(5)
    u = torch.randn(M, ldu, generator=g) * 3.0
    grid = torch.linspace(-12.0, 12.0, F)
    u[0, :F], u[1, :F], u[2, :F] = grid, grid, grid
    u[1, F:2 * F], u[2, F:2 * F] = 1.0, -0.75
    u[3, :8] = torch.tensor([-12.0, -9.0, -7.5, -5.0, 0.0, 1e-3, 6.0, 12.0])
    u = u.to(dtype)
    x, gate = u[:, :F].double(), u[:, F:2 * F].double()
    z2 = 2.0 * (2.0 / torch.pi) ** 0.5 * (x + 0.044715 * x ** 3)
    ref = x * torch.sigmoid(z2) * gate
    assert float((t5_oracle.gelu_new(x[4:]) * gate[4:] - ref[4:]).abs().max()) < 1e-12  # the same function
    bound = 2.0 * _ulp(ref, 24) if dtype == torch.float32 else 0.5 * _ulp(ref, 8) + 2.0 ** -19 * ref.abs()
    ud = u.cuda()
    out = torch.empty(M, ldo, dtype=dtype, device="cuda")
    _fill_sentinel(out)
    L.call("uwu_gated_act_fwd", ud.data_ptr(), out.data_ptr(), M, F, ldu, ldo, L.GATE["gated-gelu"], L.dt(ud), L.stream())
    err = (out[:, :F].cpu().double() - ref).abs()
    print(f"[gated_act {dtype}] worst |got - ref| / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), int((err > bound).sum())
    assert _is_sentinel(out[:, F:]) and torch.equal(ud.cpu(), u)


def test_gated_act_refusals():
    from uwudiff_amd import lib as L

    u = torch.zeros(8 * 128 + 64, dtype=BF, device="cuda")
    y = torch.empty(8 * 64, dtype=BF, device="cuda")
    _fill_sentinel(y)
    U, Y = u.data_ptr(), y.data_ptr()
    for args in ((None, Y, 8, 64, 128, 64, 0, L.BF16), (U, None, 8, 64, 128, 64, 0, L.BF16), (U, Y, 0, 64, 128, 64, 0, L.BF16),
                 (U, Y, 8, 60, 128, 64, 0, L.BF16), (U, Y, 8, 64, 120, 64, 0, L.BF16), (U, Y, 8, 64, 128, 56, 0, L.BF16),
                 (U, Y, 8, 64, 132, 64, 0, L.BF16), (U, Y, 8, 64, 128, 64, 1, L.BF16), (U, Y, 8, 64, 128, 64, 0, 4),
                 (U + 2, Y, 8, 64, 128, 64, 0, L.BF16), (U, U + 128, 8, 64, 128, 128, 0, L.BF16)):
        with pytest.raises(L.UwuError, match="gated_act_fwd"):
            L.call("uwu_gated_act_fwd", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(y) and not bool(u.any())


def test_rel_bias_gather_is_exact_and_clamps():
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops
    from uwudiff_amd.text_model import t5_offset_buckets

    g = torch.Generator().manual_seed(6)
    for T, H, nb in ((1, 1, 32), (77, 5, 32), (512, 64, 32), (93, 3, 16)):
        w = torch.randn(nb, H, generator=g)
        bucket = t5_offset_buckets(T, nb, 128)
        out = ops.t5_rel_bias(w.cuda(), bucket.cuda())
        assert out.dtype == torch.float32 and torch.equal(out.cpu(), w[bucket.long()].t())
        # the same table as the oracle's [H, T, T] bias, read at key - query + T - 1
        pos = torch.arange(T)
        assert torch.equal(out.cpu()[:, pos[None, :] - pos[:, None] + T - 1], t5_oracle.position_bias(w, T, nb, 128))
    wild = torch.tensor([-3, 0, 40, 31, 7], dtype=torch.int32)
    w = torch.randn(32, 4, generator=g)
    assert torch.equal(ops.t5_rel_bias(w.cuda(), wild.cuda()).cpu(), w[wild.long().clamp(0, 31)].t())
    out = torch.empty(64, device="cuda")
    _fill_sentinel(out)
    W, Bk, O = w.cuda(), wild.cuda(), out.data_ptr()
    for args in ((None, Bk.data_ptr(), O, 32, 4, 5), (W.data_ptr(), None, O, 32, 4, 5), (W.data_ptr(), Bk.data_ptr(), None, 32, 4, 5),
                 (W.data_ptr(), Bk.data_ptr(), O, 0, 4, 5), (W.data_ptr(), Bk.data_ptr(), O, 32, 0, 5), (W.data_ptr(), Bk.data_ptr(), O, 32, 4, 4),
                 (W.data_ptr(), Bk.data_ptr(), O, 32, 4, 1025), (W.data_ptr(), Bk.data_ptr() + 2, O, 32, 4, 5)):
        with pytest.raises(L.UwuError, match="t5_rel_bias"):
            L.call("uwu_t5_rel_bias", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(out)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_token_embed_is_exact_and_clamps(dtype):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    B, T, D, V = 3, 93, 136, 1000
    g = torch.Generator().manual_seed(1)
    tok = torch.randn(V, D, generator=g).to(dtype)
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[0, 0], ids[0, 1], ids[1, 5], ids[2, 92] = V - 1, 0, V + 17, -4  # the last row; the first; out of range on both sides
    out = ops.token_embed(ids.cuda(), tok.cuda())
    assert out.dtype == dtype and torch.equal(out.cpu(), tok[ids.clamp(0, V - 1)].reshape(B * T, D))
    o = torch.empty(B * T * D, dtype=dtype, device="cuda")
    _fill_sentinel(o)
    i, p = ids.cuda(), tok.cuda()
    for args in ((None, p.data_ptr(), o.data_ptr(), B, T, D, V, L.dt(p)), (i.data_ptr(), None, o.data_ptr(), B, T, D, V, L.dt(p)),
                 (i.data_ptr(), p.data_ptr(), None, B, T, D, V, L.dt(p)), (i.data_ptr(), p.data_ptr(), o.data_ptr(), B, T, 132, V, L.dt(p)),
                 (i.data_ptr(), p.data_ptr(), o.data_ptr(), B, T, D, 0, L.dt(p)), (i.data_ptr(), p.data_ptr(), o.data_ptr(), 0, T, D, V, L.dt(p)),
                 (i.data_ptr(), p.data_ptr() + 4, o.data_ptr(), B, T, D, V, L.dt(p)), (i.data_ptr(), p.data_ptr(), o.data_ptr(), B, T, D, V, 9)):
        with pytest.raises(L.UwuError, match="token_embed"):
            L.call("uwu_token_embed", *args, L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(o)


# ---------------------------------------------------------------------------------------------- the whole model
def _cfg(**kw):
    return dict(t5_oracle.TINY, **kw)


# name -> (config, sequence lengths (right-padded rows), T, also run in bf16)
CASES = {
    "tiny": (_cfg(), [77, 40, 5], 77, True),
    "heads-wider-than-model": (_cfg(d_model=192, num_heads=2, num_layers=2), [77, 40, 5], 77, True),  # H * 64 = 128 != d_model
    "width-1024": (_cfg(d_model=1024, num_heads=16, d_ff=2816, num_layers=2), [77, 23], 77, True),
    "xxl-block": (_cfg(d_model=4096, num_heads=64, d_ff=10240, num_layers=1, vocab_size=512), [24, 9], 24, False),  # N = 12288, 20480; K = 10240
    "tiny-T256": (_cfg(), [256, 100, 9], 256, True),
}
_cache = {}


def _case(name):
    """(config, state dict, ids, mask, fp64 oracle outputs, bf16 CPU oracle outputs or None), computed once per module run"""
    if name not in _cache:
        cfg, lengths, T, low = CASES[name]
        sd = t5_oracle.random_state_dict(cfg, seed=len(name))
        ids, mask = t5_oracle.tokens(cfg, lengths, seed=11, T=T)
        ref = t5_oracle.forward(sd, cfg, ids, mask)
        _cache[name] = (cfg, sd, ids, mask, ref, t5_oracle.forward(sd, cfg, ids, mask, dtype=BF) if low else None)
    return _cache[name]


def _native(cfg, sd, compute_dtype):
    from uwudiff_amd.text_model import T5EncoderModel

    m = T5EncoderModel.from_config(cfg, compute_dtype=compute_dtype, init_weights=False, device="cuda")
    m.load_state_dict(sd)
    return m


def _errs(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


def _outputs(model, ids, mask):
    out = model(ids.cuda(), attention_mask=mask.cuda(), output_hidden_states=True, return_dict=False)
    short = model(ids.cuda(), attention_mask=mask.cuda())
    assert len(out) == 2 and len(short) == 1 and torch.equal(short[0], out[0])
    last, hidden = out
    assert len(hidden) == model.config.num_layers + 1 and torch.equal(hidden[-1], last)
    named = {"last_hidden_state": last}
    named.update({f"hidden_states[{i}]": h for i, h in enumerate(hidden)})
    return named


def _ref_of(ref, name):
    return ref["hidden_states"][int(name[14:-1])] if name.startswith("hidden_states") else ref[name]


def test_oracle_sees_the_direction_of_the_bias():
    """from the oracle alone: with random_state_dict's bias table (std 1) the reversed bias moves the tiny case's last hidden state
    by 0.5 relative L2 -- 500x the fp32 bar and 5x the bf16 bound the model test measures (twice the CPU bf16 oracle's error), so
    neither whole-model comparison can pass a model that indexes the bias backwards"""
    cfg, sd, ids, mask, ref, low = _case("tiny")
    rev = t5_oracle.forward(sd, cfg, ids, mask, reverse_bias=True)
    moved = _errs(rev["last_hidden_state"], ref["last_hidden_state"])[0]
    bar = 2.0 * _errs(low["last_hidden_state"], ref["last_hidden_state"])[0]
    print(f"[t5 oracle] reversed bias: rel L2 {moved:.3f}; bf16 bound {bar:.3e}")
    assert moved >= 5.0 * bar and moved >= 100.0 * 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_model_fp32_matches_fp64_oracle(name):
    """every returned tensor: relative L2 and max-abs / max-abs <= 1e-3 (the project's fp32 parity bar)"""
    cfg, sd, ids, mask, ref, _ = _case(name)
    m = _native(cfg, sd, "fp32")
    for what, got in _outputs(m, ids, mask).items():
        want = _ref_of(ref, what)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
        l2, mx = _errs(got, want)
        print(f"[t5 fp32 {name}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[3]])
def test_model_bf16_within_twice_the_cpu_bf16_oracle(name):
    """The bound is measured in the test (tests/test_text_model_gpu.py's rule): the oracle run once in torch.bfloat16 on the CPU, its
    relative-L2 and max-abs / max-abs errors against the fp64 oracle, per returned tensor; the HIP result stays within 2x each."""
    cfg, sd, ids, mask, ref, low = _case(name)
    m = _native(cfg, sd, "bf16")
    rows = []
    for what, got in _outputs(m, ids, mask).items():
        want = _ref_of(ref, what)
        assert got.dtype == BF and tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all()), what
        hip, cpu = _errs(got, want), _errs(_ref_of(low, what), want)
        rows.append((what, hip, cpu))
        print(f"[t5 bf16 {name}] {what}: rel L2 HIP {hip[0]:.3e} / CPU bf16 oracle {cpu[0]:.3e} = {hip[0] / max(cpu[0], 1e-30):.2f}; "
              f"max-abs HIP {hip[1]:.3e} / CPU {cpu[1]:.3e} = {hip[1] / max(cpu[1], 1e-30):.2f}")
    for what, hip, cpu in rows:
        assert hip[0] <= 2.0 * cpu[0] and hip[1] <= 2.0 * cpu[1], (what, hip, cpu)


def test_bias_cache_is_dropped_when_weights_change():
    """the gathered bias is kept per T and rebuilt after a load: a second state dict gives the second model's output"""
    cfg, sd, ids, mask, ref, _ = _case("tiny")
    m = _native(cfg, sd, "fp32")
    first = m(ids.cuda(), attention_mask=mask.cuda())[0]
    assert list(m._bias) == [77] and m(ids.cuda(), attention_mask=mask.cuda())[0].equal(first)
    held = m._bias[77]
    m(ids.cuda(), attention_mask=mask.cuda())
    assert m._bias[77] is held  # steady state: nothing is gathered again
    other = dict(sd)
    key = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    other[key] = sd[key].flip(0)
    m.load_state_dict(other)
    assert not m._bias
    l2, _ = _errs(m(ids.cuda(), attention_mask=mask.cuda())[0], t5_oracle.forward(other, cfg, ids, mask)["last_hidden_state"])
    assert l2 <= 1e-3 and _errs(first, t5_oracle.forward(other, cfg, ids, mask)["last_hidden_state"])[0] > 1e-2


# ---------------------------------------------------------------------------------------------- ConcatTextEncoders
def _native_clip(cfg, sd):
    from uwudiff_amd.text_model import CLIPTextModel

    m = CLIPTextModel.from_config(cfg, compute_dtype="fp32", init_weights=False)
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize("zero_for_padding", [True, False], ids=["zero_pad", "keep_pad"])
def test_concat_text_encoders_assembles_clip_and_t5(zero_for_padding):
    """native CLIP-L-like, bigG-like (plain CLIPTextModels) and T5 models in fp32 mode, buckets [0, 0, 1], layer_idx [-1, -2, -1],
    pooled from the second, the mask from T5: (emb, normed, pooled, mask) against text_encoders.py:139-264 applied to the oracles'
    outputs -- bucket 0 is the two CLIP widths side by side, bucket 1 the T5 states zero-padded on the feature axis and appended
    on the sequence axis; the mask is ones for the CLIP bucket followed by T5's attention mask"""
    from uwudiff_amd.conditioning import ConcatTextEncoders

    models, toks, embs, normeds = [], [], [], []
    for ccfg, li, up, seed in ((clip_oracle.TINY_QUICK, -1, False, 15), (clip_oracle.TINY_GELU, -2, True, 9)):
        sd = clip_oracle.random_state_dict(ccfg, seed=seed)
        ids, mask = clip_oracle.tokens(ccfg, [5, 40, 77], seed=11)
        ref = clip_oracle.forward(sd, ccfg, ids, mask)
        models.append((_native_clip(ccfg, sd), dict(concat_bucket=0, layer_idx=li, use_pooled=up, need_mask=False)))
        toks.append({"input_ids": ids, "attention_mask": mask})
        w = mask[..., None].double() if zero_for_padding else 1.0
        embs.append(ref["hidden_states"][li] * w)
        normeds.append(clip_oracle.final_layer_norm(sd, ccfg, ref["hidden_states"][li]) * w)
        if up:
            want_pooled = ref["pooled"]
    cfg, sd, ids, mask, ref, _ = _case("tiny")
    models.append((_native(cfg, sd, "fp32"), dict(concat_bucket=1, layer_idx=-1, use_pooled=False, need_mask=True)))
    toks.append({"input_ids": ids, "attention_mask": mask})
    w = mask[..., None].double() if zero_for_padding else 1.0
    t5 = torch.nn.functional.pad(ref["hidden_states"][-1] * w, (0, 128))
    want_emb = torch.cat([torch.cat(embs, -1), t5], dim=1)
    want_normed = torch.cat([torch.cat(normeds, -1), torch.nn.functional.pad(ref["last_hidden_state"] * w, (0, 128))], dim=1)
    te = ConcatTextEncoders(tokenizers=["a", "b", "c"], text_model_and_configs=models, zero_for_padding=zero_for_padding).cuda()
    emb, normed, pooled, attn = te(toks)
    assert tuple(emb.shape) == (3, 154, 256) and tuple(pooled.shape) == (3, 128) and emb.dtype == torch.float32
    assert torch.equal(attn.cpu(), torch.cat([torch.ones(3, 77, dtype=torch.long), mask], dim=1))
    for what, got, want in (("emb", emb, want_emb), ("normed", normed, want_normed), ("pooled", pooled, want_pooled)):
        l2, mx = _errs(got, want)
        print(f"[concat clip + t5 zero_for_padding={zero_for_padding}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)
    assert not bool(emb[:, 77:, 128:].any())  # the narrower bucket's padding on the feature axis
    if zero_for_padding:
        assert not bool(emb[2, 77 + 5:].any()) and not bool(normed[1, 77 + 40:].any())


# ---------------------------------------------------------------------------------------------- trainer
def test_trainer_encodes_captions_with_clip_and_t5():
    """two steps of DMTrainer from configs/demo_training_sd3te.yaml, cut down to a small UNet and small text configurations (the
    nodes' `config=` override; the classes, hub names and subfolders are the YAML's): finite losses, and the denoiser is handed a
    context [B, 77 + T5 tokens, widest bucket] and the mask [B, 77 + T5 tokens]: ones, then T5's attention mask"""
    from duwu.trainer import DMTrainer
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.text_model import CLIPTextModel, T5EncoderModel
    from uwudiff_amd.unet import TINY_UNET_CONFIG

    mc = load_yaml(os.path.join(ROOT, "configs", "demo_training_sd3te.yaml")).trainer.model_config
    small = [dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512),
             dict(hidden_size=192, num_attention_heads=3, num_hidden_layers=2, intermediate_size=768),
             dict(d_model=384, num_heads=2, d_ff=512, num_layers=2)]
    for pair, cfg in zip(mc.te.text_model_and_configs, small):
        pair[0]["config"] = cfg
    mc.te["max_length"] = 96  # the T5 stand-in tokenizer's 512 capped, as the reference's max_length does
    mc["unet"] = {"_target_": "duwu.modules.unet_patch.UNet2DFromScratch.from_config", "_load_config_": {"precision": "torch.float32"},
                  "config": dict(TINY_UNET_CONFIG, in_channels=4, out_channels=4, cross_attention_dim=384, sample_size=8,
                                 projection_class_embeddings_input_dim=192 + 6 * 256)}
    torch.manual_seed(1215)
    tr = DMTrainer(mc, use_warm_up=False).cuda()
    assert [type(m) for m in tr.te.text_models] == [CLIPTextModel, CLIPTextModel, T5EncoderModel]
    assert all(m.flat.dtype == torch.float32 and m.flat.is_cuda and m.compute_dtype == "bf16" for m in tr.te.text_models)
    assert [t.model_max_length for t in tr.te.tokenizers] == [77, 77, 96]
    seen = []
    tr.unet.register_forward_pre_hook(lambda mod, args, kwargs: seen.append((tuple(kwargs["encoder_hidden_states"].shape),
                                                                             kwargs["encoder_attention_mask"].cpu().clone(),
                                                                             tuple(kwargs["added_cond_kwargs"]["text_embeds"].shape))),
                                      with_kwargs=True)
    opt = tr.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    captions = ["a photo of a cat", "DUMMY TEST with a few more words in it"]
    tokens = tr.te.tokenize(captions)
    assert int(tokens[2]["input_ids"].max()) < 32100 and tokens[2]["attention_mask"].sum(1).tolist() == [6, 10]
    batch = (torch.randn(2, 3, 64, 64).cuda(), captions, tokens, {"time_ids": torch.tensor([[1024, 1024, 0, 0, 1024, 1024.0]] * 2)}, {})
    for step in range(2):
        out = tr.training_step(batch, step)
        assert bool(torch.isfinite(out["loss"])), step
        out["loss"].backward()
        opt.step()
        opt.zero_grad()
    want_mask = torch.cat([torch.ones(2, 77, dtype=torch.long), tokens[2]["attention_mask"]], dim=1)
    assert len(seen) == 2
    for ctx_shape, mask, pooled_shape in seen:
        assert ctx_shape == (2, 77 + 96, 384) and pooled_shape == (2, 192) and torch.equal(mask.long(), want_mask)
