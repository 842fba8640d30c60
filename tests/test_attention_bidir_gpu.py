"""GPU: uwu_attention_bidir_fwd (bidirectional self-attention without a bias, d = 64, T <= 1024: the CLIP image tower's) against an fp64
softmax on the operands as the kernel sees them (bf16-rounded for bf16), with the tolerances of this kernel family
(tests/test_text_model_gpu.py ``_tol``).  The lengths are the ones at which the code takes another path: 1 (one query), 17 (a tail
inside the first MFMA tile), 50 (ViT-B/32), 64 / 65 (exactly one 64-query block and 64-key chunk, and one past it), 257 (ViT-L/14),
577 (ViT-L/14 at 336: past the T5 kernel's cap of 512) and 1024 (the cap)."""
import pytest
import torch

from tests.test_text_model_gpu import BF, D_HEAD, _fill_sentinel, _is_sentinel, _tol

pytestmark = pytest.mark.gpu


def _ref_attn(q, k, v, mask, scale):
    """q / k / v [B, T, H, 64] (already rounded to the kernel's dtype) -> fp64 [B*T, H*64]; mask int64 [B, T] or None"""
    B, T, H, d = q.shape
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * T, H * d)


def _run_attn(q, k, v, mask, packed, scale, guard=8, tail=None):
    """q / k / v [B, T, H, 64] on the CPU in the kernel's dtype -> o [B*T, H*64] on the CPU.  The output goes into the middle of a
    buffer of sentinels; `tail`: rows appended after the last sequence of K and V (memory the kernel must not read into its result)."""
    from uwudiff_amd import lib as L

    B, T, H, d = q.shape
    HD = H * d
    rows = [t.reshape(B * T, HD) for t in (q, k, v)]
    if tail is not None:
        assert not packed
        rows[1], rows[2] = (torch.cat([r, tail.reshape(-1, HD)]) for r in rows[1:])
    if packed:
        qkv = torch.cat(rows, dim=1).cuda()
        qd, kd, vd = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    else:
        qd, kd, vd = (r.cuda() for r in rows)
    buf = torch.empty(B * T + 2 * guard, HD, dtype=q.dtype, device="cuda")
    _fill_sentinel(buf)
    o = buf[guard:guard + B * T]
    md = None if mask is None else mask.cuda()
    L.call("uwu_attention_bidir_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None if md is None else md.data_ptr(), o.data_ptr(),
           B, T, H, d, qd.stride(0), kd.stride(0), vd.stride(0), HD, scale, L.dt(qd), L.stream())
    torch.cuda.synchronize()
    assert _is_sentinel(buf[:guard]) and _is_sentinel(buf[guard + B * T:]), "guard rows overwritten"
    return o.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,B,H", [(1, 2, 2), (17, 2, 2), (50, 2, 2), (64, 2, 2), (65, 2, 2), (257, 2, 2), (577, 2, 2), (1024, 1, 1)])
def test_attention_bidir_matches_fp64(T, B, H, dtype):
    """separate tensors and a packed [B*T, 3*H*64] projection read in place, no key mask (what the ViT passes)"""
    g = torch.Generator().manual_seed(1000 + T)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    q = q * 1.5  # scores with a spread of a few units: a softmax that is neither flat nor one-hot
    scale = D_HEAD ** -0.5
    ref = _ref_attn(q, k, v, None, scale)
    for packed in (False, True):
        o = _run_attn(q, k, v, None, packed, scale)
        assert o.dtype == dtype and bool(torch.isfinite(o).all())
        print(f"[attention_bidir] T={T} B={B} H={H} {dtype} packed={packed}: max |got - ref| = {float((o.double() - ref).abs().max()):.3e}")
        torch.testing.assert_close(o.double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_bidir_applies_the_scale(dtype):
    B, T, H = 2, 50, 2
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    ref = _ref_attn(q, k, v, None, 0.31)
    assert float((ref - _ref_attn(q, k, v, None, D_HEAD ** -0.5)).abs().max()) > 0.05
    torch.testing.assert_close(_run_attn(q, k, v, None, True, 0.31).double(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_bidir_hidden_keys_never_contribute(dtype):
    """T = 65, per-key mask (batch 0 hides keys 3, 40 .. 63 and 64: part of the first chunk and the whole second one; batch 1 hides key 0
    and sees the lone key of the second chunk).  NaN is planted in every hidden K / V row and in 32 rows of memory after row T of the
    last sequence; the reference is computed on the clean tensors.  The output is finite and equals the reference."""
    B, T, H = 2, 65, 2
    g = torch.Generator().manual_seed(65)
    q, k, v = (torch.randn(B, T, H, D_HEAD, generator=g).to(dtype) for _ in range(3))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[0, 3] = 0
    mask[0, 40:] = 0
    mask[1, 0] = 0
    ref = _ref_attn(q, k, v, mask, D_HEAD ** -0.5)
    kp, vp = k.clone(), v.clone()
    hidden = mask == 0
    kp[hidden] = float("nan")
    vp[hidden] = float("nan")
    tail = torch.full((32, H, D_HEAD), float("nan"), dtype=dtype)
    got = _run_attn(q, kp, vp, mask, False, D_HEAD ** -0.5, tail=tail)
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got.double(), ref, **_tol(dtype))
    # without a mask the rows after the last sequence are still never read: T is padded to the tile inside the kernel
    got = _run_attn(q, k, v, None, False, D_HEAD ** -0.5, tail=tail)
    assert bool(torch.isfinite(got).all())
    torch.testing.assert_close(got.double(), _ref_attn(q, k, v, None, D_HEAD ** -0.5), **_tol(dtype))


def test_attention_bidir_refusals():
    """d = 80 (ViT-H/14), T = 0, T = 1025, a misaligned base, a stride that is not a multiple of 8, and the rest of what
    uwu_attention_relbias_fwd refuses: a UwuError that names the entry point, and nothing is launched (the output keeps its sentinel)"""
    from uwudiff_amd import lib as L

    H, T = 2, 16
    a = torch.zeros(1100 * 3 * H * D_HEAD + 64, dtype=BF, device="cuda")
    m = torch.ones(1100, dtype=torch.long, device="cuda")
    out = torch.empty(1100 * H * D_HEAD, dtype=BF, device="cuda")
    _fill_sentinel(out)
    p, o = a.data_ptr(), out.data_ptr()
    hd = H * D_HEAD

    def call(q=p, k=p + 2 * hd, v=p + 4 * hd, mask=m.data_ptr(), y=o, B=1, T=T, H=H, d=D_HEAD, ld=(3 * hd, 3 * hd, 3 * hd, hd),
             scale=0.125, dtype=L.BF16):
        L.call("uwu_attention_bidir_fwd", q, k, v, mask, y, B, T, H, d, *ld, scale, dtype, L.stream())

    for kw in (dict(d=80), dict(T=0), dict(T=1025), dict(q=p + 8), dict(y=o + 2), dict(ld=(3 * hd + 4, 3 * hd, 3 * hd, hd)),
               dict(ld=(3 * hd, 3 * hd, 3 * hd, hd + 4)), dict(q=None), dict(k=None), dict(v=None), dict(y=None), dict(d=72), dict(d=128),
               dict(mask=m.data_ptr() + 4), dict(ld=(3 * hd, 3 * hd, hd - 8, hd)), dict(B=0), dict(H=0), dict(B=65536, H=1),
               dict(scale=0.0), dict(scale=float("nan")), dict(dtype=3)):
        with pytest.raises(L.UwuError, match="attention_bidir_fwd"):
            call(**kw)
    with pytest.raises(L.UwuError, match="ViT-H/14"):
        call(d=80)
    torch.cuda.synchronize()
    assert _is_sentinel(out)
    call()  # the same buffers with nothing wrong: runs (zeros in, zeros out)
    call(mask=None)
    call(T=1024)
    torch.cuda.synchronize()
    assert bool((out[:1024 * hd] == 0).all()) and _is_sentinel(out[1024 * hd:])
