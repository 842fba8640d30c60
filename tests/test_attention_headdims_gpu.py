"""Attention at the Stable Diffusion 1.x head widths: 40, 80 and 160 (8 heads at 320 / 640 / 1280 channels).

bf16 with whole 64-row query tiles runs on the MFMA kernels at 40 and 80; everything else -- fp32, query counts that are no
multiple of 64, and width 160 in both dtypes -- runs on the generic kernels.  Checks and bars are those
of test_kernels_gpu.py::test_attention_fwd_bwd and, for the key bias, of test_unet_ops_gpu.py::test_attention_sdxl_level1_bf16.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def tol(dtype):
    return dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)


def cmp(a, b, **kw):
    torch.testing.assert_close(a.detach().float().cpu(), b.detach().float().cpu(), **kw)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64)


def dev(t, dtype):
    """The kernel's input on the device; returns (device tensor, the same rounded values in fp64 on the CPU)."""
    d = t.to(dtype)
    return d.cuda(), d.double()


def _attention_ref64(q, k, v, do, bias, scale, chunk=512):
    """fp64 softmax(scale q k^T + bias) v and its gradients, [H, T, d] per head, over blocks of queries."""
    H, Tq, d = q.shape
    o, lse, dq = torch.empty_like(q), torch.empty(H, Tq, dtype=q.dtype), torch.empty_like(q)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for i in range(0, Tq, chunk):
        qc, doc = q[:, i:i + chunk], do[:, i:i + chunk]
        s = torch.einsum("hqd,hkd->hqk", qc, k) * scale
        if bias is not None:
            s = s + bias
        lc = torch.logsumexp(s, -1)
        p = torch.exp(s - lc[..., None])
        oc = torch.einsum("hqk,hkd->hqd", p, v)
        ds = p * (torch.einsum("hqd,hkd->hqk", doc, v) - (doc * oc).sum(-1, keepdim=True))
        o[:, i:i + chunk], lse[:, i:i + chunk] = oc, lc
        dq[:, i:i + chunk] = torch.einsum("hqk,hkd->hqd", ds, k) * scale
        dk += torch.einsum("hqk,hqd->hkd", ds, qc) * scale
        dv += torch.einsum("hqk,hqd->hkd", p, doc)
    return o, lse, dq, dk, dv


def _inputs(B, Tq, Tk, H, d, packed, dtype):
    torch.manual_seed(0)
    D = H * d
    if packed:
        qkv = torch.randn(B * Tq, 3 * D).to(dtype)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        qkv_d = qkv.cuda()
        qd, kd, vd = qkv_d[:, :D], qkv_d[:, D:2 * D], qkv_d[:, 2 * D:]
        dqkv = torch.empty_like(qkv_d)
        grads = dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
    else:
        q, k, v = (torch.randn(B * Tq, D).to(dtype), torch.randn(B * Tk, D).to(dtype), torch.randn(B * Tk, D).to(dtype))
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        grads = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    do = torch.randn(B * Tq, D).to(dtype)
    return (q, k, v, do), (qd, kd, vd, do.cuda()), grads


CASES = [
    # d = 40: one 64-wide LDS block, a half-filled third contraction step
    (2, 64, 64, 2, 40, True), (1, 128, 77, 8, 40, False), (1, 320, 320, 2, 40, False),
    (2, 100, 40, 3, 40, False),  # generic route (Tq no multiple of 64)
    (1, 16, 16, 8, 40, True),    # generic route: the mid block at 256 x 256 images
    # d = 80: a second LDS block holding 16 columns
    (2, 256, 256, 2, 80, True), (1, 64, 77, 8, 80, False),
    (1, 192, 300, 1, 80, False),  # two key blocks of the dK / dV kernel (boundary at 256)
    # d = 160: generic kernels in both dtypes
    (2, 64, 64, 1, 160, True), (1, 128, 77, 2, 160, False), (1, 16, 16, 8, 160, True),
]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,Tq,Tk,H,d,packed", CASES)
def test_attention_fwd_bwd_sd15_head_dims(B, Tq, Tk, H, d, packed, dtype):
    from uwudiff_amd import ops

    D = H * d
    (q, k, v, do), (qd, kd, vd, dod), (dq, dk, dv) = _inputs(B, Tq, Tk, H, d, packed, dtype)

    def heads(t, T):
        return t.float().reshape(B, T, H, d).transpose(1, 2)

    qr, kr, vr = [heads(t, T).detach().requires_grad_(True) for t, T in ((q, Tq), (k, Tk), (v, Tk))]
    orf = F.scaled_dot_product_attention(qr, kr, vr)
    orf.backward(heads(do, Tq))
    lse_ref = torch.logsumexp(qr.detach() @ kr.detach().transpose(-1, -2) / math.sqrt(d), dim=-1)

    o, lse = ops.attention_fwd(qd, kd, vd, B, Tq, Tk, H, d)
    cmp(o, orf.transpose(1, 2).reshape(B * Tq, D), **tol(dtype))
    cmp(lse, lse_ref, rtol=1e-4, atol=1e-4 if dtype == torch.float32 else 3e-2)
    ops.attention_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, B, Tq, Tk, H, d)
    t = tol(dtype) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    cmp(dq, qr.grad.transpose(1, 2).reshape(B * Tq, D), **t)
    cmp(dk, kr.grad.transpose(1, 2).reshape(B * Tk, D), **t)
    cmp(dv, vr.grad.transpose(1, 2).reshape(B * Tk, D), **t)


@pytest.mark.parametrize("d", [40, 80])
def test_attention_key_bias_sd15_head_dims(d):
    """Cross-attention to 77 text tokens under an encoder_attention_mask that differs between the two samples (bf16, MFMA
    kernels) against fp64; key 0 stays visible."""
    from uwudiff_amd import ops

    B, H, Tq, Tk = 2, 8, 256, 77
    D = H * d
    (qd, q64), (kd, k64), (vd, v64), (dod, do64) = (dev(_randn(B * T, D, seed=s), BF)
                                                    for s, T in ((1, Tq), (2, Tk), (3, Tk), (4, Tq)))
    keep = (torch.rand(B, Tk, generator=_gen(5)) > 0.4).double()
    keep[:, 0] = 1
    assert not torch.equal(keep[0], keep[1])
    bias = (1 - keep) * -10000.0
    kb = bias.float().cuda()
    o, lse = ops.attention_fwd(qd, kd, vd, B, Tq, Tk, H, d, key_bias=kb)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops.attention_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, B, Tq, Tk, H, d, key_bias=kb)
    torch.cuda.synchronize()

    def heads(t, T, b):
        return t.reshape(B, T, H, d)[b].transpose(0, 1)

    def flat(t, T):
        return t.transpose(0, 1).reshape(T, D)

    for b in range(B):
        o_r, lse_r, dq_r, dk_r, dv_r = _attention_ref64(heads(q64, Tq, b), heads(k64, Tk, b), heads(v64, Tk, b),
                                                        heads(do64, Tq, b), bias[b], d ** -0.5)
        rows = lambda t, T: t.cpu().double().reshape(B, T, D)[b]
        torch.testing.assert_close(rows(o, Tq), flat(o_r, Tq), rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(lse.cpu().double()[b], lse_r, rtol=1e-4, atol=3e-2)
        for name, got, ref, T in (("dq", dq, dq_r, Tq), ("dk", dk, dk_r, Tk), ("dv", dv, dv_r, Tk)):
            ref = flat(ref, T)
            err = (rows(got, T) - ref).abs().max().item()
            print(f"d={d} sample {b} {name}: max err {err:.3e}, max |ref| {ref.abs().max().item():.3e}")
            assert err < 1.5e-2 * ref.abs().max().item() + 1e-3, (name, b, err, ref.abs().max().item())


@pytest.mark.parametrize("B,Tq,Tk,H,d,packed", [(1, 64, 77, 2, 64, False), (1, 320, 320, 2, 72, False)])
def test_attention_old_head_dims_stay_deterministic(B, Tq, Tk, H, d, packed):
    """The dispatch of the widths that existed before still lands on deterministic kernels: two runs, the same bits."""
    from uwudiff_amd import ops

    _, (qd, kd, vd, dod), _ = _inputs(B, Tq, Tk, H, d, packed, BF)
    runs = []
    for _ in range(2):
        o, lse = ops.attention_fwd(qd, kd, vd, B, Tq, Tk, H, d)
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        ops.attention_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, B, Tq, Tk, H, d)
        runs.append((o, dq, dk, dv))
    for name, a, b in zip(("o", "dq", "dk", "dv"), *runs):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name
