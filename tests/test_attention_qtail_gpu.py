"""The MFMA attention kernels at query counts that are no multiple of 64 (the QTAIL instantiations of attention_mfma.hip, DESIGN.md
4.35): bf16, T > 256, forward and the two-kernel backward, self- and cross-attention, with and without a key bias.

Four checks per shape: (1) o, lse, dq, dk, dv against an fp64 softmax attention written here, within the bounds
tests/test_attention_headdims_gpu.py applies to whole-tile shapes (restated below); (2) bit-equality with the whole-tile kernels on the
same problem with the queries padded by zero rows to the next multiple of 64 (no tolerance: a padded row adds exact zeros in the same
tile order); (3) poison: every tensor the kernels read by query row carries 64 rows of NaN behind its last batch and every output 64
sentinel rows -- results finite, sentinels untouched, and batch 1 (whose row 0 is "row T" of batch 0) equal to a B = 1 run of batch 1
alone; (4) two runs give the same bits.

Head widths 72 and 128 ship no QTAIL kernel (their guarded dK / dV kernels need scratch memory): ragged query counts
stay on the generic kernels at 72 (checks 1, 3, 4 apply to those) and stay refused at 128, which has no generic kernel."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B, H = 2, 3
TAIL = 64  # poisoned rows (or floats) behind every tensor
WIDTHS = [40, 64, 72, 80, 128]
# one real row in the last tile; a whole 32-row wave over half a 64-row tile; 63 rows; a tail that opens a new 128-query workgroup with
# three idle waves; 385 = 6 whole tiles + 1 (an odd tile count); 449: two key blocks of 256 in the dK / dV kernel, the second ragged
SELF_T = [257, 288, 319, 321, 385, 449]
CROSS = (300, 77)


# ---------------------------------------------------------------------------------------------- inputs and the fp64 reference
@functools.lru_cache(maxsize=None)
def _values(d, Tq, Tk, biased):
    """bf16-rounded q, k, v, dO as [B * T, H * d] CPU tensors (self-attention: Tq == Tk), the key bias fp32 [B, Tk] or None"""
    g = torch.Generator().manual_seed(1000 * d + Tq)
    D = H * d
    q, k, v, do = (torch.randn(B * T, D, generator=g).to(BF) for T in (Tq, Tk, Tk, Tq))
    bias = None
    if biased:  # the encoder_attention_mask form, different per sample; key 0 stays visible
        keep = (torch.rand(B, Tk, generator=g) > 0.4).float()
        keep[:, 0] = 1
        assert not torch.equal(keep[0], keep[1])
        bias = (1 - keep) * -10000.0
    return q, k, v, do, bias


@functools.lru_cache(maxsize=None)
def _ref64(d, Tq, Tk, biased):
    """fp64 softmax(scale q k^T + bias) v and its gradients of the rounded inputs: o, dq [B * Tq, D], lse [B, H, Tq], dk, dv [B * Tk, D]"""
    q, k, v, do, bias = _values(d, Tq, Tk, biased)
    scale = d ** -0.5

    def heads(t, T):
        return t.double().reshape(B, T, H, d).transpose(1, 2)  # [B, H, T, d]

    q, k, v, do = heads(q, Tq), heads(k, Tk), heads(v, Tk), heads(do, Tq)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhqk,bhkd->bhqd", p, v)
    ds = p * (torch.einsum("bhqd,bhkd->bhqk", do, v) - (do * o).sum(-1, keepdim=True))
    dq = torch.einsum("bhqk,bhkd->bhqd", ds, k) * scale
    dk = torch.einsum("bhqk,bhqd->bhkd", ds, q) * scale
    dv = torch.einsum("bhqk,bhqd->bhkd", p, do)

    def flat(t, T):
        return t.transpose(1, 2).reshape(B * T, H * d)

    return flat(o, Tq), lse, flat(dq, Tq), flat(dk, Tk), flat(dv, Tk)


def _poisoned(body):
    """`body` on the device with TAIL rows (1-D: floats) of NaN behind it: (the whole buffer, the view of the body)"""
    full = torch.full((body.shape[0] + TAIL, *body.shape[1:]), float("nan"), dtype=body.dtype, device="cuda")
    full[:body.shape[0]] = body
    return full, full[:body.shape[0]]


def _device_inputs(d, Tq, Tk, biased, packed):
    q, k, v, do, bias = _values(d, Tq, Tk, biased)
    D = H * d
    if packed:
        assert Tq == Tk
        _, qkv = _poisoned(torch.cat([q, k, v], dim=1))
        qd, kd, vd = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        qd, kd, vd = (_poisoned(t)[1] for t in (q, k, v))
    return qd, kd, vd, _poisoned(do)[1], None if bias is None else bias.cuda()


# ---------------------------------------------------------------------------------------------- the kernels, on buffers of the test's own
def _run(qd, kd, vd, dod, bias, nb, Tq, Tk, d, packed):
    """uwu_attention_fwd / _bwd (or their key-bias forms) on views whose storage goes on for TAIL poisoned rows; o, lse, delta and the
    gradients are allocated here with TAIL rows / floats of NaN behind them.  Returns the bodies and the tails."""
    from uwudiff_amd import lib as L

    D = H * d
    scale = d ** -0.5

    def nan(*shape, dtype=BF):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    o_full, lse_full, delta_full = nan(nb * Tq + TAIL, D), nan(nb * H * Tq + TAIL, dtype=torch.float32), nan(nb * H * Tq + TAIL, dtype=torch.float32)
    if packed:
        g_full = nan(nb * Tq + TAIL, 3 * D)
        dq, dk, dv = g_full[:nb * Tq, :D], g_full[:nb * Tq, D:2 * D], g_full[:nb * Tq, 2 * D:]
        tails = [g_full[nb * Tq:]]
    else:
        fulls = [nan(nb * T + TAIL, D) for T in (Tq, Tk, Tk)]
        dq, dk, dv = (f[:nb * T] for f, T in zip(fulls, (Tq, Tk, Tk)))
        tails = [f[nb * T:] for f, T in zip(fulls, (Tq, Tk, Tk))]
    assert (dq.stride(0), dk.stride(0), dv.stride(0)) == (qd.stride(0), kd.stride(0), vd.stride(0)) and dod.stride(0) == D
    dims = (nb, Tq, Tk, H, d, qd.stride(0), kd.stride(0), vd.stride(0), D, scale, L.BF16, L.stream())
    kb = () if bias is None else (bias.data_ptr(),)
    L.call("uwu_attention_fwd" if bias is None else "uwu_attention_bias_fwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), *kb,
           o_full.data_ptr(), lse_full.data_ptr(), *dims)
    L.call("uwu_attention_bwd" if bias is None else "uwu_attention_bias_bwd", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), *kb,
           o_full.data_ptr(), dod.data_ptr(), lse_full.data_ptr(), delta_full.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), *dims)
    torch.cuda.synchronize()
    out = dict(o=o_full[:nb * Tq], lse=lse_full[:nb * H * Tq].view(nb, H, Tq), dq=dq, dk=dk, dv=dv)
    tails += [o_full[nb * Tq:], lse_full[nb * H * Tq:], delta_full[nb * H * Tq:]]
    return out, tails


def _padded_run(d, Tq, Tk, biased):
    """the same problem on the WHOLE-TILE kernels: zero rows appended to q and dO up to the next multiple of 64, keys and values as
    separate tensors of the true length"""
    q, k, v, do, bias = _values(d, Tq, Tk, biased)
    Tp = (Tq + 63) // 64 * 64
    D = H * d

    def pad(t):
        out = torch.zeros(B, Tp, D, dtype=BF)
        out[:, :Tq] = t.view(B, Tq, D)
        return out.view(B * Tp, D)

    qd, kd, vd, dod = (_poisoned(t)[1] for t in (pad(q), k, v, pad(do)))
    out, _ = _run(qd, kd, vd, dod, None if bias is None else bias.cuda(), B, Tp, Tk, d, packed=False)
    return dict(o=out["o"].view(B, Tp, D)[:, :Tq].reshape(B * Tq, D), lse=out["lse"][:, :, :Tq],
                dq=out["dq"].view(B, Tp, D)[:, :Tq].reshape(B * Tq, D), dk=out["dk"], dv=out["dv"])


def _close(a, b, **kw):
    torch.testing.assert_close(a.detach().double().cpu(), b.double(), **kw)


def _check(d, Tq, Tk, biased, packed):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    D = H * d
    qd, kd, vd, dod, bias = _device_inputs(d, Tq, Tk, biased, packed)
    ld = (qd.stride(0), kd.stride(0), vd.stride(0), D)
    on_mfma = ops.attention_route(Tq, Tk, d, *ld) and ops.attention_route(Tq, Tk, d, *ld, backward=True)
    assert on_mfma is (d in (40, 64, 80))  # the widths that ship QTAIL kernels
    if d == 128:  # no QTAIL kernel and no generic kernel of this width: a ragged query count is refused, as before
        with pytest.raises(L.UwuError):
            _run(qd, kd, vd, dod, bias, B, Tq, Tk, d, packed)
        return
    out, tails = _run(qd, kd, vd, dod, bias, B, Tq, Tk, d, packed)

    # (3) poison: finite results, untouched sentinels
    for name, t in out.items():
        assert bool(torch.isfinite(t.float()).all()), name
    for t in tails:
        assert bool(torch.isnan(t.float()).all())

    # (1) fp64, the bounds of tests/test_attention_headdims_gpu.py for bf16 on whole tiles
    o_r, lse_r, dq_r, dk_r, dv_r = _ref64(d, Tq, Tk, biased)
    _close(out["o"], o_r, rtol=2e-2, atol=2e-2)
    _close(out["lse"], lse_r, rtol=1e-4, atol=3e-2)
    for name, ref in (("dq", dq_r), ("dk", dk_r), ("dv", dv_r)):
        err = (out[name].double().cpu() - ref).abs().max().item()
        print(f"d={d} Tq={Tq} Tk={Tk} bias={biased} packed={packed} {name}: max err {err:.3e}, max |ref| {ref.abs().max().item():.3e}")
        if biased:  # test_attention_key_bias_sd15_head_dims
            assert err < 1.5e-2 * ref.abs().max().item() + 1e-3, (name, err)
        else:       # test_attention_fwd_bwd_sd15_head_dims
            _close(out[name], ref, rtol=3e-2, atol=3e-2)

    # (4) two runs, the same bits
    again, _ = _run(qd, kd, vd, dod, bias, B, Tq, Tk, d, packed)
    for name in out:
        assert torch.equal(out[name], again[name]), name

    # (3) batch 1 alone: its row 0 is row Tq of batch 0
    one, _ = _run(qd[Tq:], kd[Tk:], vd[Tk:], dod[Tq:], None if bias is None else bias[1:].contiguous(), 1, Tq, Tk, d, packed)
    for name in ("o", "dq"):
        assert torch.equal(out[name][Tq:], one[name]), name
    assert torch.equal(out["lse"][1:], one["lse"])
    for name in ("dk", "dv"):
        assert torch.equal(out[name][Tk:], one[name]), name

    # (2) the whole-tile kernels on the zero-padded problem: bit for bit
    if on_mfma:
        pad = _padded_run(d, Tq, Tk, biased)
        for name in ("o", "lse", "dq", "dk", "dv"):
            assert torch.equal(out[name], pad[name]), (name, float((out[name].float() - pad[name].float()).abs().max()))


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "separate"])
@pytest.mark.parametrize("T", SELF_T)
@pytest.mark.parametrize("d", WIDTHS)
def test_self_attention_ragged_query_count(d, T, packed):
    _check(d, T, T, False, packed)


@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "keybias"])
@pytest.mark.parametrize("d", WIDTHS)
def test_cross_attention_ragged_query_count(d, biased):
    _check(d, CROSS[0], CROSS[1], biased, False)
