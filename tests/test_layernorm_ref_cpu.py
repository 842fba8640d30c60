"""The fp64 LayerNorm reference of tests/test_layernorm_gpu.py (tests/layernorm_oracle.py) against torch.autograd in
float64, and the helpers its bars rest on (bfloat16 neighbours, the hard inputs)."""
import pytest
import torch
import torch.nn.functional as F

from tests import layernorm_oracle as O

F64 = torch.float64


@pytest.mark.parametrize("B,T,D,affine", [(2, 5, 16, False), (3, 7, 24, False), (1, 7, 24, True), (1, 12, 40, True)])
@pytest.mark.parametrize("with_y,with_dx_in", [(True, True), (False, True), (True, False)])
def test_reference_matches_autograd(B, T, D, affine, with_y, with_dx_in):
    torch.manual_seed(B * 100 + D)
    M = B * T
    x = (torch.randn(M, D, dtype=F64) + 16.0).requires_grad_(True)
    y = torch.randn(M, D, dtype=F64, requires_grad=True) if with_y else None
    mod = (0.5 * torch.randn(B, 3, D, dtype=F64)).requires_grad_(True)
    gate, shift, scale = mod[:, 0], mod[:, 1], mod[:, 2]
    dh = torch.randn(M, D, dtype=F64)
    dx_in = torch.randn(M, D, dtype=F64) if with_dx_in else None
    eps = 1e-6

    rep = lambda v: v.repeat_interleave(T, 0)  # noqa: E731
    xo = x + rep(gate) * y if with_y else x + 0.0
    if affine:
        h = F.layer_norm(xo, (D,), weight=scale[0], bias=shift[0], eps=eps)
    else:
        h = F.layer_norm(xo, (D,), eps=eps) * (1 + rep(scale)) + rep(shift)
    loss = (h * dh).sum() + ((xo * dx_in).sum() if with_dx_in else 0.0)
    grads = torch.autograd.grad(loss, [xo, mod] + ([y] if with_y else []))

    with torch.no_grad():
        xo_ref = O.residual(x, T, y, gate if with_y else None)
        f = O.forward(xo_ref, T, shift=shift, scale=scale, eps=eps, affine=affine)
        b = O.backward(dh, xo_ref, f["mean"], f["rstd"], T, scale=scale, dx_in=dx_in, y=y, gate=gate if with_y else None,
                       affine=affine)
    tol = dict(rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(xo_ref, xo.detach(), rtol=0, atol=0)
    torch.testing.assert_close(f["h"], h.detach(), **tol)
    torch.testing.assert_close(f["mean"], xo.detach().mean(1), **tol)
    torch.testing.assert_close(f["rstd"], 1 / torch.sqrt(xo.detach().var(1, unbiased=False) + eps), **tol)
    torch.testing.assert_close(b["dx"], grads[0], **tol)
    torch.testing.assert_close(b["dshift"], grads[1][:, 1], **tol)
    torch.testing.assert_close(b["dscale"], grads[1][:, 2], **tol)
    if with_y:
        torch.testing.assert_close(b["dy"], grads[2], **tol)
        torch.testing.assert_close(b["dgate"], grads[1][:, 0], **tol)
        assert (b["A_dgate"] >= b["dgate"].abs()).all()
    else:
        assert "dy" not in b and "dgate" not in b
    assert (b["A_dshift"] >= b["dshift"].abs()).all() and (b["A_dscale"] >= b["dscale"].abs()).all()


def test_reference_in_fp32_is_close_to_fp64():
    """The E32 yardstick: the same functions in float32 land within float32 rounding of the float64 result."""
    B, T, D = 2, 16, 64
    x, y, dh, dx_in, mod = O.hard_inputs(B, T, D, 64, torch.float32)
    gate, shift, scale = mod[:, 0], mod[:, 1], mod[:, 2]
    out = {}
    for dt in (F64, torch.float32):
        xo = O.residual(x, T, y, gate, dtype=dt)
        f = O.forward(xo, T, shift=shift, scale=scale, dtype=dt)
        assert f["h"].dtype == dt and f["mean"].dtype == dt
        out[dt] = (f, O.backward(dh, x, f["mean"].float(), f["rstd"].float(), T, scale=scale, dx_in=dx_in, y=y, gate=gate,
                                 dtype=dt))
    for k in ("h", "mean", "rstd"):
        assert (out[F64][0][k] - out[torch.float32][0][k].double()).abs().max() < 1e-3, k
    for k in ("dx", "dy", "dshift", "dscale", "dgate"):
        assert out[torch.float32][1][k].dtype == torch.float32
        assert (out[F64][1][k] - out[torch.float32][1][k].double()).abs().max() < 1e-2, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hard_inputs(dtype):
    B, T, D, off = 3, 20, 48, 64
    x, y, dh, dx_in, mod = O.hard_inputs(B, T, D, off, dtype)
    assert x.dtype == dtype and x.shape == (B * T, D) and mod.shape == (B, 3, D) and mod.dtype == torch.float32
    z = O.zero_rows(B, T)
    assert len(set((z // T).tolist())) == B  # one per sample
    assert (x[z] == 0).all() and (y[z] == 0).all()
    keep = torch.ones(B * T, dtype=torch.bool)
    keep[z] = False
    xm = x.double()[keep]
    mass = [D // 3, D - 1]
    plain = [c for c in range(D) if c not in mass]
    assert ((xm[:, plain].mean(1).abs() - off).abs() < 1.0).all()  # rows sit at +-off ...
    assert (xm[:, plain].mean(1) > 0).any() and (xm[:, plain].mean(1) < 0).any()
    assert 0.7 < xm[:, plain].std(1).mean() < 1.3  # ... with unit variance ...
    assert 50 < (xm[:, mass] - xm[:, plain].mean(1, keepdim=True)).std() < 200  # ... and two massive channels
    x32, y32, _, _, mod32 = O.hard_inputs(B, T, D, off, torch.float32)
    f = O.forward(O.residual(x32, T, y32, mod32[:, 0]), T, shift=mod32[:, 1], scale=mod32[:, 2])
    assert all(torch.isfinite(v).all() for v in f.values())
    assert torch.equal(f["h"][z], mod32[:, 1].double())  # the all-zero row: h == shift exactly


def test_bf16_neighbours():
    v = torch.tensor([1.0, -1.0, 0.0, 3.0e-3, -65.3, 1.0 + 2.0 ** -9, 256.0], dtype=F64)
    g = v.float().bfloat16()
    assert O.is_bf16_neighbour(g, v).all()
    up, dn = O.bf16_step(g, True), O.bf16_step(g, False)
    assert (up.double() > g.double()).all() and (dn.double() < g.double()).all()
    assert up[0].item() == 1.0 + 2.0 ** -7 and dn[0].item() == 1.0 - 2.0 ** -8 and dn[2].item() < 0 < up[2].item()
    # the neighbour on the other side of v is accepted, the one after it is not
    other = torch.where(g.double() > v, dn, up)
    inexact = g.double() != v
    assert O.is_bf16_neighbour(other, v)[inexact].all() and inexact.any()
    two_up, two_dn = O.bf16_step(up, True), O.bf16_step(dn, False)
    assert not O.is_bf16_neighbour(two_up, v).any() and not O.is_bf16_neighbour(two_dn, v).any()


def test_ratio_bar():
    ref = torch.tensor([1.0, -2.0, 4.0], dtype=F64)
    ref32 = (ref + torch.tensor([1e-6, 0.0, -2e-6], dtype=F64))
    e32, r = O.ratio(ref + 4e-6, ref, ref32)
    assert e32 == pytest.approx(2e-6) and r == pytest.approx(2.0)
    # the two-ulp floor takes over when the fp32 evaluation is exact; a per-element A is honoured
    e32, r = O.ratio(ref + 2.0 ** -20, ref, ref, A=torch.tensor([1.0, 2.0, 8.0], dtype=F64))
    assert e32 == 0.0 and r == pytest.approx(8.0)
    # a bf16 output gets 2^-8 |ref| on top; NaN never passes
    assert O.ratio(ref * (1 + 2.0 ** -9), ref, ref32, bf16_out=True)[1] == 0.0
    assert O.ratio(ref * float("nan"), ref, ref32)[1] == float("inf")
