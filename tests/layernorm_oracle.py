"""Plain two-pass LayerNorm (+ adaLN modulation, + residual gate) forward and backward, the reference of
tests/test_layernorm_gpu.py.  Every function evaluates the formulas of include/uwu_hip.h in the order written there, in the
dtype it is given: float64 is the reference, float32 is the yardstick of what fp32 arithmetic can reach (E32).

    x_out = x + gate*y
    h     = xhat*(1 + scale) + shift          (xhat*w + b when `affine`)
    dx    = rstd*(g - mean(g) - xhat*mean(g*xhat)) + dx_in,   g = dh*(1 + scale)   (dh*w when `affine`)
    dy    = gate*dx
    dshift = sum_T dh ; dscale = sum_T dh*xhat ; dgate = sum_T dx*y

Modulation vectors are [B, D] (one row per sample of T tokens) or [1, D] (one row for every token: mod_ld = 0).
tests/test_layernorm_ref_cpu.py checks these functions against torch.autograd in float64.
"""
import functools

import torch

F64 = torch.float64


def _rows(v, T, dtype):
    """[B, D] -> [B*T, D] (a [1, D] vector broadcasts)."""
    v = v.to(dtype)
    return v if v.shape[0] == 1 else v.repeat_interleave(T, 0)


def residual(x, T, y=None, gate=None, dtype=F64):
    return x.to(dtype) if y is None else x.to(dtype) + _rows(gate, T, dtype) * y.to(dtype)


def forward(x_out, T, *, shift=None, scale=None, eps=1e-6, affine=False, dtype=F64):
    """mean, rstd, xhat, h of the residual stream x_out [B*T, D]."""
    x_out = x_out.to(dtype)
    mean = x_out.mean(1)
    xc = x_out - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1) + eps)
    xhat = xc * rstd[:, None]
    h = xhat
    if scale is not None:
        s = _rows(scale, T, dtype)
        h = xhat * (s if affine else 1.0 + s) + _rows(shift, T, dtype)
    return dict(mean=mean, rstd=rstd, xhat=xhat, h=h)


def backward(dh, x, mean, rstd, T, *, scale=None, dx_in=None, y=None, gate=None, affine=False, dtype=F64):
    """Every output of the backward kernel from exactly the statistics it is handed, and for each column sum the absolute
    sum of its terms (A_*: the scale of its rounding error)."""
    dh, x, mean, rstd = dh.to(dtype), x.to(dtype), mean.to(dtype), rstd.to(dtype)
    M, D = x.shape
    B = M // T
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dh
    if scale is not None:
        s = _rows(scale, T, dtype)
        g = dh * (s if affine else 1.0 + s)
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if dx_in is not None:
        dx = dx + dx_in.to(dtype)
    out = dict(dx=dx)

    def colsum(t):
        return t.view(B, T, D).sum(1), t.abs().view(B, T, D).sum(1)

    out["dshift"], out["A_dshift"] = colsum(dh)
    out["dscale"], out["A_dscale"] = colsum(dh * xhat)
    if y is not None:
        out["dy"] = _rows(gate, T, dtype) * dx
        out["dgate"], out["A_dgate"] = colsum(dx * y.to(dtype))
    return out


def zero_rows(B, T):
    """One row of every sample."""
    return torch.arange(B) * T + (3 + 7 * torch.arange(B)) % T


@functools.lru_cache(maxsize=2)
def hard_inputs(B, T, D, off, dtype, seed=0):
    """The rows LayerNorm meets in a residual stream, rounded to `dtype`: unit variance, a per-row mean of +-off, two
    "massive" channels at 100x, and one all-zero row per sample (x and y both, so that x_out is zero there too).
    Returns x, y, dh, dx_in [B*T, D] and mod [B, 3, D] = 0.5 randn (gate, shift, scale).  Do not modify the results."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 104729 * T + D + 13 * off)
    M = B * T
    x = torch.randn(M, D, generator=g)
    x[:, [D // 3, D - 1]] *= 100.0
    x += off * (2.0 * (torch.arange(M) % 2) - 1.0)[:, None]
    y = torch.randn(M, D, generator=g)
    z = zero_rows(B, T)
    x[z] = 0.0
    y[z] = 0.0
    dh = torch.randn(M, D, generator=g)
    dx_in = torch.randn(M, D, generator=g)
    mod = 0.5 * torch.randn(B, 3, D, generator=g)
    return x.to(dtype), y.to(dtype), dh.to(dtype), dx_in.to(dtype), mod


def bf16_step(t, up):
    """The next bfloat16 above (up) or below a finite bfloat16 tensor."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    key = torch.where(i < 0, -(i & 0x7FFF), i) + (1 if up else -1)  # monotonic in the value; -0 and +0 share key 0
    bits = torch.where(key < 0, ((-key) | 0x8000) - 0x10000, key)
    return bits.to(torch.int16).view(torch.bfloat16)


def is_bf16_neighbour(got, ref):
    """True where the bfloat16 `got` is one of the two bfloat16 values that bracket the float64 `ref`."""
    g = got.double()
    above = (g >= ref) & (bf16_step(got, up=False).double() <= ref)
    below = (g <= ref) & (bf16_step(got, up=True).double() >= ref)
    return above | below


def ratio(got, ref, ref32, A=None, bf16_out=False):
    """(E32, worst ratio): E32 = max |fp32 evaluation - fp64|, ratio = max over the elements of
    (|got - ref| - [bf16 output] 2^-8 |ref|) / max(E32, 2^-23 A), A = max |ref| unless a per-element A is given.
    The bar of the test is ratio <= 4."""
    ref = ref.double()
    e32 = (ref32.double() - ref).abs().max().item()
    if A is None:
        A = ref.abs().max()
    den = (2.0 ** -23 * A.double()).clamp_min(max(e32, 1e-300))
    err = (got.double() - ref).abs()
    if bf16_out:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    r = (err / den).max().item()
    return e32, (r if r == r else float("inf"))
