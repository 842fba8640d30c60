"""Plain references of the kernels at the edges of the denoiser step, for tests/test_edge_kernels_gpu.py: the fp32 Linears with a
handful of rows (csrc/skinny.hip), the sinusoidal timestep features, patchify / unpatchify, the positional add and the bf16
transpose (csrc/embed.hip), and the axial RoPE rotation, its factor table and its three gradients (csrc/rope.hip).

Every function evaluates the formulas of include/uwu_hip.h in the dtype it is given, on exactly the (already rounded) inputs
the device gets: float64 is the reference, float32 is the yardstick of what fp32 arithmetic can reach (E32).  Sums come with the
absolute sum of their terms (A: the scale of their rounding error).  Nothing here touches a device.
tests/test_edge_ref_cpu.py checks these functions against torch.autograd, F.unfold, torch.t and the reference's own RoPE output.

    Linear      y = x w^T + b ;  dx = dy w ;  dw = dy^T x ;  db = sum_m dy
    features    [cos(t f_j) | sin(t f_j)],  f_j = exp(-ln(max_period) j / half)
    patchify    tok[(b, th, tw), (c, ph, pw)] = img[b, c, th p + ph, tw p + pw]
    RoPE        theta[r, h, i] = pos[r, 0] exp(fh[h, i])  (i < d/4),  pos[r, 1] exp(fw[h, i - d/4])  (i >= d/4)
                y[2i] = x[2i] (cos - sin),  y[2i+1] = x[2i+1] (cos + sin)          (rotate_half negates the EVEN element)
                dx = dy * the same factors ;  dtheta = -ga a (sin + cos) + gb b (cos - sin) ;  d log-freq = sum_r dtheta theta
"""
import math

import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


# ------------------------------------------------------------------------------------------------------------------ Linear
def linear(x, w, b=None, dtype=F64):
    """y [M, N] = x [M, K] w [N, K]^T (+ b) and A = |x| |w|^T (+ |b|)."""
    x, w = x.to(dtype), w.to(dtype)
    y, A = x @ w.T, x.abs() @ w.abs().T
    if b is not None:
        y, A = y + b.to(dtype), A + b.to(dtype).abs()
    return y, A


def linear_dgrad(dy, w, dtype=F64):
    """dx [M, K] = dy [M, N] w [N, K] and A = |dy| |w|."""
    dy, w = dy.to(dtype), w.to(dtype)
    return dy @ w, dy.abs() @ w.abs()


def linear_wgrad(dy, x, dtype=F64):
    """dw [N, K] = dy^T x, db [N] = the column sums of dy, and the absolute sums of their terms."""
    dy, x = dy.to(dtype), x.to(dtype)
    return dict(dw=dy.T @ x, A_dw=dy.abs().T @ x.abs(), db=dy.sum(0), A_db=dy.abs().sum(0))


def silu(y):
    y = y.double()
    return y / (1.0 + torch.exp(-y))


def linear_inputs(M, N, K, seed=0):
    """x [M, K], w [N, K] / sqrt(K), b [N] spread over [-20, 20] (both tails of the SiLU epilogue), dy [M, N]; fp32.
    Do not modify the results."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 104729 * N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.linspace(-20.0, 20.0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([-20.0])
    dy = torch.randn(M, N, generator=g)
    return x, w, b, dy


# ------------------------------------------------------------------------------------------------------- timestep features
def timestep_features(t, dim, max_period=10000.0, dtype=F64):
    """[B, dim] = [cos(t f_j) | sin(t f_j)], f_j = exp(-ln(max_period) j / half), evaluated in `dtype`."""
    half = dim // 2
    j = torch.arange(half, dtype=dtype)
    if dtype == F64:
        s = math.log(max_period) * j / half
    else:  # the chain in fp32: ln rounded, the product rounded, the quotient rounded
        s = torch.tensor(math.log(max_period), dtype=dtype) * j / torch.tensor(float(half), dtype=dtype)
    a = t.to(dtype)[:, None] * torch.exp(-s)[None, :]
    return torch.cat((torch.cos(a), torch.sin(a)), dim=1)


def timestep_budget(t, dim, max_period=10000.0):
    """First-order error budget of an fp32 evaluation, per element [B, dim]:  |a| (3 s + 3) 2^-24 + 2^-22  with a = t f_j and
    s = ln(max_period) j / half.  The exponent argument s is the result of three roundings (ln, product, quotient: 3 s 2^-25
    ... bounded by 1.5 s 2^-24), expf adds a relative 2^-24 or two and the product t f one more, so the angle is off by at most
    |a| (3 s + 3) 2^-24 with room; cos / sin move by no more than the angle does, and their own rounding and the fp64 -> fp32
    rounding of the result stay below 2^-22."""
    half = dim // 2
    s = math.log(max_period) * torch.arange(half, dtype=F64) / half
    a = (t.double()[:, None] * torch.exp(-s)[None, :]).abs()
    bud = a * (3.0 * s[None, :] + 3.0) * 2.0 ** -24 + 2.0 ** -22
    return torch.cat((bud, bud), dim=1)


# ---------------------------------------------------------------------------------------------------- patchify / transpose
def patch_index(B, C, H, W, p):
    """[B gh gw, C p p] int64: the flat index into img [B, C, H, W] that each token feature is taken from."""
    gh, gw = H // p, W // p
    b, th, tw, c, ph, pw = torch.meshgrid(torch.arange(B), torch.arange(gh), torch.arange(gw), torch.arange(C), torch.arange(p),
                                          torch.arange(p), indexing="ij")
    src = ((b * C + c) * H + (th * p + ph)) * W + (tw * p + pw)
    return src.reshape(B * gh * gw, C * p * p)


def patchify(img, p):
    """img [B, C, H, W] -> tokens [B gh gw, C p p], values untouched."""
    B, C, H, W = img.shape
    return img.reshape(-1)[patch_index(B, C, H, W, p)]


def unpatchify(tok, B, C, H, W, p):
    """tokens [B gh gw, C p p] -> img [B, C, H, W], values untouched."""
    img = torch.empty(B * C * H * W, dtype=tok.dtype)
    img[patch_index(B, C, H, W, p).reshape(-1)] = tok.reshape(-1)
    return img.view(B, C, H, W)


def transpose(src):
    """dst[c][r] = src[r][c], written out as an index map."""
    rows, cols = src.shape
    r, c = torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij")
    dst = torch.empty(cols, rows, dtype=src.dtype)
    dst[c.reshape(-1), r.reshape(-1)] = src.reshape(-1)
    return dst


def add_pos(x, pos, B, T, D):
    """x [B T, D] (fp32 or bf16) + pos [T, D] (fp32), the sum in fp32, rounded once to x's dtype.  (One fp32 addition of two
    fp32 values is exact arithmetic followed by one rounding: the result is defined bit for bit.)"""
    return (x.float().view(B, T, D) + pos.float()[None]).view(B * T, D).to(x.dtype)


# -------------------------------------------------------------------------------------------------------------------- RoPE
def rope_angles(pos, fh, fw, rows, dtype=F64):
    """theta [rows, H, d/2]; pos [pos_rows, 2], row r uses pos[r % pos_rows]; fh, fw [H, d/4]."""
    p = pos.to(dtype)[torch.arange(rows) % pos.shape[0]]
    th_h = p[:, 0, None, None] * torch.exp(fh.to(dtype))[None]
    th_w = p[:, 1, None, None] * torch.exp(fw.to(dtype))[None]
    return torch.cat((th_h, th_w), dim=-1)


def rope_table(pos, fh, fw, rows, dtype=F64):
    """The factors m [rows, H d] of y = x * m: (cos - sin, cos + sin) per pair."""
    th = rope_angles(pos, fh, fw, rows, dtype)
    cs, sn = torch.cos(th), torch.sin(th)
    return torch.stack((cs - sn, cs + sn), dim=-1).reshape(rows, -1)


def rope_fwd(x, pos, fh, fw, dtype=F64):
    """x [rows, H d] -> y, the rotation of the reference (rope.py) written per pair."""
    return x.to(dtype) * rope_table(pos, fh, fw, x.shape[0], dtype)


def rope_bwd(x, dy, pos, fh, fw, dtype=F64, e_fast=None):
    """dx [rows, H d], dfh, dfw [H, d/4] and, for the two sums, the absolute sum of their terms (A_dfh, A_dfw).
    With e_fast (a function |theta| -> the absolute error of the device's cos -+ sin at that angle) also F_dfh, F_dfw: that
    error carried through dtheta * theta, sum_r (|ga a| + |gb b|) (e_fast + |theta| delta) |theta|, delta = (|f| + 4) 2^-24
    (the relative error of the device's theta itself: the rounded exponent argument, the exponential, the product)."""
    rows = x.shape[0]
    H, q4 = fh.shape
    th = rope_angles(pos, fh, fw, rows, dtype)
    cs, sn = torch.cos(th), torch.sin(th)
    xx, gg = x.to(dtype).view(rows, H, 2 * q4, 2), dy.to(dtype).view(rows, H, 2 * q4, 2)
    a, b, ga, gb = xx[..., 0], xx[..., 1], gg[..., 0], gg[..., 1]
    dx = torch.stack((ga * (cs - sn), gb * (cs + sn)), dim=-1).reshape(rows, -1)
    t1, t2 = ga * a * (-sn - cs) * th, gb * b * (cs - sn) * th
    out = dict(dx=dx)
    dfr, A = (t1 + t2).sum(0), (t1.abs() + t2.abs()).sum(0)
    out.update(dfh=dfr[:, :q4], dfw=dfr[:, q4:], A_dfh=A[:, :q4], A_dfw=A[:, q4:])
    if e_fast is not None:
        f = torch.cat((fh, fw), dim=-1).to(dtype).abs()
        delta = (f + 4.0) * 2.0 ** -24
        F = (((ga * a).abs() + (gb * b).abs()) * (e_fast(th.abs()) + th.abs() * delta[None]) * th.abs()).sum(0)
        out.update(F_dfh=F[:, :q4], F_dfw=F[:, q4:])
    return out


F_LO, F_HI = math.log(math.pi) - 1.0, math.log(10.0 * math.pi)  # log-frequencies: |theta| = |p| e^f <= 10 pi < 32 for |p| <= 1


def rope_inputs(rows, H, d, pos_rows, dtype, seed=0):
    """x, dy [rows, H d] of unit scale rounded to `dtype`; pos [pos_rows or rows, 2] in [-1, 1], distinct per row and per axis;
    fh != fw [H, d/4] in [F_LO, F_HI], distinct per head and index.  Row 0 sits at (1, -1), fh[0, 0] = F_HI and fw[H-1, -1] is just
    below it, so |theta| reaches 10 pi on one axis and nearly on the other.  Do not modify the results."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 104729 * H + 13 * d + pos_rows)
    x = torch.randn(rows, H * d, generator=g).to(dtype)
    dy = torch.randn(rows, H * d, generator=g).to(dtype)
    pos = torch.rand(pos_rows or rows, 2, generator=g) * 2.0 - 1.0
    pos[0, 0], pos[0, 1] = 1.0, -1.0
    q4 = d // 4
    fh = F_LO + (F_HI - F_LO) * torch.rand(H, q4, generator=g)
    fw = F_LO + (F_HI - F_LO) * torch.rand(H, q4, generator=g)
    fh[0, 0] = F_HI
    fw[H - 1, q4 - 1] = F_HI - 2.0 ** -6
    return x, dy, pos.float(), fh.float(), fw.float()


# -------------------------------------------------------------------------------------------------------------------- bars
def _bar_parts(got, ref, ref32, A, bf16_out, floor):
    ref = ref.double()
    e32 = (ref32.double() - ref).abs().max().item()
    A = ref.abs() if A is None else A.double()
    den = (2.0 ** -23 * A).clamp_min(max(e32, 1e-300))
    if floor is not None:
        den = torch.maximum(den, floor.double())
    err = (got.double() - ref).abs()
    if bf16_out:
        err = err - 2.0 ** -8 * ref.abs()
    return e32, err, den


def _worst(v, got):
    r = v.max().item()
    return r if r == r and bool(torch.isfinite(got.double()).all()) else float("inf")


def ratio(got, ref, ref32, A=None, bf16_out=False, extra=None, floor=None):
    """(E32, worst ratio): E32 = max |fp32 evaluation - fp64| over the tensor, ratio = max over the elements of
    (|got - ref| - [bf16 output] 2^-8 |ref| - extra) / max(E32, 2^-23 A, floor); A = |ref| per element unless given.
    The bar of the tests is ratio <= 4.  NaN never passes."""
    e32, err, den = _bar_parts(got, ref, ref32, A, bf16_out, floor)
    if extra is not None:
        err = err - extra.double()
    return e32, _worst(err.clamp_min(0.0) / den, got)


def bar_use(got, ref, ref32, extra, A=None, bf16_out=False, floor=None, margin=4.0):
    """The worst share of the whole bar  margin * max(E32, 2^-23 A, floor) + extra  that the error takes (after the bf16 term):
    what `ratio` cannot show where `extra` covers the error and it reads 0."""
    _, err, den = _bar_parts(got, ref, ref32, A, bf16_out, floor)
    return _worst(err.clamp_min(0.0) / (margin * den + extra.double()), got)
