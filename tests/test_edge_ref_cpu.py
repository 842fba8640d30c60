"""The fp64 references of tests/test_edge_kernels_gpu.py (tests/edge_oracle.py) against independent things: torch.autograd in
float64 for the Linear and RoPE gradients, F.unfold for patchify, torch.t for the transpose, the formula of
tests/test_rope_gpu.py and the reference-generated tests/golden/axial_rope.npz for the rotation; and the bounds its bars rest on."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import edge_oracle as O
from tests.golden_util import load

F64 = torch.float64
TOL = dict(rtol=1e-11, atol=1e-11)


def ref_formula(x, pos, fh, fw):
    """The rotation as tests/test_rope_gpu.py states it (rope.py: x cos + rotate_half(x) sin)."""
    th = torch.cat((pos[..., None, None, 0] * fh.exp(), pos[..., None, None, 1] * fw.exp()), dim=-1).repeat_interleave(2, -1)
    rh = torch.stack((-x[..., 0::2], x[..., 1::2]), dim=-1).flatten(-2, -1)
    return x * th.cos() + rh * th.sin()


# ------------------------------------------------------------------------------------------------------------------ Linear
@pytest.mark.parametrize("M,N,K", [(1, 1, 4), (5, 17, 36), (33, 9, 132)])
def test_linear_matches_autograd(M, N, K):
    x, w, b, dy = (t.double() for t in O.linear_inputs(M, N, K))
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.linear(xr, wr, br)
    gx, gw, gb = torch.autograd.grad((y * dy).sum(), [xr, wr, br])
    yo, A = O.linear(x, w, b)
    torch.testing.assert_close(yo, y.detach(), **TOL)
    torch.testing.assert_close(O.linear(x, w)[0], F.linear(x, w), **TOL)
    dx, A_dx = O.linear_dgrad(dy, w)
    g = O.linear_wgrad(dy, x)
    torch.testing.assert_close(dx, gx, **TOL)
    torch.testing.assert_close(g["dw"], gw, **TOL)
    torch.testing.assert_close(g["db"], gb, **TOL)
    assert (A >= yo.abs() - 1e-12).all() and (A_dx >= dx.abs() - 1e-12).all()
    assert (g["A_dw"] >= g["dw"].abs() - 1e-12).all() and (g["A_db"] >= g["db"].abs() - 1e-12).all()
    # A is the sum of the absolute terms, spelled out for one element
    assert A[M - 1, N - 1].item() == pytest.approx(((x[M - 1] * w[N - 1]).abs().sum() + b[N - 1].abs()).item(), rel=1e-12)
    torch.testing.assert_close(O.silu(yo), F.silu(yo), **TOL)


def test_linear_inputs_reach_both_silu_tails():
    x, w, b, dy = O.linear_inputs(16, 17, 68)
    assert x.dtype == w.dtype == b.dtype == dy.dtype == torch.float32
    assert b.min().item() == -20.0 and b.max().item() == 20.0 and len(set(b.tolist())) == 17
    assert 0.5 < (x @ w.T).std().item() < 2.0  # unit-scale products under the bias


@pytest.mark.parametrize("K", [4, 36, 512, 1280])
def test_fp32_chain_stays_inside_the_bar_and_a_dropped_term_does_not(K):
    """What the bar rests on: a sequential numpy fp32 chain (the worst summation order; the kernels sum 64 partial chains)
    stays below half of its first-order bound (K + 2) 2^-24 A and inside 4 * 2^-23 A, and the same chain without its last term
    is outside 4 * 2^-23 A in most outputs."""
    rng = np.random.default_rng(K)
    x, w = rng.standard_normal((64, K)).astype(np.float32), (rng.standard_normal((64, K)) / K ** 0.5).astype(np.float32)
    acc, short = np.zeros(64, np.float32), np.zeros(64, np.float32)
    for k in range(K):
        acc = (acc + x[:, k] * w[:, k]).astype(np.float32)
        if k < K - 1:
            short = acc.copy()
    xt, wt = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    ref, A = (xt * wt).sum(1), (xt * wt).abs().sum(1)
    bar = 4 * 2.0 ** -23 * A
    err = (torch.from_numpy(acc).double() - ref).abs()
    assert (err <= 0.5 * (K + 2) * 2.0 ** -24 * A).all() and (err <= bar).all()
    assert ((torch.from_numpy(short).double() - ref).abs() > bar).double().mean() >= 0.7


# ------------------------------------------------------------------------------------------------------- timestep features
T_VALUES = [0.0, 1e-3, 0.5, 1.0, 14.6146, 37.0, 250.5, 999.0, 999.999]


@pytest.mark.parametrize("dim", [2, 6, 256, 320])
def test_timestep_features(dim):
    t = torch.tensor(T_VALUES)
    ref = O.timestep_features(t, dim)
    half = dim // 2
    assert ref.shape == (len(T_VALUES), dim) and ref.dtype == F64
    # an independent statement: python floats, element by element
    for b in (1, 4, 8):
        for j in (0, half // 2, half - 1):
            a = float(t[b]) * math.exp(-math.log(10000.0) * j / half)
            assert ref[b, j].item() == pytest.approx(math.cos(a), abs=1e-12)
            assert ref[b, half + j].item() == pytest.approx(math.sin(a), abs=1e-12)
    assert torch.equal(ref[0], torch.cat((torch.ones(half), torch.zeros(half))).double())  # t = 0
    # the budget holds the torch fp32 restatement and a numpy restatement of the kernel's chain with room
    bud = O.timestep_budget(t, dim)
    ref32 = O.timestep_features(t, dim, dtype=torch.float32)
    assert ref32.dtype == torch.float32
    assert ((ref32.double() - ref).abs() <= 0.5 * bud).all()
    j = np.arange(half, dtype=np.float32)
    f = np.exp((-np.float32(math.log(10000.0)) * j / np.float32(half)).astype(np.float32)).astype(np.float32)
    a = (t.numpy()[:, None] * f[None, :]).astype(np.float32)
    chain = torch.from_numpy(np.concatenate((np.cos(a), np.sin(a)), axis=1).astype(np.float32))
    assert ((chain.double() - ref).abs() <= 0.5 * bud).all()
    # ... and not a wrong frequency: half + 1 in the denominator moves the sines of t >= 14.6 (j >= 1) outside 4 x the budget
    if dim >= 6:
        jj = torch.arange(half, dtype=F64)
        wrong = t.double()[:, None] * torch.exp(-math.log(10000.0) * jj / (half + 1))[None]
        off = (torch.cat((wrong.cos(), wrong.sin()), 1) - ref).abs() > 4 * bud
        assert off[4:, half + 1:].double().mean() >= 0.99


# -------------------------------------------------------------------------------------------------------------- index maps
@pytest.mark.parametrize("B,C,H,W,p", [(1, 1, 1, 1, 1), (2, 4, 8, 12, 2), (1, 3, 12, 8, 4), (2, 3, 6, 9, 3)])
def test_patchify_matches_unfold(B, C, H, W, p):
    img = torch.arange(B * C * H * W, dtype=torch.float32).view(B, C, H, W)  # every element distinct
    tok = O.patchify(img, p)
    want = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(B * (H // p) * (W // p), C * p * p)
    assert torch.equal(tok, want)
    assert torch.equal(O.unpatchify(tok, B, C, H, W, p), img)
    assert torch.equal(F.fold(want.view(B, -1, C * p * p).transpose(1, 2), (H, W), kernel_size=p, stride=p), img)
    idx = O.patch_index(B, C, H, W, p).reshape(-1)
    assert torch.equal(idx.sort().values, torch.arange(B * C * H * W))  # a permutation


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (65, 97)])
def test_transpose_matches_torch_t(rows, cols):
    src = torch.randn(rows, cols).bfloat16()
    assert torch.equal(O.transpose(src), src.t().contiguous())


def test_add_pos_rounds_once():
    B, T, D = 3, 5, 8
    g = torch.Generator().manual_seed(0)
    x, pos = torch.randn(B * T, D, generator=g), torch.randn(T, D, generator=g)
    assert torch.equal(O.add_pos(x, pos, B, T, D), x + pos.repeat(B, 1))
    xb = x.bfloat16()
    got = O.add_pos(xb, pos, B, T, D)
    exact = xb.double() + pos.repeat(B, 1).double()
    assert got.dtype == torch.bfloat16 and torch.equal(got, exact.float().bfloat16())
    assert ((got.double() - exact).abs() <= 2.0 ** -8 * exact.abs() + 1e-30).all()


# -------------------------------------------------------------------------------------------------------------------- RoPE
def test_rope_matches_the_reference_golden():
    _, d = load("axial_rope")
    x, pos, y = d["x"], d["pos"], d["y"]  # [B, T, H, dim], [B, T, 2]
    Bq, T, H, dim = x.shape
    got = O.rope_fwd(x.reshape(Bq * T, H * dim), pos.reshape(Bq * T, 2), d["freqs_h"], d["freqs_w"])
    torch.testing.assert_close(got.view(Bq, T, H, dim), y.double(), rtol=1e-5, atol=2e-6)  # the golden is an fp32 evaluation
    got32 = O.rope_fwd(x.reshape(Bq * T, H * dim), pos.reshape(Bq * T, 2), d["freqs_h"], d["freqs_w"], dtype=torch.float32)
    assert got32.dtype == torch.float32
    torch.testing.assert_close(got32.view(Bq, T, H, dim), y, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("rows,H,d,pos_rows", [(7, 1, 4, 0), (12, 3, 8, 0), (12, 3, 72, 4), (6, 2, 64, 2)])
def test_rope_matches_formula_and_autograd(rows, H, d, pos_rows):
    x, dy, pos, fh, fw = (t.double() for t in O.rope_inputs(rows, H, d, pos_rows, torch.float32))
    assert (fh != fw).all() and len(set(torch.cat((fh, fw)).reshape(-1).tolist())) == 2 * H * (d // 4)
    assert len(set(pos.reshape(-1).tolist())) == pos.numel() and pos.abs().max() <= 1.0
    full_pos = pos[torch.arange(rows) % pos.shape[0]]
    xr, fhr, fwr = x.clone().requires_grad_(True), fh.clone().requires_grad_(True), fw.clone().requires_grad_(True)
    y = ref_formula(xr.view(rows, H, d), full_pos, fhr, fwr).reshape(rows, H * d)
    gx, gfh, gfw = torch.autograd.grad((y * dy).sum(), [xr, fhr, fwr])
    torch.testing.assert_close(O.rope_fwd(x, pos, fh, fw), y.detach(), **TOL)
    torch.testing.assert_close(O.rope_table(pos, fh, fw, rows), ref_formula(torch.ones(rows, H, d, dtype=F64), full_pos, fh,
                                                                            fw).reshape(rows, H * d), **TOL)
    b = O.rope_bwd(x, dy, pos, fh, fw, e_fast=lambda a: torch.full_like(a, 1e-6))
    torch.testing.assert_close(b["dx"], gx, **TOL)
    torch.testing.assert_close(b["dfh"], gfh, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(b["dfw"], gfw, rtol=1e-10, atol=1e-9)
    assert (b["A_dfh"] >= b["dfh"].abs() - 1e-9).all() and (b["A_dfw"] >= b["dfw"].abs() - 1e-9).all()
    assert (b["F_dfh"] > 0).all() and (b["F_dfw"] > 0).all() and b["F_dfh"].shape == fh.shape
    th = O.rope_angles(pos, fh, fw, rows)
    assert th.abs().max().item() == pytest.approx(10 * math.pi, rel=1e-6) and th.abs().max() < 32.0
    b32 = O.rope_bwd(x, dy, pos, fh, fw, dtype=torch.float32)
    assert b32["dfh"].dtype == torch.float32 and (b32["dfh"].double() - b["dfh"]).abs().max() < 1e-2


def test_ratio_bar():
    ref = torch.tensor([1.0, -2.0, 4.0], dtype=F64)
    ref32 = ref + torch.tensor([1e-6, 0.0, -2e-6], dtype=F64)
    e32, r = O.ratio(ref + 4e-6, ref, ref32)
    assert e32 == pytest.approx(2e-6) and r == pytest.approx(2.0)
    # the two-ulp floor takes over when the fp32 evaluation is exact: per element, |ref| unless A is given
    e32, r = O.ratio(ref + 2.0 ** -20, ref, ref)
    assert e32 == 0.0 and r == pytest.approx(8.0)
    assert O.ratio(ref + 2.0 ** -20, ref, ref, A=torch.tensor([8.0, 8.0, 8.0]))[1] == pytest.approx(1.0)
    # a bf16 output gets 2^-8 |ref| on top, `extra` is taken off the error, `floor` widens the denominator; NaN never passes
    assert O.ratio(ref * (1 + 2.0 ** -9), ref, ref32, bf16_out=True)[1] == 0.0
    assert O.ratio(ref + 4e-6, ref, ref32, extra=torch.full((3,), 2e-6))[1] == pytest.approx(1.0)
    assert O.ratio(ref + 4e-6, ref, ref32, floor=torch.full((3,), 4e-6))[1] == pytest.approx(1.0)
    assert O.ratio(ref * float("nan"), ref, ref32)[1] == float("inf")
    assert O.ratio(ref, ref, ref32 * float("nan"))[1] == float("inf")
    # the share of the whole bar 4 * 2e-6 + extra: 4e-6 of 1e-5
    assert O.bar_use(ref + 4e-6, ref, ref32, torch.full((3,), 2e-6)) == pytest.approx(0.4)
    assert O.bar_use(ref * float("nan"), ref, ref32, torch.full((3,), 2e-6)) == float("inf")
