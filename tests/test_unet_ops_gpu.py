"""The UNet's own HIP kernels one at a time against plain fp64 torch references on the CPU.

Each kernel is called through its uwudiff_amd/ops.py wrapper (lib.call where there is none) at shapes the UNet
dispatches and at the edges of its index arithmetic.  The references are written with torch.nn.functional, indexing
and autograd in fp64, never with the project's own code.  Bounds:

- fp32 elementwise: |got - ref| <= 1e-6 |ref| + 1e-6 max|ref| per element (the absolute term covers the GELU / SiLU
  tails, where 1 + erf(x) and x / (1 + e^-x) lose relative precision by design).
- bf16 elementwise: at most 1 bf16 ulp from the fp64 result rounded once to bf16, or the fp32 bound where larger.
- data movement and plain adds: bit-exact.  Sums: exact on integer-valued inputs.

GroupNorm statistics go through float atomics, so nothing here asserts that two launches agree bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64)


def _ints(*shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).double()


def _bf16_rne(v):
    """fp64 -> the nearest bf16 value (ties to even), rounded once (as fp64)."""
    m, e = torch.frexp(v)  # v = m 2^e, 0.5 <= |m| < 1: 8 significant bits = m * 2^8 rounded
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)


def _bf16_ulp(r):
    _, e = torch.frexp(r.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(r), e - 8)


def _report(name, ok, got, ref):
    if bool(ok.all()):
        return
    err = (got - ref).abs()
    i = int(torch.argmax(torch.where(ok, torch.zeros_like(err), err + 1)))
    raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements out of bound; e.g. flat index {i}: "
                         f"got {got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}; "
                         f"max |err| {err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}")


def _cpu64(t, shape):
    return t.detach().cpu().double().reshape(shape)


def check_ew(name, got, ref, dtype):
    """Elementwise-kernel bound against the fp64 reference `ref` (see the module docstring)."""
    got = _cpu64(got, ref.shape)
    f32 = (got - ref).abs() <= 1e-6 * ref.abs() + 1e-6 * ref.abs().max()
    if dtype == torch.float32:
        return _report(name, f32, got, ref)
    r16 = _bf16_rne(ref)
    _report(name, f32 | ((got - r16).abs() <= _bf16_ulp(r16)), got, ref)


def check_bound(name, got, ref, bound, dtype=torch.float32):
    """|got - ref| <= bound; bf16 outputs may instead sit within 1 ulp of the fp64 result rounded to bf16."""
    got = _cpu64(got, ref.shape)
    ok = (got - ref).abs() <= bound
    if dtype == BF:
        r16 = _bf16_rne(ref)
        ok = ok | ((got - r16).abs() <= _bf16_ulp(r16))
    _report(name, ok, got, ref)


def check_equal(name, got, ref):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    if not torch.equal(got, ref):
        ok = got == ref
        _report(name, ok, got.double(), ref.double())


def dev(t, dtype):
    """The kernel's input on the device; returns (device tensor, the same rounded values in fp64 on the CPU)."""
    d = t.to(dtype)
    return d.cuda(), d.double()


# ---- bf16 rounding helpers are themselves checked against torch's own fp32 -> bf16 conversion ----------------------
def test_bf16_helpers_match_torch():
    v = torch.cat([_randn(4096, seed=0) * 100, torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0])])
    v32 = v.float().double()  # exactly representable in fp32: torch rounds fp32 -> bf16 once
    assert torch.equal(_bf16_rne(v32), v32.float().bfloat16().double())
    r = v32.float().bfloat16().double()
    nxt = torch.nextafter(r.float().bfloat16(), torch.tensor(float("inf"), dtype=BF)).double()
    nz = (r > 0)
    assert torch.equal(_bf16_ulp(r)[nz], (nxt - r)[nz])


# ---- GroupNorm (+ SiLU) ---------------------------------------------------------------------------------------------
GN_EPS = 1e-5
GN_CASES = [  # B, HW, C, G, silu
    (3, 37, 40, 8, True),      # C = 40: 5 slots, RY = 51 rows per iteration, thread 255 idle; 5-channel groups
    (1, 16384, 320, 32, True),  # SDXL level 0 at 128 x 128; 10-channel groups straddle 8-channel slots
    (3, 4099, 640, 16, False),  # the last row block is partial
    (12, 37, 1280, 32, True),  # B = 12 changes gn_rows_per_block
    (3, 1, 2560, 16, True),    # two passes over the slots (NS = 2, RY = 1); one row
    (1, 4099, 4096, 8, False),  # the widest C: NS = 2, 512-channel groups, partial last row block
]


def _gn_ref(x, gamma, beta, dy, G, silu):
    """fp64 group_norm (+ silu) of x [B, HW, C]: outputs, per-(b, group) mean / rstd, gradients, and the sums of |term|
    behind dgamma / dbeta (the scale their fp32 accumulation error is measured against)."""
    B, HW, C = x.shape
    xg = x.reshape(B, HW, G, C // G)
    mean = xg.mean(dim=(1, 3))
    rstd = (xg - mean[:, None, :, None]).square().mean(dim=(1, 3)).add(GN_EPS).rsqrt()
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    z = F.group_norm(xr.transpose(1, 2), G, gr, br, eps=GN_EPS).transpose(1, 2)
    z.retain_grad()
    y = F.silu(z) if silu else z
    y.backward(dy)
    xhat = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, HW, C)
    return dict(y=y.detach(), mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad,
                dgamma_abs=(z.grad * xhat).abs().sum((0, 1)), dbeta_abs=z.grad.abs().sum((0, 1)))


def _gn_inputs(B, HW, C, offset, dtype, seed):
    """Unit-variance x with a common offset and per-channel offsets of 0.5 sigma; gamma ~ 1 +- 0.5, beta ~ 0.3."""
    x = _randn(B, HW, C, seed=seed) + offset + 0.5 * _randn(C, seed=seed + 1)
    xd, x64 = dev(x, dtype)
    dyd, dy64 = dev(_randn(B, HW, C, seed=seed + 2), dtype)
    gamma = (1.0 + 0.5 * _randn(C, seed=seed + 3)).float()
    beta = (0.3 * _randn(C, seed=seed + 4)).float()
    return xd, x64, dyd, dy64, gamma, beta


def _gn_run_and_check(B, HW, C, G, silu, dtype, offset, seed):
    from uwudiff_amd import ops

    xd, x64, dyd, dy64, gamma, beta = _gn_inputs(B, HW, C, offset, dtype, seed)
    ref = _gn_ref(x64, gamma.double(), beta.double(), dy64, G, silu)
    gd, bd = gamma.cuda(), beta.cuda()
    xd2, dyd2 = xd.reshape(B * HW, C), dyd.reshape(B * HW, C)
    y, mean, rstd = ops.groupnorm_fwd(xd2, gd, bd, B, HW, C, G, GN_EPS, silu)
    # dgamma / dbeta are views of the flat fp32 gradient buffer: the kernel adds onto what is there
    init = _randn(2, C, seed=seed + 5).float() * 10
    flat = init.cuda().reshape(-1)
    dx = ops.groupnorm_bwd(dyd2, xd2, mean, rstd, gd, bd, flat[:C], flat[C:], B, HW, C, G, silu)
    torch.cuda.synchronize()

    std = ref["rstd"].reciprocal()
    check_bound("mean", mean, ref["mean"], 1e-5 * std + 2e-6 * ref["mean"].abs())
    check_bound("rstd", rstd, ref["rstd"], 2e-5 * ref["rstd"])
    check_bound("y", y, ref["y"], 1e-4, dtype)
    check_bound("dx", dx, ref["dx"], 1e-4 * ref["dx"].abs().max().item(), dtype)
    g0 = init.double()
    check_bound("dgamma (accumulated)", flat[:C], g0[0] + ref["dgamma"], 2e-5 * ref["dgamma_abs"] + 1e-6 * g0[0].abs())
    check_bound("dbeta (accumulated)", flat[C:], g0[1] + ref["dbeta"], 2e-5 * ref["dbeta_abs"] + 1e-6 * g0[1].abs())
    return ref, (xd2, dyd2, gd, bd, mean, rstd, dx)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,HW,C,G,silu", GN_CASES)
def test_groupnorm_fwd_bwd_fp64(B, HW, C, G, silu, dtype):
    _gn_run_and_check(B, HW, C, G, silu, dtype, offset=0.0, seed=B * 7 + C)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("offset", [0.0, 16.0, 64.0])
def test_groupnorm_large_group_mean(offset, dtype):
    """A group mean far from zero against a unit spread: E[x^2] - E[x]^2 in fp32 cancels (rstd was off by 1.5e-4 at
    16 sigma and 4e-3 at 64 sigma); the statistics must be shift-invariant."""
    _gn_run_and_check(1, 4099, 640, 32, True, dtype, offset=offset, seed=11)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_groupnorm_bwd_null_parameter_gradients(dtype):
    """Frozen norms pass null dgamma / dbeta: dx must not change, and a null one must not stop the other's update."""
    from uwudiff_amd import ops

    B, HW, C, G = 2, 1031, 320, 32
    ref, (xd, dyd, gd, bd, mean, rstd, dx_full) = _gn_run_and_check(B, HW, C, G, True, dtype, offset=3.0, seed=21)
    dx_none = ops.groupnorm_bwd(dyd, xd, mean, rstd, gd, bd, None, None, B, HW, C, G, True)
    check_bound("dx (null dgamma, dbeta)", dx_none, ref["dx"], 1e-4 * ref["dx"].abs().max().item(), dtype)
    # the same sums in a different atomic order: agreement to fp32 rounding, not bit equality
    check_bound("dx (null) vs dx", dx_none, _cpu64(dx_full, ref["dx"].shape), 1e-6 * ref["dx"].abs().max().item(), dtype)
    for keep in ("dgamma", "dbeta"):
        buf = torch.full((C,), 5.0, device="cuda")
        dg, db = (buf, None) if keep == "dgamma" else (None, buf)
        ops.groupnorm_bwd(dyd, xd, mean, rstd, gd, bd, dg, db, B, HW, C, G, True)
        check_bound(f"{keep} alone", buf, 5.0 + ref[keep], 2e-5 * ref[keep + "_abs"] + 1e-6 * 5.0)


# ---- im2col / col2im 3x3 --------------------------------------------------------------------------------------------
def _im2col_ref(x, B, H, W, C, s):
    """x [B*H*W, C] -> [B*Ho*Wo, 9*C], zero padding 1, taps in (ky, kx, c) order (the conv weight layout)."""
    xp = F.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    taps = [xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, dim=3).reshape(B * Ho * Wo, 9 * C)


def _col2im_ref(dcol, B, H, W, C, s):
    x = torch.zeros(B * H * W, C, dtype=torch.float64, requires_grad=True)
    _im2col_ref(x, B, H, W, C, s).backward(dcol)
    return x.grad


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W,C", [(1, 1, 8), (1, 7, 12), (2, 2, 320), (7, 9, 12), (16, 16, 8), (7, 9, 320)])
def test_im2col_col2im_3x3(H, W, C, stride, dtype):
    from uwudiff_amd import ops

    B = 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd, x64 = dev(_randn(B * H * W, C, seed=H * 31 + W * 7 + C), dtype)
    col = ops.im2col3x3(xd, B, H, W, C, stride)
    check_equal("im2col", col, _im2col_ref(x64, B, H, W, C, stride).to(dtype))

    # col2im is the adjoint of im2col: exact on integers ...
    dci, dci64 = dev(_ints(B * Ho * Wo, 9 * C, seed=C + stride), dtype)
    check_equal("col2im (integers)", ops.col2im3x3(dci, B, H, W, C, stride),
                _col2im_ref(dci64, B, H, W, C, stride).to(dtype))
    # ... and <im2col(x), y> = <x, col2im(y)> on general data, to the rounding of col2im's output
    yd, y64 = dev(_randn(B * Ho * Wo, 9 * C, seed=C + 5), dtype)
    lhs = (_im2col_ref(x64, B, H, W, C, stride) * y64).sum().item()
    rhs = (x64 * _cpu64(ops.col2im3x3(yd, B, H, W, C, stride), x64.shape)).sum().item()
    scale = (x64.abs() * _col2im_ref(y64.abs(), B, H, W, C, stride)).sum().item()
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8
    assert abs(lhs - rhs) <= 4 * eps * scale, (lhs, rhs, scale)


# ---- GEGLU ----------------------------------------------------------------------------------------------------------
def _geglu_inputs(M, F_, dtype, seed):
    h = _randn(M, F_, seed=seed)
    gate = torch.linspace(-12, 12, M * F_, dtype=torch.float64)[torch.randperm(M * F_, generator=_gen(seed + 1))]
    hgd, hg64 = dev(torch.cat([h, gate.reshape(M, F_)], 1), dtype)
    dod, do64 = dev(_randn(M, F_, seed=seed + 2), dtype)
    return hgd, hg64, dod, do64


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,F_", [(1, 4), (4097, 4), (77, 5120), (4097, 1280), (77, 2560), (1, 2560)])
def test_geglu_fwd_bwd(M, F_, dtype):
    """out = h * gelu(gate) with exact-erf GELU (diffusers GEGLU); gate spans [-12, 12]: both tails and the exp term."""
    from uwudiff_amd import ops

    hgd, hg64, dod, do64 = _geglu_inputs(M, F_, dtype, seed=M + F_)
    h, g = hg64[:, :F_], hg64[:, F_:].clone().requires_grad_(True)
    act = F.gelu(g, approximate="none")
    check_ew("geglu out", ops.geglu_fwd(hgd), h * act, dtype)
    (dgelu,) = torch.autograd.grad(act, g, torch.ones_like(act))
    dhg = ops.geglu_bwd(hgd, dod)
    check_ew("geglu dh", dhg[:, :F_], do64 * act.detach(), dtype)
    check_ew("geglu dgate", dhg[:, F_:], do64 * h * dgelu, dtype)


# ---- nearest 2x upsample ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,C", [(5, 7, 4), (3, 5, 1280), (1, 1, 4)])
def test_upsample2x(H, W, C, dtype):
    from uwudiff_amd import ops

    B = 3
    xd, x64 = dev(_randn(B * H * W, C, seed=H + W + C), dtype)
    up_ref = x64.reshape(B, H, W, C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(-1, C)
    check_equal("upsample2x", ops.upsample2x(xd, B, H, W, C), up_ref.to(dtype))

    def down_ref(d):  # the adjoint: the sum of the four children
        return d.reshape(B, H, 2, W, 2, C).sum((2, 4)).reshape(-1, C)

    di, di64 = dev(_ints(B * 4 * H * W, C, seed=C), dtype)
    check_equal("upsample2x backward (integers)", ops.upsample2x(di, B, H, W, C, backward=True), down_ref(di64).to(dtype))
    yd, y64 = dev(_randn(B * 4 * H * W, C, seed=C + 1), dtype)
    lhs = (up_ref * y64).sum().item()
    rhs = (x64 * _cpu64(ops.upsample2x(yd, B, H, W, C, backward=True), x64.shape)).sum().item()
    scale = (x64.abs() * down_ref(y64.abs())).sum().item()
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8
    assert abs(lhs - rhs) <= 4 * eps * scale, (lhs, rhs, scale)


# ---- time-embedding add and its gradient ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("HW,C", [(37, 4), (1023, 1280)])
def test_add_rowvec(HW, C, dtype):
    from uwudiff_amd import ops

    B = 3
    x, v = _randn(B, HW, C, seed=HW).to(dtype), _randn(B, C, seed=C).to(dtype)
    out = ops.add_rowvec(x.cuda().reshape(B * HW, C), v.cuda(), B, HW, C)
    check_equal("add_rowvec", out, (x.float() + v.float()[:, None, :]).to(dtype).reshape(B * HW, C))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("HW,C,ldx", [(37, 4, 4), (37, 4, 12), (4099, 1280, 1280), (1023, 1280, 1288)])
def test_colsum_batched(HW, C, ldx, dtype):
    """dv[b, c] = sum_p d[b, p, c] (the gradient of add_rowvec), per-sample slabs of leading dimension ldx."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    B = 3
    x = torch.full((B * HW, ldx), float("nan"), dtype=torch.float64)  # columns past C must never be read
    x[:, :C] = _ints(B * HW, C, seed=HW + C)
    x = x.to(dtype)
    ref = x[:, :C].double().reshape(B, HW, C).sum(1).float()
    xd = x.cuda()
    if ldx == C:
        check_equal("colsum_batched", ops.colsum_batched(xd, B, HW, C), ref)
    out = torch.full((B, C), float("nan"), device="cuda")
    L.call("uwu_colsum_batched", L.ptr(xd), L.dt(xd), B, HW, C, ldx, L.ptr(out), 0, L.stream())
    check_equal("colsum_batched accumulate=0", out, ref)
    init = _ints(B, C, seed=3, lo=-1000, hi=1000).float()
    out = init.cuda()
    L.call("uwu_colsum_batched", L.ptr(xd), L.dt(xd), B, HW, C, ldx, L.ptr(out), 1, L.stream())
    check_equal("colsum_batched accumulate=1", out, init + ref)


# ---- NCHW fp32 <-> channels-last layout ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C,H,W,cpad", [(2, 3, 1, 1, 3), (3, 4, 5, 7, 8), (1, 4, 32, 32, 8), (2, 320, 3, 5, 320)])
def test_nchw_cl_layout(B, C, H, W, cpad, dtype):
    """nchw_to_cl / cl_to_nchw against permute + .to(dtype) (round to nearest even), and the round trip; cpad > C is
    conv_in / conv_out's zero padding of the 4 latent channels to 8."""
    from uwudiff_amd import ops

    x = _randn(B, C, H, W, seed=C * H + W).float() * 3
    # values halfway between two bf16 numbers: the conversion must round ties to even
    x.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(2 + 2.0 ** -7), 2.0 ** -100 * (1 + 2.0 ** -8)])
    xp = torch.cat([x, x.new_zeros(B, cpad - C, H, W)], 1)
    cl = ops.nchw_to_cl(xp.cuda(), dtype)
    cl_ref = xp.permute(0, 2, 3, 1).reshape(B * H * W, cpad).to(dtype)
    check_equal("nchw_to_cl", cl, cl_ref)
    back = ops.cl_to_nchw(cl, B, cpad, H * W)
    check_equal("cl_to_nchw", back, cl_ref.float().reshape(B, H * W, cpad).permute(0, 2, 1).contiguous())
    check_equal("round trip", back.view(B, cpad, H, W)[:, :C], x.to(dtype).float())
    other = _randn(B * H * W, cpad, seed=5).to(dtype)  # cl_to_nchw on its own (the UNet's output path)
    check_equal("cl_to_nchw (direct)", ops.cl_to_nchw(other.cuda(), B, cpad, H * W),
                other.float().reshape(B, H * W, cpad).permute(0, 2, 1).contiguous())


# ---- uwu_add and SiLU at extreme inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("amp", [1.0, 20.0, 90.0, 1e4])
def test_add_and_silu_extreme_inputs(amp, dtype):
    from uwudiff_amd import ops

    n = 4100
    x = amp * torch.linspace(-1, 1, n, dtype=torch.float64)[torch.randperm(n, generator=_gen(1))]
    if amp == 1.0:
        x = 4 * _randn(n, seed=2)
    xd, x64 = dev(x, dtype)
    dyd, dy64 = dev(_randn(n, seed=3), dtype)
    y = ops.silu_fwd(xd)
    dx = ops.silu_bwd(xd, dyd)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    xr = x64.clone().requires_grad_(True)
    yr = F.silu(xr)
    (dxr,) = torch.autograd.grad(yr, xr, dy64)
    check_ew("silu", y, yr.detach(), dtype)
    check_ew("silu backward", dx, dxr, dtype)
    bd, b64 = dev(-x.flip(0) * 0.75, dtype)
    s = ops.add(xd, bd)
    assert torch.isfinite(s).all()
    check_equal("add", s, (x64.float() + b64.float()).to(dtype))


# ---- attention at the SDXL 128 x 128 level-1 shapes --------------------------------------------------------------------
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


@pytest.mark.parametrize("Tq,Tk,masked", [(4096, 4096, False), (4096, 77, False), (4096, 77, True)])
def test_attention_sdxl_level1_bf16(Tq, Tk, masked):
    """Self-attention at T = 4096 (4 x 128 x 128 latents, level 1) and cross-attention to 77 text tokens, with and
    without the encoder_attention_mask key bias; error measures of test_kernels_gpu.py::test_attention_key_bias."""
    from uwudiff_amd import ops

    B, H, d = 1, 2, 64
    D = H * d
    (qd, q64), (kd, k64), (vd, v64), (dod, do64) = (dev(_randn(B * T, D, seed=s), BF)
                                                    for s, T in ((1, Tq), (2, Tk), (3, Tk), (4, Tq)))
    bias = None
    if masked:
        keep = (torch.rand(B, Tk, generator=_gen(5)) > 0.4).double()
        keep[:, 0] = 1
        bias = (1 - keep) * -10000.0

    def heads(t, T):
        return t.reshape(T, H, d).transpose(0, 1)

    o_r, lse_r, dq_r, dk_r, dv_r = _attention_ref64(heads(q64, Tq), heads(k64, Tk), heads(v64, Tk), heads(do64, Tq),
                                                    None if bias is None else bias[0], d ** -0.5)
    kb = None if bias is None else bias.float().cuda()
    o, lse = ops.attention_fwd(qd, kd, vd, B, Tq, Tk, H, d, key_bias=kb)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops.attention_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, B, Tq, Tk, H, d, key_bias=kb)
    torch.cuda.synchronize()

    def flat(t, T):
        return t.transpose(0, 1).reshape(T, D)

    torch.testing.assert_close(o.cpu().double(), flat(o_r, Tq), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse.cpu().double().reshape(H, Tq), lse_r, rtol=1e-4, atol=3e-2)
    for name, got, ref, T in (("dq", dq, dq_r, Tq), ("dk", dk, dk_r, Tk), ("dv", dv, dv_r, Tk)):
        ref = flat(ref, T)
        err = (got.cpu().double() - ref).abs().max().item()
        assert err < 1.5e-2 * ref.abs().max().item() + 1e-3, (name, err, ref.abs().max().item())


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_unet_ops_reject_bad_arguments_without_launching():
    """Bad shapes are a negative return code (UwuError with the library's message), never a launch."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    x6 = torch.zeros(2 * 3 * 3, 6, device="cuda", dtype=BF)  # C = 6: not a multiple of 4
    x8 = torch.zeros(2 * 3 * 3, 8, device="cuda", dtype=BF)
    with pytest.raises(L.UwuError, match="im2col3x3"):
        ops.im2col3x3(x6, 2, 3, 3, 6)
    with pytest.raises(L.UwuError, match="im2col3x3"):
        ops.im2col3x3(x8, 2, 3, 3, 8, stride=3)
    with pytest.raises(L.UwuError, match="col2im3x3"):
        ops.col2im3x3(torch.zeros(2 * 9, 9 * 6, device="cuda", dtype=BF), 2, 3, 3, 6)
    with pytest.raises(L.UwuError, match="col2im3x3"):
        ops.col2im3x3(torch.zeros(2 * 9, 9 * 8, device="cuda", dtype=BF), 2, 3, 3, 8, stride=3)
    with pytest.raises(L.UwuError, match="upsample2x"):
        ops.upsample2x(x6, 2, 3, 3, 6)
    with pytest.raises(L.UwuError, match="upsample2x"):
        ops.upsample2x(torch.zeros(2 * 36, 6, device="cuda", dtype=BF), 2, 3, 3, 6, backward=True)
    with pytest.raises(L.UwuError, match="add_rowvec"):
        ops.add_rowvec(x6, torch.zeros(2, 6, device="cuda", dtype=BF), 2, 9, 6)
    with pytest.raises(L.UwuError, match="geglu_fwd"):
        ops.geglu_fwd(torch.zeros(5, 12, device="cuda", dtype=BF))
    with pytest.raises(L.UwuError, match="geglu_bwd"):
        ops.geglu_bwd(torch.zeros(5, 12, device="cuda", dtype=BF), torch.zeros(5, 6, device="cuda", dtype=BF))
    with pytest.raises(L.UwuError, match="colsum"):
        ops.colsum_batched(x6, 2, 9, 6)
    g, b = torch.ones(4104, device="cuda"), torch.zeros(4104, device="cuda")
    for C, G in ((64, 24), (4104, 8), (40, 3)):  # G does not divide C; C > 4096
        xg = torch.zeros(16, C, device="cuda", dtype=BF)
        with pytest.raises(L.UwuError, match="groupnorm_fwd"):
            ops.groupnorm_fwd(xg, g[:C], b[:C], 2, 8, C, G, 1e-5, True)
        st = torch.zeros(2 * G, device="cuda")
        with pytest.raises(L.UwuError, match="groupnorm_bwd"):
            ops.groupnorm_bwd(xg, xg, st, st, g[:C], b[:C], None, None, 2, 8, C, G, True)
    torch.cuda.synchronize()  # nothing was launched, nothing faulted
