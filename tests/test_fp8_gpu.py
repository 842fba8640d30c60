"""fp8 (OCP e4m3 / e5m2) path of BASELINE config 5: the quantising kernels and the block-scaled-MFMA GEMM.

Checker: fp32 CPU matmul on operands de-quantised with ``torch.float8_e4m3fn`` / ``torch.float8_e5m2`` (the reference
has no fp8 path; its Linear is nn.Linear under bf16 autocast).  Exact on integer-valued operands (this also pins the
lane -> k mapping of v_mfma_scale_f32_16x16x128_f8f6f4 for both operands), tolerance on random data.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
FMAX = {0: 448.0, 1: 57344.0}


def deq(u8, fmt):
    return u8.cpu().view(F8[fmt]).float()


def ref_quant(x, s, fmt):
    return (x.float().cpu() * s).clamp(-FMAX[fmt], FMAX[fmt]).to(F8[fmt])


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,K", [(64, 64), (200, 136), (1024, 1152)])
def test_quantize_matches_torch_float8(fmt, dtype, M, K):
    from uwudiff_amd import ops

    torch.manual_seed(M + K + fmt)
    x = (torch.randn(M, K) * 3).to(dtype)
    x[0, 0] = 1e6  # saturates
    x[1, 1] = -1e6
    xd = x.cuda()
    scale = torch.tensor([7.25], device="cuda")
    amax = torch.zeros(1, device="cuda")
    cs = torch.zeros(K, device="cuda")
    Mp = (M + 15) // 16 * 16
    out, _ = ops.fp8_quantize(xd, scale, fmt, amax=amax, colsum=cs)
    want = ref_quant(x, 7.25, fmt)
    assert torch.equal(out.cpu().view(F8[fmt]).view(torch.uint8), want.view(torch.uint8))
    if M % 16 == 0:
        _, out_t = ops.fp8_quantize(xd, scale, fmt, rowmajor=False, transposed=True)
        assert torch.equal(out_t.cpu(), want.view(torch.uint8).t().contiguous())
    assert float(amax) == float(x.float().abs().max())
    # per column, the worst case of its fp32 adds: a value passes 3 adds in its thread (4 rows), 3 shuffle adds (8 row groups),
    # 3 across the waves and one atomic per 128-row tile, each rounding by at most half an ulp of a partial sum that never
    # exceeds the column's absolute sum S: (9 + tiles) * 2^-24 * S, in whatever order the atomics land.  The two 1e6 outliers
    # loosen their own columns only (0.6 .. 1.0) -- every other column is held to ~1e-3 where one bar of 1 stood.
    ref_cs = x.double().sum(0)
    bar = (9 + (M + 127) // 128) * 2.0 ** -24 * x.double().abs().sum(0)
    err = (cs.cpu().double() - ref_cs).abs()
    assert bool((err <= bar).all()), float((err / bar).max())
    a2 = ops.fp8_amax(xd)
    assert float(a2) == float(x.float().abs().max())


def test_update_scales_policy():
    from uwudiff_amd import ops

    amax = torch.tensor([2.0, 0.0, 4.0], device="cuda")
    scale = torch.tensor([0.0, 3.0, 1.0], device="cuda")
    fmt = torch.tensor([0, 0, 1], device="cuda", dtype=torch.int32)
    ops.fp8_update_scales(amax, scale, fmt)
    assert scale.tolist() == [224.0, 3.0, 14336.0] and amax.tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("fmt_a", [0, 1])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 264, 384), (1024, 1152, 1152), (512, 4608, 1152)])
def test_gemm_fp8_exact_on_integers(fmt_a, M, N, K):
    """Small integers are exact in both formats and in the fp32 accumulator: any lane / k-permutation mismatch between the
    two operands, a swapped output orientation or a wrong scale shows up as a wrong integer."""
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-2, 3, (N, K), generator=g).float()
    a[:, ::7] = 0  # asymmetric sparsity pattern along k
    b[::5] = 1.0
    sa, sb = torch.tensor([2.0], device="cuda"), torch.tensor([0.5], device="cuda")
    a8, _ = ops.fp8_quantize(a.cuda(), sa, fmt_a)
    b8, _ = ops.fp8_quantize(b.cuda(), sb, 0)
    c = ops.gemm_fp8(a8, b8, sa, sb, fmt_a=fmt_a)
    want = (a @ b.t())
    # the fp32 accumulator holds these integers exactly; the only rounding is the final RNE to bf16
    assert torch.equal(c.float().cpu(), want.bfloat16().float())


@pytest.mark.parametrize("fmt_a", [0, 1])
@pytest.mark.parametrize("M,N,K,bias", [(256, 256, 512, False), (300, 264, 768, True), (1024, 1152, 1152 + 128, True),
                                        (2048 + 40, 1152, 4608, False), (49152, 1152, 1152 + 128, True)],
                         ids=["one_tile", "ragged", "xl_width_10steps", "ragged_rows_36steps", "xl2_bench_rows"])
def test_gemm_p8f_exact_on_integers_and_equal_to_the_two_stage_kernel(fmt_a, M, N, K, bias, monkeypatch):
    """The 8-phase fp8 kernel (gemm_p8f.hip; UWU_GEMM_P8F=1 forces it for every shape it can run: K a multiple of 256, >= 512):
    persistent workgroups, the element stream running on across tile boundaries, quadrant epilogues inside the next tile's first
    K step.  Exact on integer operands for both operand formats, ragged M / N, with and without bias, one tile per workgroup up to
    960 tiles on 256 workgroups -- and bit-identical to gemm_f8_kernel (UWU_GEMM_P8F=0) on random operands (same MFMA, same k
    order per accumulator, same epilogue)."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + fmt_a)
    a = torch.randint(-3, 4, (M, K), generator=g, device="cuda").float()
    b = torch.randint(-2, 3, (N, K), generator=g, device="cuda").float()
    a[:, ::7] = 0
    b[::5] = 1.0
    bv = torch.randint(-4, 5, (N,), generator=g, device="cuda").float() if bias else None
    sa, sb = torch.tensor([2.0], device="cuda"), torch.tensor([0.5], device="cuda")
    a8, _ = ops.fp8_quantize(a, sa, fmt_a)
    b8, _ = ops.fp8_quantize(b, sb, 0)
    epi = L.EPI_BIAS if bias else L.EPI_NONE
    monkeypatch.setenv("UWU_GEMM_P8F", "1")
    c = ops.gemm_fp8(a8, b8, sa, sb, fmt_a=fmt_a, bias=bv, epilogue=epi)
    c_again = ops.gemm_fp8(a8, b8, sa, sb, fmt_a=fmt_a, bias=bv, epilogue=epi)
    want = a @ b.t() + (bv if bias else 0)
    assert torch.equal(c.float(), want.bfloat16().float())
    assert torch.equal(c, c_again)
    # random fp8 bytes (finite values only): bit-identical to the two-stage kernel
    ra = torch.randint(0, 120, (M, K), generator=g, device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, (M, K), generator=g, device="cuda", dtype=torch.uint8) << 7)
    rb = torch.randint(0, 120, (N, K), generator=g, device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, (N, K), generator=g, device="cuda", dtype=torch.uint8) << 7)
    s1, s2 = torch.tensor([37.0], device="cuda"), torch.tensor([3.0], device="cuda")
    new = ops.gemm_fp8(ra, rb, s1, s2, fmt_a=fmt_a, bias=bv, epilogue=epi)
    monkeypatch.setenv("UWU_GEMM_P8F", "0")
    old = ops.gemm_fp8(ra, rb, s1, s2, fmt_a=fmt_a, bias=bv, epilogue=epi)
    assert torch.isfinite(new.float()).all() and torch.equal(new, old)


@pytest.mark.parametrize("fmt_a", [0, 1])
@pytest.mark.parametrize("No,Ki,M", [(1152, 1152, 8192), (4608, 1152, 4096 + 2048), (1152 + 8, 384, 16384), (3456, 1152, 49152)],
                         ids=["25tiles", "90tiles_48steps", "ragged", "xl2_qkv"])
def test_gemm_p8f_weight_gradient_slices(fmt_a, No, Ki, M, monkeypatch):
    """Weight gradient on the 8-phase kernel: (K slice, tile) units, fp32 partial slabs, splitk reduce.  Exact on integers (the
    partial sums and their sum are integers below 2^24) and accumulating into a non-zero dW; against the two-stage kernel's
    result to fp32 summation order on random operands."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    g = torch.Generator(device="cuda").manual_seed(No + Ki + fmt_a)
    dyt = torch.randint(-3, 4, (No, M), generator=g, device="cuda").float()
    xt = torch.randint(-2, 3, (Ki, M), generator=g, device="cuda").float()
    sa, sb = torch.tensor([2.0], device="cuda"), torch.tensor([0.5], device="cuda")
    a8, _ = ops.fp8_quantize(dyt, sa, fmt_a)
    b8, _ = ops.fp8_quantize(xt, sb, 0)
    dw0 = torch.randint(-5, 6, (No, Ki), generator=g, device="cuda").float()
    monkeypatch.setenv("UWU_GEMM_P8F_PART", "1")
    dw = dw0.clone()
    ops.gemm_fp8(a8, b8, sa, sb, fmt_a=fmt_a, epilogue=L.EPI_ACCUM, out=dw)
    assert torch.equal(dw, dw0 + dyt @ xt.t())
    ra = torch.randint(0, 120, (No, M), generator=g, device="cuda", dtype=torch.uint8)
    rb = torch.randint(0, 120, (Ki, M), generator=g, device="cuda", dtype=torch.uint8)
    s1, s2 = torch.tensor([4096.0], device="cuda"), torch.tensor([64.0], device="cuda")
    new = ops.gemm_fp8(ra, rb, s1, s2, fmt_a=fmt_a, epilogue=L.EPI_ACCUM, out=torch.zeros(No, Ki, device="cuda"))
    monkeypatch.setenv("UWU_GEMM_P8F_PART", "0")
    old = ops.gemm_fp8(ra, rb, s1, s2, fmt_a=fmt_a, epilogue=L.EPI_ACCUM, out=torch.zeros(No, Ki, device="cuda"))
    torch.testing.assert_close(new, old, rtol=1e-5, atol=1e-5 * float(old.abs().max()))


@pytest.mark.parametrize("epi", ["none", "bias", "bias_gelu", "dgelu"])
def test_gemm_fp8_random_with_epilogues(epi):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    torch.manual_seed(3)
    M, N, K = 1024, 768, 1152
    a, b = torch.randn(M, K), torch.randn(N, K) * 0.05
    bias = torch.randn(N)
    aux = torch.randn(M, N).bfloat16()
    sa = torch.tensor([448.0 / float(a.abs().max())], device="cuda")
    sb = torch.tensor([448.0 / float(b.abs().max())], device="cuda")
    a8, _ = ops.fp8_quantize(a.cuda(), sa, 0)
    b8, _ = ops.fp8_quantize(b.cuda(), sb, 0)
    ref = (deq(a8, 0) @ deq(b8, 0).t()) / (float(sa) * float(sb))  # what the kernel must compute (fp32)
    if epi == "none":
        c = ops.gemm_fp8(a8, b8, sa, sb)
    elif epi == "bias":
        c = ops.gemm_fp8(a8, b8, sa, sb, bias=bias.cuda(), epilogue=L.EPI_BIAS)
        ref = ref + bias
    elif epi == "bias_gelu":
        c, c2 = ops.gemm_fp8(a8, b8, sa, sb, bias=bias.cuda(), epilogue=L.EPI_BIAS_GELU)
        ref = ref + bias
        torch.testing.assert_close(c2.float().cpu(), torch.nn.functional.gelu(ref, approximate="tanh"), rtol=2e-2, atol=2e-2)
    else:
        c = ops.gemm_fp8(a8, b8, sa, sb, aux=aux.cuda(), epilogue=L.EPI_DGELU)
        u = aux.float().requires_grad_(True)
        torch.nn.functional.gelu(u, approximate="tanh").sum().backward()
        ref = ref * u.grad
    torch.testing.assert_close(c.float().cpu(), ref, rtol=1e-2, atol=2e-2)  # bf16 output rounding
    # and the quantisation itself stays within fp8's error of the unquantised product
    full = a @ b.t()
    assert ((deq(a8, 0) @ deq(b8, 0).t()) / (float(sa) * float(sb)) - full).norm() / full.norm() < 6e-2


@pytest.mark.parametrize("fmt_a", [0, 1])
def test_gemm_fp8_weight_gradient_accumulates(fmt_a):
    """dW[N_out, K_in] += dY^T . X through the transposed fp8 copies (contraction over M tokens, split-K partial sums)."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    torch.manual_seed(5)
    M, No, Ki = 4096, 1152, 384
    dy, x = torch.randn(M, No) * 1e-3, torch.randn(M, Ki)
    sa = torch.tensor([FMAX[fmt_a] / float(dy.abs().max())], device="cuda")
    sb = torch.tensor([448.0 / float(x.abs().max())], device="cuda")
    db = torch.zeros(No, device="cuda")
    _, dyt = ops.fp8_quantize(dy.cuda(), sa, fmt_a, rowmajor=False, transposed=True, colsum=db)
    _, xt = ops.fp8_quantize(x.cuda(), sb, 0, rowmajor=False, transposed=True)
    dw0 = torch.randn(No, Ki)
    dw = dw0.clone().cuda()
    ops.gemm_fp8(dyt, xt, sa, sb, fmt_a=fmt_a, epilogue=L.EPI_ACCUM, out=dw)
    ref = dw0 + (deq(dyt, fmt_a) @ deq(xt, 0).t()) / (float(sa) * float(sb))
    torch.testing.assert_close(dw.cpu(), ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(db.cpu(), dy.sum(0), rtol=1e-4, atol=1e-6)
    full = dw0 + dy.t() @ x
    assert (dw.cpu() - full).norm() / full.norm() < 8e-2


@pytest.mark.parametrize("epi,M,N,K", [("bias_gelu", 1024, 768, 1152), ("dgelu", 1024, 768, 1152), ("bias_gelu", 640, 1536, 384),
                                       ("dgelu", 896, 512, 256)])
def test_gemm_fp8_emit_matches_quantised_result(epi, M, N, K):
    """The epilogue that emits the next GEMM's fp8 operand (row-major + transposed) against the two-pass form: the bf16
    pre-activation matches the plain kernel's (to a flipped bf16 rounding), the transposed image is the exact transpose of the row-major one,
    the bytes are the RNE quantisation of the fp32 result (the plain path rounds to bf16 first: checked within one fp8 step),
    amax / column sums match.  M = 640 / 896: a ragged last 256-row tile."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    torch.manual_seed(11)
    fmt_a = 1 if epi == "dgelu" else 0
    a, b = torch.randn(M, K) * (1e-2 if fmt_a else 1.0), torch.randn(N, K) * 0.05
    bias = torch.randn(N)
    aux = torch.randn(M, N).bfloat16()
    sa = torch.tensor([FMAX[fmt_a] / float(a.abs().max())], device="cuda")
    sb = torch.tensor([448.0 / float(b.abs().max())], device="cuda")
    a8, _ = ops.fp8_quantize(a.cuda(), sa, fmt_a)
    b8, _ = ops.fp8_quantize(b.cuda(), sb, 0)
    ref = (deq(a8, fmt_a) @ deq(b8, 0).t()) / (float(sa) * float(sb))
    amax = torch.zeros(1, device="cuda")
    if epi == "bias_gelu":
        fq = 0
        u_plain, f_plain = ops.gemm_fp8(a8, b8, sa, sb, bias=bias.cuda(), epilogue=L.EPI_BIAS_GELU)
        val = torch.nn.functional.gelu(ref + bias, approximate="tanh")
        qs = torch.tensor([448.0 / float(val.abs().max()) * 0.9], device="cuda")
        C, q8, q8t = ops.gemm_fp8_emit(a8, b8, sa, sb, qs, epilogue=L.EPI_BIAS_GELU, bias=bias.cuda(), amax=amax)
        # (alpha * acc + bias contracts to an fma in one epilogue and not in the other: a bf16 rounding may flip)
        torch.testing.assert_close(C.float(), u_plain.float(), rtol=2.0 ** -7, atol=1e-6)
        assert (C == u_plain).float().mean().item() > 0.99
        plain = f_plain
    else:
        fq = 1
        cs = torch.zeros(N, device="cuda")
        cs_plain = torch.zeros(N, device="cuda")
        plain = ops.gemm_fp8(a8, b8, sa, sb, fmt_a=fmt_a, aux=aux.cuda(), epilogue=L.EPI_DGELU, out2=cs_plain)
        u = aux.float().requires_grad_(True)
        torch.nn.functional.gelu(u, approximate="tanh").sum().backward()
        val = ref * u.grad
        qs = torch.tensor([57344.0 / float(val.abs().max()) * 0.9], device="cuda")
        C, q8, q8t = ops.gemm_fp8_emit(a8, b8, sa, sb, qs, epilogue=L.EPI_DGELU, fmt_a=fmt_a, aux=aux.cuda(), colsum=cs, amax=amax)
        assert C is None
        torch.testing.assert_close(cs.cpu(), val.sum(0), rtol=2e-3, atol=2e-3 * float(val.abs().sum(0).max()))
        torch.testing.assert_close(cs, cs_plain, rtol=1e-3, atol=1e-3 * float(cs_plain.abs().max()))
    torch.cuda.synchronize()
    assert torch.equal(q8t, q8.t().contiguous())
    got = deq(q8, fq) / float(qs)
    step = {0: 2.0 ** -3, 1: 2.0 ** -2}[fq]  # relative spacing of e4m3 / e5m2
    tol = step * val.abs() + (2.0 ** -9 if fq == 0 else 2.0 ** -16) / float(qs) + 1e-6  # one step (a flipped rounding) + the subnormal step
    assert ((got - val).abs() <= tol).all(), float(((got - val).abs() - tol).max())
    # against the two-pass form (bf16 rounding first, then the quantiser): equal bytes almost everywhere
    two_pass, _ = ops.fp8_quantize(plain, qs, fq)
    same = (two_pass == q8).float().mean().item()
    assert same > 0.9, same
    torch.testing.assert_close(amax.cpu(), val.abs().max().reshape(1), rtol=2e-2, atol=0)


@pytest.mark.parametrize("D,B,T,with_y", [(1152, 3, 256, True), (384, 2, 96, False), (768, 1, 320, True), (1536, 2, 160, True)])
def test_layernorm_emits_fp8_images(D, B, T, with_y):
    """fp8 mode: LayerNorm + modulate writing the next GEMM's e4m3 operand (row-major + transposed) instead of bf16 h.
    Residual stream and statistics bit-equal to the plain kernel's; the bytes = RNE quantisation of the fp32 output (within one
    e4m3 step where a rounding flips); the transposed image is the exact transpose; amax recorded.  Rows straddle samples; D = 1536 takes the 32-row tiles (two 64-row tiles would not fit a CU's LDS)."""
    from uwudiff_amd import ops

    torch.manual_seed(21)
    M, ML = B * T, 3 * D + 8
    x_in = torch.randn(M, D).bfloat16().cuda()
    y = torch.randn(M, D).bfloat16().cuda() if with_y else None
    mod = (torch.randn(B, ML) * 0.5).cuda()
    g, sh, sc = mod[:, 0:D], mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    kw = dict(shift=sh, scale=sc, mod_ld=ML)
    if with_y:
        kw.update(y=y, gate=g)
    x_out, h, mean, rstd = ops.add_ln_modulate_fwd(x_in, B, T, **kw)
    xo = x_out.float()
    href = torch.nn.functional.layer_norm(xo, (D,), eps=1e-6) * (1 + sc.repeat_interleave(T, 0)) + sh.repeat_interleave(T, 0)
    qs = torch.tensor([448.0 / float(href.abs().max()) * 0.9], device="cuda")
    amax = torch.zeros(1, device="cuda")
    x_out2, q8, q8t, mean2, rstd2 = ops.add_ln_modulate_fwd_q8(x_in, B, T, qs, amax=amax, **kw)
    torch.cuda.synchronize()
    if with_y:
        assert torch.equal(x_out2, x_out)
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    assert torch.equal(q8t, q8.t().contiguous())
    got = deq(q8, 0) / float(qs)
    val = href.cpu()
    tol = 2.0 ** -3 * val.abs() + 2.0 ** -9 / float(qs) + 1e-6
    assert ((got - val).abs() <= tol).all(), float(((got - val).abs() - tol).max())
    two_pass, _ = ops.fp8_quantize(h, qs, 0)
    assert (two_pass == q8).float().mean().item() > 0.9
    torch.testing.assert_close(amax.cpu(), val.abs().max().reshape(1), rtol=1e-2, atol=0)


# ------------------------------------------------------------------------------------------------ whole model, fp8 Linears
XL2_CUT = dict(depth=2, hidden=1152, heads=16, patch=2, sample_size=32, in_channels=4, out_channels=4, cond_dim=1280)


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("scaling", ["jit", "delayed"])
def test_dit_xl2_width_fp8_close_to_oracle(scaling):
    """DiT-XL/2 width (1152, 16 heads; depth cut to 2) with the block Linears on fp8 operands: forward and every parameter
    gradient against the fp32 CPU oracle.  fp8 tolerances (e4m3 has 3 mantissa bits: ~3 % per element, averaged down by
    the contractions); the bf16 path's are 3e-2 / 6e-2.  Delayed scaling: the second step uses the first step's amax."""
    from oracle.dit import DiTOracle
    from uwudiff_amd.dit import DiT, DiTConfig

    torch.manual_seed(0)
    ora = DiTOracle(**XL2_CUT)
    with torch.no_grad():
        for p in ora.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() > 1 else 0.02))
    model = DiT(DiTConfig(compute_dtype="fp8", fp8_scaling=scaling, **XL2_CUT), init="dit").cuda()
    model.load_state_dict(ora.state_dict())
    B = 8
    g = torch.Generator().manual_seed(1)
    for step in range(2 if scaling == "delayed" else 1):
        x = torch.randn(B, 4, 32, 32, generator=g)
        t = torch.randint(0, 1000, (B,), generator=g)
        pooled = torch.randn(B, 1280, generator=g)
        dout = torch.randn(B, 4, 32, 32, generator=g) / 1024
        ora.zero_grad()
        yo = ora(x, t, added_cond_kwargs={"text_embeds": pooled})[0]
        yo.backward(dout)
        model.flat.grad = torch.zeros_like(model.flat.data)
        y = model(x.cuda(), t.cuda(), added_cond_kwargs={"text_embeds": pooled.cuda()})[0]
        y.backward(dout.cuda())
        torch.cuda.synchronize()
    assert model._f8_mode == (2 if scaling == "delayed" else 1)
    assert _rel(y, yo) < 6e-2, _rel(y, yo)
    og = dict(ora.named_parameters())
    bad = {n: _rel(model.grad_view(n), og[n].grad) for n, _ in model.named_tensors()
           if _rel(model.grad_view(n), og[n].grad) >= 0.12}
    assert not bad, bad


def _fp8_pair(scaling):
    from uwudiff_amd.dit import DiT, DiTConfig

    torch.manual_seed(5)
    a = DiT(DiTConfig(compute_dtype="fp8", fp8_scaling=scaling, **XL2_CUT), init="random").cuda()
    b = DiT(DiTConfig(compute_dtype="fp8", fp8_scaling=scaling, **XL2_CUT), init="random").cuda()
    b.load_state_dict(a.state_dict())
    return a, b


def _fp8_step(model, x, t, pooled, dout):
    model.flat.grad = torch.zeros_like(model.flat.data)
    y = model(x, t, added_cond_kwargs={"text_embeds": pooled})[0]
    y.backward(dout)
    torch.cuda.synchronize()
    return y.detach().clone(), model.flat.grad.clone()


@pytest.mark.parametrize("scaling", ["delayed", "jit"])
def test_dit_fp8_block_recomputation_equals_plain_backward(scaling):
    """block recomputation in fp8 mode.  The rerun of a block inside the backward reuses the fp8 scratch
    images (x8 / dy8 / dy8t, the buffers the emitting GEMMs hand du through), re-records amax and -- just-in-time scaling --
    rewrites scale[role]; correctness rests on launch order only.  Three steps (just-in-time, delayed, delayed + emitting
    epilogues) of two models with identical weights, one plain, one with enable_gradient_checkpointing(): outputs bit-equal,
    gradients equal up to the order of their fp32 atomic adds -- the tolerance of the bf16 / fp32 recomputation test."""
    plain, ckpt = _fp8_pair(scaling)
    ckpt.enable_gradient_checkpointing()
    g = torch.Generator().manual_seed(7)
    B = 8
    for step in range(3):
        x = torch.randn(B, 4, 32, 32, generator=g).cuda()
        t = torch.randint(0, 1000, (B,), generator=g).float().cuda()
        pooled = torch.randn(B, 1280, generator=g).cuda()
        dout = (torch.randn(B, 4, 32, 32, generator=g) / 1024).cuda()
        y0, g0 = _fp8_step(plain, x, t, pooled, dout)
        y1, g1 = _fp8_step(ckpt, x, t, pooled, dout)
        assert plain._f8_mode == ckpt._f8_mode == (2 if scaling == "delayed" and step > 0 else 1)
        assert torch.equal(y0, y1), (step, (y0 - y1).abs().max().item())
        l2 = ((g1 - g0).norm() / g0.norm()).item()
        mx = ((g1 - g0).abs().max() / g0.abs().max()).item()
        assert l2 < 1e-4 and mx < 1e-3, (step, l2, mx)
    assert ckpt._ws.numel() < plain._ws.numel()


def test_dit_fp8_emit_switch_compares_two_paths(monkeypatch):
    """UWU_F8_EMIT is re-read after a change inside a process (UwuEnv), so this A/B really runs the emitting epilogues
    against the two-pass quantisation: same losses / gradients within the fp8 tolerance of the emitting GEMM's own test (the
    pre-activation's rounding may flip in < 1 % of the elements), and NOT the same bits (two code paths)."""
    a, b = _fp8_pair("delayed")
    g = torch.Generator().manual_seed(9)
    B = 8
    differs = False
    for step in range(3):
        x = torch.randn(B, 4, 32, 32, generator=g).cuda()
        t = torch.randint(0, 1000, (B,), generator=g).float().cuda()
        pooled = torch.randn(B, 1280, generator=g).cuda()
        dout = (torch.randn(B, 4, 32, 32, generator=g) / 1024).cuda()
        monkeypatch.setenv("UWU_F8_EMIT", "1")
        y0, g0 = _fp8_step(a, x, t, pooled, dout)
        monkeypatch.setenv("UWU_F8_EMIT", "0")
        y1, g1 = _fp8_step(b, x, t, pooled, dout)
        assert _rel(y1, y0) < 2e-2 and _rel(g1, g0) < 5e-2, (step, _rel(y1, y0), _rel(g1, g0))
        differs = differs or not torch.equal(g0, g1)
    assert differs  # steps 1 and 2 run delayed scaling: the switch selects different kernels there
