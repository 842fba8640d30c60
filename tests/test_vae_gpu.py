"""GPU: the AutoencoderKL (uwudiff_amd/vae.py) and its three kernels against references computed on the CPU.

  uwu_conv3x3_s2br_fwd    F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2) in fp64: exact on small-integer operands (the
                          convention of tests/test_conv_gpu.py), and on randn data inside that file's bound
                          2^-8 |ref| + n 2^-24 S
  uwu_attention_d512_fwd  F.scaled_dot_product_attention on the CPU (on the bf16-rounded operands for bf16) with
                          tests/test_kernels_gpu.py's tolerances; T = 16384 inside a memory budget that leaves no room for T x T
  uwu_posterior_draw      mean + exp(0.5 clamp(logvar, -30, 20)) eps with eps from uwu_philox_normal at the same (seed, offset)
  the whole model         tests/vae_oracle.py in fp64 with the same weights: fp32 mode to 1e-3, bf16 mode to twice the error of
                          the oracle itself run in bfloat16 on the CPU
"""
import pytest
import torch
import torch.nn.functional as F

from tests import vae_oracle

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BF16_NAN, F32_NAN = 0x7FC1, 0x7FC00001  # sentinel bit patterns for memory no kernel may touch


# ---------------------------------------------------------------------------------------------- stride-2 convolution
def _cl(t, dtype):  # NCHW -> [B*H*W, C] channels-last on the device
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().to(dtype).cuda()


def _wk(w):  # [Cout, C, 3, 3] -> [Cout, 9*C] tap-major
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _ref_s2br(x, w, b):
    return F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), None if b is None else b.double(), stride=2)


S2BR_EXACT = [  # B, H, W, C, Cout, dtype, implicit GEMM?
    (2, 16, 16, 128, 128, BF, True),
    (1, 32, 32, 256, 256, BF, True),
    (2, 8, 8, 512, 512, BF, True),
    (32, 7, 9, 128, 128, BF, True),     # odd H and W (Ho 3, Wo 4): no tap of the last row / column is padded
    (4, 9, 16, 256, 256, BF, True),     # odd H, even W
    (8, 3, 16, 512, 512, BF, True),     # a 3-row image: one output row, whose third tap row is inside
    (3, 64, 64, 128, 128, BF, True),    # several 256-row tiles per image, tiles that start mid-row
    (1, 7, 9, 128, 128, BF, False),     # B Ho Wo = 12: fails the implicit conditions -> gather + GEMM
    (2, 8, 8, 8, 16, BF, False),        # C, Cout < 32 -> gather + GEMM
    (2, 8, 10, 128, 128, torch.float32, False),   # the fp32 path
    (1, 7, 7, 256, 256, torch.float32, False),
]


def _int_data(B, H, W, C, Cout, seed):
    """integers: x in [-2, 2]; +-1 weights with about 256 non-zero terms per output; bias in [-3, 3] -> every product, partial
    sum and result is an integer below 256 in magnitude (checked), which bf16 and the fp32 accumulator hold exactly"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    w = torch.randint(0, 2, (Cout, C, 3, 3), generator=g).float() * 2 - 1
    w = w * (torch.rand(Cout, C, 3, 3, generator=g) < min(0.25, 256.0 / (9 * C)))
    bias = torch.randint(-3, 4, (Cout,), generator=g).float()
    return x, w, bias


@pytest.mark.parametrize("B,H,W,C,Cout,dtype,implicit", S2BR_EXACT)
def test_conv3x3_s2br_exact_on_integers(B, H, W, C, Cout, dtype, implicit):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    x, w, bias = _int_data(B, H, W, C, Cout, 1000 * H + 10 * W + C + B)
    ref = _ref_s2br(x, w, bias)
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    assert ref.shape == (B, Cout, Ho, Wo) and float(ref.abs().max()) < 256
    need = L.load().uwu_conv3x3_s2br_ws_bytes(B, H, W, C, Cout, L.BF16 if dtype == BF else L.F32)
    assert (need == 0) == implicit, need
    if not implicit:
        assert need == B * Ho * Wo * 9 * C * (2 if dtype == BF else 4)
    y = ops.conv3x3_s2br_fwd(_cl(x, dtype), _wk(w).to(dtype).cuda(), bias.cuda(), B, H, W, C, Cout)
    assert y.dtype == dtype and y.shape == (B * Ho * Wo, Cout)
    got = y.double().cpu().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    bad = got != ref
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} wrong; first at {bad.nonzero()[0].tolist()}"
    # without a bias, into a buffer with guard rows
    yb = torch.empty(B * Ho * Wo + 64, Cout, dtype=dtype, device="cuda")
    (yb.view(torch.int16) if dtype == BF else yb.view(torch.int32)).fill_(BF16_NAN if dtype == BF else F32_NAN)
    xd, wd = _cl(x, dtype), _wk(w).to(dtype).cuda()
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    L.call("uwu_conv3x3_s2br_fwd", L.ptr(xd), L.ptr(wd), None, L.ptr(yb), B, H, W, C, Cout, L.dt(xd), L.ptr(ws), need, L.stream())
    got = yb[:B * Ho * Wo].double().cpu().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    assert torch.equal(got, _ref_s2br(x, w, None))
    tail = yb[B * Ho * Wo:]
    assert bool(((tail.view(torch.int16) == BF16_NAN) if dtype == BF else (tail.view(torch.int32) == F32_NAN)).all())


@pytest.mark.parametrize("B,H,W,C", [(1, 64, 64, 128), (2, 32, 32, 256), (2, 16, 16, 512), (8, 7, 9, 128), (1, 7, 9, 256)])
def test_conv3x3_s2br_real_fp64_bound(B, H, W, C):
    """randn data rounded to bf16 once, against fp64: |got - ref| <= 2^-8 |ref| + n 2^-24 S (tests/test_conv_gpu.py's _within: one
    bf16 rounding of the result plus the any-order fp32 accumulation bound of n terms whose absolute values sum to S)"""
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(7 * H + W + C)
    r = lambda t: t.bfloat16().double()  # noqa: E731
    x = r(torch.randn(B, C, H, W, generator=g))
    w = r(torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5)
    bias = torch.randn(C, generator=g).double()
    y = ops.conv3x3_s2br_fwd(_cl(x, BF), _wk(w).bfloat16().cuda(), bias.float().cuda(), B, H, W, C, C)
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)  # noqa: E731
    ref = cl(_ref_s2br(x, w, bias))
    S = cl(_ref_s2br(x.abs(), w.abs(), bias.abs()))
    got = y.double().cpu()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (9 * C + 1) * 2.0 ** -24 * S
    print(f"[conv3x3_s2br real] {(B, H, W, C)}: worst |got - ref| / bound = {(err / bound).max().item():.4f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())


def test_conv3x3_s2br_refusals():
    """null pointer, misalignment, C = 0, H < 2, a missing workspace: a UwuError that names the entry point; nothing is launched
    (the output keeps its sentinel)"""
    from uwudiff_amd import lib as L

    n = 1 << 16
    a, w, f = torch.zeros(n, dtype=BF, device="cuda"), torch.zeros(n, dtype=BF, device="cuda"), torch.zeros(n, device="cuda")
    out = torch.empty(n, dtype=BF, device="cuda")
    out.view(torch.int16).fill_(BF16_NAN)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    ok = (2, 8, 8, 32, 32)

    def call(x=a.data_ptr(), wt=w.data_ptr(), b=f.data_ptr(), y=out.data_ptr(), shape=ok, dtype=L.BF16, wsp=ws.data_ptr(),
             wsn=ws.numel()):
        L.call("uwu_conv3x3_s2br_fwd", x, wt, b, y, *shape, dtype, wsp, wsn, L.stream())

    cases = [dict(x=None), dict(wt=None), dict(y=None), dict(x=a.data_ptr() + 8), dict(wt=w.data_ptr() + 8),
             dict(y=out.data_ptr() + 8), dict(b=f.data_ptr() + 4), dict(shape=(2, 8, 8, 0, 32)), dict(shape=(2, 8, 8, 32, 0)),
             dict(shape=(0, 8, 8, 32, 32)), dict(shape=(2, 1, 8, 32, 32)), dict(shape=(2, 8, 8, 36, 32)), dict(dtype=7),
             dict(shape=(1, 7, 9, 32, 32), wsp=None, wsn=0), dict(shape=(1, 7, 9, 32, 32), wsn=64),
             dict(shape=(2, 8, 8, 34, 32), dtype=L.F32)]
    for kw in cases:
        with pytest.raises(L.UwuError, match="conv3x3_s2br_fwd"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == BF16_NAN).all())
    call()  # the same buffers with nothing wrong: runs
    torch.cuda.synchronize()
    assert bool((out[:2 * 4 * 4 * 32] == 0).all())


# ---------------------------------------------------------------------------------------------- attention, d = 512
def _sdpa64(q, k, v):
    return F.scaled_dot_product_attention(q.double()[:, None], k.double()[:, None], v.double()[:, None])[:, 0]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 64, 240, 400, 1024, 4096])
def test_attention_d512_matches_sdpa(T, B, dtype):
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(T + B)
    q, k, v = (torch.randn(B, T, 512, generator=g).to(dtype) for _ in range(3))
    o = ops.attention_d512_fwd(*(t.reshape(B * T, 512).cuda() for t in (q, k, v)), B, T)
    assert o.dtype == dtype and o.shape == (B * T, 512)
    ref = _sdpa64(q, k, v).reshape(B * T, 512)
    got = o.double().cpu()
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    print(f"[attention_d512] T={T} B={B} {dtype}: max |got - ref| = {(got - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_attention_d512_packed_projection_and_peaked_scores(dtype):
    """q / k / v as column slices of one [B*T, 1536] tensor (row stride 1536), and scores large enough that the softmax is
    nearly one-hot: the running maximum has to move while the keys are walked"""
    from uwudiff_amd import ops

    B, T = 2, 400
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * T, 1536, generator=g)
    qkv[:, :1024] *= 3.0
    qkv = qkv.to(dtype)
    d = qkv.cuda()
    o = ops.attention_d512_fwd(d[:, :512], d[:, 512:1024], d[:, 1024:], B, T)
    ref = _sdpa64(*(qkv[:, i * 512:(i + 1) * 512].reshape(B, T, 512) for i in range(3))).reshape(B * T, 512)
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(o.double().cpu(), ref, **tol)


def test_attention_d512_long_sequence_has_no_score_matrix():
    """T = 16384 (a 1024 x 1024 image), bf16: the call stays inside operands + output + 64 MB of device memory -- a T x T score
    tensor alone would be 512 MB in bf16 -- and 256 sampled query rows match SDPA"""
    from uwudiff_amd import ops

    T = 16384
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator().manual_seed(16384)
    q, k, v = (torch.randn(T, 512, generator=g).bfloat16() for _ in range(3))
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    o = ops.attention_d512_fwd(qd, kd, vd, 1, T)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    budget = 4 * T * 512 * 2 + (64 << 20)
    print(f"[attention_d512] T={T}: peak device memory {peak / 2 ** 20:.1f} MB, budget {budget / 2 ** 20:.1f} MB")
    assert peak <= budget
    rows = torch.randperm(T, generator=g)[:256]
    ref = _sdpa64(q[rows][None], k[None], v[None])[0]
    torch.testing.assert_close(o[rows.cuda()].double().cpu(), ref, rtol=2e-2, atol=2e-2)


def test_attention_d512_refusals():
    from uwudiff_amd import lib as L

    a = torch.zeros(64 * 520, dtype=BF, device="cuda")
    out = torch.empty(64 * 512, dtype=BF, device="cuda")
    out.view(torch.int16).fill_(BF16_NAN)
    p, o = a.data_ptr(), out.data_ptr()

    def call(q=p, k=p, v=p, y=o, B=1, T=64, ld=(512, 512, 512, 512), scale=512 ** -0.5, dtype=L.BF16):
        L.call("uwu_attention_d512_fwd", q, k, v, y, B, T, *ld, scale, dtype, L.stream())

    for kw in (dict(q=None), dict(y=None), dict(k=p + 8), dict(y=o + 2), dict(T=0), dict(B=0), dict(ld=(504, 512, 512, 512)),
               dict(ld=(516, 512, 512, 512)), dict(ld=(512, 512, 512, 256)), dict(scale=0.0), dict(dtype=3)):
        with pytest.raises(L.UwuError, match="attention_d512_fwd"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == BF16_NAN).all())


# ---------------------------------------------------------------------------------------------- posterior draw
def _moments(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    mom = torch.randn(B * h * w, 8, generator=g)
    mom[:, 4:] *= 4.0
    mom[::7, 5] = 41.5    # beyond the upper clamp (20)
    mom[3::11, 6] = -77.0  # beyond the lower clamp (-30)
    return mom


def _nchw(t, B, h, w):  # [B*h*w, 4] -> [B, 4, h, w]
    return t.reshape(B, h * w, 4).permute(0, 2, 1).reshape(B, 4, h, w)


@pytest.mark.parametrize("B,h,w", [(2, 8, 8), (1, 12, 20), (3, 1, 1), (16, 32, 32)])
def test_posterior_draw_formula(B, h, w):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    mom = _moments(B, h, w, seed=B + h)
    seed, offset = 0x1234_5678_9ABC, 4096 + 8 * h
    n = B * 4 * h * w
    eps = torch.empty(n, device="cuda")
    L.call("uwu_philox_normal", L.ptr(eps), n, seed, offset, L.stream())
    z, mu, lv = ops.posterior_draw(mom.cuda(), B, 4, h * w, seed, offset, sample=True, mean=True, logvar=True)
    mean = _nchw(mom[:, :4], B, h, w).double()
    logvar = _nchw(mom[:, 4:], B, h, w).double().clamp(-30.0, 20.0)
    assert float(_nchw(mom[:, 4:], B, h, w).max()) > 20 and (B * h * w < 12 or float(mom[:, 4:].min()) < -30)
    assert torch.equal(mu.cpu().reshape(B, 4, h, w).double(), mean)
    assert torch.equal(lv.cpu().reshape(B, 4, h, w).double(), logvar)
    ref = mean + torch.exp(0.5 * logvar) * eps.cpu().double().reshape(B, 4, h, w)
    torch.testing.assert_close(z.cpu().double().reshape(B, 4, h, w), ref, rtol=1e-6, atol=1e-6)
    # the draw alone, and the moments alone, give the same tensors
    z2, none_mu, none_lv = ops.posterior_draw(mom.cuda(), B, 4, h * w, seed, offset)
    assert none_mu is None and none_lv is None and torch.equal(z2, z)


def test_latent_dist_sampling_follows_the_generator():
    from uwudiff_amd.vae import DiagonalGaussianDistribution

    B, h, w = 2, 8, 8
    dist = DiagonalGaussianDistribution(_moments(B, h, w, seed=9).cuda(), B, 4, h, w)
    torch.manual_seed(77)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    off0 = gen.get_offset()
    z1 = dist.sample()
    assert gen.get_offset() == off0 + B * 4 * h * w // 4  # one counter per four elements (a multiple of the granule 4)
    z2 = dist.sample()
    assert z1.shape == (B, 4, h, w) and z1.dtype == torch.float32 and not torch.equal(z1, z2)
    torch.manual_seed(77)
    assert torch.equal(dist.sample(), z1) and torch.equal(dist.sample(), z2)
    g = torch.Generator(device="cuda").manual_seed(77)
    assert torch.equal(dist.sample(generator=g), z1)  # the same seed and offset 0 in a generator of its own
    assert torch.equal(dist.mode(), dist.mean) and dist.mean.shape == (B, 4, h, w)
    assert float(dist.logvar.max()) == 20.0 and float(dist.logvar.min()) == -30.0
    torch.testing.assert_close(dist.std, torch.exp(0.5 * dist.logvar))
    torch.testing.assert_close(dist.var, torch.exp(dist.logvar))


# ---------------------------------------------------------------------------------------------- the whole model
@pytest.fixture(scope="module")
def oracle():
    torch.manual_seed(1215)
    return vae_oracle.AutoencoderKL().eval().double()


def _model(oracle, compute_dtype):
    from uwudiff_amd.vae import AutoencoderKL

    m = AutoencoderKL.from_pretrained("sdxl-vae", compute_dtype=compute_dtype, init_weights=False)
    m.load_state_dict({k: v.float() for k, v in oracle.state_dict().items()})
    return m.cuda()


def _errs(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def vae_fp32(oracle):
    return _model(oracle, "fp32")


@pytest.fixture(scope="module")
def vae_bf16(oracle):
    return _model(oracle, "bf16")


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 96, 160)])
def test_model_fp32_matches_fp64_oracle(oracle, vae_fp32, shape):
    """encode: .mean and .logvar; decode: .sample; relative L2 and max-abs / max-abs <= 1e-3 (the project's fp32 bar; the fp32
    CPU oracle itself sits at 8e-7 / 2e-6 against fp64)"""
    g = torch.Generator().manual_seed(shape[2] + shape[3])
    x = torch.randn(shape, generator=g)
    with torch.no_grad():
        mean, logvar = oracle.moments(x.double())
        z = mean + 0.5 * torch.randn(mean.shape, generator=g).double()
        img = oracle.decode(z)
    dist = vae_fp32.encode(x.cuda()).latent_dist
    dec = vae_fp32.decode(z.float().cuda())
    assert dec.sample is dec[0] and dec.sample.shape == shape and dist.mean.shape == mean.shape
    for what, got, ref in (("mean", dist.mean, mean), ("logvar", dist.logvar, logvar), ("decode", dec.sample, img)):
        l2, mx = _errs(got, ref)
        print(f"[vae fp32 {shape}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)


def test_model_bf16_within_twice_the_cpu_bf16_oracle(oracle, vae_bf16):
    """[2, 3, 128, 128].  The bound is measured in the test: the oracle run once with module and input cast to torch.bfloat16 on
    the CPU, its relative-L2 and max-abs / max-abs errors against the fp64 oracle on the same input (encoder: mean and logvar
    stacked; decoder: the image decoded from the fp64 mean).  The HIP result stays within 2x each: both pipelines round every
    tensor to bf16 and differ in summation order and in where the norms round."""
    import copy

    g = torch.Generator().manual_seed(128)
    x = torch.randn(2, 3, 128, 128, generator=g)
    with torch.no_grad():
        mean, logvar = oracle.moments(x.double())
        img = oracle.decode(mean)
        ob = copy.deepcopy(oracle).bfloat16()
        mb, lb = ob.moments(x.bfloat16())
        ib = ob.decode(mean.bfloat16())
    ref_enc = torch.cat([mean, logvar], dim=1)
    cpu = _errs(torch.cat([mb, lb], dim=1), ref_enc) + _errs(ib, img)
    dist = vae_bf16.encode(x.cuda()).latent_dist
    dec = vae_bf16.decode(mean.float().cuda()).sample
    hip = _errs(torch.cat([dist.mean, dist.logvar], dim=1), ref_enc) + _errs(dec, img)
    names = ("encoder rel L2", "encoder max-abs", "decoder rel L2", "decoder max-abs")
    for nm, h, c in zip(names, hip, cpu):
        print(f"[vae bf16 128x128] {nm}: HIP {h:.3e}, CPU bf16 oracle {c:.3e}, ratio {h / c:.2f}")
    for nm, h, c in zip(names, hip, cpu):
        assert h <= 2.0 * c, (nm, h, c)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,HW,C,silu", [(2, 4096, 128, True), (3, 1031, 256, False), (2, 240, 512, True)])
def test_groupnorm_fwd_det_is_reproducible_and_matches_fp64(B, HW, C, silu, dtype):
    """the fixed-order GroupNorm forward the VAE runs on: y, mean, rstd inside the bounds tests/test_unet_ops_gpu.py sets for
    uwu_groupnorm_fwd (mean 1e-5 sigma + 2e-6 |mean|, rstd 2e-5, y 1e-4 or one bf16 ulp), the same bits from two launches, and a
    sample's rows the same bits alone (B = 1) as inside the batch"""
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(HW + C)
    x = (torch.randn(B, HW, C, generator=g, dtype=torch.float64) + 3.0).to(dtype)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)).float()
    beta = (0.3 * torch.randn(C, generator=g)).float()
    xd, gd, bd = x.reshape(B * HW, C).cuda(), gamma.cuda(), beta.cuda()
    y, mean, rstd = ops.groupnorm_fwd_det(xd, gd, bd, B, HW, C, 32, 1e-6, silu)
    y2, mean2, rstd2 = ops.groupnorm_fwd_det(xd, gd, bd, B, HW, C, 32, 1e-6, silu)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    for i in range(B):
        yi, mi, ri = ops.groupnorm_fwd_det(xd[i * HW:(i + 1) * HW], gd, bd, 1, HW, C, 32, 1e-6, silu)
        assert torch.equal(yi, y[i * HW:(i + 1) * HW]) and torch.equal(mi, mean[i * 32:(i + 1) * 32]) and torch.equal(ri, rstd[i * 32:(i + 1) * 32])
    x64 = x.double()
    xg = x64.reshape(B, HW, 32, C // 32)
    m64 = xg.mean(dim=(1, 3))
    r64 = (xg - m64[:, None, :, None]).square().mean(dim=(1, 3)).add(1e-6).rsqrt()
    z = F.group_norm(x64.transpose(1, 2), 32, gamma.double(), beta.double(), eps=1e-6).transpose(1, 2)
    ref = (F.silu(z) if silu else z).reshape(B * HW, C)
    assert bool(((mean.double().cpu() - m64.reshape(-1)).abs() <= 1e-5 / r64.reshape(-1) + 2e-6 * m64.reshape(-1).abs()).all())
    assert bool(((rstd.double().cpu() - r64.reshape(-1)).abs() <= 2e-5 * r64.reshape(-1)).all())
    got = y.double().cpu()
    ok = (got - ref).abs() <= 1e-4
    if dtype == BF:
        r16 = ref.float().bfloat16().double()
        _, e = torch.frexp(r16.abs().clamp_min(2.0 ** -126))
        ok = ok | ((got - r16).abs() <= torch.ldexp(torch.ones_like(r16), e - 8))
    assert bool(ok.all()), int((~ok).sum())


def test_model_bf16_real_shape_and_batch_additivity(vae_bf16):
    """[2, 3, 256, 256] in bf16: encode -> [2, 4, 32, 32] finite, decode of it -> [2, 3, 256, 256] finite, and B = 2 against two
    B = 1 calls: BIT-EQUAL.  No kernel with float atomics lies on the VAE's path: its GroupNorms run uwu_groupnorm_fwd_det (fixed
    summation order, a row partition that does not depend on B), and every GEMM / convolution / attention row is computed
    from its own sample's rows in an order that does not depend on the batch."""
    g = torch.Generator().manual_seed(256)
    x = torch.randn(2, 3, 256, 256, generator=g).cuda()
    torch.manual_seed(3)
    dist = vae_bf16.encode(x).latent_dist
    z = dist.sample()
    assert z.shape == (2, 4, 32, 32) and z.dtype == torch.float32 and bool(torch.isfinite(z).all())
    img = vae_bf16.decode(z).sample
    assert img.shape == (2, 3, 256, 256) and img.dtype == torch.float32 and bool(torch.isfinite(img).all())
    d1 = [vae_bf16.encode(x[i:i + 1]).latent_dist for i in range(2)]
    img1 = torch.cat([vae_bf16.decode(z[i:i + 1]).sample for i in range(2)])
    pairs = (("encode mean", dist.mean, torch.cat([d.mean for d in d1])), ("encode logvar", dist.logvar, torch.cat([d.logvar for d in d1])),
             ("decode", img, img1))
    for what, a, b in pairs:
        print(f"[vae bf16 256x256] {what}: B = 2 vs 2 x B = 1: bit-equal {torch.equal(a, b)}, max |diff| {(a - b).abs().max().item():.3e}, "
              f"max |value| {b.abs().max().item():.3e}")
    for what, a, b in pairs:
        assert torch.equal(a, b), what


def test_trainer_encodes_pixels_with_the_autoencoder():
    """DMTrainer with the reference's vae node: [2, 3, 64, 64] pixels -> noisy latents [2, 4, 8, 8], and the same noisy latents from
    vae.encode(x).latent_dist.sample() + the loss, run separately from the same generator state: the same bits (the VAE's path has
    no float atomics and the draws follow the generator)."""
    from duwu.trainer import DMTrainer

    cfg = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": {"depth": 1, "hidden": 128, "heads": 2, "sample_size": 8}},
           "te": None,
           "vae": {"_target_": "diffusers.AutoencoderKL.from_pretrained", "_load_config_": {"precision": "torch.float16", "to_freeze": True},
                   "pretrained_model_name_or_path": "madebyollin/sdxl-vae-fp16-fix"}}
    torch.manual_seed(1215)
    tr = DMTrainer(cfg, vae_std=1 / 0.13025, use_warm_up=False).cuda()
    from uwudiff_amd.vae import AutoencoderKL

    assert isinstance(tr.vae, AutoencoderKL) and tr.vae.flat.dtype == torch.float32 and tr.vae.flat.is_cuda
    x = torch.randn(2, 3, 64, 64).cuda()
    batch = (x, ["", ""], [], {}, {})
    torch.manual_seed(99)
    out = tr.training_step(batch, 0)
    noisy = out["aux_output"].noisy_latent
    assert noisy.shape == (2, 4, 8, 8) and bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(noisy).all())
    assert tr.loss._latent_norm == (0.0, 1 / 0.13025)
    torch.manual_seed(99)
    z = tr.vae.encode(x).latent_dist.sample()
    _, aux = tr.loss(z, tr.unet, encoder_hidden_states=None, encoder_attention_mask=None, added_cond_kwargs={"text_embeds": None},
                     cross_attention_kwargs={})
    l2, _ = _errs(aux.noisy_latent, noisy.cpu())
    print(f"[vae trainer] noisy latent, step vs separate encode + loss: bit-equal {torch.equal(aux.noisy_latent, noisy)}, rel L2 {l2:.3e}")
    assert torch.equal(aux.noisy_latent, noisy)
