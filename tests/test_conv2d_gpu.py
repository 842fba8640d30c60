"""GPU: the InceptionV3 extractor's kernels one by one against float64 on the rounded inputs -- ``uwu_conv2d_fwd`` at every kernel
family of the net (rectangular pictures, M tails, 48 / 80 / 448 channels, channel slices on both sides, ReLU on and off, refusals),
``uwu_inception_stem``, ``uwu_pool2d_fwd``, ``uwu_global_avgpool`` and ``uwu_fid_stats_accum``.

Bounds.  Convolution in bf16: ``2^-8 |y| + 2^-20 sum |x| |w|`` -- one rounding of the output to bf16 (half an ulp is 2^-9, the factor
two leaves the ties room) plus an fp32 accumulation in any order.  In fp32: ``2^-23 |y| + n 2^-24 sum |x| |w|`` with n = KH KW C terms,
the bound of the fp32 ``im2col + uwu_gemm`` convolution tests (tests/test_conv_gpu.py).  Statistics: ``B 2^-50 sum_b |f_i f_j|``.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float32]
SENTINEL = -77.0


def _rows(x):  # [B, C, H, W] -> channels-last rows [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


# (B, H, W, C, Cout, kernel, stride, padding): every family at the net's widths, each once on a rectangular picture
CONV_CASES = [
    (3, 5, 9, 128, 128, (1, 7), 1, (0, 3)), (3, 5, 9, 128, 128, (7, 1), 1, (3, 0)),
    (1, 17, 17, 160, 192, (1, 7), 1, (0, 3)), (1, 17, 17, 160, 192, (7, 1), 1, (3, 0)),
    (3, 5, 3, 128, 128, (1, 7), 1, (0, 3)),  # narrower than the kernel
    (1, 35, 35, 288, 384, (3, 3), 2, (0, 0)), (3, 17, 17, 192, 320, (3, 3), 2, (0, 0)), (3, 9, 7, 192, 320, (3, 3), 2, (0, 0)),
    (3, 9, 9, 32, 32, (3, 3), 1, (0, 0)), (1, 9, 9, 80, 192, (3, 3), 1, (0, 0)), (3, 9, 11, 80, 192, (3, 3), 1, (0, 0)),
    (3, 7, 7, 48, 64, (5, 5), 1, (2, 2)), (1, 35, 35, 48, 64, (5, 5), 1, (2, 2)), (3, 7, 5, 48, 64, (5, 5), 1, (2, 2)),
    (3, 8, 8, 384, 384, (1, 3), 1, (0, 1)), (3, 8, 8, 384, 384, (3, 1), 1, (1, 0)),
    (1, 8, 5, 384, 384, (1, 3), 1, (0, 1)), (1, 8, 5, 384, 384, (3, 1), 1, (1, 0)),
    (1, 17, 17, 192, 48, (1, 1), 1, (0, 0)), (1, 17, 17, 64, 80, (1, 1), 1, (0, 0)), (1, 17, 17, 1280, 448, (1, 1), 1, (0, 0)),
    (3, 5, 9, 64, 80, (1, 1), 1, (0, 0)),
    (3, 6, 10, 96, 96, (3, 3), 1, (1, 1)), (1, 8, 8, 448, 384, (3, 3), 1, (1, 1)),
]


def _conv_id(c):
    return "B{}_{}x{}_{}to{}_k{}x{}_s{}".format(c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], c[6])


def _check_conv(case, dtype, relu, sliced, route="conv"):
    from uwudiff_amd import ops

    B, H, W, C, Cout, k, s, p = case
    g = torch.Generator().manual_seed(hash(case) % 2 ** 31)
    xoff, ldx = (8, C + 24) if sliced else (0, C)
    yoff, ldy = (16, Cout + 40) if sliced else (0, Cout)
    xbuf = torch.randn(B * H * W, ldx, generator=g).to(dtype)  # the channels outside the slice hold data a wrong offset would read
    w = (torch.randn(Cout, C, *k, generator=g) * (2.0 / (C * k[0] * k[1])) ** 0.5).to(dtype)
    bias = torch.randn(Cout, generator=g) * 0.5
    Ho, Wo = ops.conv2d_out_hw(H, W, k, s, p)
    out = torch.full((B * Ho * Wo, ldy), SENTINEL, dtype=dtype)
    x64 = _nchw(xbuf[:, xoff:xoff + C].double(), B, H, W)
    ref = F.conv2d(x64, w.double(), bias.double(), s, p)
    mag = F.conv2d(x64.abs(), w.double().abs(), None, s, p)
    assert ref.shape[2:] == (Ho, Wo)
    if relu:
        ref = ref.relu()
    assert ops.conv2d_ok(B, H, W, C, Cout, k, s, p, ldx, xoff, ldy, yoff, dtype)
    wk = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().cuda()
    if route == "gemm":  # the explicit route of the small 1x1 layers: uwu_gemm + uwu_relu_rows on the same slices
        got = ops.conv1x1_gemm_fwd(xbuf.cuda(), wk, bias.cuda(), C, Cout, relu=relu, xoff=xoff, out=out.cuda(), yoff=yoff).cpu()
    else:
        got = ops.conv2d_fwd(xbuf.cuda(), wk, bias.cuda(), B, H, W, C, Cout, k, s, p, relu=relu, xoff=xoff, out=out.cuda(), yoff=yoff).cpu()
    y = _nchw(got[:, yoff:yoff + Cout].double(), B, Ho, Wo)
    n = k[0] * k[1] * C
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * mag if dtype == torch.bfloat16 else 2.0 ** -23 * ref.abs() + n * 2.0 ** -24 * mag
    err = (y - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[conv2d/{route} {_conv_id(case)} {dtype} relu={relu} sliced={sliced}] worst |got - ref| / bound = {ratio:.4f} (max err {float(err.max()):.3e})")
    assert bool(torch.isfinite(y).all()) and bool((err <= bound).all()), ratio
    rest = torch.cat([got[:, :yoff], got[:, yoff + Cout:]], 1)
    assert bool((rest == SENTINEL).all()), "the channels beside the slice were written"


@gpu
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv2d_fwd_fp64_bound_on_slices(case, dtype, relu):
    """reads a channel slice, writes a channel slice of a wider buffer whose other channels must stay bit-equal"""
    _check_conv(case, dtype, relu, True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [CONV_CASES[0], CONV_CASES[6], CONV_CASES[13], CONV_CASES[19]], ids=_conv_id)
def test_conv2d_fwd_fp64_bound_whole_rows(case, dtype):
    _check_conv(case, dtype, True, False)


@gpu
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[5] == (1, 1)] + [(3, 8, 8, 2048, 320, (1, 1), 1, (0, 0))], ids=_conv_id)
def test_conv1x1_gemm_route_fp64_bound_on_slices(case, dtype, relu):
    """the route the extractor takes for its 17 x 17 and 8 x 8 1x1 layers, held to the convolution's own bound"""
    _check_conv(case, dtype, relu, True, route="gemm")


@gpu
def test_conv1x1_gemm_route_refusals():
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    x, w, b = torch.zeros(16, 64, device="cuda").bfloat16(), torch.zeros(32, 32, device="cuda").bfloat16(), torch.zeros(32, device="cuda")
    out = torch.full((16, 64), SENTINEL, device="cuda", dtype=torch.bfloat16)
    for kw in (dict(xoff=40), dict(xoff=4), dict(yoff=40), dict(yoff=4)):
        with pytest.raises(L.UwuError):
            ops.conv1x1_gemm_fwd(x, w, b, 32, 32, relu=True, out=out, **kw)
    with pytest.raises(L.UwuError):
        L.call("uwu_relu_rows", L.ptr(out), 16, 60, 64, 0, L.BF16, L.stream())
    with pytest.raises(L.UwuError):
        L.call("uwu_relu_rows", L.ptr(out), 16, 32, 64, 40, L.BF16, L.stream())
    assert bool((out == SENTINEL).all())


# bf16 launches 128-pixel workgroups once those give two per CU (256 CUs: 512 tiles of 128 pixels x 64 channels), and among those
# 96-channel workgroups where 96 divides Cout and 64 does not.  M = 3 * 75 * 75 = 16875 pixels are 132 such tiles: 3 channel tiles stay
# below the threshold (64-pixel workgroups), 5 go above it; M is odd, 24 channels leave the 32-channel step a quarter empty, 264 output
# channels leave the last channel tile 8 wide.  M = 3 * 150 * 150 = 67500 pixels are 528 tiles already with one channel tile: Cout = 96
# runs the 96-channel workgroups, Cout = 64 the 64-channel ones at the same M.
TILE_CASES = [(3, 75, 75, 24, 192, (3, 3), 1, (1, 1)), (3, 75, 75, 24, 264, (3, 3), 1, (1, 1)), (3, 150, 150, 8, 96, (3, 3), 1, (1, 1)),
              (3, 150, 150, 8, 64, (1, 3), 1, (0, 1)), (1, 35, 35, 64, 96, (3, 3), 1, (1, 1))]


@gpu
@pytest.mark.parametrize("case", TILE_CASES, ids=["below_64px", "above_128px", "above_128px_96ch", "above_128px_64ch", "below_96ch"])
def test_conv2d_fwd_on_both_sides_of_the_tile_thresholds(case):
    _check_conv(case, torch.bfloat16, True, True)


@gpu
def test_conv2d_refused_shapes_leave_the_output_untouched():
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    B, H, W = 1, 6, 6
    x = torch.randn(B * H * W, 64, device="cuda").bfloat16()
    bias = torch.zeros(64, device="cuda")
    bad = [dict(C=12, Cout=64, kernel=(3, 3)), dict(C=64, Cout=60, kernel=(3, 3)), dict(C=64, Cout=64, kernel=(2, 2)),
           dict(C=64, Cout=64, kernel=(7, 7)), dict(C=64, Cout=64, kernel=(3, 3), stride=3), dict(C=64, Cout=64, kernel=(1, 3), padding=(0, 3)),
           dict(C=64, Cout=64, kernel=(1, 1), xoff=8), dict(C=32, Cout=64, kernel=(1, 1), xoff=4), dict(C=64, Cout=64, kernel=(1, 1), yoff=8),
           dict(C=64, Cout=64, kernel=(5, 5), padding=0, H=4)]
    for kw in bad:
        kw = dict(dict(stride=1, padding=0, xoff=0, yoff=0, H=H), **kw)
        h = kw.pop("H")
        xx = x[:B * h * W]
        C, Cout, k = kw["C"], kw["Cout"], kw["kernel"]
        w = torch.zeros(Cout, k[0] * k[1] * C, device="cuda", dtype=torch.bfloat16)
        Ho, Wo = ops.conv2d_out_hw(h, W, k, kw["stride"], kw["padding"])
        out = torch.full((max(B * Ho * Wo, 1), 64), SENTINEL, device="cuda", dtype=torch.bfloat16)
        assert not ops.conv2d_ok(B, h, W, C, Cout, k, kw["stride"], kw["padding"], 64, kw["xoff"], 64, kw["yoff"], torch.bfloat16), kw
        with pytest.raises(L.UwuError):
            ops.conv2d_fwd(xx, w, bias[:Cout], B, h, W, C, Cout, k, kw["stride"], kw["padding"], xoff=kw["xoff"], out=out, yoff=kw["yoff"])
        assert bool((out == SENTINEL).all()), kw
    assert not ops.conv2d_ok(1, 6, 6, 64, 64, (3, 3), dtype=torch.float16)
    assert ops.conv2d_ok(1, 6, 6, 64, 64, (3, 3)) and ops.conv2d_ok(3, 35, 35, 48, 80, (5, 5), 1, 2, dtype=torch.float32)
    assert L.load().uwu_conv2d_ws_bytes(1, 6, 6, 64, 64, 3, 3, 1, 1, 1, 64, 0, 64, 0, L.BF16) == 0


# ---------------------------------------------------------------------------------------------- stem
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_inception_stem_operand_is_exact(dtype):
    from tests import inception_oracle as io
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (2, 3, 11, 14), generator=g, dtype=torch.uint8)
    fl = torch.rand(2, 3, 11, 14, generator=g) * 1.2 - 0.1  # some outside [0, 1]
    fl[0, 0, 0, :4] = torch.tensor([float("nan"), 1.0, 0.0, 254.9 / 255])
    fl[1, 2, :8, :8] = (torch.arange(64).float() * 4 / 255).view(8, 8)  # k / 255
    k = torch.arange(256).float()
    ramp = torch.cat([k / 255, (k[:255] + 0.9) / 255, torch.ones(1)]).view(1, 1, 16, 32).expand(1, 3, 16, 32).contiguous()  # every k / 255 and
    got = ops.inception_stem(ramp.cuda(), dtype).cpu()  # (k + 0.9) / 255 through the product: k comes back as k, k + 0.9 as k (truncated)
    want = F.unfold(io.preprocess(ramp, True), 3, stride=2).transpose(1, 2).reshape(-1, 27)
    assert torch.equal(got[:, :27].double(), want)
    centre = (got[:, 4].double() * 128 + 128).view(7, 15)  # column (c = 0, ky = 1, kx = 1): pixel (2 oy + 1, 2 ox + 1)
    assert torch.equal(centre, torch.cat([k, k[:255], torch.tensor([255.0])]).view(16, 32)[1:14:2, 1:30:2].double())
    for images, normalize in ((u8, False), (fl, True)):
        pre = io.preprocess(torch.nan_to_num(images, nan=0.0) if normalize else images, normalize)  # [B, 3, H, W]
        want = F.unfold(pre, 3, stride=2).transpose(1, 2).reshape(-1, 27)  # columns (c, ky, kx), rows (b, oy, ox)
        got = ops.inception_stem(images.cuda(), dtype).cpu()
        assert got.shape == (2 * 5 * 6, 32) and got.dtype == dtype
        assert torch.equal(got[:, :27].double(), want), "the operand is exact in both dtypes: (v - 128) / 128 of an integer"
        assert not got[:, 27:].any()


# ---------------------------------------------------------------------------------------------- pools
def _check_pool(mode, B, H, W, C, dtype, x=None):
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(H * 100 + W)
    xoff, yoff = 8, 16
    x = (torch.randn(B, C, H, W, generator=g) if x is None else x).to(dtype)
    xbuf = torch.randn(B * H * W, C + 24, generator=g).to(dtype)
    xbuf[:, xoff:xoff + C] = _rows(x)
    x64 = x.double()
    ref = {"max_s2": lambda: F.max_pool2d(x64, 3, 2), "max_s1p1": lambda: F.max_pool2d(x64, 3, 1, 1),
           "avg_s1p1": lambda: F.avg_pool2d(x64, 3, 1, 1, count_include_pad=False)}[mode]()
    Ho, Wo = ref.shape[2:]
    out = torch.full((B * Ho * Wo, C + 40), SENTINEL, dtype=dtype)
    got = ops.pool2d_fwd(xbuf.cuda(), B, H, W, C, mode, xoff=xoff, out=out.cuda(), yoff=yoff).cpu()
    y = _nchw(got[:, yoff:yoff + C].double(), B, Ho, Wo)
    if mode == "avg_s1p1":  # nine fp32 additions and a division, then one rounding to the storage dtype
        mag = F.avg_pool2d(x64.abs(), 3, 1, 1, count_include_pad=False)
        bound = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23) * ref.abs() + 10 * 2.0 ** -24 * mag
        assert bool(((y - ref).abs() <= bound).all())
    else:
        assert torch.equal(y, ref)  # a maximum is one of its inputs
    assert bool((torch.cat([got[:, :yoff], got[:, yoff + C:]], 1) == SENTINEL).all())
    return y


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_pools(dtype):
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    for B, H, W, C in [(3, 7, 7, 64), (3, 6, 6, 64), (2, 7, 6, 80), (1, 147, 147, 64)]:  # 7 -> 3, 6 -> 2, 147 -> 73
        y = _check_pool("max_s2", B, H, W, C, dtype)
        assert y.shape[2:] == ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
    neg = -torch.rand(2, 64, 5, 7) - 0.5
    y = _check_pool("max_s1p1", 2, 5, 7, 64, dtype, x=neg)  # the padding never wins and is not 0
    assert float(y.max()) <= -0.5
    for B, H, W, C in [(2, 1, 1, 64), (2, 3, 3, 64), (2, 3, 5, 48), (1, 35, 35, 192)]:
        _check_pool("avg_s1p1", B, H, W, C, dtype)
    ones = _check_pool("avg_s1p1", 1, 3, 3, 64, dtype, x=torch.ones(1, 64, 3, 3))  # divisors 4 / 6 / 9: a constant stays a constant
    assert bool((ones == 1).all())
    ramp = torch.arange(9.0).view(1, 1, 3, 3).expand(1, 64, 3, 3).contiguous()
    got = _check_pool("avg_s1p1", 1, 3, 3, 64, torch.float32, x=ramp)[0, 0]
    assert torch.allclose(got, torch.tensor([[2.0, 2.5, 3.0], [3.5, 4.0, 4.5], [5.0, 5.5, 6.0]], dtype=torch.float64))
    x = torch.zeros(4, 64, device="cuda", dtype=dtype)
    with pytest.raises(L.UwuError):
        ops.pool2d_fwd(x, 1, 2, 2, 64, "max_s2")
    with pytest.raises(L.UwuError):
        ops.pool2d_fwd(x, 1, 2, 2, 60, "avg_s1p1", xoff=0)
    # the global average: fp32 [B, C], 64 additions in fp32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3 * 64, 2048, generator=g).to(dtype)
    got = ops.global_avgpool(x.cuda(), 3, 64, 2048).cpu()
    ref = x.double().view(3, 64, 2048).mean(1)
    assert got.dtype == torch.float32 and got.shape == (3, 2048)
    assert bool(((got.double() - ref).abs() <= 2.0 ** -23 * ref.abs() + 65 * 2.0 ** -24 * x.double().abs().view(3, 64, 2048).mean(1)).all())


# ---------------------------------------------------------------------------------------------- statistics
D = 2048


def _acc():
    return torch.zeros(1 + D + D * D, dtype=torch.float64, device="cuda")


def _split(acc):
    a = acc.cpu().numpy()
    return a[0], a[1:1 + D], a[1 + D:].reshape(D, D)


@pytest.fixture(scope="module")
def stats_data():
    g = torch.Generator().manual_seed(7)
    f = (torch.randn(68, D, generator=g) * torch.rand(D, generator=g) + 0.3).contiguous()
    f64 = f.double().numpy()
    return f, f64


@gpu
def test_fid_stats_accum_against_numpy_float64(stats_data):
    from uwudiff_amd import ops

    f, f64 = stats_data
    fd = f.cuda()
    runs = {}
    for parts in ([1], [3], [64], [64, 3], [3, 64], [1, 3, 64]):  # B = 1, 3, 64 alone, two updates in a row, another split of the same rows
        acc, again, row = _acc(), _acc(), 0
        for b in parts:
            ops.fid_stats_accum(fd[row:row + b].contiguous(), acc)
            ops.fid_stats_accum(fd[row:row + b].contiguous(), again)
            row += b
        assert torch.equal(acc, again), "the same batches in the same order must give the same bits"
        n, s, outer = _split(acc)
        x = f64[:row]
        assert n == row
        tol = row * 2.0 ** -50 * (np.abs(x).T @ np.abs(x))
        assert (np.abs(outer - x.T @ x) <= tol).all() and (np.abs(s - x.sum(0)) <= row * 2.0 ** -50 * np.abs(x).sum(0)).all(), parts
        runs[tuple(parts)] = (outer, tol)
    a, b = runs[(64, 3)], runs[(3, 64)]
    assert (np.abs(a[0] - b[0]) <= a[1]).all()  # different splits of the same rows agree to the same bound
    assert np.array_equal(a[0], a[0].T)  # f_i f_j and f_j f_i are the same products in the same order


@gpu
def test_fid_stats_covariance_under_cancellation():
    """features of mean 1 and spread 1e-3: cov = (outer - n mu mu^T) / (n - 1) cancels six digits.  outer / n is about 1 and is held to
    n 2^-50 relative by the test above, n mu mu^T likewise; so the covariance (about 1e-6) is held to 4 n 2^-50 absolute."""
    from uwudiff_amd import ops
    from uwudiff_amd.metrics import moments_from_sums

    g = torch.Generator().manual_seed(11)
    n = 64
    f = (1 + 1e-3 * torch.randn(n, D, generator=g)).contiguous()
    acc = _acc()
    ops.fid_stats_accum(f[:40].cuda().contiguous(), acc)
    ops.fid_stats_accum(f[40:].cuda().contiguous(), acc)
    host = acc.cpu()
    mean, cov = moments_from_sums(int(host[0]), host[1:1 + D], host[1 + D:].view(D, D))
    ref = np.cov(f.double().numpy().T)
    err = np.abs(cov.numpy() - ref).max()
    print(f"[fid stats] covariance under cancellation: max |err| = {err:.3e} (entries about {np.abs(ref).max():.1e}, bound {4 * n * 2.0 ** -50:.1e})")
    assert err <= 4 * n * 2.0 ** -50
    assert np.abs(mean.numpy() - f.double().numpy().mean(0)).max() <= 2.0 ** -50


@gpu
def test_fid_stats_refusals():
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    with pytest.raises(L.UwuError):
        ops.fid_stats_accum(torch.zeros(2, D, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"))
    with pytest.raises(L.UwuError):
        ops.fid_stats_accum(torch.zeros(2, 100, device="cuda"), torch.zeros(1 + 100 + 100 * 100, dtype=torch.float64, device="cuda"))
    with pytest.raises(L.UwuError):
        ops.fid_stats_accum(torch.zeros(2, D, device="cuda", dtype=torch.bfloat16), _acc())
