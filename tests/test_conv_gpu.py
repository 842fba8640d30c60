"""Implicit-GEMM 3x3 convolution (uwu_conv3x3_fwd / _dgrad / _wgrad; the UNet resblock / down-sample / up-sample convs,
reference src/duwu/modules/unet_patch.py:13-57 -> diffusers Conv2d) against torch.nn.functional.conv2d on the CPU.

Integer-valued bf16 operands make the comparison EXACT (every product and partial sum is an integer the fp32 accumulator
holds): a wrong tap offset, padding row, stride rule, channel-chunk order or K-slice shows up as a wrong integer.

Four groups of cases:
  CASES     the first seven shapes (powers of two, at most 12 workgroups), with their original data
  OFFGRID   widths and image sizes that are not powers of two (divmod24's reciprocal is inexact, a 256-row tile starts in
            the middle of an image row), odd sides under stride 2, GEMM row counts that are no multiple of the tile,
            1 x 1 and 3-row images, and one case next to the 2^24-row limit
  SDXL      the UNet's own convolutions at 4 x 128 x 128 latents, with the batch that reaches each path of the weight
            gradient's dispatch (K slices, tile orientation, XCD partition) and several rounds of workgroups per launch
  REAL      randn data against an fp64 reference with a derived bound, all three directions
plus direct calls of the C ABI for what ops.py never does (guard rows, no scratch, NULL bias / db, refusals), and one
test without the gpu marker that checks the case list itself."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
ARGS = "B,H,W,C,Cout,stride"

CASES = [  # B, H, W, C, Cout, stride
    (2, 8, 8, 32, 32, 1),
    (1, 16, 16, 64, 96, 1),
    (3, 8, 16, 32, 64, 1),      # H != W, M = 384 (not a multiple of the 256-row tile)
    (2, 16, 16, 64, 64, 2),
    (1, 32, 32, 320, 320, 1),   # SDXL level-0 width: 5 channel chunks of 64, Cout = 2.5 column tiles
    (2, 16, 16, 320, 640, 2),   # SDXL down-sample
    (1, 8, 8, 1280, 1280, 1),
]

OFFGRID = [
    (2, 12, 12, 32, 32, 1),     # W = 12, H*W = 144: inexact reciprocal; a 256-row tile starts mid-row and mid-image
    (1, 24, 24, 64, 96, 1),     # W = 24
    (1, 20, 24, 96, 64, 1),     # H != W, H*W = 480, C = 96 (three 32-chunks)
    (2, 24, 24, 64, 64, 2),     # stride 2, Wo = 12
    (1, 96, 96, 32, 32, 2),     # W = 96 in, Wo = 48 out; dgrad rows = 9216
    (32, 7, 7, 32, 64, 2),      # odd sides under stride 2 (Ho = Wo = 4); dgrad M = 1568, not a multiple of 256
    (8, 7, 9, 64, 32, 2),       # odd, H != W (4 x 5 out, Mo = 160); dgrad M = 504, not a multiple of 32
    (4, 3, 8, 32, 32, 1),       # H = 3: every pixel touches a padded row or is the centre row
    (32, 1, 1, 32, 32, 1),      # 1 x 1 image: only the centre tap is inside
    (32, 1, 1, 32, 32, 2),
    (2, 16, 16, 32, 1280, 1),   # wgrad with more row tiles than column tiles (part_m)
]
# 11 520 000 rows, near the 2^24 limit: 2779 rows (pixel 479 of an image, each in a different tile) need divmod24's
# correction; 737 MB per activation tensor, 45 000 workgroups, wgrad K = 11.5 M.  One test of its own (memory).
NEAR_LIMIT = (24000, 20, 24, 32, 32, 1)

# case -> K slices of the weight gradient (both tile orientations give the same count for every one of these)
SDXL = {
    (1, 128, 128, 320, 320, 1): 8,     # level 0; 192 workgroups; wgrad 8 slices x 64 steps
    (4, 128, 128, 320, 320, 2): 8,     # down-sample; dgrad 768 workgroups (more than one round of the chip)
    (1, 64, 64, 640, 640, 1): 4,       # wgrad 115 tiles: 4 slices, xs = 4, 32 steps per slice
    (1, 64, 64, 960, 640, 1): 2,       # wgrad 170 tiles: 2 slices; C = 960
    (1, 64, 64, 1920, 640, 1): 1,      # wgrad 340 tiles: 1 slice, 128 x 256 orientation; C = 1920
    (4, 32, 32, 640, 1280, 1): 2,      # wgrad tall, 2 slices of 64 steps
    (1, 32, 32, 2560, 1280, 1): 1,     # wgrad tall, 900 tiles; K = 23040 in forward
    (12, 128, 128, 320, 320, 1): 8,    # benchmark batch: 2304 workgroups; wgrad 8 slices x 768 steps
    (12, 64, 64, 1280, 1280, 1): 8,    # wgrad tall with 8 slices of 192 steps; 1920 workgroups forward
}
THIN = OFFGRID + list(SDXL)

REAL = [
    (1, 24, 24, 96, 64, 1),
    (8, 7, 9, 64, 32, 2),
    (1, 64, 64, 640, 640, 1),
    (1, 32, 32, 2560, 1280, 1),
    (4, 128, 128, 320, 320, 2),
]

REFUSED = [  # shapes the implicit kernels do not take
    (1, 7, 9, 32, 32, 2),     # B Ho Wo = 20, not a multiple of 32
    (2, 8, 8, 48, 32, 1),     # C not a multiple of 32
    (2, 8, 8, 32, 48, 1),     # Cout not a multiple of 32
    (2, 8, 8, 0, 32, 1),      # C = 0
    (2, 10, 10, 32, 32, 3),   # stride 3 (B Ho Wo = 32: the stride is the only reason)
    (2, 0, 8, 32, 32, 1),     # H = 0 (B Ho Wo = 0 is a multiple of 32)
]

BF16_NAN, F32_NAN = 0x7FC1, 0x7FC00001  # sentinel bit patterns (as int16 / int32) for memory no kernel may touch


def _data(B, H, W, C, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    w = torch.randint(-1, 2, (Cout, C, 3, 3), generator=g).float()
    keep = torch.rand(Cout, C, 3, 3, generator=g) < 0.25  # sparse weights keep the sums small enough for bf16
    w = w * keep
    bias = torch.randint(-3, 4, (Cout,), generator=g).float()
    return x, w, bias


def _cl(t):  # NCHW -> [B*H*W, C] channels-last bf16 on the device
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().bfloat16().cuda()


def _wk(w):  # [Cout, C, 3, 3] -> [Cout, 9*C] tap-major (this build's parameter layout)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _out(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ---- data of the OFFGRID / SDXL groups: exact for any K, every K index checked -------------------------------------------
def _seed(B, H, W, C, Cout, stride):
    return 100003 * B + 1009 * H + 101 * W + 7 * C + 3 * Cout + stride


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).float()


def _thin_w(Cout, C, n, g):
    """+-1 weights of density min(0.25, 512 / n), n = length of the sum they enter: about 512 non-zero terms of
    magnitude <= 2 per output, so |output| stays below 256 (where bf16 stops holding every integer) at any C.  Thinning
    leaves some (co, tap) rows and (tap, c) columns empty (at C = 32, Cout = 1280 about one row in 10^4): each gets one
    +-1 entry, so that no K index of forward (tap, c) or dgrad (tap, co) goes unchecked."""
    p = min(0.25, 512.0 / n)
    sign = torch.randint(0, 2, (Cout, C, 3, 3), generator=g, dtype=torch.int8) * 2 - 1
    w = (sign * (torch.rand(Cout, C, 3, 3, generator=g) < p)).float()
    wt = w.view(Cout, C, 9)
    co, tap = torch.nonzero(wt.abs().sum(1) == 0, as_tuple=True)
    wt[co, (co + tap) % C, tap] = (1 - 2 * ((co + tap) % 2)).float()
    c, tap = torch.nonzero(wt.abs().sum(0) == 0, as_tuple=True)
    wt[(c + tap) % Cout, c, tap] = (1 - 2 * ((c + tap) % 2)).float()
    return w


def _assert_covering(w):
    assert bool((w != 0).any(dim=1).all()), "a (co, tap) weight row is empty: that K index of dgrad goes unchecked"
    assert bool((w != 0).any(dim=0).all()), "a (tap, c) weight column is empty: that K index of forward goes unchecked"


def _fwd_ref(B, H, W, C, Cout, stride):
    g = torch.Generator().manual_seed(_seed(B, H, W, C, Cout, stride))
    x = _ints(-2, 2, (B, C, H, W), g)
    w = _thin_w(Cout, C, 9 * C, g)
    bias = _ints(-3, 3, (Cout,), g)
    _assert_covering(w)
    want = F.conv2d(x, w, bias, stride=stride, padding=1)
    assert want.abs().max().item() <= 256, "forward reference leaves the range bf16 holds exactly"
    return x, w, bias, want.permute(0, 2, 3, 1).reshape(-1, Cout)


def _dgrad_ref(B, H, W, C, Cout, stride):
    g = torch.Generator().manual_seed(_seed(B, H, W, C, Cout, stride) + 1)
    Ho, Wo = _out(H, W, stride)
    dy = _ints(-2, 2, (B, Cout, Ho, Wo), g)
    w = _thin_w(Cout, C, 9 * Cout, g)
    _assert_covering(w)
    want = torch.nn.grad.conv2d_input((B, C, H, W), w, dy, stride=stride, padding=1)
    assert want.abs().max().item() <= 256, "dgrad reference leaves the range bf16 holds exactly"
    return dy, w, want.permute(0, 2, 3, 1).reshape(-1, C)


def _wgrad_ref(B, H, W, C, Cout, stride):
    g = torch.Generator().manual_seed(_seed(B, H, W, C, Cout, stride) + 2)
    Ho, Wo = _out(H, W, stride)
    x = _ints(-2, 2, (B, C, H, W), g)
    dy = _ints(-1, 1, (B, Cout, Ho, Wo), g)
    dw = torch.nn.grad.conv2d_weight(x, (Cout, C, 3, 3), dy, stride=stride, padding=1)
    db = dy.sum(dim=(0, 2, 3))
    assert dw.abs().max().item() + 1 < 2 ** 24 and db.abs().max().item() + 2 < 2 ** 24, "wgrad reference is not exact in fp32"
    return dy, x, _wk(dw), db


def _same(got, want, what):
    """torch.equal with a message that says where and how much: which rows, the first wrong value."""
    got, want = got.float().cpu(), want.float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        r, c = bad[0].tolist() if bad.shape[1] == 2 else (bad[0].item(), 0)
        rows = torch.unique(bad[:, 0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, in {rows.numel()} rows "
                             f"(first rows {rows[:8].tolist()}, last {rows[-1].item()}); first at ({r}, {c}): "
                             f"got {got[r][c].item() if got.dim() == 2 else got[r].item()}, "
                             f"want {want[r][c].item() if want.dim() == 2 else want[r].item()}")


def _wgrad_scratch(C, Cout, Mo):
    from uwudiff_amd import lib as L

    need = L.load().uwu_conv3x3_wgrad_scratch_bytes(C, Cout, Mo)
    return need, torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")


# ---- the first seven cases, unchanged -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize(ARGS, CASES)
def test_conv3x3_fwd_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    x, w, bias = _data(B, H, W, C, Cout, seed=B + C)
    xd = _cl(x)
    assert ops.conv3x3_implicit_ok(xd, B, H, W, C, Cout, stride)
    y = ops.conv3x3_fwd(xd, _wk(w).bfloat16().cuda(), bias.cuda(), B, H, W, C, Cout, stride)
    want = F.conv2d(x, w, bias, stride=stride, padding=1)
    want = want.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert torch.equal(y.float().cpu(), want.bfloat16().float())


@gpu
@pytest.mark.parametrize(ARGS, CASES)
def test_conv3x3_dgrad_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    x, w, _ = _data(B, H, W, C, Cout, seed=7 + C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator().manual_seed(3)
    dy = torch.randint(-2, 3, (B, Cout, Ho, Wo), generator=g).float()
    xr = x.clone().requires_grad_(True)
    F.conv2d(xr, w, None, stride=stride, padding=1).backward(dy)
    dx = ops.conv3x3_dgrad(_cl(dy), _wk(w).bfloat16().cuda(), B, H, W, C, Cout, stride)
    want = xr.grad.permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(dx.float().cpu(), want.bfloat16().float())


@gpu
@pytest.mark.parametrize(ARGS, CASES)
def test_conv3x3_wgrad_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    x, w, _ = _data(B, H, W, C, Cout, seed=11 + C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator().manual_seed(5)
    dy = torch.randint(-1, 2, (B, Cout, Ho, Wo), generator=g).float()
    wr = w.clone().requires_grad_(True)
    br = torch.zeros(Cout, requires_grad=True)
    F.conv2d(x, wr, br, stride=stride, padding=1).backward(dy)
    dw = torch.ones(Cout, 9 * C, device="cuda")   # accumulates on top of existing contents
    db = torch.full((Cout,), 2.0, device="cuda")
    ops.conv3x3_wgrad(_cl(dy), _cl(x), dw, db, B, H, W, C, Cout, stride)
    assert torch.equal(dw.cpu(), _wk(wr.grad) + 1.0)
    assert torch.equal(db.cpu(), br.grad + 2.0)


@gpu
def test_conv3x3_random_close_and_fallback_rule():
    from uwudiff_amd import ops

    torch.manual_seed(0)
    B, H, W, C, Cout = 2, 32, 32, 320, 320
    x, w, bias = torch.randn(B, C, H, W), torch.randn(Cout, C, 3, 3) * 0.02, torch.randn(Cout)
    y = ops.conv3x3_fwd(_cl(x), _wk(w).bfloat16().cuda(), bias.cuda(), B, H, W, C, Cout, 1)
    want = F.conv2d(x.bfloat16().float(), w.bfloat16().float(), bias, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    torch.testing.assert_close(y.float().cpu(), want, rtol=2e-2, atol=2e-2)
    xd = _cl(x)
    assert not ops.conv3x3_implicit_ok(xd, B, H, W, 8, 320, 1)         # conv_in: 4 -> padded 8 channels
    assert not ops.conv3x3_implicit_ok(xd.float(), B, H, W, C, Cout, 1)  # fp32 parity mode keeps im2col + exact-fp32 MFMA


# ---- A. exact integer cases off the 2^n grid and at the UNet's shapes ---------------------------------------------------
def _run_fwd_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    x, w, bias, want = _fwd_ref(B, H, W, C, Cout, stride)
    xd = _cl(x)
    del x
    assert ops.conv3x3_implicit_ok(xd, B, H, W, C, Cout, stride)
    y = ops.conv3x3_fwd(xd, _wk(w).bfloat16().cuda(), bias.cuda(), B, H, W, C, Cout, stride)
    _same(y, want, "y")


def _run_dgrad_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    dy, w, want = _dgrad_ref(B, H, W, C, Cout, stride)
    dyd = _cl(dy)
    del dy
    dx = ops.conv3x3_dgrad(dyd, _wk(w).bfloat16().cuda(), B, H, W, C, Cout, stride)
    _same(dx, want, "dx")


def _run_wgrad_exact(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    dy, x, want_dw, want_db = _wgrad_ref(B, H, W, C, Cout, stride)
    dyd, xd = _cl(dy), _cl(x)
    del dy, x
    dw = torch.ones(Cout, 9 * C, device="cuda")   # accumulates on top of existing contents
    db = torch.full((Cout,), 2.0, device="cuda")
    ops.conv3x3_wgrad(dyd, xd, dw, db, B, H, W, C, Cout, stride)
    _same(dw, want_dw + 1.0, "dw")
    _same(db, want_db + 2.0, "db")


@gpu
@pytest.mark.parametrize(ARGS, THIN)
def test_conv3x3_fwd_exact_shapes(B, H, W, C, Cout, stride):
    _run_fwd_exact(B, H, W, C, Cout, stride)


@gpu
@pytest.mark.parametrize(ARGS, THIN)
def test_conv3x3_dgrad_exact_shapes(B, H, W, C, Cout, stride):
    _run_dgrad_exact(B, H, W, C, Cout, stride)


@gpu
@pytest.mark.parametrize(ARGS, THIN)
def test_conv3x3_wgrad_exact_shapes(B, H, W, C, Cout, stride):
    from uwudiff_amd import lib as L

    case = (B, H, W, C, Cout, stride)
    if case in SDXL:
        # The slice count is what puts the case on its path of launch_tr.  If a retuning of tr_split moves it, this line
        # fails: pick a new shape for the path then.  Exact where only the streaming kernel can ask for scratch; where
        # 9 C or Cout is a multiple of 384 the function may return the larger need of the 384-wide kernels, so only >=
        # can be asserted there (a weaker guard).
        Ho, Wo = _out(H, W, stride)
        need = L.load().uwu_conv3x3_wgrad_scratch_bytes(C, Cout, B * Ho * Wo)
        slices = SDXL[case] * Cout * 9 * C * 4
        if (9 * C) % 384 and Cout % 384:
            assert need == slices, (need, slices)
        else:
            assert need >= slices, (need, slices)
    _run_wgrad_exact(B, H, W, C, Cout, stride)


@gpu
def test_conv3x3_near_row_limit_exact():
    """All three directions on 11.52 M rows (the limit is 2^24 - 1): divmod24's correction branch runs on the device
    (divisor 480, rows from 10 186 559 on), and so does the 64-bit address arithmetic (737 MB per activation tensor).
    Exact equality over every row is the check; one direction at a time, each freed before the next."""
    import gc

    for run in (_run_fwd_exact, _run_dgrad_exact, _run_wgrad_exact):
        run(*NEAR_LIMIT)
        gc.collect()
        torch.cuda.empty_cache()


# ---- B. what ops.py never does: the C ABI called directly ----------------------------------------------------------------
def _sentinel(rows, cols, dtype):
    t = torch.empty(rows, cols, dtype=dtype, device="cuda")
    if dtype == torch.bfloat16:
        t.view(torch.int16).fill_(BF16_NAN)
    else:
        t.view(torch.int32).fill_(F32_NAN)
    return t


def _untouched(t):
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == BF16_NAN).all())
    return bool((t.view(torch.int32) == F32_NAN).all())


@gpu
@pytest.mark.parametrize(ARGS, [(3, 8, 16, 32, 64, 1), (8, 7, 9, 64, 32, 2), (2, 12, 12, 32, 32, 1)])
def test_conv3x3_guard_rows(B, H, W, C, Cout, stride):
    """M is not a multiple of the 256-row tile (nor Cout / 9 C of the weight gradient's): the rows behind the result
    must come back bit-identical."""
    from uwudiff_amd import lib as L

    Ho, Wo = _out(H, W, stride)
    Mo, Mi = B * Ho * Wo, B * H * W
    x, w, bias, want = _fwd_ref(B, H, W, C, Cout, stride)
    y = _sentinel(Mo + 256, Cout, torch.bfloat16)
    xd, wd, bd = _cl(x), _wk(w).bfloat16().cuda(), bias.cuda()  # (named: L.ptr keeps no reference to its tensor)
    L.call("uwu_conv3x3_fwd", L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(y), B, H, W, C, Cout, stride, L.BF16, L.stream())
    _same(y[:Mo], want, "y")
    assert _untouched(y[Mo:]), "forward wrote behind its last row"

    dy, w, want = _dgrad_ref(B, H, W, C, Cout, stride)
    dx = _sentinel(Mi + 256, C, torch.bfloat16)
    dyd, wd = _cl(dy), _wk(w).bfloat16().cuda()
    L.call("uwu_conv3x3_dgrad", L.ptr(dyd), L.ptr(wd), L.ptr(dx), B, H, W, C, Cout, stride, L.BF16, L.stream())
    _same(dx[:Mi], want, "dx")
    assert _untouched(dx[Mi:]), "dgrad wrote behind its last row"

    dy, x, want_dw, want_db = _wgrad_ref(B, H, W, C, Cout, stride)
    dw = _sentinel(Cout + 64, 9 * C, torch.float32)
    dw[:Cout] = 1.0
    db = torch.full((Cout,), 2.0, device="cuda")
    need, sc = _wgrad_scratch(C, Cout, Mo)
    dyd, xd = _cl(dy), _cl(x)
    L.call("uwu_conv3x3_wgrad", L.ptr(dyd), L.ptr(xd), L.ptr(dw), L.ptr(db), B, H, W, C, Cout, stride, L.BF16, L.ptr(sc), need,
           L.stream())
    _same(dw[:Cout], want_dw + 1.0, "dw")
    _same(db, want_db + 2.0, "db")
    assert _untouched(dw[Cout:]), "wgrad wrote behind its last row"


@gpu
@pytest.mark.parametrize(ARGS, [(1, 32, 32, 320, 320, 1), (1, 64, 64, 640, 640, 1)])
def test_conv3x3_wgrad_without_scratch(B, H, W, C, Cout, stride):
    """scratch = NULL and a scratch one byte too small take the atomic path: same integers as the scratch path.
    db = NULL leaves dw as it is with db."""
    from uwudiff_amd import lib as L

    Ho, Wo = _out(H, W, stride)
    dy, x, want_dw, want_db = _wgrad_ref(B, H, W, C, Cout, stride)
    dyd, xd = _cl(dy), _cl(x)
    need, sc = _wgrad_scratch(C, Cout, B * Ho * Wo)
    assert need > 1

    def run(scratch, nbytes, with_db=True):
        dw = torch.ones(Cout, 9 * C, device="cuda")
        db = torch.full((Cout,), 2.0, device="cuda") if with_db else None
        L.call("uwu_conv3x3_wgrad", L.ptr(dyd), L.ptr(xd), L.ptr(dw), L.ptr(db), B, H, W, C, Cout, stride, L.BF16,
               L.ptr(scratch), nbytes, L.stream())
        return dw, db

    for what, (scratch, nbytes) in {"scratch": (sc, need), "NULL": (None, 0), "one byte short": (sc, need - 1)}.items():
        dw, db = run(scratch, nbytes)
        _same(dw, want_dw + 1.0, f"dw ({what})")
        _same(db, want_db + 2.0, f"db ({what})")
    for what, (scratch, nbytes) in {"scratch": (sc, need), "NULL": (None, 0)}.items():
        dw, _ = run(scratch, nbytes, with_db=False)
        _same(dw, want_dw + 1.0, f"dw (db = NULL, {what})")


@gpu
@pytest.mark.parametrize(ARGS, [(2, 12, 12, 32, 32, 1), (1, 32, 32, 320, 320, 1)])
def test_conv3x3_fwd_without_bias(B, H, W, C, Cout, stride):
    from uwudiff_amd import lib as L

    x, w, bias, want = _fwd_ref(B, H, W, C, Cout, stride)
    Ho, Wo = _out(H, W, stride)
    y = torch.empty(B * Ho * Wo, Cout, dtype=torch.bfloat16, device="cuda")
    xd, wd = _cl(x), _wk(w).bfloat16().cuda()
    L.call("uwu_conv3x3_fwd", L.ptr(xd), L.ptr(wd), None, L.ptr(y), B, H, W, C, Cout, stride, L.BF16, L.stream())
    _same(y, want - bias[None, :], "y (bias = NULL)")


@gpu
def test_conv3x3_refusals():
    """Shapes and operands the implicit kernels do not take: each entry point answers with a UwuError that names it and
    launches nothing (the outputs keep their sentinel), and conv3x3_implicit_ok says no to the same shapes."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    n = 1 << 18  # far more than any of the shapes below would touch
    a, b = torch.zeros(n, dtype=torch.bfloat16, device="cuda"), torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(n, device="cuda")
    out16, out32, outb = _sentinel(1, n, torch.bfloat16), _sentinel(1, n, torch.float32), _sentinel(1, n, torch.float32)
    sc = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def calls(shape, dtype=L.BF16, off=None):
        o = lambda k: 8 if off == k else 0  # noqa: E731
        yield "conv3x3_fwd", lambda: L.call("uwu_conv3x3_fwd", a.data_ptr() + o(0), b.data_ptr() + o(1), f.data_ptr() + o(3),
                                            out16.data_ptr() + o(2), *shape, dtype, L.stream())
        yield "conv3x3_dgrad", lambda: L.call("uwu_conv3x3_dgrad", a.data_ptr() + o(0), b.data_ptr() + o(1),
                                              out16.data_ptr() + o(2), *shape, dtype, L.stream())
        yield "conv3x3_wgrad", lambda: L.call("uwu_conv3x3_wgrad", a.data_ptr() + o(0), b.data_ptr() + o(1),
                                              out32.data_ptr() + o(2), outb.data_ptr(), *shape, dtype, sc.data_ptr(),
                                              sc.numel(), L.stream())

    def refused(shape, dtype=L.BF16, off=None):
        for name, fn in calls(shape, dtype, off):
            if off == 3 and name != "conv3x3_fwd":
                continue  # the fourth operand (bias) exists in forward only
            with pytest.raises(L.UwuError) as e:
                fn()
            text = str(e.value)
            assert name + ":" in text[text.index("):"):], (name, shape, off, text)  # the library's own message names it
        torch.cuda.synchronize()
        assert _untouched(out16) and _untouched(out32) and _untouched(outb), (shape, dtype, off)

    for shape in REFUSED:
        refused(shape)
        assert not ops.conv3x3_implicit_ok(a, *shape), shape
    ok = (2, 8, 8, 32, 32, 1)
    assert ops.conv3x3_implicit_ok(a, *ok)
    refused(ok, dtype=L.F32)
    assert not ops.conv3x3_implicit_ok(f, *ok)
    for off in range(4):  # one operand 8 bytes off the 16-byte alignment, each in turn
        refused(ok, off=off)


# ---- C. real-valued data against fp64, all three directions --------------------------------------------------------------
def _real(B, H, W, C, Cout, stride):
    """randn activations and gradients, weights randn / sqrt(9 C), each rounded to bf16 once (returned as fp64)."""
    g = torch.Generator().manual_seed(_seed(B, H, W, C, Cout, stride) + 3)
    Ho, Wo = _out(H, W, stride)
    r = lambda t: t.bfloat16().double()  # noqa: E731
    x = r(torch.randn(B, C, H, W, generator=g))
    w = r(torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5)
    dy = r(torch.randn(B, Cout, Ho, Wo, generator=g))
    return x, w, dy


def _within(got, ref, S, n, eps_out, what):
    """|got - ref| <= eps_out |ref| + n 2^-24 S, every element.  eps_out: one rounding of the result (2^-8 for bf16: half
    an ulp is 2^-9, the factor 2 leaves the tie cases room; 2^-23 for fp32).  n 2^-24 S is the any-order bound n u S of an
    fp32 accumulation of n terms whose absolute values sum to S, with u = 2^-24 taken twice the round-to-nearest
    constant so that an accumulator that truncates is covered too."""
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = eps_out * ref.abs() + n * 2.0 ** -24 * S
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"[conv3x3 real] {what}: worst |got - ref| / bound = {ratio:.4f} (max err {err.max().item():.3e})")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (what, ratio)
    return ratio


@gpu
@pytest.mark.parametrize(ARGS, REAL)
def test_conv3x3_real_fwd_fp64_bound(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    x, w, _ = _real(B, H, W, C, Cout, stride)
    y = ops.conv3x3_fwd(_cl(x), _wk(w).bfloat16().cuda(), None, B, H, W, C, Cout, stride)
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)  # noqa: E731
    ref = cl(F.conv2d(x, w, None, stride=stride, padding=1))
    S = cl(F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=1))
    _within(y, ref, S, 9 * C, 2.0 ** -8, f"y {(B, H, W, C, Cout, stride)}")


@gpu
@pytest.mark.parametrize(ARGS, REAL)
def test_conv3x3_real_dgrad_fp64_bound(B, H, W, C, Cout, stride):
    from uwudiff_amd import ops

    _, w, dy = _real(B, H, W, C, Cout, stride)
    dx = ops.conv3x3_dgrad(_cl(dy), _wk(w).bfloat16().cuda(), B, H, W, C, Cout, stride)
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)  # noqa: E731
    ref = cl(torch.nn.grad.conv2d_input((B, C, H, W), w, dy, stride=stride, padding=1))
    S = cl(torch.nn.grad.conv2d_input((B, C, H, W), w.abs(), dy.abs(), stride=stride, padding=1))
    _within(dx, ref, S, 9 * Cout, 2.0 ** -8, f"dx {(B, H, W, C, Cout, stride)}")


@gpu
@pytest.mark.parametrize(ARGS, REAL)
def test_conv3x3_real_wgrad_fp64_bound(B, H, W, C, Cout, stride):
    """dw, db from zero against fp64; and with scratch the split-K reduce has a fixed order: two calls from the same
    initial dw give the same dw bits.  (db: the K slices add their column sums with fp32 atomics, in no fixed order, so
    on real data db is held to the fp64 bound only; on integers it is exact, see the *_exact tests.)"""
    from uwudiff_amd import lib as L

    x, _, dy = _real(B, H, W, C, Cout, stride)
    Ho, Wo = _out(H, W, stride)
    Mo = B * Ho * Wo
    dyd, xd = _cl(dy), _cl(x)
    need, sc = _wgrad_scratch(C, Cout, Mo)
    outs = []
    for _ in range(2):
        dw, db = torch.zeros(Cout, 9 * C, device="cuda"), torch.zeros(Cout, device="cuda")
        L.call("uwu_conv3x3_wgrad", L.ptr(dyd), L.ptr(xd), L.ptr(dw), L.ptr(db), B, H, W, C, Cout, stride, L.BF16, L.ptr(sc),
               need, L.stream())
        outs.append((dw, db))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), "dw differs between two identical calls"
    ref = _wk(torch.nn.grad.conv2d_weight(x, (Cout, C, 3, 3), dy, stride=stride, padding=1))
    S = _wk(torch.nn.grad.conv2d_weight(x.abs(), (Cout, C, 3, 3), dy.abs(), stride=stride, padding=1))
    _within(outs[0][0], ref, S, Mo, 2.0 ** -23, f"dw {(B, H, W, C, Cout, stride)}")
    _within(outs[0][1], dy.sum(dim=(0, 2, 3)), dy.abs().sum(dim=(0, 2, 3)), Mo, 2.0 ** -23, f"db {(B, H, W, C, Cout, stride)}")


# ---- D. the case list itself, without a GPU ------------------------------------------------------------------------------
def test_conv3x3_case_list_is_sound():
    """What the GPU tests rely on, checked where there is no GPU: every case is one the implicit kernels accept
    (B Ho Wo a multiple of 32, channels multiples of 32, fewer than 2^24 rows), and the OFFGRID data are exact in bf16 /
    fp32 and leave no weight row or column empty (the _*_ref helpers assert that; the near-limit case is too large to
    compute here and is checked by arithmetic only)."""
    from uwudiff_amd import lib as L

    ok = L.load().uwu_conv3x3_implicit_ok  # host code only
    every = CASES + OFFGRID + [NEAR_LIMIT] + list(SDXL) + REAL
    assert not any(ok(*shape, L.BF16) for shape in REFUSED) and not ok(*CASES[0], L.F32)
    for B, H, W, C, Cout, stride in every:
        assert ok(B, H, W, C, Cout, stride, L.BF16), (B, H, W, C, Cout, stride)
        Ho, Wo = _out(H, W, stride)
        assert (B * Ho * Wo) % 32 == 0, (B, H, W, C, Cout, stride)
        assert C % 32 == 0 and Cout % 32 == 0 and C >= 32 and Cout >= 32 and stride in (1, 2)
        assert B * H * W < 2 ** 24 and B * Ho * Wo < 2 ** 24 and 9 * C < 2 ** 24
    assert len(set(every[:-len(REAL)])) == len(every) - len(REAL), "a case is listed twice"
    B, H, W, C, Cout, stride = NEAR_LIMIT
    # rows past 10 186 559 with divisor 480 are where the rounded reciprocal is one too high; one tensor is 737 MB
    assert H * W == 480 and 10_186_559 + 480 * 1000 < B * H * W == 11_520_000 and B * H * W * C * 2 > 700e6
    for case in OFFGRID:
        _, _, _, y = _fwd_ref(*case)
        _, _, dx = _dgrad_ref(*case)
        _, _, dw, db = _wgrad_ref(*case)
        B, H, W, C, Cout, stride = case
        Ho, Wo = _out(H, W, stride)
        assert y.shape == (B * Ho * Wo, Cout) and dx.shape == (B * H * W, C) and dw.shape == (Cout, 9 * C) and db.shape == (Cout,)
