"""The fp8 operand chain of BASELINE config 5 per code, per boundary and per ragged tile, against tests/fp8_oracle.py.

Every case calls the C ABI directly with leading dimensions over the row length and guard rows; padding and guards hold a
sentinel that must survive bit for bit.  Bytes are compared through the oracle's canon(): the two zero codes are one, NaN is
"decodes to NaN".

  1  quantiser      every finite code, every tie, both neighbours of every tie, +-0, below half the smallest subnormal, +-max,
                    the next float above it, +-inf -- in a [401, 67] matrix (row length coprime to 8, ragged on both tiles), four
                    scales, fp32 and bf16 input, both images from one call; a planted NaN stays NaN
  2  quantiser      ragged shapes, integer data: bytes, amax and twice-accumulated column sums are exact
  3  amax           off the 8-grid, through the unrolled loop, the maximum in every stream; Inf -> inf, NaN not recorded
  4  update_scales  the stored scale is the fp32 quotient where that is finite and positive, else the previous scale, else 1
  5  GEMM decode    one non-zero byte per row (every finite code, every k residue mod 128, every K step) against a dense
                    operand: each output is ONE exact product; both kernels (named by uwu_gemm_last_kernel), both sides, the
                    weight-gradient form on both kernels at a shape each takes; NaN / Inf codes
  6  emitting GEMM  saturated GELU block bit for bit, moderate values by the band rule below, a NaN code stays NaN
  7  LayerNorm emitter  the band rule against float64 on the stored residual sum, a NaN row stays NaN

Band rule (6, 7): a byte may differ from the RNE of the float64 value by one code only, and then the float64 value lies within
4 * E32 of a rounding boundary; E32 = max |the same formula in torch fp32 on the CPU - float64| (times q_scale), 4 the margin of
the epilogue, LayerNorm and attention suites.  By the reference alone fewer than 1 % of the elements lie in that band (asserted).
The worst observed ratios and the bytes the hardware gives for NaN and negative underflow: profiles/fp8_chain_mi355x.txt
(every test prints them, "[fp8-chain] ...", pytest -s).
"""
import pytest
import torch

from tests import fp8_oracle as O
from tests import gemm_oracle as G
from tests import layernorm_oracle as LN

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
FMTS = [O.E4M3, O.E5M2]
S8 = 0xA5         # sentinel byte of the fp8 images
SF = -777.0       # sentinel of float buffers
XPAD = 1.0e30     # padding of the quantiser's input: a read past K would show in amax and the column sums
GUARD = 2
MARGIN = 4.0
DT = {F32: "fp32", BF16: "bf16"}


def _L():
    from uwudiff_amd import lib as L
    return L


def place(t, ld, fill, guard=GUARD):
    """[rows, n] -> device [rows + guard, ld] with padding columns and guard rows holding `fill`."""
    buf = torch.full((t.shape[0] + guard, ld), fill, dtype=t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


def blank(rows, cols, ld, fill, dtype, guard=GUARD):
    return torch.full((rows + guard, ld), fill, dtype=dtype, device="cuda")


def inside(buf, rows, cols, fill, what):
    """The [rows, cols] corner on the CPU after checking that everything else still holds the sentinel."""
    b = buf.cpu()
    f = torch.full((), fill, dtype=b.dtype)
    assert bool((b[rows:] == f).all()), f"{what}: wrote past row {rows}"
    assert bool((b[:rows, cols:] == f).all()), f"{what}: wrote past column {cols}"
    return b[:rows, :cols].contiguous()


def scalar(v):
    return torch.tensor([v], dtype=F32, device="cuda")


def quantize(x, M, K, s, fmt, ldo, ldt, amax=None, colsum=None):
    """One uwu_fp8_quantize call on a placed x -> (out [M, K], out_t [K, M]) on the CPU, guards checked."""
    L = _L()
    out, out_t = blank(M, K, ldo, S8, torch.uint8), blank(K, M, ldt, S8, torch.uint8)
    sd = scalar(s)  # (alive until the kernel has run)
    L.call("uwu_fp8_quantize", L.ptr(x), L.dt(x), M, K, x.shape[1], L.ptr(sd), fmt, L.ptr(out), ldo, L.ptr(out_t), ldt,
           L.ptr(amax), L.ptr(colsum), L.stream())
    torch.cuda.synchronize()
    return inside(out, M, K, S8, "out"), inside(out_t, K, M, S8, "out_t")


# ------------------------------------------------------------------------------------------------- 1  every code and boundary
@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT.get)
@pytest.mark.parametrize("fmt", FMTS, ids=O.NAME.get)
def test_quantize_every_code_and_boundary(fmt, dtype):
    M, K, ldx, ldo, ldt = 401, 67, 72, 72, 416
    w = O.boundary_values(fmt, dtype)
    flat = w.repeat((M * K + len(w) - 1) // len(w))[:M * K]
    # the list (about 1000 values) repeats 26 times: each value meets every position of a lane's 8-element chunk and every one
    # of the four packed rows
    i = torch.arange(M * K)
    seen8, seen4 = torch.zeros(len(w), 8, dtype=torch.bool), torch.zeros(len(w), 4, dtype=torch.bool)
    seen8[i % len(w), (i % K) % 8] = True
    seen4[i % len(w), (i // K) % 4] = True
    assert bool(seen8.all()) and bool(seen4.all())
    for s in (1.0, 2.0 ** -3, 2.0 ** 5, 7.25):
        x = (flat.float() / s).to(dtype).view(M, K)
        if s != 7.25:  # a power of two: the scaled value is the boundary value itself
            assert torch.equal((x.float() * s).view(-1), flat.float())
        out, out_t = quantize(place(x, ldx, XPAD), M, K, s, fmt, ldo, ldt)
        want = O.quantize(x, s, fmt)
        bad = (O.canon(out, fmt) != O.canon(want, fmt)).nonzero()
        assert len(bad) == 0, (s, [(i, j, float(x[i, j]) * s, int(out[i, j]), int(want[i, j])) for i, j in bad[:8].tolist()])
        assert torch.equal(out_t, out.t().contiguous()), s
    neg = out[(x < 0) & (x.float().abs() * 7.25 < O.MIN_SUB[fmt] / 2)]
    print(f"[fp8-chain] quantiser {O.NAME[fmt]} {DT[dtype]}: negative underflow -> bytes {sorted(set(neg.tolist()))}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT.get)
@pytest.mark.parametrize("fmt", FMTS, ids=O.NAME.get)
def test_quantize_keeps_nan(fmt, dtype):
    """A NaN input leaves as a byte that decodes to NaN in both images (it used to leave as the code of -max); every other
    byte is what it is without the NaN; amax does not record it, the column sum of its column is NaN."""
    L = _L()
    M, K, ldx, ldo, ldt = 129, 67, 72, 72, 144
    g = torch.Generator().manual_seed(3 + fmt)
    x = torch.randint(-8, 9, (M, K), generator=g).to(dtype)
    spots = [(0, 0), (2, 5), (127, 63), (128, 66), (77, 64)]  # vector loads, the per-element tail, both row tiles
    x[1, 1] = 8.0
    for i, j in spots:
        x[i, j] = float("nan")
    amax = torch.zeros(1, device="cuda")
    cs = torch.zeros(K, device="cuda")
    out, out_t = quantize(place(x, ldx, XPAD), M, K, 3.0, fmt, ldo, ldt, amax=amax, colsum=cs)
    want = O.quantize(x, 3.0, fmt)
    assert bool(torch.isnan(O.decode(want, fmt))[tuple(zip(*spots))].all())  # (the reference keeps NaN)
    assert O.same(out, want, fmt), sorted(set(out[tuple(zip(*spots))].tolist()))
    assert torch.equal(out_t, out.t().contiguous())
    assert float(amax) == 8.0
    nan_cols = torch.zeros(K, dtype=torch.bool)
    nan_cols[[j for _, j in spots]] = True
    assert torch.equal(torch.isnan(cs.cpu()), nan_cols)
    assert torch.equal(cs.cpu()[~nan_cols], x.float().sum(0)[~nan_cols])
    print(f"[fp8-chain] quantiser {O.NAME[fmt]} {DT[dtype]}: NaN -> bytes {sorted(set(out[tuple(zip(*spots))].tolist()))}")


# ------------------------------------------------------------------------------------------------------------ 2  ragged shapes
RAGGED = [(1, 1, 8, 8, 16), (5, 3, 8, 8, 16), (127, 63, 64, 64, 128), (129, 65, 72, 72, 144), (200, 133, 136, 136, 208),
          (33, 200, 200, 208, 48)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT.get)
@pytest.mark.parametrize("fmt", FMTS, ids=O.NAME.get)
@pytest.mark.parametrize("M,K,ldx,ldo,ldt", RAGGED, ids=lambda v: str(v))
def test_quantize_ragged_shapes_exact(M, K, ldx, ldo, ldt, fmt, dtype):
    g = torch.Generator().manual_seed(M * 1000 + K)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    x[M // 2, K // 2] = -8.0  # (the maximum is there whatever the draw)
    xd = place(x.to(dtype), ldx, XPAD)
    amax = torch.cat([torch.zeros(1), torch.full((7,), SF)]).cuda()
    cs = torch.cat([torch.full((K,), 3.0), torch.full((8,), SF)]).cuda()
    for run in (1, 2):
        out, out_t = quantize(xd, M, K, 1.0, fmt, ldo, ldt, amax=amax[:1], colsum=cs)
        want = O.quantize(x, 1.0, fmt)
        assert torch.equal(out, want)  # integers: byte for byte, no zero-sign question
        assert torch.equal(out_t, want.t().contiguous())
        assert torch.equal(cs.cpu()[:K], 3.0 + run * x.sum(0)), run
    assert amax.cpu().tolist() == [8.0] + [SF] * 7
    assert cs.cpu()[K:].tolist() == [SF] * 8
    assert torch.equal(xd.cpu()[:M, :K], x.to(dtype))


# --------------------------------------------------------------------------------------------------------------------- 3  amax
def _amax_big_n():
    """Past four strides of the whole grid (the unrolled loop runs at least once in every thread), then 77 whole vectors and a tail
    of 5 for the second loop: csrc/quant.hip amax_kernel, grid = min(2048, 2 per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = min(2048, 2 * cus)
    return grid * 2048, 4 * grid * 2048 + 8 * 77 + 5


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT.get)
@pytest.mark.parametrize("which", ["small", "unrolled"])
def test_amax_positions_and_tails(which, dtype):
    L = _L()
    stride, big = _amax_big_n()
    sizes = [1, 5, 8, 13] if which == "small" else [big]
    for n in sizes:
        g = torch.Generator(device="cuda").manual_seed(n % 1000)
        buf = (torch.rand(n + 16, generator=g, device="cuda") - 0.5).to(dtype)  # |x| <= 0.5
        buf[n:] = 1.0e6  # directly behind the tensor: must not be picked up
        spots = {0, n - 1}
        if n >= 8:
            spots.add((n // 8) * 8 - 8 + 3)  # inside the last whole 8-vector
        if which == "unrolled":
            spots.update(j * stride + 8 * 1234 + j for j in range(4))  # one place in each of the four unrolled streams
            spots.add(4 * stride + 8 * 40 + 2)  # the vector loop behind the unrolled one
        amax = torch.cat([torch.zeros(1), torch.full((7,), SF)]).cuda()
        for t, p in enumerate(sorted(spots)):
            keep = buf[p].clone()
            buf[p] = 3.0 if t % 2 else -3.0
            amax[0] = 0.0
            L.call("uwu_fp8_amax", L.ptr(buf), L.dt(buf), n, L.ptr(amax), L.stream())
            assert amax.cpu().tolist() == [3.0] + [SF] * 7, (n, p)
            buf[p] = keep
        amax[0] = 0.0
        L.call("uwu_fp8_amax", L.ptr(buf), L.dt(buf), n, L.ptr(amax), L.stream())
        assert float(amax[0]) == float(buf[:n].float().abs().max()), n
        # the running maximum is kept (atomic max, the caller zeroes it)
        amax[0] = 7.0
        L.call("uwu_fp8_amax", L.ptr(buf), L.dt(buf), n, L.ptr(amax), L.stream())
        assert amax.cpu().tolist() == [7.0] + [SF] * 7


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT.get)
def test_amax_contract_for_non_finite_input(dtype):
    """As include/uwu_hip.h states it: an Inf element makes amax inf; a NaN element is not recorded (fmaxf drops it) -- the
    bytes keep NaN visible instead (test_quantize_keeps_nan)."""
    L = _L()
    for n in (13, 8 * 300 + 5):
        x = torch.linspace(-2.0, 1.0, n).to(dtype).cuda()
        for p in (0, n // 2, n - 1):
            for bad, want in ((float("nan"), 2.0), (float("inf"), float("inf")), (-float("inf"), float("inf"))):
                y = x.clone()
                y[p] = bad
                if p == 0:
                    y[1] = -2.0  # (the maximum itself sits at element 0)
                amax = torch.zeros(1, device="cuda")
                L.call("uwu_fp8_amax", L.ptr(y), L.dt(y), n, L.ptr(amax), L.stream())
                assert float(amax) == want, (n, p, bad)


# ------------------------------------------------------------------------------------------------------------ 4  update_scales
def test_update_scales_edges():
    """scale = FMT_MAX / (amax * margin) in fp32 where that quotient is finite and positive; otherwise the previous scale, or
    1 where there was none (0, NaN, inf, negative); amax is reset in every case; a stored scale is finite and positive.
    The quotient overflows for amax = 1e-40 / 1e-37 and is 0 for FLT_MAX at margin 2: inf and 0 used to be stored."""
    L = _L()
    flt_max = torch.finfo(F32).max
    amaxes = [0.3, 2.5, 0.0, 1e-40, 1e-37, flt_max, float("inf"), float("nan")]
    prevs = [0.0, 3.0, float("nan"), float("inf"), -2.0]
    rows = [(a, p, f) for a in amaxes for p in prevs for f in FMTS]
    for margin in (1.0, 2.0):
        a = torch.tensor([r[0] for r in rows], dtype=F32)
        p = torch.tensor([r[1] for r in rows], dtype=F32)
        f = torch.tensor([r[2] for r in rows], dtype=torch.int32)
        q = torch.tensor([O.FMAX[r[2]] for r in rows], dtype=F32) / (a * torch.tensor(margin, dtype=F32))
        ok = torch.isfinite(q) & (q > 0) & (a > 0)
        keep = torch.isfinite(p) & (p > 0)
        want = torch.where(ok, q, torch.where(keep, p, torch.ones_like(p)))
        # the cases the issue names, spelled out
        for r, w in zip(rows, want.tolist()):
            if r[0] in (0.0, 1e-40, 1e-37, float("inf")) or r[0] != r[0]:
                assert w == (3.0 if r[1] == 3.0 else 1.0), (r, w)
        n = len(rows)
        ad = torch.cat([a, torch.full((8,), SF)]).cuda()
        sd = torch.cat([p, torch.full((8,), SF)]).cuda()
        L.call("uwu_fp8_update_scales", L.ptr(ad), L.ptr(sd), L.ptr(f.cuda()), n, margin, L.stream())
        got = sd.cpu()
        bad = [(r, g, w) for r, g, w in zip(rows, got[:n].tolist(), want.tolist()) if g != w]
        assert not bad, (margin, bad[:6])
        assert bool((torch.isfinite(got[:n]) & (got[:n] > 0)).all())
        assert ad.cpu().tolist() == [0.0] * n + [SF] * 8 and got[n:].tolist() == [SF] * 8


# -------------------------------------------------------------------------------------------------------------- 5  GEMM decode
def _one_per_row(rows, K, fmt, seed):
    """uint8 [rows, K] with one non-zero byte per row: row r carries finite code c(r) at column k(r) = 131 r mod K (131 is
    coprime to K: no two rows share a column while rows <= K; 131 = 3 mod 128 walks every residue mod 128)."""
    codes = O.finite_codes(fmt)
    g = torch.Generator().manual_seed(seed)
    c = codes[(torch.arange(rows) + int(torch.randint(0, len(codes), (1,), generator=g))) % len(codes)]
    k = (131 * torch.arange(rows)) % K
    assert set(c.tolist()) == set(codes.tolist()) and set((k % 128).tolist()) == set(range(128))
    assert set((k // 128).tolist()) == set(range(K // 128)) and rows <= K and len(set(k.tolist())) == rows
    m = torch.zeros(rows, K, dtype=torch.uint8)
    m[torch.arange(rows), k] = c
    return m, c, k


def _dense(rows, K, fmt, seed):
    codes = O.finite_codes(fmt)
    g = torch.Generator().manual_seed(seed)
    m = codes[torch.randint(0, len(codes), (rows, K), generator=g)]
    assert set(m.view(-1).tolist()) == set(codes.tolist())
    return m


def _decode_fixture(M, N, K, fmt_a, sparse):
    """(A bytes, B bytes, the exact product A . B^T in float32): each element is one product of two table values."""
    if sparse == "A":
        a, c, k = _one_per_row(M, K, fmt_a, 11 + fmt_a)
        b = _dense(N, K, O.E4M3, 5)
        prod = O.decode(c, fmt_a)[:, None] * O.decode(b[:, k].t().contiguous(), O.E4M3)  # [M, N]
    else:
        b, c, k = _one_per_row(N, K, O.E4M3, 13)
        a = _dense(M, K, fmt_a, 7 + fmt_a)
        prod = O.decode(a[:, k], fmt_a) * O.decode(c, O.E4M3)[None, :]
    assert torch.equal(prod.double(), (O.decode(a, fmt_a).double() @ O.decode(b, O.E4M3).double().t()))  # one term each
    return a, b, prod


def _gemm_fp8(ad, bd, M, N, K, fmt_a, epi, sa, sb, c, bias=None, scratch=None):
    L = _L()
    L.call("uwu_gemm_fp8", L.ptr(ad), L.ptr(bd), L.ptr(c), None, L.ptr(bias), None, M, N, K, ad.shape[1], bd.shape[1], c.shape[1], 0,
           fmt_a, epi, L.ptr(sa), L.ptr(sb), L.ptr(scratch), scratch.numel() if scratch is not None else 0, L.stream())
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("sparse", ["A", "B"])
@pytest.mark.parametrize("fmt_a", FMTS, ids=O.NAME.get)
@pytest.mark.parametrize("kernel,K", [("gemm_f8", 384), ("gemm_p8f", 768)])
def test_gemm_fp8_decodes_every_code_in_every_k_position(kernel, K, fmt_a, sparse, bias, monkeypatch):
    L = _L()
    M, N = 300, 264
    monkeypatch.setenv("UWU_GEMM_P8F", "1" if kernel == "gemm_p8f" else "0")
    a, b, prod = _decode_fixture(M, N, K, fmt_a, sparse)
    sa, sb = scalar(4.0), scalar(0.5)  # alpha = 1 / 2: a power of two, the scaled product stays exact
    g = torch.Generator().manual_seed(17)
    bv = torch.randint(-4, 5, (N,), generator=g).float() if bias else None
    biasd = torch.cat([bv, torch.full((8,), SF)]).cuda() if bias else None
    # operand padding and guard rows hold the NaN code: a byte read past K or past the last row would show
    ad, bd = place(a, K + 16, O.NAN_CODE), place(b, K + 16, O.NAN_CODE)
    ldc = N + 8

    def run(ad_, bd_):
        c = blank(M, N, ldc, SF, BF16)
        _gemm_fp8(ad_, bd_, M, N, K, fmt_a, L.EPI_BIAS if bias else L.EPI_NONE, sa, sb, c, bias=biasd)
        return inside(c, M, N, SF, kernel)

    want = (prod * 0.5 + 0.0) + (bv if bias else 0.0)  # fp32: the product exact, one rounding in the bias add, as on the device
    want = want.bfloat16()
    if not bias:
        assert torch.equal(want.double(), prod.double() * 0.5)  # (exact in bf16: tests/test_fp8_ref_cpu.py)
    got = run(ad, bd)
    assert L.load().uwu_gemm_last_kernel().decode() == kernel
    bad = (_bits(got) != _bits(want)).nonzero()
    assert len(bad) == 0, [(i, j, float(got[i, j]), float(want[i, j])) for i, j in bad[:8].tolist()]
    assert torch.equal(ad.cpu()[:M, :K], a) and torch.equal(bd.cpu()[:N, :K], b)
    if sparse == "B" or bias:
        return
    # NaN / Inf codes: exactly the row (column) that meets the code is non-finite, every other element keeps its bits
    r, col = 131, 77
    cases = [("A", r, O.NAN_CODE), ("B", col, O.NAN_CODE)] + ([("A", r, O.INF_CODE), ("A", r, O.INF_CODE | 0x80)] if fmt_a == O.E5M2 else [])
    for side, idx, code in cases:
        a2, b2 = ad.clone(), bd.clone()
        (a2 if side == "A" else b2)[idx, (131 * idx) % K if side == "A" else 200] = code
        out = run(a2, b2)
        hit = torch.zeros(M, N, dtype=torch.bool)
        if side == "A":
            hit[idx] = True
        else:
            hit[:, idx] = True
        assert bool((~torch.isfinite(out.float()))[hit].all()) and torch.equal(_bits(out)[~hit], _bits(want)[~hit]), (side, code)


@pytest.mark.parametrize("part", ["0", "1"])
@pytest.mark.parametrize("fmt_a", FMTS, ids=O.NAME.get)
@pytest.mark.parametrize("M,N,K", [(300, 260, 1024), (300, 1020, 1024)], ids=["4tiles", "8tiles"])
def test_gemm_fp8_weight_gradient_form_decodes_every_code(M, N, K, fmt_a, part, monkeypatch):
    """EPI_ACCUM into fp32 (split-K partial slabs + reduce): two calls into zeros give exactly twice the product.
    UWU_GEMM_P8F_PART can only switch the 8-phase kernel OFF; it runs where uwu_gemm_p8f_split finds a slice count whose fill of
    one-unit-per-CU rounds outweighs 2.5 % per slice, i.e. tiles > 0.025 CUs while the units fit one round (csrc/gemm_p8f.hip).
    (300, 260, 1024) has 4 tiles: both settings run gemm_f8_kernel's split-K form there.  (300, 1020, 1024) has 8 (ragged in M
    and N; 1020 rows still fit one non-zero per row into K = 1024): UWU_GEMM_P8F_PART=1 runs gemm_p8f_kernel in two K slices of
    four steps.  uwu_gemm_last_kernel() must name the kernel the case is about."""
    L = _L()
    monkeypatch.setenv("UWU_GEMM_P8F_PART", part)
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * tiles <= cus  # (one round of units for 1 or 2 slices: the rule above is the whole condition)
    p8f = part == "1" and tiles > 0.025 * cus  # (256 CUs: 8 tiles yes, 4 tiles no)
    sa, sb = scalar(4.0), scalar(0.5)
    nbytes = L.load().uwu_gemm_fp8_scratch_bytes(M, N, K)
    for sparse in ("A", "B"):
        a, b, prod = _decode_fixture(M, N, K, fmt_a, sparse)
        ad, bd = place(a, K + 16, O.NAN_CODE), place(b, K + 16, O.NAN_CODE)
        c = blank(M, N, N + 4, SF, F32)
        c[:M, :N] = 0.0
        scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
        scratch[nbytes:] = S8
        for _ in range(2):
            _gemm_fp8(ad, bd, M, N, K, fmt_a, L.EPI_ACCUM, sa, sb, c, scratch=scratch[:nbytes])
            assert L.load().uwu_gemm_last_kernel().decode() == ("gemm_p8f(split-K)" if p8f else "gemm_f8(split-K)")
        got = inside(c, M, N, SF, "accum")
        assert bool((scratch[nbytes:] == S8).all())
        want = 2.0 * (prod * 0.5 + 0.0)
        bad = (_bits(got) != _bits(want)).nonzero()
        assert len(bad) == 0, (sparse, [(i, j, float(got[i, j]), float(want[i, j])) for i, j in bad[:8].tolist()])


# ---------------------------------------------------------------------------------------------------------- band rule (6, 7)
def band_check(label, got, ref64, e32, fmt):
    """got: bytes; ref64: the float64 value already multiplied by q_scale; e32: E32 in the same units."""
    want = O.quantize_value(ref64, fmt)
    dist = O.code_distance(got, want, fmt)
    bd = O.boundary_distance(ref64, fmt)
    in_band = float((bd <= MARGIN * e32).double().mean())
    diff = dist > 0
    worst = float((bd[diff] / e32).max()) if bool(diff.any()) else 0.0
    print(f"[fp8-chain] {label}: E32 {e32:.2e}, {int(diff.sum())} of {diff.numel()} bytes off the fp64 RNE, worst boundary distance "
          f"{worst:.2f} E32, {100 * in_band:.3f} % of the elements within {MARGIN:.0f} E32 of a boundary")
    assert in_band < 0.01, f"{label}: the inputs put {in_band:.3%} of the elements into the band"
    assert int(dist.max()) <= 1, f"{label}: a byte {int(dist.max())} codes from the fp64 RNE"
    assert worst <= MARGIN, f"{label}: a byte differs {worst:.2f} E32 from a rounding boundary"
    return worst


# ------------------------------------------------------------------------------------------------------ 6  emitting epilogue
KEPT = (8.0, 12.0, -12.0, 30.0, -30.0)  # HARD_VALUES exact in the kernel's formula (tests/test_fp8_ref_cpu.py)
EMIT_SHAPES = [(256, 256, 128), (272, 304, 256)]


def _emit(epi, ad, bd, M, N, K, fmt_a, sa, sb, qs, bias=None, aux=None, colsum=None, amax=None):
    """-> (C [M, N] bf16 or None, q8 [M, N], q8t [N, M]) on the CPU; ldc, ldq, ldqt 16 over the row; guards checked."""
    L = _L()
    gelu = epi == L.EPI_BIAS_GELU
    c = blank(M, N, N + 16, SF, BF16) if gelu else None
    q8, q8t = blank(M, N, N + 16, S8, torch.uint8), blank(N, M, M + 16, S8, torch.uint8)
    qd = scalar(qs)  # (alive until the kernel has run)
    L.call("uwu_gemm_fp8_emit", L.ptr(ad), L.ptr(bd), L.ptr(c), L.ptr(colsum), L.ptr(bias), L.ptr(aux), M, N, K, ad.shape[1],
           bd.shape[1], N + 16, aux.shape[1] if aux is not None else 0, fmt_a, epi, L.ptr(sa), L.ptr(sb), L.ptr(q8), N + 16,
           L.ptr(q8t), M + 16, L.ptr(qd), L.ptr(amax), L.stream())
    torch.cuda.synchronize()
    return (inside(c, M, N, SF, "C") if gelu else None), inside(q8, M, N, S8, "q8"), inside(q8t, N, M, S8, "q8t")


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("M,N,K", EMIT_SHAPES, ids=lambda v: str(v))
def test_emit_bias_gelu_saturated_block_is_exact(M, N, K):
    """Integer operands; rows 5 and M - 3 hold nothing but a one at k = 0, where B carries KEPT in turn for the columns
    n < 48 and n >= N - 24 (zero bias there): those pre-activations are KEPT exactly, gelu = x or -0 exactly, and the bytes are
    RNE(value * 7.25) bit for bit (8 * 7.25 = 58 is a tie of e4m3).  Everything else is bounded by 22 + 4 < 30, so amax is the
    block's 30 exactly.  The bf16 pre-activation is exact everywhere."""
    L = _L()
    rows = [5, M - 3]
    cols = torch.cat([torch.arange(48), torch.arange(N - 24, N)])
    a, b = _ints((M, K), -1, 1, M + 1), _ints((N, K), -1, 1, N + 2)
    b[:, 23:] = 0.0
    a[:, 0] = 0.0
    b[:, 0] = 0.0
    a[rows] = 0.0
    a[rows, 0] = 1.0
    b[cols, 0] = torch.tensor(KEPT).repeat(len(cols) // len(KEPT) + 1)[:len(cols)]
    bias = _ints((N,), -4, 4, 3)
    bias[cols] = 0.0
    pre = a @ b.t() + bias
    block = torch.zeros(M, N, dtype=torch.bool)
    block[torch.tensor(rows)[:, None], cols[None, :]] = True
    assert set(pre[block].tolist()) == set(KEPT) and float(pre[~block].abs().max()) < 30.0
    val = torch.where(pre > 0, pre, torch.zeros_like(pre))  # on the block
    assert torch.equal(O.gelu_sig(pre)[block], val[block]) and torch.equal(G.gelu_tanh(pre)[block], val[block])
    sa, sb, qs = scalar(2.0), scalar(0.5), 7.25
    ad, bd = place(O.quantize(a, 2.0, O.E4M3), K + 16, O.NAN_CODE), place(O.quantize(b, 0.5, O.E4M3), K + 16, O.NAN_CODE)
    amax = torch.cat([torch.zeros(1), torch.full((7,), SF)]).cuda()
    biasd = torch.cat([bias, torch.full((8,), SF)]).cuda()
    C, q8, q8t = _emit(L.EPI_BIAS_GELU, ad, bd, M, N, K, O.E4M3, sa, sb, qs, bias=biasd, amax=amax)
    assert torch.equal(C.float(), pre)  # integers below 256: exact in bf16
    want = O.quantize(val, qs, O.E4M3)
    assert O.same(q8[block], want[block], O.E4M3), (q8[block][:12].tolist(), want[block][:12].tolist())
    assert torch.equal(q8t, q8.t().contiguous())
    assert amax.cpu().tolist() == [30.0] + [SF] * 7
    # the rest of the tile: integer pre-activations, every byte within one code of the fp64 RNE
    ref = G.gelu_tanh(pre.double()) * qs
    assert int(O.code_distance(q8, O.quantize_value(ref, O.E4M3), O.E4M3).max()) <= 1


@pytest.mark.parametrize("M,N,K", EMIT_SHAPES, ids=lambda v: str(v))
def test_emit_dgelu_saturated_aux_is_exact(M, N, K):
    """aux is KEPT everywhere (gelu' = 1 or 0 exactly), integer operands with an e5m2 A: every value is acc or 0, every byte is
    RNE(value * 7.25), the column sums on top of an integer fill and amax are exact."""
    L = _L()
    a, b = _ints((M, K), -3, 3, M + 5), _ints((N, K), -2, 2, N + 6)
    aux = torch.tensor(KEPT)[torch.randint(0, len(KEPT), (M, N), generator=torch.Generator().manual_seed(9))]
    acc = a @ b.t()
    assert torch.equal(O.dgelu_sig(aux), (aux > 0).float()) and torch.equal(G.dgelu_tanh(aux), (aux > 0).float())
    val = acc * (aux > 0).float()
    sa, sb, qs = scalar(2.0), scalar(0.5), 7.25
    ad, bd = place(O.quantize(a, 2.0, O.E5M2), K + 16, O.NAN_CODE), place(O.quantize(b, 0.5, O.E4M3), K + 16, O.NAN_CODE)
    auxd = place(aux.bfloat16(), N + 8, SF)
    amax = torch.cat([torch.zeros(1), torch.full((7,), SF)]).cuda()
    cs = torch.cat([torch.full((N,), 3.0), torch.full((8,), SF)]).cuda()
    _, q8, q8t = _emit(L.EPI_DGELU, ad, bd, M, N, K, O.E5M2, sa, sb, qs, aux=auxd, colsum=cs, amax=amax)
    assert O.same(q8, O.quantize(val, qs, O.E5M2), O.E5M2)
    assert torch.equal(q8t, q8.t().contiguous())
    assert torch.equal(cs.cpu()[:N], 3.0 + val.sum(0)) and cs.cpu()[N:].tolist() == [SF] * 8
    assert amax.cpu().tolist() == [float(val.abs().max())] + [SF] * 7


def _moderate(M, N, K, fmt_a):
    """Integer operand bytes handed over with scales 8 and 2 (alpha = 1 / 16): acc / 16 is exact, a few units.  A is even except for
    a column of ones that meets ones in B, so acc is odd: no value is an exact zero, which the band rule would count as lying
    on a boundary wherever 4 E32 exceeds half the smallest subnormal (e5m2)."""
    a, b = 2.0 * _ints((M, K), -1, 1, M + K), _ints((N, K), -2, 2, N + K)
    a[:, 0] = 1.0
    b[:, 0] = 1.0
    assert bool(((a @ b.t()) % 2 == 1).all())
    return a, b, (a @ b.t()) / 16.0, place(O.quantize(a, 1.0, fmt_a), K + 16, O.NAN_CODE), place(O.quantize(b, 1.0, O.E4M3), K + 16, O.NAN_CODE)


@pytest.mark.parametrize("M,N,K", EMIT_SHAPES, ids=lambda v: str(v))
def test_emit_bias_gelu_moderate_values_and_nan(M, N, K):
    L = _L()
    a, b, acc, ad, bd = _moderate(M, N, K, O.E4M3)
    bias = _ints((N,), -2, 2, 4)
    pre = acc + bias  # exact in fp32 (multiples of 1 / 16 below 2^8)
    assert torch.equal(pre.double(), (a.double() @ b.double().t()) / 16.0 + bias.double())
    qs = float(torch.tensor(400.0 / float(G.gelu_tanh(pre.double()).abs().max()), dtype=F32))
    ref = G.gelu_tanh(pre.double()) * qs
    e32 = float(((G.gelu_tanh(pre) * torch.tensor(qs, dtype=F32)).double() - ref).abs().max())
    sa, sb = scalar(8.0), scalar(2.0)
    biasd = torch.cat([bias, torch.full((8,), SF)]).cuda()
    amax = torch.zeros(1, device="cuda")
    C, q8, q8t = _emit(L.EPI_BIAS_GELU, ad, bd, M, N, K, O.E4M3, sa, sb, qs, bias=biasd, amax=amax)
    assert torch.equal(_bits(C), _bits(pre.bfloat16()))
    assert torch.equal(q8t, q8.t().contiguous())
    band_check(f"emit bias_gelu {M}x{N}x{K}", q8, ref, e32, O.E4M3)
    assert abs(float(amax) - float(ref.abs().max()) / qs) <= MARGIN * e32 / qs
    # one NaN code in A: that row of both images decodes to NaN, the bf16 row is NaN, every other row keeps its bytes
    r = M - 7
    ad[r, 3] = O.NAN_CODE
    C2, p8, p8t = _emit(L.EPI_BIAS_GELU, ad, bd, M, N, K, O.E4M3, sa, sb, qs, bias=biasd)
    other = torch.arange(M) != r
    assert bool(torch.isnan(O.decode(p8[r], O.E4M3)).all()), sorted(set(p8[r].tolist()))
    assert bool(torch.isnan(C2[r].float()).all())
    assert torch.equal(p8[other], q8[other]) and torch.equal(_bits(C2[other]), _bits(C[other]))
    assert torch.equal(p8t, p8.t().contiguous())


@pytest.mark.parametrize("M,N,K", EMIT_SHAPES, ids=lambda v: str(v))
def test_emit_dgelu_moderate_values_and_nan(M, N, K):
    L = _L()
    a, b, acc, ad, bd = _moderate(M, N, K, O.E5M2)
    aux = (1.5 * torch.randn(M, N, generator=torch.Generator().manual_seed(M + N))).bfloat16()
    ref1 = acc.double() * G.dgelu_tanh(aux.double())
    qs = float(torch.tensor(40000.0 / float(ref1.abs().max()), dtype=F32))
    ref = ref1 * qs
    v32 = acc * G.dgelu_tanh(aux.float())
    e32 = float(((v32 * torch.tensor(qs, dtype=F32)).double() - ref).abs().max())
    sa, sb = scalar(8.0), scalar(2.0)
    auxd = place(aux, N + 8, SF)
    cs = torch.zeros(N, device="cuda")
    amax = torch.zeros(1, device="cuda")
    _, q8, q8t = _emit(L.EPI_DGELU, ad, bd, M, N, K, O.E5M2, sa, sb, qs, aux=auxd, colsum=cs, amax=amax)
    assert torch.equal(q8t, q8.t().contiguous())
    band_check(f"emit dgelu {M}x{N}x{K}", q8, ref, e32, O.E5M2)
    e_cs = float((v32.sum(0).double() - ref1.sum(0)).abs().max())
    A_cs = ref1.abs().sum(0)
    assert bool(((cs.cpu().double() - ref1.sum(0)).abs() <= MARGIN * torch.clamp(2.0 ** -23 * A_cs, min=e_cs)).all())
    assert abs(float(amax) - float(ref1.abs().max())) <= MARGIN * e32 / qs
    r = 9
    ad[r, 130 % K] = O.NAN_CODE
    _, p8, p8t = _emit(L.EPI_DGELU, ad, bd, M, N, K, O.E5M2, sa, sb, qs, aux=auxd)
    other = torch.arange(M) != r
    assert bool(torch.isnan(O.decode(p8[r], O.E5M2)).all()), sorted(set(p8[r].tolist()))
    assert torch.equal(p8[other], q8[other]) and torch.equal(p8t, p8.t().contiguous())


# ------------------------------------------------------------------------------------------------------ 7  LayerNorm emitter
def _ln_q8(x, y, mod, B, T, D, qs, amax=None):
    """-> (x_out [M, D] or None, q8 [M, D], q8t [D, M], mean, rstd) on the CPU; ldq = D + 16, ldqt = M + 16, guards checked."""
    L = _L()
    M = B * T
    q8, q8t = blank(M, D, D + 16, S8, torch.uint8), blank(D, M, M + 16, S8, torch.uint8)
    xo = blank(M, D, D, SF, BF16) if y is not None else None
    stat = torch.full((2, M + 8), SF, device="cuda")
    gate, shift, scale = mod[:, 0], mod[:, 1], mod[:, 2]
    qd = scalar(qs)  # (alive until the kernel has run)
    L.call("uwu_add_ln_modulate_fwd_q8", L.ptr(x), L.ptr(y), gate.data_ptr() if y is not None else None, shift.data_ptr(),
           scale.data_ptr(), 3 * D, L.ptr(xo if y is not None else x), L.ptr(q8), D + 16, L.ptr(q8t), M + 16, L.ptr(qd),
           L.ptr(amax), stat[0].data_ptr(), stat[1].data_ptr(), B, T, D, 1e-6, L.stream())
    torch.cuda.synchronize()
    st = stat.cpu()
    assert st[:, M:].eq(SF).all()
    return (inside(xo, M, D, SF, "x_out") if y is not None else None, inside(q8, M, D, S8, "q8"), inside(q8t, D, M, S8, "q8t"),
            st[0, :M].clone(), st[1, :M].clone())


@pytest.mark.parametrize("with_y", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("D", [384, 520, 1152, 1536])
def test_layernorm_emitter_band_and_nan(D, with_y):
    """D = 384: one pass; 520: a ragged second pass; 1152: three passes, 8 waves; 1536: the 4-wave tile."""
    L = _L()
    B, T = 4, 32
    M = B * T
    x, y, _, _, mod = LN.hard_inputs(B, T, D, 0, BF16)
    xd, yd, modd = x.cuda(), (y.cuda() if with_y else None), mod.cuda()
    # the plain kernel: residual stream and statistics must be the same bits
    xo_p = torch.empty_like(xd) if with_y else xd
    h = torch.empty_like(xd)
    mean_p, rstd_p = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    L.call("uwu_add_ln_modulate_fwd", L.ptr(xd), L.ptr(yd), modd[:, 0].data_ptr() if with_y else None, modd[:, 1].data_ptr(),
           modd[:, 2].data_ptr(), 3 * D, L.ptr(xo_p), L.ptr(h), L.ptr(mean_p), L.ptr(rstd_p), B, T, D, 1e-6, 0, L.dt(xd), L.stream())
    stored = xo_p.cpu()
    r64 = LN.forward(stored, T, shift=mod[:, 1], scale=mod[:, 2], dtype=F64)["h"]
    # (the two "massive" channels reach 30 - 80 standard deviations: they take the top codes, the bulk sits around 1 - 2)
    qs = float(torch.tensor(100.0 / float(r64.abs().max()), dtype=F32))
    ref = r64 * qs
    h32 = LN.forward(stored, T, shift=mod[:, 1], scale=mod[:, 2], dtype=F32)["h"] * torch.tensor(qs, dtype=F32)
    e32 = float((h32.double() - ref).abs().max())
    amax = torch.zeros(1, device="cuda")
    xo, q8, q8t, mean, rstd = _ln_q8(xd, yd, modd, B, T, D, qs, amax=amax)
    if with_y:
        assert torch.equal(_bits(xo), _bits(stored))
    assert torch.equal(mean, mean_p.cpu()) and torch.equal(rstd, rstd_p.cpu())
    assert torch.equal(q8t, q8.t().contiguous())
    band_check(f"layernorm q8 D={D} {'residual' if with_y else 'plain'}", q8, ref, e32, O.E4M3)
    assert abs(float(amax) - float(r64.abs().max())) <= MARGIN * e32 / qs
    # one NaN in one input row: its bytes all decode to NaN, x_out of it is NaN, every other row of every output keeps its bits
    r = 77
    x2 = xd.clone()
    x2[r, D - 3] = float("nan")
    xo2, p8, p8t, mean2, rstd2 = _ln_q8(x2, yd, modd, B, T, D, qs)
    other = torch.arange(M) != r
    assert bool(torch.isnan(O.decode(p8[r], O.E4M3)).all()), sorted(set(p8[r].tolist()))
    assert torch.equal(p8[other], q8[other]) and torch.equal(p8t, p8.t().contiguous())
    assert torch.equal(mean2[other], mean[other]) and torch.equal(rstd2[other], rstd[other])
    assert bool(torch.isnan(mean2[r])) and bool(torch.isnan(rstd2[r]))
    if with_y:
        assert bool(torch.isnan(xo2[r, D - 3].float())) and torch.equal(_bits(xo2[other]), _bits(xo[other]))
