"""The kernels at the edges of the denoiser step against float64: the fp32 Linears with at most 64 rows (csrc/skinny.hip, every
<MT, NPW, EPI> and <R, KC> instantiation and every slab-length clamp), the timestep features, patchify / unpatchify, the
positional add and the bf16 transpose (csrc/embed.hip, fp32 and bf16, past the element-wise grid cap), and the axial RoPE
rotation, its factor table and its gradients (csrc/rope.hip; strided, in place, shared positions).

Reference (tests/edge_oracle.py, checked by tests/test_edge_ref_cpu.py): the formulas of include/uwu_hip.h in float64 on the
rounded inputs the device gets.  Every call goes through the C ABI, so offsets, strides and guards are the test's: every output
buffer is filled with a sentinel and has guard elements (rows, columns) around the part the kernel owns, which must stay
bit-identical, and every input must read back unchanged.

Bars.  E32 = max over the tensor of |the same formulas in torch fp32 on the CPU - fp64|.  Per element
    |got - ref| <= 4 * max(E32, 2^-23 * A) + (bf16 output ? 2^-8 * |ref| : 0)
with A = the absolute sum of the terms of that element (|x| |w|^T + |b| for a Linear, |dy|^T |x| + |the previous contents| for an
accumulated weight gradient, ...) and |ref| for elementwise outputs.  The margin of 4 covers summation order only.  Additions:
  * Y2 = silu(Y): against float64 SiLU of the device's own Y, 1e-6 |ref| + 1e-6 max |ref| (the rule of tests/test_unet_ops_gpu.py
    for the same x / (1 + __expf(-x))); the bias is spread over [-20, 20].
  * timestep features: 4 * max(E32, |a| (3 s + 3) 2^-24 + 2^-22), a = t f_j, s = ln(max_period) j / half
    (edge_oracle.timestep_budget).
  * RoPE: the kernels use the hardware exp / sin / cos.  E_FAST(|theta|) = twice the worst |cos -+ sin - fp64| that
    tools/probes/probe_fastmath.hip measured in the octave of |theta| (twice: the probe samples, it does not enumerate; its
    table is in profiles/edge_kernels_accuracy_mi355x.txt).  Rotated element: + |x| E_FAST; log-frequency gradient:
    + sum_rows (|ga a| + |gb b|) (E_FAST + |theta| delta) |theta|, delta = (|f| + 4) 2^-24.  |theta| reaches 10 pi (the largest
    frequency of the shipped init at the edge of the position grid) and stays below 32.
  * patchify, unpatchify, add_pos and the transpose are exact: bit-identical (bf16: round-to-nearest-even of the fp32 value).
Each test prints its ratios ("[edge-acc] ...", pytest -s; RoPE: also `use`, the share of the whole bar taken) before it
asserts; profiles/edge_kernels_accuracy_mi355x.txt records them.
"""
import pytest
import torch

from tests import edge_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
MARGIN = 4.0
GUARD = 64  # elements after (and `off` elements before) every flat buffer
GUARD_ROWS = 2
SENTINEL = -777.0
NAME = {F32: "fp32", BF16: "bf16"}
BOTH = (F32, BF16)
EPI_NONE, EPI_BIAS, EPI_BIAS_SILU = 0, 1, 4
EPI_NAME = {EPI_NONE: "none", EPI_BIAS: "bias", EPI_BIAS_SILU: "bias_silu"}

# worst |fast - fp64| of cs - sn and cs + sn per octave of |theta|: [0, 1/4), [1/4, 1/2), ..., [16, 32)
# (tools/probes/probe_fastmath.hip on one MI355X; the only constants of this file that come from a measurement)
PROBED_WORST = (2.325e-07, 2.600e-07, 4.930e-07, 9.000e-07, 2.053e-06, 3.700e-06, 7.819e-06, 1.460e-05)


def e_fast(a):
    """E_FAST(|theta|): twice the probed worst of the octave |theta| lies in."""
    assert a.max() < 32.0
    octave = (torch.floor(torch.log2(a.double().clamp_min(2.0 ** -10))) + 3).clamp(0, len(PROBED_WORST) - 1).long()
    return 2.0 * torch.tensor(PROBED_WORST, dtype=F64)[octave]


# ---------------------------------------------------------------------------------------------------------------- buffers
class Buf:
    """A [rows, ld] device buffer (a flat one: rows = 1) behind `off` guard elements and in front of GUARD_ROWS guard rows plus
    GUARD elements, sentinel-filled; `init` (a [rows, <= ld] tensor) goes to its top-left corner."""

    def __init__(self, rows, ld, dtype=F32, off=0, init=None, fill=SENTINEL):
        self.rows, self.ld, self.off = rows, ld, off
        self.n = (rows + (GUARD_ROWS if rows > 1 else 0)) * ld
        host = torch.full((off + self.n + GUARD,), fill, dtype=dtype)
        if init is not None:
            assert init.dtype == dtype
            host[off:off + self.n].view(-1, ld)[:init.shape[0], :init.shape[1]] = init
        self.host, self.dev = host, host.cuda()

    def ptr(self, col=0):
        return self.dev.data_ptr() + (self.off + col) * self.dev.element_size()

    def unchanged(self):
        return torch.equal(self.dev.cpu(), self.host)

    def read(self, cols=None, col0=0):
        """The block [rows, col0 : col0 + cols] the kernel owns; everything else must be what it was."""
        cols = self.ld - col0 if cols is None else cols
        now = self.dev.cpu()
        blk = now[self.off:self.off + self.n].view(-1, self.ld)[:self.rows, col0:col0 + cols].clone()
        now[self.off:self.off + self.n].view(-1, self.ld)[:self.rows, col0:col0 + cols] = \
            self.host[self.off:self.off + self.n].view(-1, self.ld)[:self.rows, col0:col0 + cols]
        assert torch.equal(now, self.host), "the kernel wrote outside the block it owns"
        return blk


def flat(t, off=0, dtype=None):
    """An input tensor as one row."""
    return Buf(1, t.numel(), dtype or t.dtype, off=off, init=t.reshape(1, -1))


def out_flat(n, dtype=F32, off=0):
    return Buf(1, n, dtype, off=off)


def call(name, *args):
    from uwudiff_amd import lib as L

    L.call(name, *args, L.stream())
    torch.cuda.synchronize()


class Bars:
    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, name, got, ref, ref32, **kw):
        """With an `extra` term the line also shows `use`, the worst share of the whole bar (MARGIN * unit + extra) taken."""
        e32, r = O.ratio(got, ref, ref32, **kw)
        use = f", use {O.bar_use(got, ref, ref32, margin=MARGIN, **kw):.2f}" if kw.get("extra") is not None else ""
        self.rows.append((name, f"E32 {e32:.1e}{use}", r))

    def add_bound(self, name, got, ref, bound):
        """A plain bound: the ratio is |got - ref| / bound * MARGIN, so that the bar is the same MARGIN."""
        err = (got.double() - ref).abs() / bound
        r = err.max().item() * MARGIN if bool(torch.isfinite(got.double()).all()) else float("inf")
        self.rows.append((name, "E32 0.0e+00", r if r == r else float("inf")))

    def done(self):
        print(f"[edge-acc] {self.label:<52s} " + "  ".join(f"{n}={r:.2f}({e})" for n, e, r in self.rows))
        bad = [(n, r) for n, _, r in self.rows if not r <= MARGIN]
        assert not bad, f"{self.label}: ratio to the bar's unit above {MARGIN}: {bad}"


# ----------------------------------------------------------------------------------------------------------------- skinny
# M, N, K, what it reaches (uwu_skinny_linear_fwd: MT = 16 / 32 / 64 for M <= 16 / <= 32 / above; NPW = 64 / MT columns per wave)
SKINNY_FWD = [
    (1, 1, 4, "degenerate everything"),
    (16, 17, 68, "<16,4> full; N leaves a one-column workgroup; K off the 64 grid"),
    (17, 9, 132, "<32,2> at its lowest M"),
    (32, 70, 36, "<32,2> full; K < 64"),
    (33, 5, 260, "<64,1> at its lowest M"),
    (64, 33, 496, "LDS exactly at what uwu_skinny_linear_ok admits: 64*496*4 + 64*64 = 131072"),
    (1, 8, 32752, "the largest K admitted at M = 1"),
]
# (uwu_skinny_linear_dgrad: R = 4 / 8 / 16 rows per wave by M, KC = 4 / 6 / 8 by K; NS = the slab length)
SKINNY_DGRAD = [
    (16, 100, 256, "<4,4>"),
    (5, 17, 257, "<4,6>"),
    (16, 3, 512, "<4,8>"),
    (17, 33, 1, "<8,4>"),
    (32, 1700, 384, "<8,6>, NS = 32 with a ragged last slab"),
    (20, 40, 385, "<8,8>"),
    (33, 70, 255, "<16,4>"),
    (64, 50, 320, "<16,6>"),
    (64, 33, 496, "<16,8>"),
    (1, 1700, 8, "NS clamped by 16 M"),
    (64, 49300, 4, "NS clamped by the LDS cap, 512"),
]
SKINNY_ALIGN = [(16, 17, 68), (17, 9, 132), (33, 5, 260)]


def _ids(cases):
    return [f"{M}x{N}x{K}" for M, N, K, *_ in cases]


def check_skinny_fwd(M, N, K, epi, off):
    x, w, b, _ = O.linear_inputs(M, N, K)
    X, W, Bi = flat(x), flat(w, off), flat(b, off)
    Y, Y2 = out_flat(M * N, off=off), out_flat(M * N, off=off)
    call("uwu_skinny_linear_fwd", X.ptr(), W.ptr(), Bi.ptr() if epi != EPI_NONE else None, Y.ptr(), Y2.ptr(), M, N, K, epi)
    assert X.unchanged() and W.unchanged() and Bi.unchanged(), "an input was written"
    y = Y.read().view(M, N)
    bias = b if epi != EPI_NONE else None
    (ref, A), (ref32, _) = O.linear(x, w, bias), O.linear(x, w, bias, dtype=F32)
    bars = Bars(f"skinny_fwd {M}x{N}x{K} {EPI_NAME[epi]} off{off}")
    bars.add("Y", y, ref, ref32, A=A)
    if epi == EPI_BIAS_SILU:
        s = O.silu(y)  # of the device's own Y: the GEMM's error is not in it
        bars.add_bound("Y2", Y2.read().view(M, N), s, 1e-6 * s.abs() + 1e-6 * s.abs().max())
        if N >= 2:
            assert y.min() < -10 and y.max() > 10, "the bias does not reach both tails"
    else:
        assert Y2.unchanged(), "Y2 written without the SiLU epilogue"
    bars.done()


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_BIAS, EPI_BIAS_SILU], ids=EPI_NAME.get)
@pytest.mark.parametrize("M,N,K,why", SKINNY_FWD, ids=_ids(SKINNY_FWD))
def test_skinny_fwd(M, N, K, why, epi):
    check_skinny_fwd(M, N, K, epi, 0)


def check_skinny_wgrad(M, N, K, with_db, off):
    x, _, _, dy = O.linear_inputs(M, N, K)
    g = torch.Generator().manual_seed(5)
    fill_w, fill_b = torch.rand(N, K, generator=g) - 0.5, torch.rand(N, generator=g) - 0.5
    X, DY = flat(x), flat(dy, off)
    DW, DB = flat(fill_w, off), flat(fill_b, off)
    call("uwu_skinny_linear_wgrad", DY.ptr(), X.ptr(), DW.ptr(), DB.ptr() if with_db else None, M, N, K)
    assert X.unchanged() and DY.unchanged(), "an input was written"
    ref, ref32 = O.linear_wgrad(dy, x), O.linear_wgrad(dy, x, dtype=F32)
    bars = Bars(f"skinny_wgrad {M}x{N}x{K} {'db' if with_db else 'no_db'} off{off}")
    # accumulated onto a nonzero fill, which is subtracted: the fill is one more term of every sum
    dw = DW.read().view(N, K).double() - fill_w.double()
    bars.add("dW", dw, ref["dw"], (fill_w + ref32["dw"]).double() - fill_w.double(), A=ref["A_dw"] + fill_w.abs().double())
    if with_db:
        db = DB.read().view(N).double() - fill_b.double()
        bars.add("db", db, ref["db"], (fill_b + ref32["db"]).double() - fill_b.double(), A=ref["A_db"] + fill_b.abs().double())
    else:
        assert DB.unchanged(), "db written although none was asked for"
    bars.done()


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "no_db"])
@pytest.mark.parametrize("M,N,K,why", SKINNY_FWD, ids=_ids(SKINNY_FWD))
def test_skinny_wgrad(M, N, K, why, with_db):
    check_skinny_wgrad(M, N, K, with_db, 0)


def check_skinny_dgrad(M, N, K, off):
    _, w, _, dy = O.linear_inputs(M, N, K)
    (ref, A), (ref32, _) = O.linear_dgrad(dy, w), O.linear_dgrad(dy, w, dtype=F32)
    DY, W = flat(dy, off), flat(w, off)
    for run in (1, 2):  # the slabs meet in atomics: two runs need not be bit-equal, each is held to the bar
        DX = out_flat(M * K, off=off)  # (overwritten, not accumulated: the sentinel must be gone)
        call("uwu_skinny_linear_dgrad", DY.ptr(), W.ptr(), DX.ptr(), M, N, K)
        assert DY.unchanged() and W.unchanged(), "an input was written"
        bars = Bars(f"skinny_dgrad {M}x{N}x{K} off{off} run{run}")
        bars.add("dX", DX.read().view(M, K), ref, ref32, A=A)
        bars.done()


@pytest.mark.parametrize("M,N,K,why", SKINNY_DGRAD, ids=_ids(SKINNY_DGRAD))
def test_skinny_dgrad(M, N, K, why):
    check_skinny_dgrad(M, N, K, 0)


@pytest.mark.parametrize("M,N,K", SKINNY_ALIGN, ids=_ids(SKINNY_ALIGN))
def test_skinny_pointers_at_a_one_element_offset(M, N, K):
    """In use W, bias, dW and db are views at arbitrary element offsets of the flat parameter store; only X must be 16-byte
    aligned.  Here every pointer but X (W, bias, Y, Y2, dY, dW, db, dX) sits one element into its buffer."""
    check_skinny_fwd(M, N, K, EPI_BIAS_SILU, 1)
    check_skinny_fwd(M, N, K, EPI_NONE, 1)
    check_skinny_wgrad(M, N, K, True, 1)
    check_skinny_dgrad(M, N, K, 1)


def test_skinny_ok_on_both_sides_of_each_boundary():
    from uwudiff_amd import lib as L

    ok = L.load().uwu_skinny_linear_ok
    assert all(ok(M, N, K) for M, N, K, _ in SKINNY_FWD)
    assert ok(64, 33, 496) and not ok(64, 33, 500)  # 64 * 500 * 4 + 64 * 64 > 128 KB
    assert ok(1, 8, 32752) and not ok(1, 8, 32756)
    assert ok(64, 384, 4) and not ok(65, 384, 4) and not ok(0, 384, 4)
    assert ok(16, 17, 68) and not ok(16, 17, 70) and not ok(16, 17, 67) and not ok(16, 17, 0)
    assert not ok(16, 0, 68)


def test_skinny_refusals_launch_nothing():
    from uwudiff_amd import lib as L

    M, N, K = 16, 17, 68
    x, w, b, dy = O.linear_inputs(M, N, K)
    # X one element off 16-byte alignment: the vector loads of the staging loop would fault or read the wrong rows
    X1, W, Bi, DY = flat(x, 1), flat(w), flat(b), flat(dy)
    Y, Y2, DW, DB = out_flat(M * N), out_flat(M * N), out_flat(N * K), out_flat(N)
    with pytest.raises(L.UwuError, match="aligned"):
        call("uwu_skinny_linear_fwd", X1.ptr(), W.ptr(), Bi.ptr(), Y.ptr(), Y2.ptr(), M, N, K, EPI_BIAS_SILU)
    with pytest.raises(L.UwuError, match="aligned"):
        call("uwu_skinny_linear_wgrad", DY.ptr(), X1.ptr(), DW.ptr(), DB.ptr(), M, N, K)
    # M = 65 for all three, K = 513 for the input gradient (K % 4 != 0 is legal there: K = 257 runs above)
    X65, DY65 = flat(torch.zeros(65, K)), flat(torch.zeros(65, N))
    DX = out_flat(65 * 513)
    with pytest.raises(L.UwuError, match="not covered"):
        call("uwu_skinny_linear_fwd", X65.ptr(), W.ptr(), Bi.ptr(), Y.ptr(), Y2.ptr(), 65, N, K, EPI_BIAS)
    with pytest.raises(L.UwuError, match="not covered"):
        call("uwu_skinny_linear_wgrad", DY65.ptr(), X65.ptr(), DW.ptr(), DB.ptr(), 65, N, K)
    with pytest.raises(L.UwuError, match="not covered"):
        call("uwu_skinny_linear_dgrad", DY65.ptr(), W.ptr(), DX.ptr(), 65, N, K)
    W513 = flat(torch.zeros(N, 513))
    with pytest.raises(L.UwuError, match="not covered"):
        call("uwu_skinny_linear_dgrad", DY.ptr(), W513.ptr(), DX.ptr(), M, N, 513)
    with pytest.raises(L.UwuError, match="not covered"):
        call("uwu_skinny_linear_fwd", X65.ptr(), W.ptr(), Bi.ptr(), Y.ptr(), Y2.ptr(), M, N, 70, EPI_BIAS)
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in (Y, Y2, DW, DB, DX)), "a refused call wrote to an output"


# ----------------------------------------------------------------------------------------------------- timestep embedding
T_VALUES = (0.0, 1e-3, 0.5, 1.0, 14.6146, 37.0, 250.5, 999.0, 999.999)
MAX_PERIOD = 10000.0


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
@pytest.mark.parametrize("dim", [2, 6, 256, 320])
@pytest.mark.parametrize("B", [1, 5, 300])
def test_timestep_embedding(B, dim, dtype):
    """B * dim / 2 is off the 256-thread grid in all but one case; B = 1 takes t = 999.999, B = 5 the five largest t, B = 300
    every t."""
    t = torch.tensor([T_VALUES[(i + 8 * B) % len(T_VALUES)] for i in range(B)])
    Tb, out = flat(t), out_flat(B * dim, dtype)
    call("uwu_timestep_embedding", Tb.ptr(), B, dim, MAX_PERIOD, out.ptr(), 0 if dtype == F32 else 1)
    assert Tb.unchanged()
    ref, ref32 = O.timestep_features(t, dim, MAX_PERIOD), O.timestep_features(t, dim, MAX_PERIOD, dtype=F32)
    bars = Bars(f"timestep_embedding B{B} dim{dim} {NAME[dtype]}")
    bars.add("emb", out.read().view(B, dim), ref, ref32, floor=O.timestep_budget(t, dim, MAX_PERIOD), bf16_out=dtype == BF16)
    bars.done()


def test_timestep_embedding_refuses_odd_dim():
    from uwudiff_amd import lib as L

    Tb, out = flat(torch.tensor([1.0, 2.0])), out_flat(2 * 8)
    with pytest.raises(L.UwuError):
        call("uwu_timestep_embedding", Tb.ptr(), 2, 7, MAX_PERIOD, out.ptr(), 0)
    assert out.unchanged()


# --------------------------------------------------------------------------------------------------- patchify / unpatchify
PATCH = [
    (1, 1, 1, 1, 1, "degenerate"),
    (2, 4, 8, 12, 2, "non-square"),
    (1, 3, 12, 8, 4, "p = 4"),
    (3, 4, 256, 256, 2, "786432 elements: the grid-stride loop runs twice"),
]


def _dt(dtype):
    return 0 if dtype == F32 else 1


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
@pytest.mark.parametrize("B,C,H,W,p,why", PATCH, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-p{c[4]}" for c in PATCH])
def test_patchify_unpatchify_exact(B, C, H, W, p, why, dtype):
    g = torch.Generator().manual_seed(B + 10 * H + p)
    n, kp = B * C * H * W, C * p * p
    img = torch.randn(B, C, H, W, generator=g)
    # patchify: the fp32 image rounded once (bf16: to nearest even), at the mapped index
    IMG, TOK = flat(img), out_flat(n, dtype)
    call("uwu_patchify", IMG.ptr(), TOK.ptr(), B, C, H, W, p, _dt(dtype))
    assert IMG.unchanged()
    tok = TOK.read().view(n // kp, kp)
    assert torch.equal(tok, O.patchify(img, p).to(dtype)), "patchify is not bit-identical"
    # unpatchify: other tokens, widened exactly
    tok2 = torch.randn(n // kp, kp, generator=g).to(dtype)
    TOK2, IMG2 = flat(tok2), out_flat(n)
    call("uwu_unpatchify", TOK2.ptr(), _dt(dtype), IMG2.ptr(), B, C, H, W, p)
    assert TOK2.unchanged()
    assert torch.equal(IMG2.read().view(B, C, H, W), O.unpatchify(tok2.float(), B, C, H, W, p)), "unpatchify is not bit-identical"
    # the round trip from the device's own tokens
    IMG3 = out_flat(n)
    call("uwu_unpatchify", TOK.ptr(), _dt(dtype), IMG3.ptr(), B, C, H, W, p)
    assert torch.equal(IMG3.read().view(B, C, H, W), img.to(dtype).float()), "the round trip is not the rounded image"


def test_patchify_refuses_ragged_images():
    from uwudiff_amd import lib as L

    IMG, TOK = flat(torch.zeros(1 * 2 * 6 * 8)), out_flat(2 * 6 * 8)
    IMG_out = out_flat(2 * 6 * 8)
    for H, W in ((6, 8), (8, 6)):  # p = 4 divides one side only
        with pytest.raises(L.UwuError):
            call("uwu_patchify", IMG.ptr(), TOK.ptr(), 1, 2, H, W, 4, 0)
        with pytest.raises(L.UwuError):
            call("uwu_unpatchify", IMG.ptr(), 0, IMG_out.ptr(), 1, 2, H, W, 4)
    assert TOK.unchanged() and IMG_out.unchanged()


# ---------------------------------------------------------------------------------------------------------------- add_pos
ADD_POS = [(1, 1, 4, "degenerate"), (3, 16, 8, "small"), (2, 257, 388, "off-grid sizes"), (6, 1024, 384, "past the grid cap")]


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
@pytest.mark.parametrize("B,T,D,why", ADD_POS, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in ADD_POS])
def test_add_pos_exact(B, T, D, why, dtype):
    g = torch.Generator().manual_seed(B + T + D)
    x, pos = torch.randn(B * T, D, generator=g).to(dtype), torch.randn(T, D, generator=g)
    X, P = flat(x), flat(pos)
    call("uwu_add_pos", X.ptr(), P.ptr(), B, T, D, _dt(dtype))
    assert P.unchanged()
    assert torch.equal(X.read().view(B * T, D), O.add_pos(x, pos, B, T, D)), "add_pos is not the fp32 sum rounded once"


# -------------------------------------------------------------------------------------------------------------- transpose
TRANSPOSE = [(1, 1, 1, 1), (31, 33, 33, 31), (32, 32, 40, 48), (65, 97, 97, 65), (384, 1536, 1536, 384)]


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", TRANSPOSE, ids=["x".join(map(str, c)) for c in TRANSPOSE])
def test_transpose_bf16_exact(rows, cols, ld_src, ld_dst):
    g = torch.Generator().manual_seed(rows + cols)
    src = torch.randn(rows, ld_src, generator=g).bfloat16()  # (the padding columns of the source hold data too)
    S, Dst = Buf(rows, ld_src, BF16, init=src), Buf(cols, ld_dst, BF16)
    call("uwu_transpose_bf16", S.ptr(), Dst.ptr(), rows, cols, ld_src, ld_dst)
    assert S.unchanged()
    assert torch.equal(Dst.read(cols=rows), O.transpose(src[:, :cols])), "the transpose is not bit-identical"


def test_transpose_bf16_refuses_short_leading_dimensions():
    from uwudiff_amd import lib as L

    S, Dst = Buf(4, 8, BF16, init=torch.zeros(4, 8, dtype=BF16)), Buf(8, 4, BF16)
    with pytest.raises(L.UwuError):
        call("uwu_transpose_bf16", S.ptr(), Dst.ptr(), 4, 8, 7, 4)
    with pytest.raises(L.UwuError):
        call("uwu_transpose_bf16", S.ptr(), Dst.ptr(), 4, 8, 8, 3)
    assert Dst.unchanged()


# ------------------------------------------------------------------------------------------------------------------- RoPE
def _expand_pairs(v):
    """[rows, H, d/2] -> [rows, H d]: one value per pair, for both of its elements."""
    return v.repeat_interleave(2, -1).reshape(v.shape[0], -1)


def check_rope(label, rows, H, d, packed, pos_rows, dtype, modes):
    """Forward, backward out of place (with and without the log-frequency gradients) and backward in place on the column
    blocks of a [rows, ldx] buffer: ldx = H d (one block) or 3 H d (a packed qkv buffer: the q and the k block are rotated by
    one call each, the v block must stay untouched)."""
    D = H * d
    nblk, ldx = (2, 3 * D) if packed else (1, D)
    ins = [O.rope_inputs(rows, H, d, pos_rows, dtype, seed=blk) for blk in range(nblk)]
    _, _, pos, fh, fw = ins[0]  # one set of positions and frequencies; x and dy differ per block
    g = torch.Generator().manual_seed(99)
    xfull, dyfull = torch.randn(rows, ldx, generator=g).to(dtype), torch.randn(rows, ldx, generator=g).to(dtype)
    for blk in range(nblk):
        xfull[:, blk * D:(blk + 1) * D], dyfull[:, blk * D:(blk + 1) * D] = ins[blk][0], ins[blk][1]
    X, DY = Buf(rows, ldx, dtype, init=xfull), Buf(rows, ldx, dtype, init=dyfull)
    pos_full = pos[torch.arange(rows) % pos.shape[0]].contiguous()
    P, PF, FH, FW = flat(pos), flat(pos_full), flat(fh), flat(fw)
    th = O.rope_angles(pos, fh, fw, rows).abs()
    ef = _expand_pairs(e_fast(th))
    bf = dtype == BF16
    esz = 4 if dtype == F32 else 2
    bars = Bars(label)

    def bwd(dx_buf, dy_buf, blk, dfh, dfw):
        c = blk * D
        if pos_rows:
            call("uwu_axial_rope_bwd_shared", X.ptr(c), dy_buf.ptr(c), P.ptr(), pos_rows, FH.ptr(), FW.ptr(), dx_buf.ptr(c),
                 dfh.ptr() if dfh else None, dfw.ptr() if dfw else None, rows, H, d, ldx, _dt(dtype))
        else:
            call("uwu_axial_rope_bwd", X.ptr(c), dy_buf.ptr(c), P.ptr(), FH.ptr(), FW.ptr(), dx_buf.ptr(c),
                 dfh.ptr() if dfh else None, dfw.ptr() if dfw else None, rows, H, d, ldx, _dt(dtype))

    for blk in range(nblk):
        x, dy = ins[blk][0], ins[blk][1]
        c, tag = blk * D, ("qk"[blk] if packed else "")
        ref, ref32 = O.rope_bwd(x, dy, pos, fh, fw, e_fast=e_fast), O.rope_bwd(x, dy, pos, fh, fw, dtype=F32)
        if "fwd" in modes:
            Y = Buf(rows, ldx, dtype)
            call("uwu_axial_rope_fwd", X.ptr(c), PF.ptr(), FH.ptr(), FW.ptr(), Y.ptr(c), rows, H, d, ldx, _dt(dtype))
            bars.add("y" + tag, Y.read(cols=D, col0=c), O.rope_fwd(x, pos, fh, fw), O.rope_fwd(x, pos, fh, fw, dtype=F32),
                     A=x.double().abs(), extra=x.double().abs() * ef, bf16_out=bf)
        if "bwd" in modes:
            DX = Buf(rows, ldx, dtype)
            DFH, DFW = flat(torch.zeros_like(fh)), flat(torch.zeros_like(fw))
            bwd(DX, DY, blk, DFH, DFW)
            bars.add("dx" + tag, DX.read(cols=D, col0=c), ref["dx"], ref32["dx"], A=dy.double().abs(),
                     extra=dy.double().abs() * ef, bf16_out=bf)
            for k, buf in (("dfh", DFH), ("dfw", DFW)):
                bars.add(k + tag, buf.read().view(fh.shape), ref[k], ref32[k], A=ref["A_" + k], extra=ref["F_" + k])
        if "bwd_nodf" in modes:
            DX = Buf(rows, ldx, dtype)
            bwd(DX, DY, blk, None, None)
            bars.add("dx'" + tag, DX.read(cols=D, col0=c), ref["dx"], ref32["dx"], A=dy.double().abs(),
                     extra=dy.double().abs() * ef, bf16_out=bf)
    if "inplace" in modes:  # dx == dy, every block in the same buffer, as the attention backward leaves dq' and dk'
        IO = Buf(rows, ldx, dtype, init=dyfull)
        DFH, DFW = flat(torch.zeros_like(fh)), flat(torch.zeros_like(fw))
        for blk in range(nblk):
            bwd(IO, IO, blk, DFH, DFW)
        refs = [O.rope_bwd(ins[b][0], ins[b][1], pos, fh, fw, e_fast=e_fast) for b in range(nblk)]
        refs32 = [O.rope_bwd(ins[b][0], ins[b][1], pos, fh, fw, dtype=F32) for b in range(nblk)]
        now = IO.dev.cpu()[:IO.n].view(-1, ldx)
        if packed:
            assert torch.equal(now[:rows, 2 * D:], dyfull[:, 2 * D:]), "the v block was written"
        assert torch.equal(now[rows:], IO.host[:IO.n].view(-1, ldx)[rows:]) and torch.equal(IO.dev.cpu()[IO.n:], IO.host[IO.n:])
        for blk in range(nblk):
            dyb = ins[blk][1].double().abs()
            bars.add("dx=" + ("qk"[blk] if packed else ""), now[:rows, blk * D:(blk + 1) * D], refs[blk]["dx"], refs32[blk]["dx"],
                     A=dyb, extra=dyb * ef, bf16_out=bf)
        for k, buf in (("dfh", DFH), ("dfw", DFW)):  # both blocks accumulate into one gradient
            bars.add(k + "=", buf.read().view(fh.shape), sum(r[k] for r in refs), sum(r[k].double() for r in refs32),
                     A=sum(r["A_" + k] for r in refs), extra=sum(r["F_" + k] for r in refs))
    assert all(t.unchanged() for t in (X, DY, P, PF, FH, FW)), "an input was written"
    bars.done()


ROPE_T = 5


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
@pytest.mark.parametrize("shared", [False, True], ids=["per_row", "shared"])
@pytest.mark.parametrize("packed", [False, True], ids=["ldx=Hd", "ldx=3Hd"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("d", [4, 8, 64, 72])
def test_rope(d, H, packed, shared, dtype):
    """rows = 3 T; shared: positions [T, 2] used by row % T (uwu_axial_rope_bwd_shared), else one position per row."""
    rows = 3 * ROPE_T
    label = f"rope d{d} H{H} ldx={'3Hd' if packed else 'Hd'} {'shared' if shared else 'per_row'} {NAME[dtype]}"
    check_rope(label, rows, H, d, packed, ROPE_T if shared else 0, dtype, ("fwd", "bwd", "bwd_nodf", "inplace"))


def test_rope_past_the_grid_cap():
    """rows H d / 2 = 524800 pairs > 2048 x 256 threads: the grid-stride loop takes a second trip; 2050 atomics per frequency."""
    check_rope("rope d64 H8 rows2050 ldx=Hd per_row bf16", 2050, 8, 64, False, 0, BF16, ("fwd", "bwd"))


@pytest.mark.parametrize("T,H,d", [(1, 3, 8), (77, 2, 64), (256, 3, 72)])
def test_rope_table(T, H, d):
    D, ldt = H * d, H * d + 8
    _, _, pos, fh, fw = O.rope_inputs(T, H, d, 0, F32, seed=7)
    P, FH, FW = flat(pos), flat(fh), flat(fw)
    TAB = Buf(T, ldt)
    call("uwu_axial_rope_table", P.ptr(), FH.ptr(), FW.ptr(), TAB.ptr(), T, H, d, ldt)
    tab = TAB.read(cols=D)  # (the 8 padding columns and the guard rows keep their sentinel)
    ones = torch.ones(T, D)
    X, Y = Buf(T, D, init=ones), Buf(T, D)
    call("uwu_axial_rope_fwd", X.ptr(), P.ptr(), FH.ptr(), FW.ptr(), Y.ptr(), T, H, d, D, 0)
    assert torch.equal(tab, Y.read()), "the table is not the forward kernel applied to ones"
    bars = Bars(f"rope_table T{T} H{H} d{d}")
    ef = _expand_pairs(e_fast(O.rope_angles(pos, fh, fw, T).abs()))
    bars.add("tab", tab, O.rope_table(pos, fh, fw, T), O.rope_table(pos, fh, fw, T, dtype=F32), A=ones.double(), extra=ef)
    bars.done()
    assert P.unchanged() and FH.unchanged() and FW.unchanged()


def test_rope_refusals():
    from uwudiff_amd import lib as L

    rows, H = 4, 2
    z = torch.zeros(rows, H * 8)
    X, DY, P = Buf(rows, H * 8, init=z), Buf(rows, H * 8, init=z), flat(torch.zeros(rows, 2))
    FH, FW = flat(torch.zeros(H, 2)), flat(torch.zeros(H, 2))
    Y, DF, TAB = Buf(rows, H * 8), out_flat(H * 2), Buf(rows, H * 8)
    with pytest.raises(L.UwuError):  # d % 4 != 0
        call("uwu_axial_rope_fwd", X.ptr(), P.ptr(), FH.ptr(), FW.ptr(), Y.ptr(), rows, H, 6, H * 6, 0)
    with pytest.raises(L.UwuError):
        call("uwu_axial_rope_bwd", X.ptr(), DY.ptr(), P.ptr(), FH.ptr(), FW.ptr(), Y.ptr(), None, None, rows, H, 6, H * 6, 0)
    with pytest.raises(L.UwuError):
        call("uwu_axial_rope_table", P.ptr(), FH.ptr(), FW.ptr(), TAB.ptr(), rows, H, 6, H * 6)
    with pytest.raises(L.UwuError, match="together"):  # dfh without dfw
        call("uwu_axial_rope_bwd", X.ptr(), DY.ptr(), P.ptr(), FH.ptr(), FW.ptr(), Y.ptr(), DF.ptr(), None, rows, H, 8, H * 8, 0)
    with pytest.raises(L.UwuError, match="together"):
        call("uwu_axial_rope_bwd_shared", X.ptr(), DY.ptr(), P.ptr(), rows, FH.ptr(), FW.ptr(), Y.ptr(), None, DF.ptr(), rows, H, 8,
             H * 8, 0)
    with pytest.raises(L.UwuError):  # ldx < H d
        call("uwu_axial_rope_fwd", X.ptr(), P.ptr(), FH.ptr(), FW.ptr(), Y.ptr(), rows, H, 8, H * 8 - 4, 0)
    assert Y.unchanged() and DF.unchanged() and TAB.unchanged()
