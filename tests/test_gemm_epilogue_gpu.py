"""Every uwu_gemm kernel family's epilogue against an exact / float64 reference (tests/gemm_oracle.py).

All families finish through epilogue_tile / epi_prefetch / flush_cs of csrc/gemm_shared.h, so comparing one family with
another (tests/test_gemm_gpu.py) cannot see an error in that shared code.  Here every case
  * sets the family's switches, runs ONE uwu_gemm call and asserts that uwu_gemm_last_kernel() names the intended family;
  * runs with compact leading dimensions and with lda, ldb, ldc, ldaux each 16 bytes over the row length (the two gemm_kernel
    families also with ldc = ldaux = N + 4 on bf16: the 8-byte store and aux forms at an N that otherwise takes the 16-byte ones);
  * writes into buffers with guard columns, two guard rows and 8 guard elements after the column sums, all holding a sentinel
    that must survive bit for bit, as must the operand, bias and aux buffers (whose padding holds the sentinel too: an operand
    read past K would show in the result).

Exact stage (integer operands, oracle.exact_operands): the first output equals the exact result rounded once to the output
type, bit for bit; dGELU equals exact * {0.5, 1, 0} within 1e-20; the column sums, accumulated by two calls on top of an integer
fill, equal fill + 2 * exact sums within 1e-12; the activation outputs meet the bar below on acc + bias known exactly.

Accuracy stage (random operands, one shape per family): per element
    |got - ref| <= 4 * max(E32, 2^-23 * A) + (bf16 output ? 2^-8 * |ref| : 0)
E32 = max over the tensor of |the same formulas in torch fp32 on the CPU - fp64|; A = the absolute sum of the terms for the
matmul outputs (|A| |B| + |bias|, times |gelu'| for dGELU) and the column sums (that, summed over the rows, plus the fill),
max |ref| for the activation outputs.  The margin of 4 is the one of the LayerNorm and attention suites (summation order); the
worst measured ratio per family and output is in profiles/gemm_epilogue_accuracy_mi355x.txt, and every test prints its
ratios ("[gemm-acc] ...", pytest -s) before it asserts.
Measured with that margin: GELU / SiLU (x * sigmoid with the 1-ulp hardware exp2 and reciprocal) 1.58 at worst, the matmul
outputs 1.17, the column sums 0.11.  dGELU's C alone exceeds it: 4.16 (bf16 operands, fp32 C, E32 1.6e-6, at aux = 4.59), because
forming 1 - s by subtraction in gelu'(x) = s + x s (1 - s) P(x) leaves an absolute error of up to 2^-23 in 1 - s, which |x| P(x)
multiplies by 20 at x = 4; torch's fp32 form 1 - tanh^2 = 4 s (1 - s), and with it E32, sees a quarter of it.  The kernel's
formula evaluated in torch fp32 on the CPU gives the same 4.160513 bit for bit, so this is rounding of the function's form and no
indexing error: the margin stays, and the function's own term (oracle.dgelu_own_error holds the derivation) is added to the
bar, + |acc| 2^-23 |x| s(x) P(x) per element, once, as the bf16 term is.  Both ratios are printed ("c" and "c(raw)").

Why each shape reaches its family (csrc/gemm.hip dispatch_trans; all with ragged last row tiles):
  gemm_reg   P8 = P8N = R3 = M64 = 0, K % 64 != 0 (bf16) / K % 32 != 0 (fp32): gemm_kernel with register staging
  gemm_gl    same switches, K % 64 == 0: gemm_kernel with LDS-DMA; bf16 -> bf16 none / bias / bias_gelu are compile-time
             epilogues, the others and every fp32-C call the run-time one (EPI = -1)
  m64        fewer than 256 tiles of 128x128, K % 64 == 0, the ring declines (too few tiles)
  p8         UWU_GEMM_P8=1: K % 64 == 0, K >= 128; p8_narrow: N % 8 == 4 (8-byte stores)
  p8n        UWU_GEMM_P8N=1: N % 384 == 0 and N % 256 != 0 (a multiple of 768 goes elsewhere), K % 128 == 0, K >= 256
  r3_256     86 x 3 tiles of 256x128 >= 256 with K >= 640; N % 256 != 0 and N % 384 != 0 keep the 256x256 / 192x384 kernels away;
             bias_silu, dgelu and fp32 C take its run-time epilogue
  big        128 x 2 tiles >= 256, K = 640, N % 256 == 0
  wide       UWU_GEMM_WIDE=1, N = 384, 86 x 3 ring tiles
  r3_128     trans_b, 86 x 3 tiles of 128x128 >= 128, 43 x 3 of 256x128 < 512, K % 64 != 0 so that the 64x128 kernel declines
  as         K = 384, M = 65536 = 256 * 256, N = 1088 in [1024, 2048], a multiple of 64
"""
import pytest
import torch

from tests import gemm_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
MARGIN = 4.0
GUARD_ROWS, GUARD_ELEMS = 2, 8
SENTINEL = -777.0
FILL = 3.0  # the column-sum accumulator's previous contents
NAME = {F32: "fp32", BF16: "bf16"}


# ---------------------------------------------------------------------------------------------------------------- device
def _place(t, ld):
    """[rows, n] -> device [rows, ld], the padding columns holding the sentinel."""
    buf = torch.full((t.shape[0], ld), SENTINEL, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.cuda()


def _pad(ld_mode, dtype):
    return 0 if ld_mode != "pad" else (8 if dtype == BF16 else 4)


def set_switches(monkeypatch, env):
    for name in O.SWITCHES:
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)


def dev_gemm(ops, M, N, K, layout, out_dtype, epi, with_cs, ld_mode, runs=1):
    """`runs` uwu_gemm calls into the same guarded buffers -> (kernel name, C, C2 or None, column sums or None) on the CPU.
    Asserts that nothing outside [M, N] of the outputs, outside [N] of the column sums, or in any input buffer changed."""
    from uwudiff_amd import lib as L

    ta, tb = layout
    a, b, bias, aux = ops
    op_dtype = a.dtype
    pa, pc = _pad(ld_mode, op_dtype), _pad(ld_mode, out_dtype)
    four = 4 if ld_mode == "c4" else 0
    lda, ldb = a.shape[1] + pa, b.shape[1] + pa
    ldc, ldaux = N + pc + four, N + pa + four
    ad, bd = _place(a, lda), _place(b, ldb)
    has_bias = epi in (O.EPI_BIAS, O.EPI_BIAS_GELU, O.EPI_BIAS_SILU)
    two = epi in (O.EPI_BIAS_GELU, O.EPI_BIAS_SILU)
    biasd = torch.cat([bias, torch.full((GUARD_ELEMS,), SENTINEL)]).cuda() if has_bias else None
    auxd = _place(aux, ldaux) if epi == O.EPI_DGELU else None
    inputs = [(t, t.clone()) for t in (ad, bd, biasd, auxd) if t is not None]
    c = torch.full((M + GUARD_ROWS, ldc), SENTINEL, device="cuda", dtype=out_dtype)
    c2 = torch.full_like(c, SENTINEL) if two else None
    cs = torch.cat([torch.full((N,), FILL), torch.full((GUARD_ELEMS,), SENTINEL)]).cuda() if with_cs else None
    second = cs if epi == O.EPI_DGELU else c2
    for _ in range(runs):
        L.call("uwu_gemm", L.ptr(ad), L.ptr(bd), L.ptr(c), L.ptr(second), L.ptr(biasd), L.ptr(auxd), M, N, K, lda, ldb, ldc,
               ldaux if auxd is not None else 0, int(ta), int(tb), L.dt(ad), L.dt(c), epi, 1, L.stream())
    name = L.load().uwu_gemm_last_kernel().decode()
    torch.cuda.synchronize()
    for t in (c, c2):
        if t is not None:
            assert torch.equal(t[M:], torch.full_like(t[M:], SENTINEL)), f"{name}: wrote past row M"
            assert torch.equal(t[:M, N:], torch.full_like(t[:M, N:], SENTINEL)), f"{name}: wrote past column N"
    if cs is not None:
        assert torch.equal(cs[N:], torch.full_like(cs[N:], SENTINEL)), f"{name}: column sums written past N"
    for t, before in inputs:
        assert torch.equal(t, before), f"{name}: an input buffer changed"
    return (name, c[:M, :N].cpu(), c2[:M, :N].cpu() if two else None, cs[:N].cpu() if cs is not None else None)


# ------------------------------------------------------------------------------------------------------------------ bars
class Bars:
    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, name, got, ref, ref32, A=None, bf16_out=False, own=None):
        e32, r = O.ratio(got, ref, ref32, A=A, bf16_out=bf16_out, own=own)
        self.rows.append((name, e32, r))
        if own is not None:  # (for the record: the ratio without the function's own error term)
            self.rows.append((name + "(raw)", e32, O.ratio(got, ref, ref32, A=A, bf16_out=bf16_out)[1]))

    def done(self):
        print(f"[gemm-acc] {self.label:<64s} " + "  ".join(f"{n}={r:.2f}(E32 {e:.1e})" for n, e, r in self.rows))
        bad = [(n, r) for n, _, r in self.rows if not r <= MARGIN and not n.endswith("(raw)")]
        assert not bad, f"{self.label}: ratio to max(E32, 2^-23 A) above {MARGIN}: {bad}"


def _ids(stage):
    out = []
    for fam, shape, layout, types, ld, (epi, with_cs) in O.cases(stage):
        ident = (f"{fam.key}-{'x'.join(map(str, shape))}-{O.LAYOUT_NAME[layout]}-{NAME[types[0]]}_{NAME[types[1]]}-{ld}-"
                 f"{O.EPI_NAME[epi]}{'+cs' if with_cs else ''}")
        out.append(pytest.param(fam, shape, layout, types, ld, epi, with_cs, id=ident))
    return out


def _label(stage, fam, shape, layout, types, ld, epi, with_cs):
    return (f"{stage} {fam.key} {'x'.join(map(str, shape))} {O.LAYOUT_NAME[layout]} {NAME[types[0]]}->{NAME[types[1]]} {ld} "
            f"{O.EPI_NAME[epi]}{'+cs' if with_cs else ''}")


# ----------------------------------------------------------------------------------------------------------- exact stage
@pytest.mark.parametrize("fam,shape,layout,types,ld,epi,with_cs", _ids("exact"))
def test_exact(fam, shape, layout, types, ld, epi, with_cs, monkeypatch):
    M, N, K = shape
    op_dtype, out_dtype = types
    set_switches(monkeypatch, fam.env)
    ops = O.operands("exact", M, N, K, *layout, op_dtype)
    name, c, c2, cs = dev_gemm(ops, M, N, K, layout, out_dtype, epi, with_cs, ld, runs=2 if with_cs else 1)
    assert name == fam.kernel, f"the call went to {name!r}, not to {fam.kernel!r}"
    # fp32 on the CPU is exact on these integers (test_gemm_ref_cpu.py: every sum stays below 2^24)
    ref = O.reference_of("exact", M, N, K, *layout, op_dtype, epi, dtype=F32)
    if epi != O.EPI_DGELU:
        assert torch.equal(c, ref["c"].to(out_dtype)), "the first output is not the exact result rounded once"
    else:
        aux = ops[3].float()
        fac = torch.where(aux == 0, 0.5, torch.where(aux > 0, 1.0, 0.0))
        acc = O.products("exact", M, N, K, *layout, op_dtype, F32)[0]
        want = (acc * fac).to(out_dtype)
        torch.testing.assert_close(c.float(), want.float(), rtol=0, atol=1e-20)
        if with_cs:
            sums = FILL + 2.0 * (acc * fac).sum(0, dtype=F64)
            torch.testing.assert_close(cs.double(), sums, rtol=0, atol=1e-12)
    if c2 is not None:
        bars = Bars(_label("exact", fam, shape, layout, types, ld, epi, with_cs))
        v = ref["c"]  # acc + bias, exact
        act = O.gelu_tanh if epi == O.EPI_BIAS_GELU else O.silu
        bars.add("c2", c2, act(v.double()), act(v), bf16_out=out_dtype == BF16)
        bars.done()


# -------------------------------------------------------------------------------------------------------- accuracy stage
def check_random(kind, fam, shape, layout, types, ld, epi, with_cs, monkeypatch, rows=None, cols=None, tag=""):
    M, N, K = shape
    op_dtype, out_dtype = types
    set_switches(monkeypatch, fam.env)
    ops = O.operands(kind, M, N, K, *layout, op_dtype)
    name, c, c2, cs = dev_gemm(ops, M, N, K, layout, out_dtype, epi, with_cs, ld)
    assert name == fam.kernel, f"the call went to {name!r}, not to {fam.kernel!r}"
    ref = O.reference_of(kind, M, N, K, *layout, op_dtype, epi)
    ref32 = O.reference_of(kind, M, N, K, *layout, op_dtype, epi, dtype=F32)
    bf = out_dtype == BF16
    bars = Bars(_label(kind + tag, fam, shape, layout, types, ld, epi, with_cs))
    sel = (lambda t: t) if rows is None else (lambda t: t[rows, :cols])
    own = sel(ref["own_c"]) if epi == O.EPI_DGELU else None
    bars.add("c", sel(c), sel(ref["c"]), sel(ref32["c"]), A=sel(ref["A_c"]), bf16_out=bf, own=own)
    if c2 is not None:
        bars.add("c2", sel(c2), sel(ref["c2"]), sel(ref32["c2"]), bf16_out=bf)
    if cs is not None:
        bars.add("colsum", cs.double() - FILL, ref["colsum"], ref32["colsum"], A=ref["A_colsum"] + FILL)
    bars.done()


@pytest.mark.parametrize("fam,shape,layout,types,ld,epi,with_cs", _ids("random"))
def test_accuracy(fam, shape, layout, types, ld, epi, with_cs, monkeypatch):
    check_random("random", fam, shape, layout, types, ld, epi, with_cs, monkeypatch)


@pytest.mark.parametrize("types", O.FAMILIES[0].types, ids=lambda t: f"{NAME[t[0]]}_{NAME[t[1]]}")
@pytest.mark.parametrize("epi,with_cs", [O.GELU, O.SILU, O.DGELU, O.DGELU_CS], ids=["bias_gelu", "bias_silu", "dgelu", "dgelu+cs"])
def test_saturated_preactivations(epi, with_cs, types, monkeypatch):
    """gemm_kernel on a row whose pre-activations (GELU, SiLU) and aux values (gelu') are +-8, +-12 and +-30, where exp2 of
    the sigmoid form overflows to inf or underflows to 0: every output finite (O.ratio gives inf otherwise) and within the
    bar over the whole tensor, and GELU / SiLU also over that row alone against its own E32 and A."""
    fam = O.FAMILIES[0]
    shape = fam.shapes[0]
    check_random("hard", fam, shape, O.NN, types, "compact", epi, with_cs, monkeypatch)
    if epi != O.EPI_DGELU:
        # (not for gelu': float64's tanh is exactly +-1 from |x| = 8 on, so the row's reference is exactly acc * {0, 1}, its own
        # E32 and, where gelu' is 0, its A are zero, and the device's more faithful 4e-19 there has nothing to be measured by)
        check_random("hard", fam, shape, O.NN, types, "compact", epi, False, monkeypatch, rows=slice(O.HARD_ROW, O.HARD_ROW + 1),
                     cols=O.HARD_COLS, tag="-row")
        # the fixture does what it says: the row's pre-activations are the listed values
        v = O.reference_of("hard", *shape, False, False, types[0], epi)["c"][O.HARD_ROW, :O.HARD_COLS]
        assert torch.equal(v, torch.tensor(O.HARD_VALUES, dtype=F64).repeat(O.HARD_COLS // len(O.HARD_VALUES)))


# ----------------------------------------------------------------------------------------------------------------- host
def test_host_refuses_what_the_cases_leave_out():
    """The layouts x types of the table that oracle.cases() leaves out are the ones uwu_gemm's 16-byte rules refuse (an operand
    whose contiguous extent is no multiple of 16 bytes): the call fails with an error."""
    from uwudiff_amd import lib as L

    seen = 0
    for fam in O.FAMILIES:
        for M, N, K in fam.shapes:
            for op_dtype, out_dtype in fam.types:
                for layout, _ in fam.combos:
                    if O.host_accepts(M, N, K, layout, op_dtype):
                        continue
                    seen += 1
                    ops = O.operands("exact", M, N, K, *layout, op_dtype)
                    with pytest.raises(L.UwuError, match="multiples? of"):
                        dev_gemm(ops, M, N, K, layout, out_dtype, O.EPI_NONE, False, "compact")
    assert seen >= 3
