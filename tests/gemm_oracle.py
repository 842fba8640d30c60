"""Plain reference of uwu_gemm's epilogues (include/uwu_hip.h), the oracle of tests/test_gemm_epilogue_gpu.py.

    acc = op(A) op(B)                 op(A) = A [M, K] or A^T of [K, M];  op(B) = B^T of [N, K] or B [K, N] (trans_b)
    EPI_NONE       C = acc
    EPI_BIAS       C = acc + bias
    EPI_BIAS_GELU  C = acc + bias,  C2 = gelu_tanh(C)     (C2 from the unrounded C)
    EPI_BIAS_SILU  C = acc + bias,  C2 = silu(C)
    EPI_DGELU      C = acc * gelu_tanh'(aux),  colsum[n] += sum_m C[m, n]   (the sums of the unrounded C)

Every function evaluates these in the dtype it is given, on the rounded operands the device gets: float64 is the reference,
float32 the yardstick of what fp32 arithmetic reaches (E32).  tests/test_gemm_ref_cpu.py checks them against torch.autograd.

Operands come from a seed in two kinds:
  exact   integers in [-3, 3], integer bias in [-8, 8], aux in {0, +10, -10}: every product, sum and bias add is an integer far
          below 2^24, so fp32 accumulation in any order is exact, and tanh-GELU's derivative at 0 / +10 / -10 is 0.5 / 1 / 0 to
          well below 1e-20 (the tanh argument is +-43.6 there; tests/test_gemm_ref_cpu.py checks the three values).
  random  randn rounded to the operand dtype, the weight scaled by K^-1/2 and the product by 2, so that pre-activations
          (acc + bias, bias ~ N(0, 1)) span about [-6, 6] at the tensor sizes used; aux ~ 1.5 randn.
"""
import functools
import math

import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_BIAS_SILU = 0, 1, 2, 3, 4
EPI_NAME = {EPI_NONE: "none", EPI_BIAS: "bias", EPI_BIAS_GELU: "bias_gelu", EPI_DGELU: "dgelu", EPI_BIAS_SILU: "bias_silu"}
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
# pre-activations of the saturation row (random_operands(hard=True)): columns n < HARD_COLS of row HARD_ROW
HARD_VALUES = (8.0, -8.0, 12.0, -12.0, 30.0, -30.0)
HARD_ROW, HARD_COLS = 5, 24


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(K0 * (x + K1 * x * x * x)))


def dgelu_tanh(x):
    t = torch.tanh(K0 * (x + K1 * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * (K0 * (1.0 + 3.0 * K1 * x * x))


def dgelu_own_error(x):
    """Absolute error bound of the device's gelu_tanh'(x) that comes from its sigmoid form (csrc/common.h dgelu_tanh_f):
        gelu'(x) = s + x s (1 - s) P(x),   s = 1 / (1 + 2^z),   P(x) = 2 k0 (1 + 3 k1 x^2),
    with 1 - s formed by subtraction.  For x > 0, s lies in [0.5, 1): 1 + 2^z is rounded to a float in [1, 2] (error <= 2^-24,
    which reaches s multiplied by s^2 <= 1) and the hardware reciprocal is good to one ulp of s (2^-24), so 1 - s, exact as a
    subtraction, carries an ABSOLUTE error of up to 2^-23 however small it is, and the product multiplies that by |x| s P(x):
    2.4e-6 at x = 4, twenty steps of 2^-23.  (torch's 1 - tanh^2 = 4 s (1 - s) has the same cancellation, scaled by 1/4: E32
    sees a quarter of it.)  For x < 0 the same expression bounds the relative error of s (1 - s).
    -> 2^-23 |x| s(x) P(x), float64."""
    x = x.double()
    s = 1.0 / (1.0 + torch.exp(-2.0 * K0 * (x + K1 * x * x * x)))
    return 2.0 ** -23 * x.abs() * s * (2.0 * K0 * (1.0 + 3.0 * K1 * x * x))


def silu(x):
    return x / (1.0 + torch.exp(-x))


def _shapes(M, N, K, ta, tb):
    return ((K, M) if ta else (M, K)), ((K, N) if tb else (N, K))


@functools.lru_cache(maxsize=4)
def exact_operands(M, N, K, ta, tb, seed=0):
    """a, b, bias, aux as float32 tensors holding integers (exact in bfloat16 as well).  Do not modify the results."""
    g = torch.Generator().manual_seed(7919 * seed + 104729 * M + 1299709 * N + K + 2 * ta + tb)
    sa, sb = _shapes(M, N, K, ta, tb)
    a = torch.randint(-3, 4, sa, generator=g).float()
    b = torch.randint(-3, 4, sb, generator=g).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    aux = torch.randint(-1, 2, (M, N), generator=g).float() * 10.0
    return a, b, bias, aux


@functools.lru_cache(maxsize=4)
def random_operands(M, N, K, ta, tb, dtype, seed=0, hard=False):
    """a, b, aux rounded to `dtype`, bias float32.  hard: reduction index 0 is set aside (zero in A) for row HARD_ROW, whose
    only non-zero is a one there, so that its pre-activations in the columns n < HARD_COLS (zero bias) are exactly HARD_VALUES in
    turn; its aux values are HARD_VALUES over the whole row.  Do not modify the results."""
    g = torch.Generator().manual_seed(15485863 * seed + 7919 * M + 104729 * N + K + 2 * ta + tb + 1)
    a = torch.randn(M, K, generator=g) * 2.0
    b = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    aux = 1.5 * torch.randn(M, N, generator=g)
    if hard:
        vals = torch.tensor(HARD_VALUES)
        a[:, 0] = 0.0
        a[HARD_ROW] = 0.0
        a[HARD_ROW, 0] = 1.0
        b[:, 0] = 0.0
        b[:HARD_COLS, 0] = vals.repeat(HARD_COLS // len(vals))
        bias[:HARD_COLS] = 0.0
        aux[HARD_ROW] = vals.repeat((N + len(vals) - 1) // len(vals))[:N]
    a = a.t().contiguous() if ta else a
    b = b.t().contiguous() if tb else b
    return a.to(dtype), b.to(dtype), bias, aux.to(dtype)


def reference(a, b, bias, aux, ta, tb, epi, dtype=F64):
    """-> dict(c, c2, colsum, A_c, A_colsum, own_c): the outputs of one epilogue in `dtype` (absent ones None) and, for the matmul
    and column-sum outputs, the absolute sum of the terms that make up each element (the scale of its rounding error: for the
    column sums, of every product under every row of the column).  own_c (dGELU): |acc| * dgelu_own_error(aux)."""
    A, B = a.to(dtype), b.to(dtype)
    A = A.t() if ta else A
    B = B if tb else B.t()
    return _finish(A @ B, A.abs() @ B.abs(), bias, aux, epi, dtype)


def _finish(acc, absacc, bias, aux, epi, dtype):
    out = dict(c=acc, c2=None, colsum=None, A_c=absacc, A_colsum=None, own_c=None)
    if epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU):
        out["c"] = acc + bias.to(dtype)
        out["A_c"] = absacc + bias.to(dtype).abs()
    if epi == EPI_BIAS_GELU:
        out["c2"] = gelu_tanh(out["c"])
    elif epi == EPI_BIAS_SILU:
        out["c2"] = silu(out["c"])
    elif epi == EPI_DGELU:
        d = dgelu_tanh(aux.to(dtype))
        out["c"] = acc * d
        out["A_c"] = absacc * d.abs()
        out["own_c"] = acc.abs().double() * dgelu_own_error(aux)
        out["colsum"] = out["c"].sum(0)
        out["A_colsum"] = out["A_c"].sum(0)
    return out


def exact_preconditions(M, N, K, ta, tb, seed=0, runs=2, fill=3.0):
    """What makes the exact stage exact for this fixture -> (max |acc| + max |bias|, the largest per-column absolute sum of
    the dGELU terms over `runs` accumulating calls plus the fill).  Both must stay below 2^24; the column sums add
    half-integers (gelu'(0) = 0.5), which fp32 holds exactly below 2^23, so the second is returned doubled."""
    a, b, bias, aux = exact_operands(M, N, K, ta, tb, seed)
    r = reference(a, b, bias, aux, ta, tb, EPI_NONE, dtype=F32)  # exact on these integers
    fac = torch.where(aux == 0, 0.5, torch.where(aux > 0, 1.0, 0.0))
    colabs = (r["c"].abs() * fac).sum(0, dtype=F64)
    return float(r["c"].abs().max() + bias.abs().max()), 2.0 * float(fill + runs * colabs.max())


def ratio(got, ref, ref32, A=None, bf16_out=False, own=None):
    """(E32, worst ratio): E32 = max |fp32 evaluation - fp64|, ratio = max over the elements of
    (|got - ref| - [bf16 output] 2^-8 |ref| - own) / max(E32, 2^-23 A), A = max |ref| unless a per-element A is given; own: a
    per-element worst-case bound of the function's own error, which enters the bar once, like the bf16 term, and not four times.
    The bar of the tests is ratio <= 4; a non-finite output gives inf."""
    ref = ref.double()
    e32 = (ref32.double() - ref).abs().max().item()
    if A is None:
        A = ref.abs().max()
    den = (2.0 ** -23 * A.double()).clamp_min(max(e32, 1e-300))
    err = (got.double() - ref).abs()
    if bf16_out:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    if own is not None:
        err = (err - own.double()).clamp_min(0.0)
    r = (err / den).max().item()
    return e32, (r if (r == r and bool(torch.isfinite(got).all())) else float("inf"))


# ---- products, computed once per fixture ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def products(kind, M, N, K, ta, tb, op_dtype, dtype, seed=0):
    """(op(A) op(B), |op(A)| |op(B)|) of a fixture (kind "exact" / "random" / "hard") in `dtype`.  Do not modify."""
    a, b, _, _ = operands(kind, M, N, K, ta, tb, op_dtype, seed)
    A, B = a.to(dtype), b.to(dtype)
    A = A.t() if ta else A
    B = B if tb else B.t()
    return A @ B, A.abs() @ B.abs()


def operands(kind, M, N, K, ta, tb, op_dtype, seed=0):
    if kind == "exact":
        a, b, bias, aux = exact_operands(M, N, K, ta, tb, seed)
        return a.to(op_dtype), b.to(op_dtype), bias, aux.to(op_dtype)
    return random_operands(M, N, K, ta, tb, op_dtype, seed, kind == "hard")


def reference_of(kind, M, N, K, ta, tb, op_dtype, epi, dtype=F64, seed=0):
    """reference() of a fixture with the matrix products taken from the cache."""
    _, _, bias, aux = operands(kind, M, N, K, ta, tb, op_dtype, seed)
    acc, absacc = products(kind, M, N, K, ta, tb, op_dtype, dtype, seed)
    return _finish(acc, absacc, bias, aux, epi, dtype)


# ---- the cases of tests/test_gemm_epilogue_gpu.py ------------------------------------------------------------------------------
NN, NT, TT = (False, False), (False, True), (True, True)
LAYOUT_NAME = {NN: "NN", NT: "NT", TT: "TT"}
# an epilogue token: (UWU_EPI_*, column sums asked for)
NONE, BIAS, GELU, SILU, DGELU, DGELU_CS = ((EPI_NONE, False), (EPI_BIAS, False), (EPI_BIAS_GELU, False), (EPI_BIAS_SILU, False),
                                           (EPI_DGELU, False), (EPI_DGELU, True))
ALL = (NONE, BIAS, GELU, SILU, DGELU, DGELU_CS)
SWITCHES = ("UWU_GEMM_AS", "UWU_GEMM_AS_BIAS", "UWU_GEMM_M64", "UWU_GEMM_WIDE", "UWU_GEMM_BIG", "UWU_GEMM_R3", "UWU_GEMM_P8",
            "UWU_GEMM_P8N")
_OLD = dict(UWU_GEMM_P8="0", UWU_GEMM_P8N="0")
_PLAIN = dict(_OLD, UWU_GEMM_R3="0", UWU_GEMM_M64="0")
_SMALL = ((NN, (NONE, BIAS, GELU)), (NT, (NONE, DGELU, DGELU_CS)))
_BB, _BF, _FF = (BF16, BF16), (BF16, F32), (F32, F32)


class Family:
    def __init__(self, key, kernel, env, shapes, combos, types=(_BB,), ld4=False, stages=("exact", "random")):
        self.key, self.kernel, self.env, self.shapes, self.combos, self.types = key, kernel, env, shapes, combos, types
        self.ld4, self.stages = ld4, stages


# key, the name uwu_gemm_last_kernel() must give, switches (every other switch of SWITCHES is unset), shapes (the first one also
# runs the random stage), layouts x epilogues, (operand, output) types.  The dispatch condition each shape meets is spelled out
# in tests/test_gemm_epilogue_gpu.py.
FAMILIES = (
    Family("gemm_reg", "gemm", _PLAIN, ((200, 72, 40), (130, 132, 200)), ((NN, ALL), (NT, ALL), (TT, (NONE, BIAS))),
           types=(_FF, _BB, _BF), ld4=True),
    Family("gemm_gl", "gemm", _PLAIN, ((260, 264, 192),), ((NN, ALL),), types=(_BB, _BF), ld4=True),
    Family("m64", "gemm_m64", _OLD, ((200, 264, 128), (130, 136, 64)), _SMALL),
    Family("p8", "gemm_p8", dict(UWU_GEMM_P8="1"), ((300, 264, 192), (260, 520, 128)), _SMALL),
    Family("p8_narrow", "gemm_p8", dict(UWU_GEMM_P8="1"), ((300, 260, 128),), ((NN, (NONE, BIAS, GELU)),)),
    Family("p8n", "gemm_p8n", dict(UWU_GEMM_P8="0", UWU_GEMM_P8N="1"), ((300, 384, 256), (130, 1152, 384)),
           ((NN, (NONE, BIAS, GELU)), (NT, (NONE,)))),
    Family("r3_256", "gemm_r3_256", dict(UWU_GEMM_P8="0"), ((21960, 264, 672),), ((NN, ALL), (NT, (NONE, DGELU, DGELU_CS))),
           types=(_BB, _BF)),
    Family("big", "gemm_big", dict(UWU_GEMM_P8="0"), ((32728, 256, 640),), _SMALL),
    Family("wide", "gemm_wide", dict(_OLD, UWU_GEMM_WIDE="1"), ((21960, 384, 640),), ((NN, (NONE, BIAS)), (NT, (NONE,)))),
    Family("r3_128", "gemm_r3_128", dict(UWU_GEMM_P8="0"), ((10952, 264, 160),), ((NT, (NONE, DGELU, DGELU_CS)),)),
    Family("as", "gemm_as", {}, ((65536, 1088, 384),), ((NN, (BIAS, GELU, DGELU)),), stages=("exact",)),
)


def host_accepts(M, N, K, layout, op_dtype):
    """uwu_gemm's 16-byte rules: the contiguous extent of each operand is a multiple of 16 bytes, N of 4."""
    ta, tb = layout
    epc = 8 if op_dtype == BF16 else 4
    return (M if ta else K) % epc == 0 and (N if tb else K) % epc == 0 and N % 4 == 0


def cases(stage):
    """-> (family, (M, N, K), layout, (operand, output dtype), ld mode, (epilogue, column sums)) of a stage.
    ld modes: "compact"; "pad": lda, ldb, ldc, ldaux each 16 bytes over the row length; "c4" (ld4 families, bf16 operands):
    ldc = N + 4 and ldaux = N + 4, the narrow store / 8-byte aux forms at an N that would otherwise take the 16-byte ones.
    A combination the host's rules refuse (host_accepts) is not a case: test_host_refuses_what_the_cases_leave_out."""
    for fam in FAMILIES:
        if stage not in fam.stages:
            continue
        for shape in (fam.shapes if stage == "exact" else fam.shapes[:1]):
            for types in fam.types:
                for layout, epis in fam.combos:
                    # (the ring kernel's K-major forms are bf16 -> bf16 only: fp32 C reaches it, with the run-time epilogue, on NN)
                    if fam.key == "r3_256" and types == _BF and layout != NN:
                        continue
                    if not host_accepts(*shape, layout, types[0]):
                        continue
                    for ld in ("compact", "pad") + (("c4",) if fam.ld4 and types[0] == BF16 else ()):
                        for epi in epis:
                            yield fam, shape, layout, types, ld, epi


def exact_fixtures():
    """The distinct (M, N, K, trans_a, trans_b) of the exact stage."""
    return sorted({(*shape, *layout) for _, shape, layout, _, _, _ in cases("exact")})
