"""Plain reference of the fp8 (OCP e4m3fn / e5m2) operand chain, the oracle of tests/test_fp8_chain_gpu.py (CPU only).

    value table   lut(fmt)[c] = the float a byte c decodes to: torch.uint8 -> view(torch.float8_*) -> float32
    quantiser     bytes = (x.float() * s).clamp(-max, max).to(float8): round to nearest even, NaN stays NaN, +-inf and
                  everything past max saturate to +-max (include/uwu_hip.h, uwu_fp8_quantize)

Comparisons go through canon(): the two zero codes (0x00, 0x80) count as one, and every byte that decodes to NaN counts as
"NaN", not as a particular byte.  tests/test_fp8_ref_cpu.py checks the properties the GPU tests lean on (every code round
trips, ties go to the even code, the fp32 neighbours of a tie go to the nearer code, saturation, NaN; every e4m3 / e5m2 x e4m3
product is exact in bfloat16).
"""
import functools

import torch

E4M3, E5M2 = 0, 1
F8 = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
FMAX = {E4M3: 448.0, E5M2: 57344.0}
MIN_SUB = {E4M3: 2.0 ** -9, E5M2: 2.0 ** -16}  # the smallest subnormal
NAME = {E4M3: "e4m3", E5M2: "e5m2"}
NAN_CODE = 0x7F  # decodes to NaN in both formats (e4m3fn: S.1111.111; e5m2: exponent 31, mantissa 3)
INF_CODE = 0x7C  # e5m2 only: +inf (e4m3fn has no infinity)


@functools.lru_cache(maxsize=None)
def lut(fmt):
    """float32 [256]: what every byte decodes to.  Do not modify."""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8[fmt]).float()


@functools.lru_cache(maxsize=None)
def finite_codes(fmt):
    """uint8: the codes that decode to a finite number (254 for e4m3fn, 248 for e5m2), ascending bytes.  Do not modify."""
    return torch.arange(256, dtype=torch.int32)[torch.isfinite(lut(fmt))].to(torch.uint8)


def decode(u8, fmt):
    return lut(fmt)[u8.long()]


def quantize(x, s, fmt):
    """The reference quantiser -> uint8 bytes."""
    return (x.float() * s).clamp(-FMAX[fmt], FMAX[fmt]).to(F8[fmt]).view(torch.uint8)


def quantize_value(v, fmt):
    """Bytes of values that are already scaled.  A float64 input is rounded straight to the fp8 grid through the code table
    (nearest, ties to the even byte), never through float32 first: no double rounding.  -0 comes out as +0 (compare with same())."""
    if v.dtype != torch.float64:
        return quantize(v, 1.0, fmt)
    lo, hi = bracket(v, fmt)
    vl, vh = decode(lo, fmt).double(), decode(hi, fmt).double()
    vc = v.clamp(-FMAX[fmt], FMAX[fmt])
    dl, dh = (vc - vl).abs(), (vh - vc).abs()
    pick_hi = (dh < dl) | ((dh == dl) & ((hi & 1) == 0))
    out = torch.where(pick_hi, hi, lo)
    return torch.where(torch.isnan(v), torch.full_like(out, NAN_CODE), out)


def bracket(v, fmt):
    """-> (lo, hi) bytes of the neighbouring finite codes with value(lo) <= clamp(v) <= value(hi) (lo == hi on a code)."""
    vals, codes = sorted_values(fmt)
    vc = torch.nan_to_num(v.double(), nan=0.0).clamp(-FMAX[fmt], FMAX[fmt])
    i_hi = torch.searchsorted(vals, vc).clamp(0, len(vals) - 1)  # first value >= v
    i_lo = torch.where(vals[i_hi] == vc, i_hi, (i_hi - 1).clamp_min(0))
    return codes[i_lo], codes[i_hi]


@functools.lru_cache(maxsize=None)
def sorted_values(fmt):
    """(float64 values ascending, their bytes) of the finite codes, -0 left out (+0 stands for zero)."""
    c = finite_codes(fmt)
    c = c[c != 0x80]
    v = decode(c, fmt).double()
    order = torch.argsort(v)
    return v[order], c[order]


def boundary_distance(v, fmt):
    """|v - the nearest rounding boundary| for float64 values already scaled: the boundaries are the midpoints between
    neighbouring codes (past +-max there is none: inf)."""
    vals, _ = sorted_values(fmt)
    mids = (vals[1:] + vals[:-1]) / 2
    vc = torch.nan_to_num(v.double(), nan=0.0)
    i = torch.searchsorted(mids, vc).clamp(0, len(mids) - 1)
    j = (i - 1).clamp_min(0)
    d = torch.minimum((mids[i] - vc).abs(), (mids[j] - vc).abs())
    return torch.where(vc.abs() > FMAX[fmt], torch.full_like(d, float("inf")), d)


def canon(u8, fmt):
    """Bytes with -0 folded into +0 and every NaN code into NAN_CODE."""
    v = decode(u8.cpu(), fmt)
    out = u8.cpu().clone()
    out[v == 0] = 0
    out[torch.isnan(v)] = NAN_CODE
    return out


def same(a, b, fmt):
    return torch.equal(canon(a, fmt), canon(b, fmt))


def code_distance(a, b, fmt):
    """How many codes apart two byte tensors are on the value-ordered list of finite codes (NaN: a large number unless both)."""
    vals, _ = sorted_values(fmt)
    va, vb = decode(canon(a, fmt), fmt).double(), decode(canon(b, fmt), fmt).double()
    na, nb = torch.isnan(va), torch.isnan(vb)
    ia = torch.searchsorted(vals, torch.nan_to_num(va).clamp(-FMAX[fmt], FMAX[fmt]))
    ib = torch.searchsorted(vals, torch.nan_to_num(vb).clamp(-FMAX[fmt], FMAX[fmt]))
    d = (ia - ib).abs()
    return torch.where(na | nb, torch.where(na & nb, torch.zeros_like(d), torch.full_like(d, 10 ** 6)), d)


# ---- the inputs of the "every code and boundary" quantiser test ------------------------------------------------------------
def midpoints(fmt):
    """float32: the midpoints between neighbouring non-negative finite codes (each exact in float32 and in bfloat16: a code has
    at most 4 significant bits, a midpoint one more), and the even code (the byte with mantissa bit 0 clear) of each pair."""
    c = finite_codes(fmt)
    c = c[c < 0x80]
    v = decode(c, fmt)
    mid = (v[1:] + v[:-1]) / 2
    even = torch.where((c[:-1] & 1) == 0, c[:-1], c[1:])
    return mid, even, c[:-1], c[1:]


def f32_step(t, up):
    return torch.nextafter(t, torch.full_like(t, float("inf") if up else -float("inf")))


def bf16_step(t, up):
    """The next bfloat16 above / below a positive finite bfloat16 tensor."""
    i = t.contiguous().view(torch.int16).to(torch.int32) + (1 if up else -1)
    return i.to(torch.int16).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def boundary_values(fmt, dtype):
    """The scaled values the quantiser is to meet, in `dtype` (float32 or bfloat16), every one of both signs: each finite code,
    each midpoint, the two neighbours of each midpoint in `dtype`, zero, 3/8 of the smallest subnormal (below half of it),
    max, the next `dtype` above max, inf.  Do not modify."""
    mid, _, _, _ = midpoints(fmt)
    codes = decode(finite_codes(fmt), fmt)
    codes = codes[codes >= 0]
    extra = torch.tensor([0.0, 0.375 * MIN_SUB[fmt], FMAX[fmt], float("inf")])
    if dtype == torch.float32:
        above_max = f32_step(torch.tensor([FMAX[fmt]]), True)
        pos = torch.cat([codes, mid, f32_step(mid, True), f32_step(mid, False), extra, above_max])
    else:
        mb = mid.bfloat16()
        assert torch.equal(mb.float(), mid) and torch.equal(codes.bfloat16().float(), codes)
        above_max = bf16_step(torch.tensor([FMAX[fmt]]).bfloat16(), True).float()
        pos = torch.cat([codes, mid, bf16_step(mb, True).float(), bf16_step(mb, False).float(), extra, above_max])
    return torch.cat([pos, -pos]).to(dtype)


# ---- GELU as the emitting epilogue evaluates it (csrc/common.h gelu_sig_f: x * s, s = 1 / (1 + 2^z)) ------------------------
def gelu_sig(x):
    """tanh-GELU in the kernel's sigmoid form, in the dtype of x."""
    ca = -2.0 * 1.4426950408889634 * 0.7978845608028654
    return x / (1.0 + torch.exp2(x * (ca + ca * 0.044715 * x * x)))


def dgelu_sig(x):
    ca = -2.0 * 1.4426950408889634 * 0.7978845608028654
    d0 = 2.0 * 0.7978845608028654
    s = 1.0 / (1.0 + torch.exp2(x * (ca + ca * 0.044715 * x * x)))
    return s + x * s * (1.0 - s) * (d0 + 3.0 * 0.044715 * d0 * x * x)
