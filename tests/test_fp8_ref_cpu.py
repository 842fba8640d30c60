"""The fp8 oracle (tests/fp8_oracle.py) checked against the definition of the two formats, on the CPU: what
tests/test_fp8_chain_gpu.py takes for granted about torch's float8 casts and about products of fp8 values."""
import pytest
import torch

from tests import fp8_oracle as O
from tests import gemm_oracle as G

FMTS = [O.E4M3, O.E5M2]


def _define(fmt):
    """The 256 values from the format's definition (OCP 8-bit floating point: e4m3fn bias 7, no inf, S.1111.111 = NaN; e5m2
    bias 15, IEEE inf / NaN)."""
    eb, mb, bias = (4, 3, 7) if fmt == O.E4M3 else (5, 2, 15)
    out = []
    for c in range(256):
        s = -1.0 if c & 0x80 else 1.0
        e, m = (c & 0x7F) >> mb, c & ((1 << mb) - 1)
        if fmt == O.E4M3 and e == 15 and m == 7:
            v = float("nan")
        elif fmt == O.E5M2 and e == 31:
            v = float("nan") if m else s * float("inf")
        elif e == 0:
            v = s * m * 2.0 ** (1 - bias - mb)
        else:
            v = s * (1 + m / (1 << mb)) * 2.0 ** (e - bias)
        out.append(v)
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("fmt", FMTS)
def test_value_table_is_the_format(fmt):
    want, got = _define(fmt), O.lut(fmt).double()
    assert torch.equal(torch.isnan(want), torch.isnan(got))
    ok = ~torch.isnan(want)
    assert torch.equal(want[ok], got[ok])
    assert len(O.finite_codes(fmt)) == (254 if fmt == O.E4M3 else 248)
    assert float(got[ok & torch.isfinite(got)].max()) == O.FMAX[fmt]
    assert float(got[got > 0].min()) == O.MIN_SUB[fmt]
    assert torch.isnan(got[O.NAN_CODE]) and (fmt == O.E4M3 or got[O.INF_CODE] == float("inf"))


@pytest.mark.parametrize("fmt", FMTS)
def test_every_finite_code_round_trips(fmt):
    c = O.finite_codes(fmt)
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        v = O.decode(c, fmt).to(dtype)
        assert torch.equal(v.float(), O.decode(c, fmt))  # (exact in bfloat16 too)
        if dtype == torch.float64:  # (the table route has one zero)
            assert O.same(O.quantize_value(v, fmt), c, fmt)
        else:
            assert torch.equal(O.quantize(v, 1.0, fmt), c)  # byte for byte, the sign of zero included


@pytest.mark.parametrize("fmt", FMTS)
def test_ties_go_to_the_even_code_and_their_neighbours_to_the_nearer_one(fmt):
    mid, even, lo, hi = O.midpoints(fmt)
    assert len(mid) == (126 if fmt == O.E4M3 else 123)
    assert torch.equal((O.decode(lo, fmt).double() + O.decode(hi, fmt).double()) / 2, mid.double())
    for sign, bit in ((1.0, 0), (-1.0, 0x80)):
        assert torch.equal(O.quantize(sign * mid, 1.0, fmt), even | bit)
        assert O.same(O.quantize_value(sign * mid.double(), fmt), even | bit, fmt)
        assert O.same(O.quantize(sign * O.f32_step(mid, True), 1.0, fmt), hi | bit, fmt)
        assert O.same(O.quantize(sign * O.f32_step(mid, False), 1.0, fmt), lo | bit, fmt)
        mb = mid.bfloat16()
        assert O.same(O.quantize(sign * O.bf16_step(mb, True), 1.0, fmt), hi | bit, fmt)
        assert O.same(O.quantize(sign * O.bf16_step(mb, False), 1.0, fmt), lo | bit, fmt)
    # float64 values a hair off a tie: the fp64 route does not round twice
    eps = mid.double() * 2.0 ** -40
    assert O.same(O.quantize_value(mid.double() + eps, fmt), hi, fmt)
    assert O.same(O.quantize_value(mid.double() - eps, fmt), lo, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_nan_stays_nan_and_everything_past_max_saturates(fmt):
    mx = O.FMAX[fmt]
    top = int(O.finite_codes(fmt)[O.decode(O.finite_codes(fmt), fmt).argmax()])
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), mx, -mx, float(O.f32_step(torch.tensor([mx]), True)), 1e30, -1e30,
                      0.375 * O.MIN_SUB[fmt], -0.375 * O.MIN_SUB[fmt], 0.0, -0.0])
    for s in (1.0, 0.125, 32.0, 7.25):
        q = O.quantize(x / s if s != 7.25 else x, s, fmt)
        v = O.decode(q, fmt)
        assert torch.isnan(v[0]) and not torch.isnan(v[1:]).any()
        assert q[1:8].tolist() == [top, top | 0x80, top, top | 0x80, top, top, top | 0x80]
    q = O.quantize(x, 1.0, fmt)
    assert O.canon(q[8:], fmt).tolist() == [0, 0, 0, 0]
    assert torch.isnan(O.decode(O.quantize_value(torch.tensor([float("nan")], dtype=torch.float64), fmt), fmt)).all()
    # canon folds the zero codes and every NaN code
    both = torch.tensor([0x00, 0x80, 0x7F, 0xFF, 0x7E, 0xFE], dtype=torch.uint8)
    assert O.canon(both, fmt)[:4].tolist() == [0, 0, O.NAN_CODE, O.NAN_CODE]
    assert O.code_distance(torch.tensor([1, 0x81], dtype=torch.uint8), torch.tensor([3, 0x01], dtype=torch.uint8), fmt).tolist() == [2, 2]


@pytest.mark.parametrize("fmt", FMTS)
def test_boundary_values_cover_what_the_quantiser_test_promises(fmt):
    for dtype in (torch.float32, torch.bfloat16):
        v = O.boundary_values(fmt, dtype).float()
        mid, _, _, _ = O.midpoints(fmt)
        have = set(v.tolist())
        for want in (O.decode(O.finite_codes(fmt), fmt), mid, -mid, torch.tensor([float("inf"), -float("inf"), O.FMAX[fmt]])):
            assert set(want.tolist()) <= have
        assert (v.abs()[(v != 0)].min() < O.MIN_SUB[fmt] / 2) and (v[torch.isfinite(v)].max() > O.FMAX[fmt])
        d = O.boundary_distance(v.double(), fmt)
        assert int((d == 0).sum()) >= 2 * len(mid)


@pytest.mark.parametrize("fmt_a", FMTS)
def test_products_with_e4m3_are_exact_in_bfloat16(fmt_a):
    """(1 + 3 or 2 mantissa bits) x (1 + 3 mantissa bits): at most 8 significant bits, the exponent within float32's range."""
    a = O.decode(O.finite_codes(fmt_a), fmt_a).double()
    b = O.decode(O.finite_codes(O.E4M3), O.E4M3).double()
    p = a[:, None] * b[None, :]
    assert torch.equal(p.float().double(), p) and torch.equal(p.bfloat16().double(), p)
    # and through power-of-two scales such as the tests use
    assert torch.equal((p * 0.5).bfloat16().double(), p * 0.5)


def test_saturated_gelu_values_are_exact_in_the_kernel_formula():
    """gemm_oracle.HARD_VALUES in the sigmoid form the epilogue evaluates, float32: gelu(x) is x for x >= 8 and -0 for x <= -12
    (2^z overflows to inf), gelu' is 1 / 0 there; x = -8 leaves ~ -3e-21, not an exact zero (the GPU test keeps the others)."""
    x = torch.tensor(G.HARD_VALUES)
    g, d = O.gelu_sig(x), O.dgelu_sig(x)
    exact = (g == torch.where(x > 0, x, torch.zeros_like(x))) & (d == (x > 0).float())
    assert [v for v, e in zip(G.HARD_VALUES, exact.tolist()) if e] == [8.0, 12.0, -12.0, 30.0, -30.0]
    # the tanh form of gemm_oracle agrees on those
    assert torch.equal(G.gelu_tanh(x)[exact], g[exact]) and torch.equal(G.dgelu_tanh(x)[exact], d[exact])
    # float64: the true values differ from x / 0 / 1 by less than any fp8 step can see
    assert (G.gelu_tanh(x.double()) - torch.where(x > 0, x, torch.zeros_like(x)).double()).abs().max() < 1e-20
