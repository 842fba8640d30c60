"""CPU: the GEMM epilogue oracle (tests/gemm_oracle.py) against torch.autograd, and the preconditions of its exact fixtures."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_oracle as O

F64 = torch.float64


def _fixture(dtype):
    M, N, K = 37, 24, 40
    a, b, bias, aux = O.random_operands(M, N, K, False, False, dtype, seed=3)
    return a.double(), b.double(), bias.double(), aux.double()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act,epi", [(lambda x: F.gelu(x, approximate="tanh"), O.EPI_BIAS_GELU), (F.silu, O.EPI_BIAS_SILU)],
                         ids=["gelu", "silu"])
def test_forward_matches_torch(act, epi, dtype):
    a, b, bias, aux = _fixture(dtype)
    u = F.linear(a, b, bias)
    r = O.reference(a, b, bias, aux, False, False, epi)
    torch.testing.assert_close(r["c"], u, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(r["c2"], act(u), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(O.reference(a, b, bias, aux, False, False, O.EPI_BIAS)["c"], u, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(O.reference(a, b, bias, aux, False, False, O.EPI_NONE)["c"], a @ b.t(), rtol=1e-13, atol=1e-13)
    # the absolute sums bound the values they scale
    assert (r["A_c"] >= r["c"].abs() - 1e-12).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gradients_match_autograd(dtype):
    """fc1 -> GELU -> fc2: the input gradient of GELU's pre-activation, du = (dy W2) * gelu'(u), and fc1's bias gradient, its
    column sums, are what EPI_DGELU computes with aux = u (trans_b: W2 is [out, in] = [K, N] for this product)."""
    a, w1, b1, _ = _fixture(dtype)
    M, N = a.shape[0], w1.shape[0]
    g = torch.Generator().manual_seed(11)
    Kout = 16
    w2 = torch.randn(Kout, N, generator=g, dtype=F64)
    dy = torch.randn(M, Kout, generator=g, dtype=F64)
    b1 = b1.clone().requires_grad_(True)
    u = F.linear(a, w1, b1)
    u.retain_grad()
    y = F.linear(F.gelu(u, approximate="tanh"), w2)
    y.backward(dy)
    r = O.reference(dy, w2, None, u.detach(), False, True, O.EPI_DGELU)
    torch.testing.assert_close(r["c"], u.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r["colsum"], b1.grad, rtol=1e-12, atol=1e-12)
    assert (r["A_colsum"] >= r["colsum"].abs() - 1e-12).all()
    # the same product from the weight in Linear layout (trans_b = 0) and from a K-major A (trans_a)
    r0 = O.reference(dy, w2.t().contiguous(), None, u.detach(), False, False, O.EPI_DGELU)
    torch.testing.assert_close(r0["c"], r["c"], rtol=1e-13, atol=1e-13)
    rt = O.reference(dy.t().contiguous(), w2, None, u.detach(), True, True, O.EPI_NONE)
    torch.testing.assert_close(rt["c"], dy @ w2, rtol=1e-13, atol=1e-13)


def test_dgelu_and_silu_derivative_forms():
    x = torch.linspace(-9.0, 9.0, 1001, dtype=F64, requires_grad=True)
    F.gelu(x, approximate="tanh").sum().backward()
    torch.testing.assert_close(O.dgelu_tanh(x.detach()), x.grad, rtol=1e-12, atol=1e-14)
    # the aux values of the exact fixtures: gelu' = 0.5, 1, 0 to well below the 1e-20 the GPU test allows
    d = O.dgelu_tanh(torch.tensor([0.0, 10.0, -10.0], dtype=F64))
    assert (d - torch.tensor([0.5, 1.0, 0.0], dtype=F64)).abs().max() < 1e-25


def test_products_cache_agrees_with_reference():
    M, N, K = 33, 24, 24
    for kind, layout in (("exact", O.NT), ("random", O.NN), ("hard", O.TT)):
        a, b, bias, aux = O.operands(kind, M + 7, N, K, *layout, torch.bfloat16)
        for epi in (O.EPI_BIAS_SILU, O.EPI_DGELU):
            r = O.reference(a, b, bias, aux, *layout, epi)
            rc = O.reference_of(kind, M + 7, N, K, *layout, torch.bfloat16, epi)
            for k in ("c", "c2", "colsum", "A_c", "A_colsum"):
                assert (r[k] is None and rc[k] is None) or torch.equal(r[k], rc[k]), (kind, epi, k)


def test_hard_row_has_the_listed_preactivations():
    for dtype in (torch.float32, torch.bfloat16):
        M, N, K = O.FAMILIES[0].shapes[0]
        r = O.reference_of("hard", M, N, K, False, False, dtype, O.EPI_BIAS)
        want = torch.tensor(O.HARD_VALUES, dtype=F64).repeat(O.HARD_COLS // len(O.HARD_VALUES))
        assert torch.equal(r["c"][O.HARD_ROW, :O.HARD_COLS], want)
        big = r["c"].abs().max().item()
        assert 4.0 < r["c"][torch.arange(M) != O.HARD_ROW].abs().max().item() < 14.0 and big == 30.0


def test_cases_cover_every_family_and_respect_the_host_rules():
    keys = {c[0].key for c in O.cases("exact")}
    assert keys == {f.key for f in O.FAMILIES}
    assert {c[0].key for c in O.cases("random")} == keys - {"as"}
    for fam, shape, layout, types, ld, _ in list(O.cases("exact")) + list(O.cases("random")):
        assert O.host_accepts(*shape, layout, types[0])
        assert set(fam.env) <= set(O.SWITCHES)


@pytest.mark.parametrize("M,N,K,ta,tb", O.exact_fixtures())
def test_exact_fixture_preconditions(M, N, K, ta, tb):
    """fp32 arithmetic in any order is exact on the fixture: max |acc| + max |bias| < 2^24, and every column sum's absolute
    sum (two accumulating runs on top of the fill, in half-integers) stays below 2^24."""
    vmax, colmax = O.exact_preconditions(M, N, K, ta, tb)
    assert vmax < 2 ** 24 and colmax < 2 ** 24, (vmax, colmax)
