"""GPU: two weight gradients in one launch of the wide streaming kernel (uwu_gemm_wgrad_pair) and the DiT backward that uses it.

A block's four bf16 weight gradients go as two grouped launches (fc1 + fc2, qkv + proj): member b's tiles follow member a's inside
every K slice, both write one split-K scratch and one reduce kernel adds the slices to both outputs.  Integer operands make
every fp32 partial sum exact, so the grouped result must equal the exact matmul bit for bit, whatever the slice count.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FC = ((1536, 384), (384, 1536))   # fc1 + fc2 of DiT-S/2: 8 + 8 tiles of 192x384, 16 K slices
ATTN = ((1152, 384), (384, 384))  # qkv + proj: 6 + 2 tiles, 32 K slices


def _operands(K, M, N, ints, seed):
    g = torch.Generator().manual_seed(seed)
    if ints:
        a, b = torch.randint(-3, 4, (K, M), generator=g).float(), torch.randint(-3, 4, (K, N), generator=g).float()
    else:
        a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    return a.bfloat16().cuda(), b.bfloat16().cuda()


_cache = {}


def _case(shapes, K, ints=True):
    """Operands and exact references of a pair, computed once per (shapes, K) and left unchanged."""
    key = (shapes, K, ints)
    if key not in _cache:
        ops_, want = [], []
        for i, (M, N) in enumerate(shapes):
            a, b = _operands(K, M, N, ints, seed=40 + i)
            ops_.append((a, b))
            if ints:
                want.append((a.float().t() @ b.float(), a.float().sum(0)))
            else:
                want.append(((a.double().t() @ b.double()).float(), a.double().sum(0).float()))
        _cache[key] = (ops_, want)
    return _cache[key]


def _run_pair(shapes, K, ops_, bias_b=True):
    from uwudiff_amd import ops

    (Ma, Na), (Mb, Nb) = shapes
    dws = [torch.full(s, 2.0, device="cuda") for s in shapes]
    dbs = [torch.full((Ma,), 3.0, device="cuda"), torch.full((Mb,), 3.0, device="cuda") if bias_b else None]
    ops.gemm_wgrad_pair(ops_[0][0], ops_[0][1], dws[0], ops_[1][0], ops_[1][1], dws[1],
                        scratch=ops.gemm_wgrad_pair_scratch(Ma, Na, Mb, Nb, K), bias_grad_a=dbs[0], bias_grad_b=dbs[1])
    return dws, dbs


# K = 8192: 16 (fc) / 8 (attn) K-steps per slice; 4096: 4 per slice of the attn pair, shorter than the 4-stage ring;
# 4256 = 133 K-steps: a ragged last slice, and slice indices past the effective count that return early
@pytest.mark.parametrize("K", [8192, 4096, 4256])
@pytest.mark.parametrize("shapes", [FC, ATTN], ids=["fc", "attn"])
def test_pair_exact(shapes, K, monkeypatch):
    from uwudiff_amd import lib as L

    monkeypatch.setenv("UWU_GEMM_TRW", "1")  # the wide kernel from K = 4096 on
    (Ma, Na), (Mb, Nb) = shapes
    assert L.load().uwu_gemm_wgrad_pair_scratch_bytes(Ma, Na, Mb, Nb, K) > 0  # these shapes are grouped
    ops_, want = _case(shapes, K)
    dws, dbs = _run_pair(shapes, K, ops_)
    for dw, db, (w, s) in zip(dws, dbs, want):
        assert torch.equal(dw, w + 2.0)
        assert torch.equal(db, s + 3.0)


def test_pair_exact_without_second_bias(monkeypatch):
    monkeypatch.setenv("UWU_GEMM_TRW", "1")
    K = 4256
    ops_, want = _case(ATTN, K)
    dws, dbs = _run_pair(ATTN, K, ops_, bias_b=False)
    assert torch.equal(dws[0], want[0][0] + 2.0) and torch.equal(dws[1], want[1][0] + 2.0)
    assert torch.equal(dbs[0], want[0][1] + 3.0)


def test_pair_exact_tall_tiles(monkeypatch):
    """Both members in the other tile orientation (384 x 192 tiles: M a multiple of 384, N not), ragged last column tile."""
    monkeypatch.setenv("UWU_GEMM_TRW", "1")
    shapes, K = ((768, 192), (384, 520)), 4256
    from uwudiff_amd import lib as L

    assert L.load().uwu_gemm_wgrad_pair_scratch_bytes(768, 192, 384, 520, K) > 0
    ops_, want = _case(shapes, K)
    dws, dbs = _run_pair(shapes, K, ops_)
    for dw, db, (w, s) in zip(dws, dbs, want):
        assert torch.equal(dw, w + 2.0)
        assert torch.equal(db, s + 3.0)


def test_pair_falls_back_to_two_launches(monkeypatch):
    """A second member (384 x 264) that the wide kernel does not take in the first member's tile orientation: the call is two
    uwu_gemm_wgrad calls, bit for bit."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    monkeypatch.setenv("UWU_GEMM_TRW", "1")
    shapes, K = ((1152, 384), (384, 264)), 4096
    assert L.load().uwu_gemm_wgrad_pair_scratch_bytes(1152, 384, 384, 264, K) == 0
    ops_, _ = _case(shapes, K)
    dws, dbs = _run_pair(shapes, K, ops_)
    for (M, N), (a, b), dw, db in zip(shapes, ops_, dws, dbs):
        rw, rb = torch.full((M, N), 2.0, device="cuda"), torch.full((M,), 3.0, device="cuda")
        ops.gemm_wgrad(a, b, rw, scratch=ops.gemm_wgrad_pair_scratch(1152, 384, 384, 264, K), bias_grad=rb)
        assert torch.equal(dw, rw)
        assert torch.equal(db, rb)


def test_pair_random(monkeypatch):
    """Non-integer bf16 operands against the fp64 product, at test_gemm_tr_random's tolerance for this kernel family (set there
    for a reduction twice as long)."""
    monkeypatch.setenv("UWU_GEMM_TRW", "1")
    K = 8192
    ops_, want = _case(FC, K, ints=False)
    dws, dbs = _run_pair(FC, K, ops_)
    for dw, (w, _) in zip(dws, want):
        torch.testing.assert_close(dw - 2.0, w, rtol=1e-4, atol=2e-2)


# ---- the driver ---------------------------------------------------------------------------------------------------------------
# Which outputs of one forward + backward are reproducible was measured per tensor on the parent commit (two runs of each setting,
# this test's model and inputs):
#   * the forward output and the eight block weight gradients are bit-identical from run to run in either setting: split-K
#     slices in a scratch, summed in a fixed order.  The activation-gradient chain never reads a weight gradient.
#   * every other gradient is an fp32 atomic sum and differs between two runs of ONE setting, on the parent as here:
#       block biases                    the fused bias gradient of gemm_trw_kernel / gemm_tr_kernel (atomicAdd per K slice)
#       x_embedder.weight, final.weight gemm_kernel's split-K accumulate epilogue (gemm.hip, atomicAdd per element)
#       x_embedder.bias, final.bias     colsum_kernel (norm.hip, atomicAdd per row block)
#       adaLN.bias                      colsum_kernel over d(mod), which add_ln_mod_bwd accumulates over the tokens of a sample
#                                       with atomicAdd (norm.hip)
#       adaLN.weight, t_embedder.*, y_embedder.*   the same d(mod) AFTER its rounding to bf16 (mod_bf16, B >= 64)
#     Identity cannot be asked of these.  The first four rows are sums of the same addends in another order, over at most
#     M = 32768 tokens: fp32 allows such a sum n u = 32768 x 2^-24 = 2e-3 of sum |addends|; the parent comparisons gave
#     1e-7 .. 3.5e-7 relative L2.  Their bound is the 1e-4 that test_dit_gpu.py already sets for gradients "up to the order of
#     fp32 atomic adds": a twentieth of the worst case, and a hundredth of what one stale K slice (1 / 16 of the tokens) does.
#     In the last row a difference of 1e-7 in d(mod) decides here and there which way an element rounds to bf16, and an element
#     that rounds the other way moves by one bf16 ulp, at most 2^-7 of its value: 2e-6 .. 4e-5 measured, a few elements each
#     time, and 2^-7 if every element did.  These tensors read nothing that a weight-gradient launch writes.
ATOMIC_REL_L2 = 1e-4
BF16_ULP_REL_L2 = 2.0 ** -7
AFTER_BF16_ROUNDING = ("adaLN.weight", "t_embedder.", "y_embedder.")
# Relative L2 difference of the fc1 / fc2 weight gradients between UWU_GEMM_TRW unset and =0 on the parent commit (one launch per
# gradient in both settings; both sides reproducible, so these are fixed numbers).  The grouped launch may differ from the
# gemm_tr launch by at most twice as much.  qkv and proj: parent 2.220e-07 / 1.975e-07 (block 0), 2.219e-07 / 2.006e-07 (block 1)
# -- grouped they use 32 K slices of 32 K-steps, exactly gemm_tr's split at this size, and must come out EQUAL to it.
PARENT_REL_L2 = {
    "blocks.0.fc1.weight": 2.363e-07, "blocks.0.fc2.weight": 2.413e-07, "blocks.1.fc1.weight": 2.385e-07, "blocks.1.fc2.weight": 2.471e-07,
}


def test_dit_backward_grouped_equals_single_launches(monkeypatch):
    """DiT-S/2 width, depth 2, batch 128 (M = 32768 tokens: the smallest batch at which the driver takes the wide kernel, here
    grouped): forward + backward twice with UWU_GEMM_TRW unset (grouped) and twice with UWU_GEMM_TRW=0 (single gemm_tr
    launches).  A deferred fc2 / proj gradient that read dy too late, or a grouped launch that wrote outside its outputs,
    shows in the block weights (order one) -- dx, the activation gradient that reaches the embedder, is not visible from
    Python; x_embedder's gradients are its only trace."""
    from uwudiff_amd.dit import DiT, DiTConfig

    cfg = dict(depth=2, hidden=384, heads=6, patch=2, sample_size=32, in_channels=4, out_channels=4, cond_dim=1280)
    torch.manual_seed(31)
    model = DiT(DiTConfig(compute_dtype="bf16", **cfg), init="random").cuda()
    B = 128
    x, t = torch.randn(B, 4, 32, 32, device="cuda"), torch.randint(0, 1000, (B,), device="cuda").float()
    c, w = torch.randn(B, 1280, device="cuda"), torch.randn(B, 4, 32, 32, device="cuda") / 4096

    def run():
        model.flat.grad = torch.zeros_like(model.flat.data)
        out = model(x, t, added_cond_kwargs={"text_embeds": c})[0]
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: model.grad_view(n).clone() for n, _ in model.named_tensors()}

    def rel_l2(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm()).item()

    monkeypatch.delenv("UWU_GEMM_TRW", raising=False)
    (y1, g1), (y1b, g1b) = run(), run()
    monkeypatch.setenv("UWU_GEMM_TRW", "0")
    (y0, g0), (y0b, g0b) = run(), run()
    assert torch.equal(y1, y0) and torch.equal(y1, y1b) and torch.equal(y0, y0b)  # the forward is untouched
    weights = [n for n in g0 if n.startswith("blocks.") and n.endswith(".weight")]
    assert len(weights) == 8
    for n in g0:
        assert torch.isfinite(g1[n]).all() and float(g0[n].abs().max()) > 0, n
        if n in weights:
            assert torch.equal(g1[n], g1b[n]) and torch.equal(g0[n], g0b[n]), n  # reproducible in each setting
            if ".qkv." in n or ".proj." in n:
                assert torch.equal(g1[n], g0[n]), n  # the same K slices as gemm_tr, summed in the same order
            else:
                d = rel_l2(g1[n], g0[n])
                print(f"{n}: rel L2 {d:.3e} (parent {PARENT_REL_L2[n]:.3e})")
                assert d <= 2 * PARENT_REL_L2[n], (n, d)
        else:  # fp32 atomic sums
            d = rel_l2(g1[n], g0[n])
            print(f"{n}: rel L2 {d:.3e}")
            assert d <= (BF16_ULP_REL_L2 if n.startswith(AFTER_BF16_ROUNDING) else ATOMIC_REL_L2), (n, d)
