"""GPU: the wide streaming weight-gradient kernel (gemm_trw_kernel) with its eight waves as two groups one barrier apart.

The grouped K loop hand-counts its vmcnt waits and splits its barriers between the two groups; it multiplies the same fragments
in the same order per accumulator as the in-phase loop (UWU_TRW_GROUPS=0), so
  * on operands in {-1, 0, 1} every fp32 partial sum is an exact integer (|sum| <= 33 000 < 2^24): dW and the fused bias gradient
    must equal the fp32 matmul / column sum bit for bit, in every one of three launches (the schedule must not depend on timing);
  * on real-valued operands dW must equal the in-phase loop's bit for bit.  (The bias gradient is an fp32 atomic sum over the K
    slices there: it differs between two launches of ONE schedule, so only the integer cases compare it.)
All shapes take the kernel the way the training step does: M or N a multiple of 384, at least 32768 tokens.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

K0 = 32768
_cache = {}


def _operand(K, width, ints, seed):
    """[K, width] bf16 on the device, made once per key and left unchanged."""
    key = (K, width, ints, seed)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(seed)
        if ints:
            _cache[key] = torch.randint(-1, 2, (K, width), generator=g, device="cuda").bfloat16()
        else:
            _cache[key] = torch.randn(K, width, generator=g, device="cuda").bfloat16()
    return _cache[key]


def _want(M, N, K):
    """Exact references of the integer case (M, N, K): (dW on top of 2.0, bias gradient on top of 3.0)."""
    key = ("want", M, N, K)
    if key not in _cache:
        a, b = _operand(K, M, True, 1), _operand(K, N, True, 2)
        _cache[key] = (a.float().t() @ b.float() + 2.0, a.float().sum(0) + 3.0)
    return _cache[key]


def _slices(M, N, K):
    """(K-steps per slice, K-steps of the last slice) as launch_trw divides K: 8 slices per XCD round, as many rounds as 32 CUs
    hold tiles, at least 8 K-steps per slice.  The slice count is the host's own; `blocks` does not reach this kernel."""
    tiles = ((M + 191) // 192) * (N // 384) if N % 384 == 0 else (M // 384) * ((N + 191) // 192)
    steps = K // 32
    split = 8 * max(32 // tiles, 1)
    while split > 8 and split * 8 > steps:
        split -= 8
    per = -(-steps // split)
    split = -(-steps // per)
    return per, steps - per * (split - 1)


# (out, in, tokens).  (384, 1536): the 384 x 192 orientation.  32768 + 160 tokens = 1029 K-steps: (1152, 384) has 40 slices of
# 26 and a last one of 15; (576, 384) has 80 slices of 13 and a last one of 2 -- and of 1 at 1028 K-steps: shorter than the three
# K-steps the ring runs ahead, the `younger < 2` tail of the vmcnt ladder from the first wait on, in both groups.
EXACT = [(384, 384, K0), (1536, 384, K0), (384, 1536, K0), (1152, 384, K0 + 160), (576, 384, K0 + 160), (576, 384, K0 + 128)]


@pytest.mark.parametrize("M,N,K", EXACT)
def test_groups_exact_integers(M, N, K):
    from uwudiff_amd import ops

    if (M, K) == (576, K0 + 160):
        assert _slices(M, N, K) == (13, 2)
    if (M, K) == (576, K0 + 128):
        assert _slices(M, N, K) == (13, 1)
    if (M, K) == (1152, K0 + 160):
        assert _slices(M, N, K) == (26, 15)
    a, b = _operand(K, M, True, 1), _operand(K, N, True, 2)
    want, bsum = _want(M, N, K)
    scratch = ops.gemm_wgrad_scratch(M, N, K)
    for _ in range(3):
        dw = torch.full((M, N), 2.0, device="cuda")
        db = torch.full((M,), 3.0, device="cuda")
        ops.gemm_wgrad(a, b, dw, scratch=scratch, bias_grad=db)
        assert torch.equal(dw, want)
        assert torch.equal(db, bsum)


PAIRS = [((1536, 384), (384, 1536)), ((1152, 384), (384, 384))]  # fc1 + fc2, qkv + proj of DiT-S/2


def _run_pair(shapes, ints):
    from uwudiff_amd import ops

    (Ma, Na), (Mb, Nb) = shapes
    ops_ = [(_operand(K0, M, ints, 1 if ints else 11), _operand(K0, N, ints, 2 if ints else 12)) for M, N in shapes]
    dws = [torch.full(s, 2.0, device="cuda") for s in shapes]
    dbs = [torch.full((s[0],), 3.0, device="cuda") for s in shapes]
    ops.gemm_wgrad_pair(ops_[0][0], ops_[0][1], dws[0], ops_[1][0], ops_[1][1], dws[1],
                        scratch=ops.gemm_wgrad_pair_scratch(Ma, Na, Mb, Nb, K0), bias_grad_a=dbs[0], bias_grad_b=dbs[1])
    return dws, dbs


@pytest.mark.parametrize("shapes", PAIRS, ids=["fc", "attn"])
def test_groups_pair_exact_integers(shapes):
    from uwudiff_amd import lib as L

    (Ma, Na), (Mb, Nb) = shapes
    assert L.load().uwu_gemm_wgrad_pair_scratch_bytes(Ma, Na, Mb, Nb, K0) > 0  # one grouped launch
    for _ in range(3):
        dws, dbs = _run_pair(shapes, True)
        for (M, N), dw, db in zip(shapes, dws, dbs):
            want, bsum = _want(M, N, K0)
            assert torch.equal(dw, want)
            assert torch.equal(db, bsum)


def _both(monkeypatch, run):
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("UWU_TRW_GROUPS", flag)
        out.append(run())
    monkeypatch.delenv("UWU_TRW_GROUPS")
    return out


@pytest.mark.parametrize("M,N,K", EXACT)
def test_groups_match_in_phase_loop(M, N, K, monkeypatch):
    from uwudiff_amd import ops

    a, b = _operand(K, M, False, 11), _operand(K, N, False, 12)
    scratch = ops.gemm_wgrad_scratch(M, N, K)

    def run():
        dw = torch.full((M, N), 2.0, device="cuda")
        db = torch.full((M,), 3.0, device="cuda")  # (asked for so that the bias MFMAs run; compared in the integer cases)
        ops.gemm_wgrad(a, b, dw, scratch=scratch, bias_grad=db)
        return dw

    grouped, in_phase = _both(monkeypatch, run)
    assert torch.equal(grouped, in_phase)
    assert not torch.equal(grouped, torch.full_like(grouped, 2.0))


@pytest.mark.parametrize("shapes", PAIRS, ids=["fc", "attn"])
def test_groups_pair_matches_in_phase_loop(shapes, monkeypatch):
    (g_dws, _), (p_dws, _) = _both(monkeypatch, lambda: _run_pair(shapes, False))
    for g, p in zip(g_dws, p_dws):
        assert torch.equal(g, p)


def test_groups_ragged_columns_stay_inside(monkeypatch):
    """N = 392: two 192-column tiles and one 8-column group.  The third tile's other DMA columns are clamped to the operand's last
    8 and multiplied like any others; none of those products may reach dW, whose rows here are 400 floats apart with a
    sentinel in the 8 floats behind each row."""
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    M, N, K = 384, 392, K0
    a, b = _operand(K, M, True, 1), _operand(K, N, True, 3)
    want, bsum = a.float().t() @ b.float() + 2.0, a.float().sum(0) + 3.0
    scratch = ops.gemm_wgrad_scratch(M, N, K)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("UWU_TRW_GROUPS", flag)
        big = torch.full((M, 400), 2.0, device="cuda")
        big[:, N:] = -7.0
        db = torch.full((M,), 3.0, device="cuda")
        L.call("uwu_gemm_wgrad", L.ptr(a), L.ptr(b), L.ptr(big), L.ptr(db), M, N, K, M, N, big.stride(0), L.dt(a), 512,
               L.ptr(scratch), scratch.numel(), L.stream())  # (ops.gemm_wgrad takes contiguous outputs only)
        assert torch.equal(big[:, :N], want)
        assert torch.equal(big[:, N:], torch.full((M, 8), -7.0, device="cuda"))
        assert torch.equal(db, bsum)
        outs.append(big)
    assert torch.equal(outs[0], outs[1])
