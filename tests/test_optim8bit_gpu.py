"""GPU: the 8-bit block-wise AdamW / Lion kernels (csrc/optimizer_8bit.hip: uwu_adamw8_step, uwu_lion8_step) one step at a time against
the fp64 oracle (tests/optim8bit_oracle.py) from the oracle's own starting state, above the grid cap, under chunking (the classes of
uwudiff_amd/optim.py), on the fixed quadratic problem, and their refusals.

A code is accepted iff it is as near to the oracle's fp64 ratio x = moment / absmax as the nearest entry, within
d = 8 * 2^-24 * (|m_old| + |g_eff|) / absmax_new (second moment: (v_old + g_eff^2) / absmax_new): the fp32 rounding of the element's
own inputs.  At most 0.1 % of the elements may hold a code other than the oracle's own."""
import numpy as np
import pytest
import torch

from tests import optim8bit_oracle as O

pytestmark = pytest.mark.gpu

T1, T2 = O.dynamic_map(True), O.dynamic_map(False)
S_SH = 9.0  # what the shadow holds where no launch wrote


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _start(n, later, rng=None):
    """(p, g, codes1, absmax1, codes2, absmax2) on the host: the fixture's state quantised by the oracle (absmax as fp32)"""
    if rng is None:
        p, g, m, v = O.fixture(n, later)
    else:  # ordinary random data of any size
        p = rng.standard_normal(n).astype(np.float32)
        g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        m, v = rng.standard_normal(n) * 1e-2, rng.standard_normal(n) ** 2 * 1e-4
    c1, a1 = O.quantise(T1, m)[1:]
    c2, a2 = O.quantise(T2, v)[1:]
    return p, g, c1, a1.astype(np.float32), c2, a2.astype(np.float32)


def _check_codes(what, T, first, x, want_c, got_c, old, g_eff, absmax_new, sel):
    n = x.shape[0]
    d = O.code_slack(first, old, g_eff, absmax_new, n)
    ok = O.code_accepted(T, x, got_c, d)[sel]
    differ = int((got_c[sel] != want_c[sel]).sum())
    print(f"{what}: {differ} of {int(ok.size)} codes differ from the oracle's own; {int((~ok).sum())} outside the bound")
    assert ok.all(), what
    return differ, int(ok.size)


def _element_mask(n, e0, e1, blocks=None):
    sel = np.zeros(n, bool)
    if blocks is None:
        sel[e0:e1] = True
    else:
        for b in blocks:
            sel[256 * b:min(256 * b + 256, n)] = True
    return sel


def _run_case(kind, n, later, zero_grad, shadow, clip, pre, e0, e1, rng=None, blocks=None):
    """one launch of the entry point over [e0, e1) and every assertion of the one-step test; ``blocks``: compare these blocks only"""
    from uwudiff_amd import lib as L

    e1 = n if e1 is None else e1
    p, g, c1, a1, c2, a2 = _start(n, later, rng)
    step = 7 if later else 1
    dp, dg = _dev(p), _dev(g)
    dc1, da1, dc2, da2 = _dev(c1), _dev(a1), _dev(c2), _dev(a2)
    dq1, dq2 = _dev(T1), _dev(T2)
    sh = torch.full((n,), S_SH, device="cuda", dtype=torch.bfloat16) if shadow else None
    dclip = torch.tensor([123.0, 0.37], device="cuda") if clip else None
    # the factor the kernel multiplies the gradient by, as it forms it
    g_eff = g.astype(np.float64) * float(np.float32(pre) * (np.float32(0.37) if clip else np.float32(1.0)))
    if kind == "adamw":
        hp = O.HP
        L.call("uwu_adamw8_step", L.ptr(dp), L.ptr(dg), L.ptr(dc1), L.ptr(dc2), L.ptr(da1), L.ptr(da2), L.ptr(dq1), L.ptr(dq2),
               L.ptr(sh), n, e0, e1, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["wd"], step, pre, L.ptr(dclip),
               zero_grad, L.stream())
        o = O.adamw8_step(p, g_eff, c1, a1, c2, a2, T1, T2, step, **hp)
    else:
        hp = O.LION_HP
        L.call("uwu_lion8_step", L.ptr(dp), L.ptr(dg), L.ptr(dc1), L.ptr(da1), L.ptr(dq1), L.ptr(sh), n, e0, e1, hp["lr"],
               hp["betas"][0], hp["betas"][1], hp["wd"], pre, L.ptr(dclip), zero_grad, L.stream())
        o = O.lion8_step(p, g_eff, c1, a1, T1, **hp)
    torch.cuda.synchronize()
    sel = _element_mask(n, e0, e1, blocks)
    bsel = np.zeros(O.blocks_of(n), bool)
    bsel[np.unique(np.nonzero(sel)[0] // 256)] = True
    got_p = _np(dp)
    keep = sel
    if kind == "lion":  # fp32 rounding of c is a few 2^-24 of its terms: outside this band its sign is determined
        out = np.abs(o["c"]) < 2.0 ** -20 * o["mag"]
        print(f"lion: {int((out & sel).sum())} of {int(sel.sum())} elements left out of the p comparison")
        assert (out & sel).sum() <= 1e-3 * sel.sum()
        keep = sel & ~out
    print(f"max |p - oracle| {np.abs(got_p[keep] - o['p'][keep]).max():.3e}")
    np.testing.assert_allclose(got_p[keep], o["p"][keep], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(da1)[bsel], o["a1"][bsel], rtol=1e-5, atol=1e-7)
    differ, total = _check_codes("state1", T1, True, o["x1"], o["c1"], _np(dc1), o["m_old"], g_eff, o["a1"], sel)
    if kind == "adamw":
        np.testing.assert_allclose(_np(da2)[bsel], o["a2"][bsel], rtol=1e-5, atol=1e-7)
        d2, t2 = _check_codes("state2", T2, False, o["x2"], o["c2"], _np(dc2), o["v_old"], g_eff, o["a2"], sel)
        differ, total = differ + d2, total + t2
    assert differ <= int(1e-3 * total), (differ, total)
    if shadow:
        r = slice(e0, e1)
        assert torch.equal(sh[r], dp[r].bfloat16())
        assert (sh[:e0].float() == S_SH).all() and (sh[e1:].float() == S_SH).all()
    r = slice(e0, e1)
    assert np.array_equal(_np(dg)[r], np.zeros(e1 - e0, np.float32) if zero_grad else g[r])
    # nothing outside [e0, e1) is touched, in any buffer
    outside = ~_element_mask(n, e0, e1)
    bout = np.ones(O.blocks_of(n), bool)
    bout[e0 // 256:-(-e1 // 256)] = False
    assert np.array_equal(got_p[outside], p[outside]) and np.array_equal(_np(dg)[outside], g[outside])
    assert np.array_equal(_np(dc1)[outside], c1[outside]) and np.array_equal(_np(da1)[bout], a1[bout])
    assert np.array_equal(_np(dc2)[outside], c2[outside]) and np.array_equal(_np(da2)[bout], a2[bout])
    return o, _np(dc1), _np(dc2)


# n, later step, zero_grad, shadow, clip, pre_scale, e0, e1
N0 = 3 * 256 + 37
CASES = [(N0, False, 1, True, False, 1.0, 0, None),
         (N0, True, 0, False, True, 0.5, 0, None),
         (N0, True, 1, True, True, 0.5, 256, None),
         (N0, True, 0, True, False, 1.0, 256, 768),
         (256, False, 0, True, False, 1.0, 0, None),
         (256, True, 1, False, True, 0.5, 0, None)]
IDS = ["step1-zero-state", "later-clip-noshadow", "later-e0-256", "later-inner-range", "one-block-step1", "one-block-later"]


# ------------------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adamw8_one_step_from_the_oracle_s_state(case):
    n, later = case[:2]
    o, c1, c2 = _run_case("adamw", *case)
    e0, e1 = case[6], n if case[7] is None else case[7]
    if n > 256 and e0 <= 256 and e1 >= 768:
        if not later:  # zero state, zero gradient: absmax 0 and the zero codes
            assert o["a1"][1] == 0 and (c1[256:512] == 127).all() and (c2[256:512] == 0).all()
        zero = np.delete(np.arange(512, 768), 17)  # one element 1e9 times the rest: the others take the zero code
        assert (c1[zero] == 127).all() and (c2[zero] == 0).all() and c1[512 + 17] == 255 and c2[512 + 17] == 255
    if e0 == 0:
        assert c1[5] == 0  # exactly at -absmax: the lowest entry
    if e1 == n and n > 256:
        assert c1[n - 3] == 255  # exactly at +absmax


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lion8_one_step_from_the_oracle_s_state(case):
    n, later = case[:2]
    o, c1, _ = _run_case("lion", *case)
    e0, e1 = case[6], n if case[7] is None else case[7]
    if n > 256 and e0 <= 256 and e1 >= 768 and not later:
        assert o["a1"][1] == 0 and (c1[256:512] == 127).all()
    if e0 == 0:
        assert c1[5] == 0


# ------------------------------------------------------------------------------------------------------------ grid stride
N_STRIDE = 2048 * 4 * 256 + 5 * 256 + 37  # the launch's cap is 2048 workgroups of 4 blocks: the loop body runs twice in some


@pytest.mark.parametrize("kind", ["adamw", "lion"])
def test_above_the_grid_cap_with_a_ragged_tail(kind):
    nb = O.blocks_of(N_STRIDE)
    blocks = sorted(set(range(0, nb, 97)) | {0, 2048 * 4 - 1, 2048 * 4, nb - 2, nb - 1})
    _run_case(kind, N_STRIDE, True, 1, True, True, 0.5, 0, None, rng=np.random.default_rng(21), blocks=blocks)


# ------------------------------------------------------------------------------------------------------------ chunking
def _stepped(name, n, chunks, grads, p0):
    from uwudiff_amd import optim

    flat = torch.nn.Parameter(_dev(p0))
    flat._uwu_bf16_shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    opt = getattr(optim, name)([flat], lr=1e-3, weight_decay=0.1)
    waited = []
    for g in grads:
        flat.grad = _dev(g)
        if chunks is None:
            opt.step(zero_grad=True)
        else:
            opt.step(chunks=chunks, before_chunk=waited.append, zero_grad=True)
        assert not flat.grad.any()
    torch.cuda.synchronize()
    assert torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16())
    if chunks is not None:
        assert waited == list(range(len(chunks))) * len(grads)
    return flat, opt.state[flat]


@pytest.mark.parametrize("name", ["FusedAdamW8bit", "FusedLion8bit"])
def test_any_chunking_gives_the_unchunked_step_s_bits(name):
    """3 steps; the chunks' offsets are multiples of 4 and not of 256 and arrive in non-ascending order (blocks straddle chunks): a
    block updated twice, or before its gradient, would show in the bits"""
    n = 10 * 256 + 37
    rng = np.random.default_rng(8)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * s).astype(np.float32) for s in (1e-2, 1.0, 1e-3)]
    cuts = [0, 100, 260, 1284, 2560 - 8, n]
    chunks = [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    chunks = [chunks[i] for i in (4, 2, 3, 0, 1)]
    assert all(off % 4 == 0 for off, _ in chunks) and sum(off % 256 != 0 for off, _ in chunks) >= 3
    whole, st_w = _stepped(name, n, None, grads, p0)
    split, st_s = _stepped(name, n, chunks, grads, p0)
    assert torch.equal(whole.detach().view(torch.int32), split.detach().view(torch.int32))
    keys = ("state1", "absmax1") + (("state2", "absmax2") if name == "FusedAdamW8bit" else ())
    assert set(st_w) == set(keys) | {"qmap" + k[-1] for k in keys} | ({"step"} if name == "FusedAdamW8bit" else set())
    for k in keys:
        assert st_w[k].dtype == (torch.uint8 if k.startswith("state") else torch.float32)
        assert torch.equal(st_w[k], st_s[k]), k
        assert st_w[k].float().abs().max() > 0
    assert float((whole.detach() - _dev(p0)).abs().max()) > 0


def test_chunks_that_leave_a_block_partly_covered_are_refused():
    from uwudiff_amd.optim import FusedAdamW8bit

    flat = torch.nn.Parameter(torch.zeros(1024, device="cuda"))
    flat.grad = torch.ones(1024, device="cuda")
    with pytest.raises(ValueError, match="partly covered"):
        FusedAdamW8bit([flat]).step(chunks=[(0, 512), (600, 424)])


# ------------------------------------------------------------------------------------------------------------ quality
def test_adamw8_stays_as_close_to_exact_adamw_as_the_oracle_s_8bit_run():
    """The fixed quadratic problem (n = 4196, g = D (p - p*) formed on the device, D = exp(N(0, 0.5)), p* = N(0, 1)), 200 steps at
    lr 1e-3.  The oracle's own 8-bit run ends at an rms distance of 0.00945 from exact fp64 AdamW (computed on the CPU:
    tests/test_optim8bit_cpu.py); the kernel's run may end at most twice as far: near-tie codes let the trajectories part, and
    nothing else should differ.  On the MI355X the kernel's run ends at 0.0116."""
    from uwudiff_amd.optim import FusedAdamW8bit

    D, pstar = O.quadratic_problem()
    pe, pq = O.quadratic_runs()
    want = float(np.sqrt(np.mean((pq - pe) ** 2)))
    flat = torch.nn.Parameter(torch.zeros(D.shape[0], device="cuda"))
    dD, dstar = _dev(D), _dev(pstar)
    opt = FusedAdamW8bit([flat], lr=O.HP["lr"], betas=O.HP["betas"], eps=O.HP["eps"], weight_decay=O.HP["wd"])
    for _ in range(200):
        flat.grad = dD * (flat.detach() - dstar)
        opt.step()
    torch.cuda.synchronize()
    got = float(np.sqrt(np.mean((_np(flat).astype(np.float64) - pe) ** 2)))
    print(f"rms distance from exact AdamW: kernel {got:.5f}, oracle's 8-bit run {want:.5f}")
    assert opt.state[flat]["step"] == 200
    assert got <= 2 * want


# ------------------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L

    n = 600
    f = torch.zeros(n + 8, device="cuda")
    c = torch.zeros(n + 8, device="cuda", dtype=torch.uint8)
    a = torch.zeros(4, device="cuda")
    q = _dev(T1)
    s = L.stream()

    def adamw(p=f.data_ptr(), g=f.data_ptr(), c1=c.data_ptr(), c2=c.data_ptr(), a1=a.data_ptr(), a2=a.data_ptr(), q1=q.data_ptr(),
              q2=q.data_ptr(), e0=0, e1=n, step=1):
        L.call("uwu_adamw8_step", p, g, c1, c2, a1, a2, q1, q2, None, n, e0, e1, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0, None, 0, s)

    def lion(p=f.data_ptr(), g=f.data_ptr(), c1=c.data_ptr(), a1=a.data_ptr(), q1=q.data_ptr(), e0=0, e1=n):
        L.call("uwu_lion8_step", p, g, c1, a1, q1, None, n, e0, e1, 1e-4, 0.9, 0.99, 0.0, 1.0, None, 0, s)

    for fn, name in ((adamw, "uwu_adamw8_step"), (lion, "uwu_lion8_step")):
        bad = [dict(p=None), dict(g=None), dict(c1=None), dict(a1=None), dict(q1=None),  # null pointers
               dict(p=f.data_ptr() + 4), dict(g=f.data_ptr() + 8), dict(c1=c.data_ptr() + 2),  # misaligned bases
               dict(e0=4), dict(e0=256, e1=256), dict(e1=500), dict(e1=n + 1), dict(e0=-256)]  # ranges that break the rule
        if fn is adamw:
            bad += [dict(c2=None), dict(a2=None), dict(q2=None), dict(c2=c.data_ptr() + 1), dict(step=0)]
        for kw in bad:
            with pytest.raises(L.UwuError, match=name + ": "):
                fn(**kw)
        fn()  # the same call with nothing wrong is taken
        fn(e0=256, e1=512)
        fn(e0=512)
    torch.cuda.synchronize()
    assert not f.any()  # (zero gradient on zero parameters: nothing moved)
