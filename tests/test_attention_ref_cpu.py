"""The fp64 attention reference of tests/test_attention_accuracy_gpu.py (tests/attention_oracle.py) against torch.autograd in
float64, the sharpness of its bars (faults seeded into the yardstick must break them) and the exactness of the routing construction
in the yardstick's arithmetic."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_oracle as O

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
MARGIN = 4.0
# (d, Tq, Tk) of the exact routing tests in tests/test_attention_accuracy_gpu.py (the last one: the rope entry points at T = 64)
ROUTING_SHAPES = [(40, 321, 321), (64, 256, 256), (72, 300, 77), (80, 449, 449), (128, 64, 200), (160, 100, 40), (32, 64, 13),
                  (64, 64, 64)]


@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("B,H,Tq,Tk,d", [(2, 3, 7, 7, 8), (1, 2, 9, 5, 16), (2, 1, 4, 13, 24)])
def test_reference_matches_autograd(B, H, Tq, Tk, d, biased):
    torch.manual_seed(100 * Tq + Tk)
    q, k, v = (torch.randn(B, H, T, d, dtype=F64, requires_grad=True) for T in (Tq, Tk, Tk))
    do = torch.randn(B, H, Tq, d, dtype=F64)
    bias = 2.0 * torch.randn(B, Tk, dtype=F64) if biased else None
    scale = 0.37
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=None if bias is None else bias[:, None, None, :], scale=scale)
    dq, dk, dv = torch.autograd.grad((o * do).sum(), [q, k, v])
    with torch.no_grad():
        e = O.evaluate(q, k, v, do, bias=bias, scale=scale, dtype=F64, round_p=False)
        s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale + (0 if bias is None else bias[:, None, None, :])
        ob, lb = O.forward_blockwise(q, k, v, bias=bias, scale=scale, dtype=F64, round_p=False, tile=4)
        # handed o and lse: the same results when they are the forward's own
        e2 = O.evaluate(q, k, v, do, bias=bias, scale=scale, dtype=F64, round_p=False, o=e["o"], lse=e["lse"])
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(e["o"], o.detach(), **tol)
    torch.testing.assert_close(e["lse"], torch.logsumexp(s.detach(), -1), **tol)
    torch.testing.assert_close(e["delta"], (do * o.detach()).sum(-1), **tol)
    for name, ref in (("dq", dq), ("dk", dk), ("dv", dv)):
        torch.testing.assert_close(e[name], ref, **tol)
        torch.testing.assert_close(e2[name], ref, **tol)
    torch.testing.assert_close(ob, o.detach(), **tol)
    torch.testing.assert_close(lb, e["lse"], **tol)


def test_handed_o_and_lse_define_the_backward():
    """p = exp(s - lse) and delta = rowsum(dO * o) of exactly the tensors handed in: other o / lse, other gradients."""
    q, k, v, do = O.hard_inputs("plain", 1, 2, 8, 12, 16, F32)
    kw = dict(scale=0.25, dtype=F64, round_p=False)
    e = O.evaluate(q, k, v, do, **kw)
    e2 = O.evaluate(q, k, v, do, o=e["o"] + 0.5, lse=e["lse"] + math.log(2.0), **kw)
    torch.testing.assert_close(e2["dv"], 0.5 * e["dv"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(e2["delta"], e["delta"] + 0.5 * do.double().sum(-1), rtol=1e-12, atol=1e-12)
    assert torch.equal(e2["o"], e["o"]) and torch.equal(e2["lse"], e["lse"])  # the forward outputs stay the forward's


def test_round_p_rounds_where_the_mfma_kernels_do():
    """l from the unrounded p (lse is independent of round_p); o, dv, dq, dk change by about 2^-9 relative; outputs unrounded."""
    q, k, v, do = O.hard_inputs("plain", 2, 2, 64, 96, 64, BF16)
    kw = dict(scale=0.125, dtype=F32)
    a, b = O.evaluate(q, k, v, do, round_p=False, **kw), O.evaluate(q, k, v, do, round_p=True, **kw)
    assert torch.equal(a["lse"], b["lse"])
    for name in ("o", "dq", "dk", "dv"):
        diff = (a[name] - b[name]).abs().max().item()
        assert 1e-5 < diff < 2e-2, (name, diff)
        assert not torch.equal(b[name], b[name].to(BF16).float()), name
    assert a["o"].dtype == F32 and O.evaluate(q, k, v, do, round_p=False, scale=0.125, dtype=F64)["o"].dtype == F64


def test_rope_contract():
    x = torch.randn(1, 2, 4, 8).to(BF16)
    tab = torch.rand(2, 4, 8) * 3 - 1.5
    r = O.rope(x, tab)
    assert r.dtype == BF16 and torch.equal(r, (x.float() * tab[None]).to(BF16))


# ------------------------------------------------------------------------------------------------------------- hard inputs
def test_hard_inputs():
    B, H, Tq, Tk, d = 2, 3, 128, 192, 64
    scale = d ** -0.5

    def scores(cls):
        q, k, v, do = O.hard_inputs(cls, B, H, Tq, Tk, d, BF16)
        assert q.dtype == BF16 and q.shape == (B, H, Tq, d) and k.shape == v.shape == (B, H, Tk, d) and do.shape == q.shape
        return torch.einsum("bhqd,bhkd->bhqk", q.double(), k.double()) * scale

    assert 0.8 < scores("plain").std() < 1.2
    assert 3.2 < scores("peaked").std() < 4.8
    s = scores("offset")
    assert s.min() > 200 and 300 < torch.logsumexp(s, -1).mean() < 350
    s = scores("rising")
    tile_max = torch.stack([s[..., t:t + 64].amax(-1) for t in (0, 64, 128)])
    assert (tile_max[1:] > tile_max[:-1]).all()  # the running maximum rises in every tile, for every query
    f = scores("falling")
    assert (f[..., :64].amax(-1) == f.amax(-1)).all()  # ... and is found in the first tile here
    q, k, v, do = O.hard_inputs("degenerate", B, H, Tq, Tk, d, F32)
    r = O.special_rows(B, Tq, Tk)
    e = O.evaluate(q, k, v, do, scale=scale, dtype=F64, round_p=False)
    for b in range(B):
        assert (q[b, :, r["zq"][b]] == 0).all() and (k[b, :, r["zk"][b]] == 0).all() and (do[b, :, r["zdo"][b]] == 0).all()
        assert torch.equal(k[b, :, r["dup"][b]], k[b, :, r["src"][b]])
        assert len({int(r[n][b]) for n in ("zk", "dup", "src")}) == 3 and r["zq"][b] != r["zdo"][b]
        torch.testing.assert_close(e["lse"][b, :, r["zq"][b]], torch.full((H,), math.log(Tk), dtype=F64))
        torch.testing.assert_close(e["o"][b, :, r["zq"][b]], v[b].double().mean(1))
        assert (e["dq"][b, :, r["zdo"][b]] == 0).all()
    for c in O.CLASSES + ("falling",):
        for dt in (F32, BF16):
            for T2 in ((100, 40), (64, 13)):
                assert all(torch.isfinite(t.float()).all() for t in O.hard_inputs(c, B, H, *T2, 32, dt))


@pytest.mark.parametrize("Tk", [13, 77, 192, 449])
def test_hard_bias(Tk):
    B = 2
    for cls in O.BIAS_CLASSES:
        bias = O.hard_bias(cls, B, Tk)
        assert bias.dtype == F32 and bias.shape == (B, Tk) and torch.isfinite(bias).all()
        assert ((bias > -100).sum(1) >= 1).all(), cls
    assert (O.hard_bias("first_tile", B, Tk)[:, :min(64, Tk - 1)] == O.HIDE).all()
    last = O.hard_bias("last_tile", B, Tk)
    t0 = (Tk - 1) // 64 * 64
    assert (last[:, :t0 + 1] == 0).all() and (last[:, t0 + 1:] == O.HIDE).all()
    one = O.hard_bias("all_but_one", B, Tk)
    assert ((one == 0).sum(1) == 1).all() and (one[torch.arange(B), O.visible_key(B, Tk)] == 0).all()
    frac = (O.hard_bias("random40", B, Tk) == O.HIDE).float().mean().item()
    assert 0.15 < frac < 0.65


# ------------------------------------------------------------------------------------------------------------ seeded faults
B_, H_, D_ = 2, 2, 64
SCALE_ = D_ ** -0.5


def _flat_ratios(got, ref, yard):
    """The bars of tests/test_attention_accuracy_gpu.py on a bf16 MFMA route: worst ratio per output."""
    return {n: O.ratio(got[n], ref[n], yard[n], bf16_out=n != "lse")[1] for n in got}


def _faulty(fault, cls, bias_cls):
    """(got, ref, yard) of one seeded fault on one input class; got = a copy of the fp32 round_p evaluation with the fault."""
    Tq, Tk = (128, 77) if fault == "double_last" else (128, 192)
    q, k, v, do = O.hard_inputs(cls, B_, H_, Tq, Tk, D_, BF16)
    bias = O.hard_bias(bias_cls, B_, Tk) if bias_cls else None
    kw = dict(scale=SCALE_, bias=bias)
    ref = O.evaluate(q, k, v, do, dtype=F64, round_p=False, **kw)
    yard = O.evaluate(q, k, v, do, dtype=F32, round_p=True, **kw)
    ykw = dict(dtype=F32, round_p=True, **kw)
    names = ("o", "lse", "dq", "dk", "dv")
    if fault == "none":
        got = O.evaluate(q.clone(), k, v, do, **ykw)
    elif fault in ("drop_key", "delta_roll", "dk_noscale"):
        got = O.evaluate(q, k, v, do, fault=fault, **ykw)
    elif fault == "double_last":  # the last key of the ragged tile counted twice
        k2, v2 = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
        b2 = None if bias is None else torch.cat([bias, bias[:, -1:]], 1)
        got = O.evaluate(q, k2, v2, do, dtype=F32, round_p=True, scale=SCALE_, bias=b2)
        for n in ("dk", "dv"):
            got[n] = torch.cat([got[n][:, :, :-2], got[n][:, :, -2:-1] + got[n][:, :, -1:]], 2)
    elif fault == "stale_alpha":  # forward only
        o, lse = O.forward_blockwise(q, k, v, stale_alpha_tile=1, **kw)
        got = dict(o=o, lse=lse)
        names = ("o", "lse")
    elif fault == "lse_off":  # the forward's lse output
        got = dict(yard)
        got["lse"] = yard["lse"] + 1e-3
    else:
        assert fault == "bias_swap", fault
        got = O.evaluate(q, k, v, do, dtype=F32, round_p=True, scale=SCALE_, bias=bias[[0, 0]])
    return {n: got[n] for n in names}, ref, yard


# fault -> the (values class, bias class) pairs that must catch it
CATCHES = {
    "drop_key": [("plain", None), ("peaked", None), ("degenerate", None), ("plain", "randn2")],
    "double_last": [("plain", None), ("peaked", None), ("plain", "randn2")],
    "stale_alpha": [("rising", None), ("peaked", None), ("plain", "first_tile")],
    "lse_off": [("plain", None), ("peaked", None), ("offset", None), ("rising", None), ("degenerate", None)],
    "delta_roll": [("plain", None), ("peaked", None), ("offset", None), ("degenerate", None)],
    "dk_noscale": [("plain", None), ("peaked", None), ("offset", None), ("rising", None), ("degenerate", None)],
    "bias_swap": [("plain", "random40"), ("plain", "randn2")],
}


@pytest.mark.parametrize("fault", list(CATCHES))
def test_seeded_faults_break_the_bars(fault):
    """Each fault is applied to a copy of the fp32 round_p = True evaluation and must push a ratio above the margin:
      one key's probability set to 0 (drop_key)           plain, peaked, degenerate, randn2 bias (o, dq, dk, dv)
      the last key of a ragged tile counted twice, Tk = 77  plain, peaked, randn2 bias (o, lse, dv)
      alpha left at 1 for the second key tile             rising (every row), peaked (rows whose maximum moves), first_tile bias (the
                                                          hidden tile is not forgotten); NOT plain: the maximum hardly moves there
      the forward's lse off by 1e-3                       every class: the lse bar is a few ulps of lse, 4e-5 at lse = 335
      delta taken from the neighbouring query row         plain, peaked, offset, degenerate (dq, dk)
      scale missing from dk                               every class
      the bias of sample 0 applied to sample 1            random40, randn2 (the per-sample biases); the tile biases are shared"""
    for cls, bias_cls in CATCHES[fault]:
        got, ref, yard = _faulty(fault, cls, bias_cls)
        r = _flat_ratios(got, ref, yard)
        print(f"[attn-fault] {fault:<12s} {cls:<10s} {bias_cls or '-':<11s} " + "  ".join(f"{n}={x:.3g}" for n, x in r.items()))
        assert max(r.values()) > MARGIN, (fault, cls, bias_cls, r)


@pytest.mark.parametrize("cls,bias_cls", [(c, None) for c in O.CLASSES + ("falling",)] + [("plain", b) for b in O.BIAS_CLASSES]
                         + [("offset", "random40")])
def test_the_unfaulted_yardstick_sits_inside_the_bars(cls, bias_cls):
    """A second evaluation of the yardstick, blockwise forward included (another tile at which p meets its rounding): within 4."""
    got, ref, yard = _faulty("none", cls, bias_cls)
    assert max(_flat_ratios(got, ref, yard).values()) <= 1.0
    q, k, v, do = O.hard_inputs(cls, B_, H_, 128, 192, D_, BF16)
    bias = O.hard_bias(bias_cls, B_, 192) if bias_cls else None
    o, lse = O.forward_blockwise(q, k, v, bias=bias, scale=SCALE_)
    r = _flat_ratios(dict(o=o, lse=lse), ref, yard)
    print(f"[attn-fault] blockwise    {cls:<10s} {bias_cls or '-':<11s} o={r['o']:.3g} lse={r['lse']:.3g}")
    assert max(r.values()) <= MARGIN, r


# ------------------------------------------------------------------------------------------------------------ exact routing
@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("d,Tq,Tk", ROUTING_SHAPES)
def test_routing_construction_is_exact_in_the_yardstick(d, Tq, Tk, biased):
    B, H = 2, 3
    r = O.routing_inputs(B, H, Tq, Tk, d, biased)
    for t in (r["q"], r["k"], r["v"], r["do"]):
        assert torch.equal(t, t.to(BF16).float())  # bf16-exact inputs
    if Tq >= Tk:  # every visible key is somebody's winner
        for b in range(B):
            want = Tk if not biased else int((r["bias"][b] == 0).sum())
            assert all(len(torch.unique(r["pi"][b, h])) == want for h in range(H))
    if biased:
        assert (torch.gather(r["bias"][:, None, :].expand(B, H, Tk), 2, r["pi"]) == 0).all()
        assert ((r["bias"] == O.HIDE).sum(1) == Tk // 3).all()
    kw = dict(bias=r["bias"], scale=r["scale"], dtype=F32, round_p=True)
    e = O.evaluate(r["q"], r["k"], r["v"], r["do"], **kw)
    e2 = O.evaluate(r["q"], r["k"], r["v"], r["do"], o=e["o"].to(BF16), lse=e["lse"], **kw)
    ob, lb = O.forward_blockwise(r["q"], r["k"], r["v"], bias=r["bias"], scale=r["scale"])
    assert torch.equal(e["o"], r["o"]) and torch.equal(ob, r["o"])
    for lse in (e["lse"], lb):
        assert ((lse.double() - r["lse"]).abs() <= 2.0 ** -22 * r["lse"].abs()).all()
    for x in (e, e2):
        assert torch.equal(x["dv"], r["dv"])
        assert (x["dq"] == 0).all() and (x["dk"] == 0).all()
    if biased:
        hidden = (r["bias"] == O.HIDE)[:, None, :, None].expand_as(r["dv"])
        assert (r["dv"][hidden] == 0).all()
    # the float64 reference agrees, so the expected values are the attention of these inputs and not only the yardstick's
    e64 = O.evaluate(r["q"], r["k"], r["v"], r["do"], bias=r["bias"], scale=r["scale"], dtype=F64, round_p=False)
    torch.testing.assert_close(e64["o"], r["o"].double(), rtol=0, atol=1e-30)
    torch.testing.assert_close(e64["dv"], r["dv"].double(), rtol=0, atol=1e-30)
    assert e64["dq"].abs().max() < 1e-30 and e64["dk"].abs().max() < 1e-30
