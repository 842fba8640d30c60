"""Every kernel the trainable attention entry points can dispatch to (uwu_attention_fwd / _bwd, uwu_attention_bias_fwd / _bwd,
uwu_attention_rope_fwd / _bwd: csrc/attention_mfma.hip, attention_p256.hip, attention_simple.hip) against a float64 reference, on
score rows that are hard for a flash-attention kernel.

Reference and yardstick (tests/attention_oracle.py, checked by tests/test_attention_ref_cpu.py): `evaluate` in float64 on the rounded
inputs the device gets.  Contract points:
  * backward: defined from the o and lse handed to it (p = exp(s - lse), delta = rowsum(dO * o)); the reference uses, in fp64, exactly
    those tensors.  Every case runs the backward twice: on the forward kernel's own o and lse, and on the fp64 o and lse rounded to
    the dtypes (which isolates the backward).
  * rope: q and k are bf16(float(x) * table) while staged; the reference rotates and rounds first, and dq / dk are gradients with
    respect to the rotated tensors.
  * key bias: finite; -10000 hides a key.

Bars.  E = max over the tensor of |yardstick - fp64|; the yardstick is the same formulas in torch fp32 on the CPU, with P and dS
rounded to bf16 where the MFMA kernels round them (MFMA routes) or unrounded (the generic kernels keep P in fp32).  Per element
    |got - ref| <= 4 * max(E, 2^-23 * A) + (bf16 output ? 2^-8 * |ref| : 0),     A = max |ref|
lse and delta are fp32 outputs on every route (delta is written by the generic kernels and by the lean d = 80 form only).  In the
`degenerate` class the special rows ("name[0]") and the other rows are each held to the E and A of their own rows.  The margin of 4
covers the summation order and the tile at which a probability meets its bf16 rounding, nothing else.  Each test prints its ratios
("[attn-acc] ...", pytest -s) before it asserts; profiles/attention_accuracy_mi355x.txt records them.

Semantics asserted on every call: 64 rows of NaN behind every input read by row and 64 sentinel rows behind every output (results
finite, sentinels untouched); two runs give the same bits; packed qkv views and separate tensors; ops.attention_route says the case
is on the route it is meant for.  Exact statements: the dq row of an all-zero dO row is zero; with every key but one hidden, o is
that key's v row bit for bit.

test_exact_routing is tolerance-free: attention_oracle.routing_inputs makes attention a gather (integers, powers of two, every
losing probability exactly 0), so one wrong index anywhere -- swizzle, transposed stager, clamped tail, key block, dS image -- moves
an output by at least 1."""
import pytest
import torch

from tests import attention_oracle as O

pytestmark = pytest.mark.gpu

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
B, H = 2, 3
TAIL = 64
MARGIN = 4.0
NAME = {F32: "fp32", BF: "bf16"}


# ---------------------------------------------------------------------------------------------------------------- device
def _poisoned(body):
    """`body` on the device with TAIL rows (1-D: floats) of NaN behind it -> the view of the body"""
    full = torch.full((body.shape[0] + TAIL, *body.shape[1:]), float("nan"), dtype=body.dtype, device="cuda")
    full[:body.shape[0]] = body
    return full[:body.shape[0]]


class Problem:
    """One attention problem on the device: flat [B*T, H*d] inputs with poison behind them."""

    def __init__(self, q, k, v, do, d, Tq, Tk, *, bias=None, tab=None, packed=False):
        self.d, self.Tq, self.Tk, self.D, self.dtype, self.packed = d, Tq, Tk, H * d, q.dtype, packed
        D = self.D
        qf, kf, vf, dof = (O.flat(t) for t in (q, k, v, do))
        if packed:
            assert Tq == Tk
            qkv = _poisoned(torch.cat([qf, kf, vf], dim=1))
            self.q, self.k, self.v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        else:
            self.q, self.k, self.v = (_poisoned(t) for t in (qf, kf, vf))
        self.do = _poisoned(dof)
        self.bias = None if bias is None else _poisoned(bias.reshape(-1))
        self.tab = None if tab is None else _poisoned(tab)  # fp32 [T, H*d]
        self.scale = float(torch.tensor(d ** -0.5, dtype=F32))

    def _dims(self):
        from uwudiff_amd import lib as L

        ld = (self.q.stride(0), self.k.stride(0), self.v.stride(0), self.D)
        if self.tab is not None:
            return (B, self.Tq, H, self.d, *ld, self.D, self.scale, L.dt(self.q), L.stream())
        return (B, self.Tq, self.Tk, H, self.d, *ld, self.scale, L.dt(self.q), L.stream())

    def _extra(self):
        if self.tab is not None:
            return "rope_", (self.tab.data_ptr(),)
        if self.bias is not None:
            return "bias_", (self.bias.data_ptr(),)
        return "", ()

    def nan(self, rows, cols=None, dtype=None):
        shape = (rows + TAIL,) if cols is None else (rows + TAIL, cols)
        return torch.full(shape, float("nan"), dtype=dtype or self.dtype, device="cuda")

    def forward(self):
        """-> o [B*Tq, D] and lse [B*H*Tq] (views of buffers with TAIL sentinel rows / floats behind them)"""
        from uwudiff_amd import lib as L

        n = B * self.Tq
        o, lse = self.nan(n, self.D), self.nan(H * n, dtype=F32)
        kind, extra = self._extra()
        L.call(f"uwu_attention_{kind}fwd", self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), *extra, o.data_ptr(), lse.data_ptr(),
               *self._dims())
        torch.cuda.synchronize()
        for name, t, m in (("o", o, n), ("lse", lse, H * n)):
            assert bool(torch.isfinite(t[:m].float()).all()), f"{name} not finite"
            assert bool(torch.isnan(t[m:].float()).all()), f"the forward wrote behind {name}"
        return o[:n], lse[:H * n]

    def backward(self, o, lse):
        """-> dq, dk, dv (flat, with the row strides of q, k, v) and delta [B*H*Tq] (NaN where the route does not write it)"""
        from uwudiff_amd import lib as L

        nq, nk, D = B * self.Tq, B * self.Tk, self.D
        delta = self.nan(H * nq, dtype=F32)
        if self.packed:
            g = self.nan(nq, 3 * D)
            dq, dk, dv = g[:nq, :D], g[:nq, D:2 * D], g[:nq, 2 * D:]
            tails = [g[nq:]]
        else:
            fulls = [self.nan(n, D) for n in (nq, nk, nk)]
            dq, dk, dv = (f[:n] for f, n in zip(fulls, (nq, nk, nk)))
            tails = [f[n:] for f, n in zip(fulls, (nq, nk, nk))]
        assert (dq.stride(0), dk.stride(0), dv.stride(0)) == (self.q.stride(0), self.k.stride(0), self.v.stride(0))
        kind, extra = self._extra()
        dl = () if kind == "rope_" else (delta.data_ptr(),)
        L.call(f"uwu_attention_{kind}bwd", self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), *extra, o.data_ptr(),
               self.do.data_ptr(), lse.data_ptr(), *dl, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), *self._dims())
        torch.cuda.synchronize()
        for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert bool(torch.isfinite(t.float()).all()), f"{name} not finite"
        for t in tails + [delta[H * nq:]]:
            assert bool(torch.isnan(t.float()).all()), "the backward wrote behind an output"
        body = delta[:H * nq]
        wrote = bool(torch.isfinite(body).all())
        assert wrote or bool(torch.isnan(body).all()), "delta partly written"
        return dict(dq=dq, dk=dk, dv=dv, delta=body if wrote else None)

    def to_heads(self, out):
        """device results -> CPU [B, H, T, d] / [B, H, Tq]"""
        res = {}
        for name, t in out.items():
            if t is None:
                continue
            if name in ("lse", "delta"):
                res[name] = t.cpu().view(B, H, self.Tq)
            else:
                res[name] = O.heads(t.cpu(), B, self.Tq if name in ("o", "dq") else self.Tk, H, self.d).contiguous()
        return res


def _assert_route(p, mfma):
    from uwudiff_amd import ops

    if p.tab is not None:
        return  # the rope entry points have one kernel each
    ld = (p.q.stride(0), p.k.stride(0), p.v.stride(0), p.D)
    for backward in (False, True):
        assert ops.attention_route(p.Tq, p.Tk, p.d, *ld, dtype=p.dtype, backward=backward) is mfma, ("backward" if backward else "forward")


# ------------------------------------------------------------------------------------------------------------------ bars
class Bars:
    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, name, got, ref, yard, bf16_out=False):
        finite = bool(torch.isfinite(got.float()).all())
        e, r = O.ratio(got, ref, yard, bf16_out=bf16_out)
        self.rows.append((name, e, r if finite else float("inf")))

    def add_rows(self, name, got, ref, yard, special, bf16_out=False):
        """special: bool [B, T] or None -- the special rows of the degenerate class and the rest, each against their own E and A"""
        if special is None:
            return self.add(name, got, ref, yard, bf16_out)
        m = special[:, None, :].expand(got.shape[:3])
        self.add(name, got[~m], ref[~m], yard[~m], bf16_out)
        self.add(name + "[0]", got[m], ref[m], yard[m], bf16_out)

    def done(self):
        print(f"[attn-acc] {self.label:<64s} " + "  ".join(f"{n}={r:.2f}(E {e:.1e})" for n, e, r in self.rows))
        bad = [(n, r) for n, _, r in self.rows if not r <= MARGIN]
        assert not bad, f"{self.label}: ratio to max(E, 2^-23 A) above {MARGIN}: {bad}"


def _special(cls, Tq, Tk):
    if cls != "degenerate":
        return None, None
    r = O.special_rows(B, Tq, Tk)
    sq, sk = torch.zeros(B, Tq, dtype=torch.bool), torch.zeros(B, Tk, dtype=torch.bool)
    for b in range(B):
        sq[b, r["zq"][b]] = sq[b, r["zdo"][b]] = True
        sk[b, r["zk"][b]] = sk[b, r["dup"][b]] = sk[b, r["src"][b]] = True
    return sq, sk


def _rope_table(T, d):
    """fp32 [T, H*d], factors in [-1.5, 1.5]"""
    g = torch.Generator().manual_seed(31 * T + d)
    return torch.rand(T, H * d, generator=g) * 3.0 - 1.5


def check(label, d, Tq, Tk, dtype, cls, bias_cls, *, mfma, rope=False, packed=False):
    q, k, v, do = O.hard_inputs(cls, B, H, Tq, Tk, d, dtype)
    bias = O.hard_bias(bias_cls, B, Tk) if bias_cls else None
    tab = _rope_table(Tq, d) if rope else None
    p = Problem(q, k, v, do, d, Tq, Tk, bias=bias, tab=tab, packed=packed)
    _assert_route(p, mfma)
    if rope:  # the contract: rotate, round, then plain attention
        th = tab.view(Tq, H, d).transpose(0, 1)
        q, k = O.rope(q, th), O.rope(k, th)
    bf = dtype == BF
    sq, sk = _special(cls, Tq, Tk)
    bars = Bars(label)
    ev = lambda dt, rp, **kw: O.evaluate(q, k, v, do, bias=bias, scale=p.scale, dtype=dt, round_p=rp, **kw)  # noqa: E731

    # forward
    o_dev, lse_dev = p.forward()
    fwd = p.to_heads(dict(o=o_dev, lse=lse_dev))
    ref, yard = ev(F64, False), ev(F32, mfma)
    bars.add_rows("o", fwd["o"], ref["o"], yard["o"], sq, bf16_out=bf)
    bars.add_rows("lse", fwd["lse"][..., None], ref["lse"][..., None], yard["lse"][..., None], sq)
    if bias_cls == "all_but_one":
        vis = O.visible_key(B, Tk)
        for b in range(B):
            assert torch.equal(fwd["o"][b], v[b, :, vis[b]][:, None, :].expand(H, Tq, d)), "o is not the visible key's v row"

    # backward, twice: the forward kernel's own o and lse; fp64 o and lse rounded to the dtypes
    first = None
    for tag, o_in, lse_in in (("", o_dev, lse_dev), ("@64", _poisoned(O.flat(ref["o"]).to(dtype)), _poisoned(ref["lse"].float().reshape(-1)))):
        out = p.backward(o_in, lse_in)
        first = first or out
        got = p.to_heads(out)
        handed = p.to_heads(dict(o=o_in, lse=lse_in))
        rb, yb = ev(F64, False, **handed), ev(F32, mfma, **handed)
        for name, sp in (("dq", sq), ("dk", sk), ("dv", sk)):
            bars.add_rows(name + tag, got[name], rb[name], yb[name], sp, bf16_out=bf)
        if "delta" in got:
            bars.add_rows("delta" + tag, got["delta"][..., None], rb["delta"][..., None], yb["delta"][..., None], sq)
        if cls == "degenerate":
            zdo = O.special_rows(B, Tq, Tk)["zdo"]
            for b in range(B):
                assert bool((got["dq"][b, :, zdo[b]] == 0).all()), "dq of an all-zero dO row is not zero"

    # two runs, the same bits
    o2, lse2 = p.forward()
    assert torch.equal(o2, o_dev) and torch.equal(lse2, lse_dev), "two forward runs differ"
    again = p.backward(o_dev, lse_dev)
    for name in ("dq", "dk", "dv"):
        assert torch.equal(again[name], first[name]), f"two backward runs differ in {name}"
    bars.done()


# ----------------------------------------------------------------------------------------------------------------- cases
def C(name, d, Tq, Tk, dtype=BF, *, bias=False, mfma=True, env=None, rope=False, falling=False):
    return dict(name=name, d=d, Tq=Tq, Tk=Tk, dtype=dtype, bias=bias, mfma=mfma, env=env or {}, rope=rope, falling=falling)


MFMA_D = (40, 64, 72, 80, 128)
QTAIL_D = (40, 64, 80)
CASES = []
for _bias in (False, True):
    for _d in MFMA_D:
        # attn_fwd_mfma on whole query tiles; backward: d = 64 without bias -> the one-kernel form (DQ), otherwise the key-block + dQ
        # kernels (d = 80: the lean form, delta from the dQ pass)
        CASES += [
            C("mfma self192", _d, 192, 192, bias=_bias, falling=_d == 64 and not _bias),  # three key tiles: both LDS stages reused
            C("mfma cross128x77", _d, 128, 77, bias=_bias, falling=_d == 128 and not _bias),  # a ragged last key tile
            C("mfma cross192x300", _d, 192, 300, bias=_bias, falling=_d == 72 and not _bias),  # two key blocks, the second with 44 keys
            C("mfma self320", _d, 320, 320, bias=_bias, falling=_d == 80 and not _bias),  # T > 256: two-kernel at every d
        ]
    for _d in QTAIL_D:  # the QTAIL forward and two-kernel backward
        CASES += [
            C("qtail self321", _d, 321, 321, bias=_bias, falling=_d == 40 and not _bias),
            C("qtail self449", _d, 449, 449, bias=_bias),  # two key blocks, the second ragged
            C("qtail cross300x77", _d, 300, 77, bias=_bias),
        ]
CASES += [C("mfma self64", 64, 64, 64, falling=False)]  # the one-kernel backward with a single query tile
for _d in (64, 72):  # T = 256: the persistent kernels of attention_p256.hip and the kernels they replace
    CASES += [
        C("t256 default", _d, 256, 256),  # forward: attn_fwd_mfma (fewer than 1024 heads); backward: attn_bwd_p256
        C("t256 p256f", _d, 256, 256, env={"UWU_ATTN_P256F": "1"}, falling=_d == 64),  # forward: attn_fwd_p256
        C("t256 perhead", _d, 256, 256, env={"UWU_ATTN_P256": "0", "UWU_ATTN_P256_D72": "0"}),  # backward: 64 one-kernel, 72 two-kernel
    ]
for _d in (32, 40, 64, 72, 80, 160):  # the generic kernels, fp32
    CASES += [C("generic 100x40", _d, 100, 40, F32, mfma=False, falling=_d == 32),
              C("generic 64x13", _d, 64, 13, F32, mfma=False)]
CASES += [C("generic 100x40", 32, 100, 40, mfma=False), C("generic 100x40", 160, 100, 40, mfma=False, falling=True),
          C("generic 64x13", 32, 64, 13, mfma=False),
          C("generic 100x40", 72, 100, 40, mfma=False)]  # bf16; d = 72 has no QTAIL kernel: a ragged query count stays here
CASES += [C("rope self64", 64, 64, 64, rope=True), C("rope self192", 64, 192, 192, rope=True, falling=True)]


def _params():
    out = []
    for c in CASES:
        if c["bias"]:
            pairs = [("plain", b) for b in O.BIAS_CLASSES] + [("offset", "random40")]
        else:
            pairs = [(cls, None) for cls in O.CLASSES + (("falling",) if c["falling"] else ())]
        env = "".join(f" {k[9:].lower()}={v}" for k, v in c["env"].items())
        for i, (cls, bias_cls) in enumerate(pairs):
            label = f"{c['name']} d{c['d']} {NAME[c['dtype']]}{env} {cls}" + (f" bias={bias_cls}" if bias_cls else "")
            packed = c["Tq"] == c["Tk"] and i % 2 == 1  # self-attention: packed qkv views and separate tensors in turn
            out.append(pytest.param(c, cls, bias_cls, packed, label + (" packed" if packed else ""), id=label.replace(" ", "-")))
    return out


@pytest.mark.parametrize("case,cls,bias_cls,packed,label", _params())
def test_accuracy(case, cls, bias_cls, packed, label, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    check(label, case["d"], case["Tq"], case["Tk"], case["dtype"], cls, bias_cls, mfma=case["mfma"], rope=case["rope"], packed=packed)


# ---------------------------------------------------------------------------------------------------------- exact routing
# (d, Tq, Tk), dtype, env: every route; fp32 has no kernel at d = 128
ROUTING = []
for _shape in ((40, 321, 321), (64, 256, 256), (72, 300, 77), (80, 449, 449), (128, 64, 200), (160, 100, 40), (32, 64, 13)):
    ROUTING.append((_shape, BF, {}))
    if _shape[0] != 128:
        ROUTING.append((_shape, F32, {}))
ROUTING += [((64, 256, 256), BF, {"UWU_ATTN_P256F": "1"}), ((64, 256, 256), BF, {"UWU_ATTN_P256": "0"})]


def _check_routing(r, p, dtype, Tq, Tk, d):
    o_dev, lse_dev = p.forward()
    fwd = p.to_heads(dict(o=o_dev, lse=lse_dev))
    outs = [p.to_heads(p.backward(o_dev, lse_dev)),
            p.to_heads(p.backward(_poisoned(O.flat(r["o"]).to(dtype)), _poisoned(r["lse"].float().reshape(-1))))]
    if dtype == BF:
        assert torch.equal(fwd["o"].float(), r["o"]), "o"
        rel = ((fwd["lse"].double() - r["lse"]).abs() / r["lse"].abs()).max().item()
        print(f"[attn-route] d{d} {Tq}x{Tk} lse rel err {rel:.3e} (2^-22 = {2.0 ** -22:.3e})")
        assert rel <= 2.0 ** -22, ("lse", rel)
        for out in outs:
            assert torch.equal(out["dv"].float(), r["dv"]), "dv"
            assert bool((out["dq"] == 0).all()) and bool((out["dk"] == 0).all()), "dq / dk"
    else:  # P is not rounded here and may differ from 1 by about 1e-4; the smallest indexing error is 1
        tol = 2.0 ** -10
        assert bool(((fwd["o"] - r["o"]).abs() <= tol * r["o"].abs().clamp_min(1)).all()), "o"
        # the generic kernels sum d / 2 + 2 rounded terms of one sign per lane: (d / 2 + 2) half-ulps at the worst
        rel = ((fwd["lse"].double() - r["lse"]).abs() / r["lse"].abs()).max().item()
        print(f"[attn-route] d{d} {Tq}x{Tk} fp32 lse rel err {rel:.3e}")
        assert rel <= (d / 2 + 2) * 2.0 ** -24, ("lse", rel)
        for out in outs:
            assert bool(((out["dv"] - r["dv"]).abs() <= tol * r["dv"].abs().clamp_min(1)).all()), "dv"
            assert bool((out["dq"].abs() <= tol).all()) and bool((out["dk"].abs() <= tol).all()), "dq / dk"


@pytest.mark.parametrize("biased", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape,dtype,env", ROUTING,
                         ids=[f"d{s[0]}-{s[1]}x{s[2]}-{NAME[t]}" + "".join(f"-{k[9:].lower()}={v}" for k, v in e.items()) for s, t, e in ROUTING])
def test_exact_routing(shape, dtype, env, biased, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d, Tq, Tk = shape
    r = O.routing_inputs(B, H, Tq, Tk, d, biased)
    packed = Tq == Tk and not biased
    p = Problem(*(r[n].to(dtype) for n in ("q", "k", "v", "do")), d, Tq, Tk, bias=r["bias"], packed=packed)
    _assert_route(p, dtype == BF and d in MFMA_D and (Tq % 64 == 0 or (Tq > 256 and d in QTAIL_D)))
    _check_routing(r, p, dtype, Tq, Tk, d)


@pytest.mark.parametrize("T", [64, 256])
def test_exact_routing_rope(T):
    """The rope entry points: the table holds +-{1/2, 1, 2}, the stored q and k are the wanted ones divided by it -- both exact."""
    d = 64
    r = O.routing_inputs(B, H, T, T, d, False)
    g = torch.Generator().manual_seed(T)
    tab = (2.0 ** torch.randint(-1, 2, (T, H * d), generator=g)) * (2.0 * torch.randint(0, 2, (T, H * d), generator=g) - 1.0)
    th = tab.view(T, H, d).transpose(0, 1)[None]
    q, k = r["q"] / th, r["k"] / th
    assert torch.equal(O.rope(q.to(BF), th[0]).float(), r["q"]) and torch.equal(O.rope(k.to(BF), th[0]).float(), r["k"])
    p = Problem(q.to(BF), k.to(BF), r["v"].to(BF), r["do"].to(BF), d, T, T, tab=tab, packed=True)
    _check_routing(r, p, BF, T, T, d)
