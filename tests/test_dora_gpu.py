"""GPU: weight decomposition (DoRA) of the LyCORIS adapters -- uwu_adapter_dora_norms / _merge / _grad against the fp64
restatement of tests/test_dora_cpu.py (both orientations, degenerate rows and columns, in place, refusals), and the UNet
with decomposed adapters against the CPU oracle fed W', the fresh network, merge_to, gradient checkpointing and the fit
loop (AdamW, Prodigy, resume).  The model helpers are copies of tests/test_lycoris_gpu.py's."""
import math
import os

import pytest
import torch

from tests.conftest import ROOT
from tests.test_dora_cpu import DORA_TOML, EPS, TOML, dora_weight

pytestmark = pytest.mark.gpu

TINY = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
            down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
            transformer_layers_per_block=(1, 2), attention_head_dim=(1, 1), cross_attention_dim=32,
            addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48,
            norm_num_groups=8)
SDXL_W = dict(TINY, block_out_channels=(320, 640), attention_head_dim=(5, 10), transformer_layers_per_block=(1, 1),
              cross_attention_dim=2048, norm_num_groups=32)
LOWRANK = {"config": {"algo": "lokr", "linear_dim": 2, "linear_alpha": 3, "factor": 4, "train_norm": True},
           "preset": {"target_module": ["Transformer2DModel"], "module_algo_map": {"FeedForward": {"algo": "lora", "linear_dim": 3}}}}
LOWRANK_DORA = {"config": dict(LOWRANK["config"], dora_wd=True, wd_on_out=False), "preset": LOWRANK["preset"]}
KINDS = {1: "lora", 2: "lokr", 3: "lokr_lowrank"}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def pad64(n):
    return (n + 63) // 64 * 64


def fbits(x):
    return int.from_bytes(torch.tensor([x], dtype=torch.float32).numpy().tobytes(), "little")


# ------------------------------------------------------------------------------------------------------------ kernels
# (kind, rows, cols, r, out_k, in_n): the shapes of the issue -- rows that straddle the merge's 4096-element workgroups with
# a width that is no multiple of 4, a row longer than one workgroup, a column over many row tiles, both LoKr forms, one row
SHAPES = [(1, 96, 300, 4, 0, 0), (1, 5, 5120, 1, 0, 0), (1, 2050, 33, 2, 0, 0), (2, 640, 2048, 0, 64, 64),
          (3, 39, 77, 2, 13, 11), (1, 1, 64, 3, 0, 0)]
SCALE = {1: 0.5, 2: 1.0, 3: 0.75}


def _factor_shapes(kind, R, C, r, out_k, in_n):
    if kind == 1:
        return [(R, r), (r, C)]
    if kind == 2:
        return [(R // out_k, C // in_n), (out_k, in_n)]
    return [(R // out_k, C // in_n), (out_k, r), (r, in_n)]


class _Seg:
    """one decomposed segment: its factors and magnitudes in p, its base values, its slots in norms"""

    def __init__(self, st, kind, R, C, r, out_k, in_n, by_row, g, zero=None):
        self.kind, self.R, self.C, self.r, self.out_k, self.in_n, self.by_row = kind, R, C, r, out_k, in_n, by_row
        self.shapes = _factor_shapes(kind, R, C, r, out_k, in_n)
        self.leaves = [torch.randn(s, generator=g) * 0.3 for s in self.shapes]
        self.base = torch.randn(R, C, generator=g)
        if zero is not None:  # (LoRA) an exactly zero row and an exactly zero column of base AND delta
            zr, zc = zero
            self.base[zr] = 0
            self.base[:, zc] = 0
            self.leaves[0][zr] = 0
            self.leaves[1][:, zc] = 0
        self.m = (1 + 0.1 * torch.randn((R, 1) if by_row else (1, C), generator=g)) * self.base.norm(
            dim=1 if by_row else 0, keepdim=True)
        if zero is not None:
            self.m[zero[0] if by_row else 0, 0 if by_row else zero[1]] = 1.5  # finite: the output is 0 * 1.5 / eps
        self.offs = []
        for t in self.leaves + [self.m]:
            self.offs.append(st["p"])
            st["p"] += pad64(t.numel())
        self.boff = st["base"]
        st["base"] += pad64(R * C)
        self.noff = st["norms"]
        st["norms"] += pad64(R if by_row else C)

    def row(self, eoff, soff):
        pa, pb, pc = (self.offs[:-1] + [0, 0])[:3]  # (LoRA: up, down)
        return [self.kind, self.R, self.C, self.boff, eoff, soff, pa, pb, pc, self.r, self.out_k, self.in_n,
                fbits(SCALE[self.kind]), self.offs[-1], self.noff, int(self.by_row)]

    def want(self, m=None):
        return dora_weight(self.base.double(), KINDS[self.kind], [t.double() for t in self.leaves], SCALE[self.kind],
                           (self.m if m is None else m).double(), self.by_row)

    def fill(self, p, base):
        for o, t in zip(self.offs, self.leaves + [self.m]):
            p[o:o + t.numel()] = t.reshape(-1)
        base[self.boff:self.boff + self.R * self.C] = self.base.reshape(-1)


def _tables(segs, eff_of=lambda s: s.boff, shadow=True):
    rows, nblk, mblk = [], [0], [0]
    for s in segs:
        rows.append(s.row(eff_of(s), s.boff if shadow else -1))
        nblk.append(nblk[-1] + (-(-s.R // 4) if s.by_row else -(-s.C // 64)))
        mblk.append(mblk[-1] + -(-(s.R * s.C) // 4096))
    host = torch.tensor(rows, dtype=torch.int64)
    return host.cuda(), host, torch.tensor(nblk).cuda(), nblk[-1], torch.tensor(mblk).cuda(), mblk[-1], len(rows)


def _dora_merge(tabs, base, p, norms, eff, shadow):
    from uwudiff_amd import lib as L

    t, host, nblk, nnb, mblk, nmb, nseg = tabs
    L.call("uwu_adapter_dora_norms", L.ptr(base), L.ptr(p), L.ptr(t), host.data_ptr(), L.ptr(nblk), nseg, nnb, L.ptr(norms),
           L.stream())
    L.call("uwu_adapter_dora_merge", L.ptr(base), L.ptr(p), L.ptr(t), host.data_ptr(), L.ptr(mblk), nseg, nmb, L.ptr(norms),
           L.ptr(eff), L.ptr(shadow), L.stream())
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def merge_case():
    """every shape in both orientations + the degenerate segment, between two plain (undecomposed) neighbours"""
    g = torch.Generator().manual_seed(11)
    st = {"p": 0, "base": 0, "norms": 0}
    # the plain neighbours: LoRA [130, 200] r = 4 in front, a norm vector [640] behind (13-field rows of uwu_adapter_merge)
    plain = []

    def plain_seg(kind, R, C):
        shapes = [(R, 4), (4, C)] if kind == 1 else [(R * C,)]
        leaves = [torch.randn(s, generator=g) for s in shapes]
        offs = []
        for t in leaves:
            offs.append(st["p"])
            st["p"] += pad64(t.numel())
        base = torch.randn(R, C, generator=g)
        boff = st["base"]
        st["base"] += pad64(R * C)
        plain.append((kind, R, C, boff, leaves, offs, base))

    plain_seg(1, 130, 200)
    segs = [_Seg(st, *sh, by_row, g) for sh in SHAPES for by_row in (True, False)]
    segs += [_Seg(st, 1, 8, 12, 2, 0, 0, by_row, g, zero=(3, 5)) for by_row in (True, False)]
    plain_seg(0, 1, 640)
    p, base = torch.zeros(st["p"]), torch.zeros(st["base"])
    for s in segs:
        s.fill(p, base)
    prow, pblk, pwant = [], [0], []
    for kind, R, C, boff, leaves, offs, b in plain:
        for o, t in zip(offs, leaves):
            p[o:o + t.numel()] = t.reshape(-1)
        base[boff:boff + R * C] = b.reshape(-1)
        d = 0.5 * leaves[0].double() @ leaves[1].double() if kind == 1 else leaves[0].double().view(R, C)
        pwant.append(b.double() + d)
        prow.append([kind, R, C, boff, boff, boff, offs[0], offs[1] if kind == 1 else 0, 0, 4 if kind == 1 else 0, 0, 0,
                     fbits(0.5 if kind == 1 else 1.0)])
        pblk.append(pblk[-1] + -(-(R * C) // 4096))
    ptab = (torch.tensor(prow, dtype=torch.int64).cuda(), torch.tensor(pblk).cuda(), len(prow), pblk[-1])
    return dict(segs=segs, plain=plain, pwant=pwant, ptab=ptab, p=p.cuda(), base=base.cuda(), st=st,
                want=[s.want() for s in segs])


def _three_launches(c, eff, shadow, base=None):
    from uwudiff_amd import lib as L

    base = c["base"] if base is None else base
    t, blk, nseg, nb = c["ptab"]
    L.call("uwu_adapter_merge", L.ptr(base), L.ptr(c["p"]), L.ptr(t), L.ptr(blk), nseg, nb, L.ptr(eff), L.ptr(shadow),
           L.stream())
    norms = torch.full((c["st"]["norms"],), float("nan"), device="cuda")
    _dora_merge(_tables(c["segs"]), base, c["p"], norms, eff, shadow)
    return norms


def test_dora_norms_and_merge_match_fp64(merge_case):
    from uwudiff_amd import lib as L

    c = merge_case
    n = c["st"]["base"]
    eff = torch.full((n,), float("nan"), device="cuda")
    sh16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    norms = _three_launches(c, eff, sh16)
    covered = torch.zeros(n, dtype=torch.bool)
    worst = 0.0
    for s, w in zip(c["segs"], c["want"]):
        got = eff[s.boff:s.boff + s.R * s.C].cpu().view(s.R, s.C)
        assert torch.isfinite(got).all(), (s.kind, s.R, s.C, s.by_row)
        err = float((got.double() - w).abs().max() / w.abs().max())
        worst = max(worst, err)
        print(f"dora merge kind {s.kind} {s.R}x{s.C} by_row={s.by_row}: {err:.3e}")
        assert err < 1e-6, (s.kind, s.R, s.C, s.by_row, err)
        cast = torch.empty(s.R * s.C, dtype=torch.bfloat16, device="cuda")
        L.call("uwu_cast_f32_to_bf16", L.ptr(eff[s.boff:s.boff + s.R * s.C].contiguous()), L.ptr(cast), s.R * s.C, L.stream())
        assert torch.equal(sh16[s.boff:s.boff + s.R * s.C], cast), (s.kind, s.R, s.C, s.by_row)
        covered[s.boff:s.boff + s.R * s.C] = True
        # the norms the backward divides by: ||V|| + eps
        V = dora_weight(s.base.double(), KINDS[s.kind], [t.double() for t in s.leaves], SCALE[s.kind], None, s.by_row)
        nw = V.norm(dim=1 if s.by_row else 0) + EPS
        ng = norms[s.noff:s.noff + nw.numel()].cpu().double()
        assert float(((ng - nw).abs() / nw).max()) < 1e-6
    print(f"dora merge worst: {worst:.3e}")
    # the degenerate segment: n = eps, exactly 0 out
    zr, zc = c["segs"][-2], c["segs"][-1]
    assert zr.by_row and not zc.by_row
    assert float(norms[zr.noff + 3]) == EPS and float(norms[zc.noff + 5]) == EPS
    assert not eff[zr.boff:zr.boff + 96].view(8, 12)[3].any() and not eff[zc.boff:zc.boff + 96].view(8, 12)[:, 5].any()
    # the plain neighbours are the plain merge's, everything else keeps the NaN fill
    for (kind, R, C, boff, *_), w in zip(c["plain"], c["pwant"]):
        got = eff[boff:boff + R * C].cpu().view(R, C)
        assert float((got.double() - w).abs().max() / w.abs().max()) < 1e-6
        covered[boff:boff + R * C] = True
    assert torch.isnan(eff.cpu()[~covered]).all() and not torch.isnan(eff.cpu()[covered]).any()
    assert not sh16.cpu()[~covered].any()
    # again: bit-identical
    eff2 = torch.full((n,), float("nan"), device="cuda")
    sh2 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    norms2 = _three_launches(c, eff2, sh2)
    assert torch.equal(eff2.nan_to_num(7.0), eff.nan_to_num(7.0)) and torch.equal(sh2, sh16)
    assert torch.equal(norms2.nan_to_num(7.0), norms.nan_to_num(7.0))
    # in place (eff aliasing base, no shadow): the same fp32 values, the padding of base untouched
    folded = c["base"].clone()
    t, blk, nseg, nb = c["ptab"]
    L.call("uwu_adapter_merge", L.ptr(folded), L.ptr(c["p"]), L.ptr(t), L.ptr(blk), nseg, nb, L.ptr(folded), None, L.stream())
    norms3 = torch.empty_like(norms)
    _dora_merge(_tables(c["segs"], shadow=False), folded, c["p"], norms3, folded, None)
    cov = covered.cuda()
    assert torch.equal(folded[cov], eff[cov]) and torch.equal(folded[~cov], c["base"][~cov])


def _grad_chain(s, G, g0, p, base):
    """norms, then uwu_adapter_dora_grad and uwu_adapter_grad on one segment; returns (g, G after)"""
    from uwudiff_amd import lib as L
    from uwudiff_amd.adapters import Spec, dora_grad_ws_elems, grad_ws_elems

    N, K = s.R, s.C
    sp = Spec.__new__(Spec)
    sp.algo, sp.r, sp.out_k, sp.in_n, sp.wd_on_out = ("lora" if s.kind == 1 else "lokr"), s.r, s.out_k, s.in_n, s.by_row
    norms = torch.full((pad64(max(N, K)),), float("nan"), device="cuda")
    t, host, nblk, nnb, _, _, nseg = _tables([s], shadow=False)
    L.call("uwu_adapter_dora_norms", L.ptr(base), L.ptr(p), L.ptr(t), host.data_ptr(), L.ptr(nblk), nseg, nnb,
           L.ptr(norms), L.stream())
    row = s.row(-1, -1)
    pa, pb, pc = row[6:9]
    Gd, g = G.cuda(), g0.cuda()
    dws = torch.empty(max(dora_grad_ws_elems(sp, N, K), 2), device="cuda")
    ws = torch.empty(max(grad_ws_elems(sp, N, K), 1), device="cuda")
    L.call("uwu_adapter_dora_grad", L.ptr(Gd), L.ptr(base[s.boff:]), N, K, s.kind, L.ptr(p), L.ptr(g), pa, pb, pc, s.r,
           s.out_k, s.in_n, SCALE[s.kind], s.offs[-1], L.ptr(norms), int(s.by_row), L.ptr(dws), dws.numel(), L.stream())
    L.call("uwu_adapter_grad", L.ptr(Gd), N, K, s.kind, L.ptr(p), L.ptr(g), pa, pb, pc, s.r, s.out_k, s.in_n, SCALE[s.kind],
           L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return g.cpu(), Gd.cpu()


@pytest.mark.parametrize("by_row", [True, False], ids=["rows", "cols"])
@pytest.mark.parametrize("shape", SHAPES + [(1, 8, 12, 2, 0, 0)], ids=lambda s: f"k{s[0]}_{s[1]}x{s[2]}")
def test_dora_grad_chain_matches_fp64_autograd(shape, by_row):
    g = torch.Generator().manual_seed(21)
    st = {"p": 0, "base": 0, "norms": 0}
    zero = (3, 5) if shape[1:3] == (8, 12) else None  # the case whose second term is 0: a zero row (rows) / column (cols)
    s = _Seg(st, *shape, by_row, g, zero=zero)
    p, base = torch.zeros(st["p"]), torch.zeros(st["base"])
    s.fill(p, base)
    G = torch.randn(s.R, s.C, generator=g)
    g0 = torch.randn(st["p"], generator=g)  # the chain ADDS to what is there
    got, dV = _grad_chain(s, G, g0, p.cuda(), base.cuda())
    # fp64 autograd of sum(G * W') with respect to every leaf, dora_scale included, and to V (a zero added to the base)
    leaves = [t.double().requires_grad_(True) for t in s.leaves]
    m = s.m.double().requires_grad_(True)
    Z = torch.zeros(s.R, s.C, dtype=torch.float64, requires_grad=True)
    W = dora_weight(s.base.double() + Z, KINDS[s.kind], leaves, SCALE[s.kind], m, by_row)
    (G.double() * W).sum().backward()
    for o, t, name in zip(s.offs, leaves + [m], [f"factor{i}" for i in range(len(leaves))] + ["dora_scale"]):
        d = got[o:o + t.numel()].double() - g0[o:o + t.numel()].double()
        e = rel(d, t.grad.reshape(-1))
        # the kernels add in fp32 to what g holds: where the gradient is far smaller than g0 (the single-row column case:
        # 1e-5 against 1) the sum's own rounding, half an ulp of g, is the floor of what can be read back
        floor = 2.0 ** -24 * float(got[o:o + t.numel()].double().norm() / t.grad.norm())
        print(f"dora grad kind {s.kind} {s.R}x{s.C} by_row={by_row} {name}: {e:.3e} (accumulation floor {floor:.1e})")
        assert e < 1e-5 + floor, (name, e)
    e = rel(dV, Z.grad)
    print(f"dora grad kind {s.kind} {s.R}x{s.C} by_row={by_row} dV: {e:.3e}")
    assert e < 1e-5
    # nothing else in g moved
    mask = torch.ones(st["p"], dtype=torch.bool)
    for o, t in zip(s.offs, leaves + [m]):
        mask[o:o + t.numel()] = False
    assert torch.equal(got[mask], g0[mask])
    got2, dV2 = _grad_chain(s, G, g0, p.cuda(), base.cuda())
    assert torch.equal(got, got2) and torch.equal(dV, dV2)  # fixed-order sums: bit-identical


def test_dora_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L

    g = torch.Generator().manual_seed(2)
    st = {"p": 0, "base": 0, "norms": 0}
    s = _Seg(st, 1, 16, 64, 4, 0, 0, True, g)
    p, base = torch.zeros(st["p"]), torch.zeros(st["base"])
    s.fill(p, base)
    p, base = p.cuda(), base.cuda()
    norms = torch.full((64,), -1.0, device="cuda")
    eff = torch.full((st["base"],), -1.0, device="cuda")
    good = s.row(s.boff, -1)

    def merge_side(name, row, null=None):
        host = torch.tensor([row], dtype=torch.int64)
        dev = host.cuda()
        nblk = torch.tensor([0, 4]).cuda()
        mblk = torch.tensor([0, 1]).cuda()
        a = dict(base=L.ptr(base), p=L.ptr(p), table=L.ptr(dev), host=host.data_ptr(), norms=L.ptr(norms))
        if null:
            a[null] = None
        if name == "uwu_adapter_dora_norms":
            L.call(name, a["base"], a["p"], a["table"], a["host"], L.ptr(nblk), 1, 4, a["norms"], L.stream())
        else:
            L.call(name, a["base"], a["p"], a["table"], a["host"], L.ptr(mblk), 1, 1, a["norms"], L.ptr(eff), None, L.stream())

    bad_rank = list(good)
    bad_rank[9] = 129
    misaligned = list(good)
    misaligned[3] = 32
    for name in ("uwu_adapter_dora_norms", "uwu_adapter_dora_merge"):
        short = name[4:]
        with pytest.raises(L.UwuError, match=short + ".*rank"):
            merge_side(name, bad_rank)
        with pytest.raises(L.UwuError, match=short + ".*misaligned"):
            merge_side(name, misaligned)
        for null in ("base", "p", "table", "host", "norms"):
            with pytest.raises(L.UwuError, match=short):
                merge_side(name, good, null=null)
    G = torch.full((16, 64), 3.0, device="cuda")
    G1 = torch.full((16 * 64 + 4,), 3.0, device="cuda")
    gr = torch.full((st["p"],), -1.0, device="cuda")

    def grad(r=4, dw=None, null=None):
        a = dict(dw=L.ptr(G) if dw is None else dw, base=L.ptr(base), p=L.ptr(p), g=L.ptr(gr), norms=L.ptr(norms))
        if null:
            a[null] = None
        L.call("uwu_adapter_dora_grad", a["dw"], a["base"], 16, 64, 1, a["p"], a["g"], good[6], good[7], 0, r, 0, 0, 0.5,
               good[13], a["norms"], 1, None, 0, L.stream())

    with pytest.raises(L.UwuError, match="adapter_dora_grad.*rank"):
        grad(r=129)
    with pytest.raises(L.UwuError, match="adapter_dora_grad.*misaligned"):
        grad(dw=L.ptr(G1) + 4)
    for null in ("dw", "base", "p", "g", "norms"):
        with pytest.raises(L.UwuError, match="adapter_dora_grad"):
            grad(null=null)
    with pytest.raises(L.UwuError, match="adapter_dora_grad.*workspace"):  # the column orientation needs its workspace
        L.call("uwu_adapter_dora_grad", L.ptr(G), L.ptr(base), 16, 64, 1, L.ptr(p), L.ptr(gr), good[6], good[7], 0, 4, 0, 0,
               0.5, good[13], L.ptr(norms), 0, None, 0, L.stream())
    torch.cuda.synchronize()
    assert (norms == -1).all() and (eff == -1).all() and (G == 3).all() and (G1 == 3).all() and (gr == -1).all()


# ------------------------------------------------------------------------------------------------------------ model
def _models(cfg, dtype, lyc, seed=0, random_adapters=True, values=None):
    from oracle.unet import UNetOracle
    from uwudiff_amd.adapters import LycorisNetwork
    from uwudiff_amd.unet import UNet2DConditionModel

    torch.manual_seed(seed)
    ora = UNetOracle(**cfg)
    with torch.no_grad():
        for n, p in ora.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (0.5 / p[0].numel() ** 0.5))
            elif n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.05)
            else:
                p.copy_(1 + torch.randn_like(p) * 0.1)
    model = UNet2DConditionModel(cfg, compute_dtype=dtype, init_weights=False).cuda()
    model.load_state_dict(ora.state_dict())
    model.requires_grad_(False)
    net = LycorisNetwork(model, lyc).cuda()
    if random_adapters:
        with torch.no_grad():  # adapter values random at 0.1; dora_scale its initial value times (1 + 0.1 randn)
            init = net.flat.data.clone()
            noise = torch.randn(net.n, generator=torch.Generator().manual_seed(seed + 9)).cuda()
            net.flat.data.copy_(noise * 0.1)
            for s in net.specs:
                if s.dora:
                    net.view(s.name, "dora_scale").copy_(net.view(s.name, "dora_scale", buf=init)
                                                         * (1 + net.view(s.name, "dora_scale")))
    if values is not None:  # the adapter values of another network of the same model, tensor by tensor
        mine = net.state_dict()
        net.load_state_dict({k: values[k] for k in mine})
    net.apply_to(model)
    return ora, model, net


def _inputs(cfg, B=2, S=16, Tk=7, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg["in_channels"], S, S, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    ctx = torch.randn(B, Tk, cfg["cross_attention_dim"], generator=g)
    pooled = torch.randn(B, 16, generator=g)
    ids = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B)
    dout = torch.randn(B, cfg["out_channels"], S, S, generator=g) / (S * S)
    return x, t, ctx, pooled, ids, dout


def _run(model, inp, backward=True):
    x, t, ctx, pooled, ids, dout = inp
    y = model(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda(),
              added_cond_kwargs={"text_embeds": pooled.cuda(), "time_ids": ids.cuda()})[0]
    if backward:
        y.backward(dout.cuda())
    torch.cuda.synchronize()
    return y.detach()


def _effective(ora, net, leaves, dtype=torch.float32):
    """W' (or W + dW, or gamma + w_norm) of every adapted tensor from leaf tensors, through the fp64 restatement's rule"""
    params = dict(ora.named_parameters())
    sub = {}
    for s in net.specs:
        L = lambda t: leaves[f"{s.key}.{t}"].to(dtype)
        if s.algo == "norm":
            sub[s.name + ".weight"] = params[s.name + ".weight"].to(dtype) + L("w_norm")
            sub[s.name + ".bias"] = params[s.name + ".bias"].to(dtype) + L("b_norm")
            continue
        if s.algo == "lora":
            kind, fs = "lora", [L("lora_up.weight"), L("lora_down.weight")]
        elif s.lowrank:
            kind, fs = "lokr_lowrank", [L("lokr_w1"), L("lokr_w2_a"), L("lokr_w2_b")]
        else:
            kind, fs = "lokr", [L("lokr_w1"), L("lokr_w2")]
        w = params[s.name + ".weight"]
        sub[s.name + ".weight"] = dora_weight(w.to(dtype).reshape(s.shape), kind, fs, s.scale,
                                              L("dora_scale") if s.dora else None, s.wd_on_out).view(w.shape)
    return sub


def _oracle_adapted(ora, net, inp):
    """the oracle with the effective weights built by torch ops from leaf adapter tensors: output, adapter gradients"""
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()
              if not k.endswith(".alpha")}
    sub = _effective(ora, net, leaves)
    x, t, ctx, pooled, ids, dout = inp
    y = torch.func.functional_call(ora, sub, (x, t), dict(encoder_hidden_states=ctx,
                                                         added_cond_kwargs={"text_embeds": pooled, "time_ids": ids}),
                                   strict=False)[0]
    y.backward(dout)
    return y.detach(), {k: v.grad for k, v in leaves.items()}


def _adapter_grads(net):
    return {f"{s.key}.{t}": net.view(s.name, t, buf=net.flat.grad).cpu() for s in net.specs for t, _ in s.tensors}


def _deviations(cfg, lyc, dtype, values=None):
    ora, model, net = _models(cfg, dtype, lyc, values=values)
    base0 = model.flat.detach().clone()
    inp = _inputs(cfg)
    y = _run(model, inp)
    yo, go = _oracle_adapted(ora, net, inp)
    got = _adapter_grads(net)
    assert set(got) == set(go)
    cat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(go)])
    out = {"y": rel(y, yo), "all": rel(cat(got), cat(go)), "each": {k: rel(got[k], go[k]) for k in go},
           "numel": {k: go[k].numel() for k in go}, "values": net.state_dict()}
    assert model.flat.grad is None and not model.flat.requires_grad
    assert torch.equal(model.flat.detach(), base0)  # the frozen base: bit-identical before and after
    return out


@pytest.mark.parametrize("cfg,lyc", [(TINY, DORA_TOML), (TINY, LOWRANK_DORA), (SDXL_W, DORA_TOML)],
                         ids=["tiny", "tiny_lowrank_cols", "sdxl_width"])
def test_dora_unet_matches_oracle_fp32(cfg, lyc):
    d = _deviations(cfg, lyc, "fp32")
    worst = max(d["each"], key=d["each"].get)
    print(f"dora fp32: y {d['y']:.3e} all {d['all']:.3e} worst {worst} {d['each'][worst]:.3e} "
          f"dora_scale {max(v for k, v in d['each'].items() if k.endswith('dora_scale')):.3e}")
    assert any(k.endswith(".dora_scale") for k in d["each"])
    assert d["y"] < 1e-3
    bad = {k: v for k, v in d["each"].items() if v > 2e-3}
    assert not bad, bad


def test_dora_unet_matches_oracle_bf16():
    """bf16 operands: the decomposed network may deviate from its oracle at most twice as far as the same model, inputs and
    adapter values do without decomposition (the parent's path against its own oracle, run here): the renormalisation
    divides bf16 noise by a norm and must not amplify it."""
    on = _deviations(TINY, DORA_TOML, "bf16")
    off = _deviations(TINY, TOML, "bf16", values=on["values"])
    big = lambda d: {k: v for k, v in d["each"].items() if d["numel"][k] >= 64}
    print(f"bf16 dora: y {on['y']:.3e} all {on['all']:.3e} worst tensor {max(big(on).values()):.3e}")
    print(f"bf16 off:  y {off['y']:.3e} all {off['all']:.3e} worst tensor {max(big(off).values()):.3e}")
    # the off path against the existing bars (tests/test_lycoris_gpu.py): a finding about the parent if it fails
    assert off["y"] < 4e-2 and off["all"] < 4e-2 and max(big(off).values()) < 0.12, off
    assert on["y"] <= 2 * off["y"]
    assert on["all"] <= 2 * off["all"]
    assert max(big(on).values()) <= 2 * max(big(off).values())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fresh_dora_network_and_merge_to(dtype):
    """A fresh decomposed network runs with W u / (u + eps): the base within 1e-6, not bit for bit.

    fp32: the output equals the bare UNet's within the floor logic of test_fresh_adapters_leave_output_unchanged
    (tests/test_lycoris_gpu.py).  bf16: that test's 1e-3 floor rests on the merged shadow being the re-cast base bit for
    bit, which the rule excludes: a weight whose fp32 value lies within eps / u of a bf16 rounding boundary rounds to the
    other neighbour (a fraction <= 2.4e-7 / 2^-8 = 6e-5 of them at u >= 0.5), and one flipped weight flips bf16 roundings
    of activations downstream.  Measured on this model: rel 1.0e-2 between the fresh decomposed and the bare output, two bare
    runs 0.0, the bare bf16 output against the fp32 oracle 1.2e-2.  So in bf16 the sharp check is on the shadow (each element
    the bf16 rounding of a value within 1e-6 of the base, all but 1e-3 of them the re-cast base itself), and the output may
    differ from the bare one by what bf16 arithmetic itself differs from the oracle: twice the bare output's own error."""
    ora, model, net = _models(TINY, dtype, DORA_TOML, random_adapters=False)
    inp = _inputs(TINY)
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        assert model.P.ad.dora
        flipped = total = 0
        for nm in model.P.ad.dora:
            b = model.P.base32(nm)
            if nm in model.P.ad.eff_off:
                assert float((model.P.w32(nm) - b).abs().max() / b.abs().max()) < 1e-6, nm
            if dtype == "bf16":
                w = model.P.w(nm).float()
                lo, hi = (b * (1 - 1e-6)).bfloat16().float(), (b * (1 + 1e-6)).bfloat16().float()
                assert bool(((w >= torch.minimum(lo, hi)) & (w <= torch.maximum(lo, hi))).all()), nm
                flipped += int((w != b.bfloat16().float()).sum())
                total += w.numel()
        if dtype == "fp32":
            assert all(nm in model.P.ad.eff_off for nm in model.P.ad.dora)
        else:
            print(f"fresh bf16: {flipped} of {total} shadow elements are not the re-cast base")
            assert flipped <= 1e-3 * total
        net.restore()
        y_bare = _run(model, inp, backward=False)
        y_bare2 = _run(model, inp, backward=False)
    print(f"fresh {dtype}: adapted vs bare {rel(y_ad, y_bare):.3e}, two bare runs {rel(y_bare2, y_bare):.3e}")
    if dtype == "fp32":
        assert rel(y_ad, y_bare) <= max(3 * rel(y_bare2, y_bare), 1e-5)
    else:
        x, t, ctx, pooled, ids, _ = inp
        with torch.no_grad():
            y_ora = ora(x, t, encoder_hidden_states=ctx, added_cond_kwargs={"text_embeds": pooled, "time_ids": ids})[0]
        print(f"fresh bf16: bare vs oracle {rel(y_bare, y_ora):.3e}")
        assert rel(y_ad, y_bare) <= 2 * rel(y_bare, y_ora)
    # merge_to: W' folded into the base weights -> a plain UNet computing the adapted output
    ora, model, net = _models(TINY, dtype, DORA_TOML)
    leaves = {k: v.detach().cpu().double() for k, v in net.state_dict().items() if not k.endswith(".alpha")}
    want = _effective(ora, net, leaves, torch.float64)
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        net.restore()
        net.merge_to(model)
        assert model.P.ad is None
        y_merged = _run(model, inp, backward=False)
        sd = model.state_dict()
        for s in net.specs:
            for suffix in ([".weight", ".bias"] if s.algo == "norm" else [".weight"]):
                w = want[s.name + suffix].detach()
                got = sd[s.name + suffix].detach().cpu().double().view(w.shape)
                assert float((got - w).abs().max() / w.abs().max()) < 1e-6, s.name
    if dtype == "fp32":
        assert rel(y_merged, y_ad) < 1e-6


@pytest.mark.parametrize("dtype,floor", [("fp32", 2e-5), ("bf16", 5e-3)])
def test_gradient_checkpointing_same_dora_gradients(dtype, floor):
    """as tests/test_lycoris_gpu.py: recomputed segments give the adapter gradients (dora_scale included) of the plain
    path to within the plain path's own run-to-run noise, measured here between two plain runs"""
    ora, model, net = _models(SDXL_W, dtype, DORA_TOML)
    inp = _inputs(SDXL_W)
    grads = []
    for ck in (False, False, True):
        model.enable_gradient_checkpointing(ck)
        if net.flat.grad is not None:
            net.flat.grad.zero_()
        _run(model, inp)
        grads.append(net.flat.grad.clone())
    model.enable_gradient_checkpointing(False)
    g0, ga, g1 = grads
    noise = rel(ga, g0)
    print(f"checkpointing {dtype}: recomputed {rel(g1, g0):.3e}, two plain runs {noise:.3e}")
    assert rel(g1, g0) <= max(3 * noise, floor), (rel(g1, g0), noise)
    sc = torch.cat([net.view(s.name, "dora_scale", buf=g0).reshape(-1) for s in net.specs if s.dora])
    assert float(sc.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ training
def _fit_cfg(tmp_path, steps, prodigy):
    from uwudiff_amd.config import load_yaml, merge

    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1,
                                 "default_root_dir": str(tmp_path)},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8},
                     "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": 1e-3, "lycoris_config": DORA_TOML}}
    if prodigy:
        # d0: Prodigy moves a value by about d per step, and d has not grown in six steps.  The package's 1e-6 is a few fp32
        # ulps of a magnitude near 0.6, and nothing where the gradient is below the optimizer's eps (the attention queries of
        # a fresh network): every dora_scale tensor can only be seen to move with a d0 well above an ulp.
        over["trainer"].update(lr=1.0, optimizer="prodigyopt.Prodigy",
                               opt_config={"weight_decay": 0.01, "use_bias_correction": True, "safeguard_warmup": True,
                                           "d0": 1e-3})
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over)
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    return cfg, lc


def _fresh(tmp_path, steps, prodigy):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, steps, prodigy)
    seed_everything(cfg.seed)
    fit = Fitter(**lc)
    dm, tr = load_all(cfg)
    return fit, dm, tr


@pytest.mark.parametrize("prodigy", [False, True], ids=["adamw", "prodigy"])
def test_fit_trains_dora_scale_and_resumes(tmp_path, prodigy):
    """6 steps on the tiny UNet with the DoRA preset: finite loss, every dora_scale moves, the base does not; a checkpoint at
    step 3 holds the dora_scale keys, restores the adapter buffer bit for bit, and the resumed run arrives at step 6 where the
    uninterrupted one does -- to the bars of test_resume_matches_uninterrupted_run (tests/test_lycoris_gpu.py), because two
    uninterrupted runs of the UNet are not bit-identical themselves (GroupNorm statistics add with fp32 atomics)."""
    from uwudiff_amd.engine import seed_everything
    from uwudiff_amd.optim import FusedAdamW, FusedProdigy

    path = str(tmp_path / "step3.ckpt")
    at3 = {}

    def save_at_3(f):
        if f.global_step == 3:
            f.save_checkpoint(path)
            at3["flat"] = tr.lycoris_model.flat.detach().clone()
            seed_everything(777)

    fit, dm, tr = _fresh(tmp_path, 6, prodigy)
    base0 = tr.unet.flat.detach().clone()
    scale0 = {s.name: tr.lycoris_model.view(s.name, "dora_scale").clone() for s in tr.lycoris_model.specs if s.dora}
    assert scale0 and all(float(v.min()) > 0 for v in scale0.values())  # the norms of the base weights
    fit.step_hooks.append(save_at_3)
    hist = fit.fit(tr, dm)
    assert type(fit._fit_state[1]) is (FusedProdigy if prodigy else FusedAdamW)
    assert fit.global_step == 6 and len(hist) == 6 and all(math.isfinite(h["loss"]) for h in hist)
    for name, v0 in scale0.items():
        assert not torch.equal(tr.lycoris_model.view(name, "dora_scale").cpu(), v0.cpu()), name
    assert torch.equal(tr.unet.flat.detach().cpu(), base0.cpu()) and tr.unet.flat.grad is None
    ck = torch.load(path, map_location="cpu", weights_only=True)
    keys = {k for k in ck["state_dict"] if k.endswith(".dora_scale")}
    assert keys == {f"lycoris_model.{s.key}.dora_scale" for s in tr.lycoris_model.specs if s.dora}

    fit2, dm2, tr2 = _fresh(tmp_path, 6, prodigy)
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        loaded["flat"] = tr2.lycoris_model.flat.detach().clone()
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert torch.equal(loaded["flat"], at3["flat"])  # what the resume starts from: the bits of step 3
    a, b = tr.lycoris_model.flat.detach(), tr2.lycoris_model.flat.detach()
    print(f"resume ({'prodigy' if prodigy else 'adamw'}): step 6 bit-identical {torch.equal(a, b)}, rel {rel(b, a):.3e}")
    assert fit2.global_step == 6
    assert [h["loss"] for h in hist_b] == pytest.approx([h["loss"] for h in hist][-3:], rel=1e-4)
    assert rel(b, a) < 1e-3
