"""GPU: LyCORIS convolution adapters -- uwu_adapter_conv_merge / uwu_adapter_conv_grad against
fp64 torch on the smallest shapes that can go wrong (columns crossing the 256-column tile in mid-tap, padded channels, odd
rows, w2 crossing the 2048-element group), then the adapted UNet against the CPU oracle fed W + dW built by torch from the
public adapter tensors (fp32, bf16, the implicit-GEMM path at SDXL widths), zero-delta start, merge_lycoris, the frozen
base, accumulation, and one launcher step of configs/demo_training_locon.yaml on the tiny UNet."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.test_lycoris_gpu import SDXL_W, TINY, _adapter_grads, _inputs, _models, _run, rel

pytestmark = pytest.mark.gpu

CONV = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers-conv.toml")
LORA, TUCKER, LOKR, LOWRANK = 4, 5, 6, 7  # UWU_ADAPTER_CONV_*
TARGETS = {"enable_conv": True, "target_module": ["Transformer2DModel", "ResnetBlock2D", "Downsample2D", "Upsample2D"],
           "target_name": ["conv_in", "conv_out"]}
# plain LoCon on the samplers / conv_in / conv_out, full LoKr on the ResNet convolutions
LOCON_LOKR = {"config": {"algo": "lora", "linear_dim": 2, "conv_dim": 3, "conv_alpha": 1.5, "train_norm": True},
              "preset": {**TARGETS, "module_algo_map": {"ResnetBlock2D": {"algo": "lokr", "factor": 4, "full_matrix": True}}}}
# low-rank LoKr on the convolutions (conv_dim 2 < max(out_k, in_n) / 2 = 4) and on the Linears
LOKR_LOW = {"config": {"algo": "lokr", "linear_dim": 2, "linear_alpha": 3, "conv_dim": 2, "conv_alpha": 3, "factor": 4},
            "preset": TARGETS}

# (kind, cout_store, cin_store, cout, cin, r, out_k, in_n)
CASES = [
    (LORA, 40, 40, 40, 40, 1, 0, 0), (LORA, 40, 40, 40, 40, 16, 0, 0), (LORA, 77, 24, 77, 24, 4, 0, 0),
    (LORA, 8, 32, 4, 32, 4, 0, 0), (LORA, 32, 8, 32, 4, 16, 0, 0),
    (TUCKER, 40, 40, 40, 40, 4, 0, 0), (TUCKER, 40, 40, 40, 40, 16, 0, 0), (TUCKER, 77, 24, 77, 24, 1, 0, 0),
    (TUCKER, 8, 32, 4, 32, 1, 0, 0), (TUCKER, 32, 8, 32, 4, 4, 0, 0),
    (LOKR, 64, 24, 64, 24, 0, 32, 8), (LOKR, 39, 10, 39, 10, 0, 13, 5), (LOKR, 8, 32, 4, 32, 0, 2, 8),
    (LOKR, 32, 8, 32, 4, 0, 8, 2),
    (LOWRANK, 32, 16, 32, 16, 3, 16, 8),
]
IDS = [f"k{c[0]}-{c[1]}x{c[2]}-{c[3]}x{c[4]}-r{c[5]}-{c[6]}x{c[7]}" for c in CASES]


def _shapes(kind, cout, cin, r, out_k, in_n):
    """the adapter tensors in the kernels' order (pa, pb, pc) and layout (tap-major)"""
    if kind == LORA:
        return [(cout, r), (r, 9, cin)]
    if kind == TUCKER:
        return [(cout, r), (r, cin), (r, 9, r)]
    if kind == LOKR:
        return [(cout // out_k, cin // in_n), (out_k, 9, in_n)]
    return [(cout // out_k, cin // in_n), (out_k, r), (r, 9, in_n)]


def _delta64(kind, V, scale):
    """dW [cout, 9, cin] in fp64 from the tensors of _shapes"""
    if kind == LORA:
        return scale * torch.einsum("oi,itc->otc", V[0], V[1])
    if kind == TUCKER:
        return scale * torch.einsum("oi,itj,jc->otc", V[0], V[2], V[1])
    w2 = V[1] if kind == LOKR else torch.einsum("kr,rtl->ktl", V[1], V[2])
    a, b = V[0].shape
    k, _, l = w2.shape
    return scale * torch.einsum("ab,ktl->aktbl", V[0], w2).reshape(a * k, 9, b * l)


def _grads64(kind, V, D, scale):
    """the adapter gradients from D = dL/dW [cout, 9, cin] (fp64), in the order of _shapes"""
    if kind == LORA:
        return [scale * torch.einsum("otc,itc->oi", D, V[1]), scale * torch.einsum("oi,otc->itc", V[0], D)]
    if kind == TUCKER:
        T = torch.einsum("itj,jc->itc", V[2], V[1])
        dT = scale * torch.einsum("oi,otc->itc", V[0], D)
        return [scale * torch.einsum("otc,itc->oi", D, T), torch.einsum("itj,itc->jc", V[2], dT),
                torch.einsum("itc,jc->itj", dT, V[1])]
    w2 = V[1] if kind == LOKR else torch.einsum("kr,rtl->ktl", V[1], V[2])
    a, b = V[0].shape
    k, _, l = w2.shape
    D6 = D.reshape(a, k, 9, b, l)
    dw1 = scale * torch.einsum("aktbl,ktl->ab", D6, w2)
    dw2 = scale * torch.einsum("aktbl,ab->ktl", D6, V[0])
    if kind == LOKR:
        return [dw1, dw2]
    return [dw1, torch.einsum("ktl,rtl->kr", dw2, V[2]), torch.einsum("kr,ktl->rtl", V[1], dw2)]


def _pack(shapes, g, n0=0):
    offs, n = [], n0
    for s in shapes:
        offs.append(n)
        n += (math.prod(s) + 63) // 64 * 64
    return offs, n


def _ws_elems(kind, cout, cin, r, out_k, in_n):
    from uwudiff_amd.adapters import Spec, conv_grad_ws_elems

    s = Spec.__new__(Spec)
    s.shape, s.algo, s.r, s.out_k, s.in_n = (cout, cin), ("lora" if kind in (LORA, TUCKER) else "lokr"), r, out_k, in_n
    s.tucker = kind == TUCKER
    return conv_grad_ws_elems(s)


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kind,co,ci,cout,cin,r,out_k,in_n", CASES, ids=IDS)
def test_conv_adapter_grad_matches_fp64(kind, co, ci, cout, cin, r, out_k, in_n):
    from uwudiff_amd import lib as L

    g = torch.Generator().manual_seed(7)
    shapes = _shapes(kind, cout, cin, r, out_k, in_n)
    offs, n = _pack(shapes, g)
    p = torch.randn(n, generator=g)
    dW = torch.randn(co, 9 * ci, generator=g)  # the padded rows and channels hold values too: they must not be read
    g0 = torch.randn(n, generator=g)  # accumulates into what is there
    scale = 0.75
    pa, pb, pc = (offs + [0])[:3]
    pd, dWd = p.cuda(), dW.cuda()
    ws = torch.empty(_ws_elems(kind, cout, cin, r, out_k, in_n), device="cuda")

    def run():
        gd = g0.cuda()
        L.call("uwu_adapter_conv_grad", L.ptr(dWd), co, ci, cout, cin, kind, L.ptr(pd), L.ptr(gd), pa, pb, pc, r, out_k, in_n,
               scale, L.ptr(ws), ws.numel(), L.stream())
        torch.cuda.synchronize()
        return gd.cpu()

    got = run()
    V = [p[o:o + math.prod(s)].view(s).double() for o, s in zip(offs, shapes)]
    D = dW.double().view(co, 9, ci)[:cout, :, :cin]
    want = _grads64(kind, V, D, scale)
    touched = torch.zeros(n, dtype=torch.bool)
    for o, s, w in zip(offs, shapes, want):
        sl = slice(o, o + math.prod(s))
        touched[sl] = True
        err = rel((got[sl] - g0[sl]).view(s), w)
        print(f"{s}: rel {err:.2e}")
        assert err < 1e-5, s
    assert torch.equal(got[~touched], g0[~touched])  # nothing outside the tensors is written
    assert torch.equal(run(), got)  # no float atomics: bit-identical


def test_conv_adapter_merge_matches_torch():
    from uwudiff_amd import lib as L

    g = torch.Generator().manual_seed(3)
    rows, blk, fblk, base_n, p_n, t_n, segs = [], [0], [0], 0, 0, 0, []
    for kind, co, ci, cout, cin, r, out_k, in_n in CASES:
        shapes = _shapes(kind, cout, cin, r, out_k, in_n)
        offs, p_n = _pack(shapes, g, p_n)
        scale = 1.0 if kind == LOKR else 0.5
        sbits = int.from_bytes(torch.tensor([scale], dtype=torch.float32).numpy().tobytes(), "little")
        pa, pb, pc = (offs + [0])[:3]
        rows.append([kind, co, 9 * ci, base_n, base_n, base_n, pa, pb, pc, r, out_k, in_n, sbits, cout, cin, ci, t_n])
        segs.append((kind, co, ci, cout, cin, shapes, offs, base_n, scale))
        blk.append(blk[-1] + -(-(co * 9 * ci) // 4096))
        fblk.append(fblk[-1] + (-(-(9 * r * cin) // 256) if kind == TUCKER else 0))
        if kind == TUCKER:
            t_n += (9 * r * cin + 63) // 64 * 64
        base_n += (co * 9 * ci + 63) // 64 * 64
    p = torch.randn(p_n, generator=g)
    base = torch.randn(base_n, generator=g)
    for kind, co, ci, cout, cin, shapes, offs, boff, scale in segs:  # the padding of a stored weight holds zeros
        w = base[boff:boff + co * 9 * ci].view(co, 9, ci)
        w[cout:] = 0
        w[:, :, cin:] = 0
    host = torch.tensor(rows, dtype=torch.int64)
    tab, bl, fb = host.cuda(), torch.tensor(blk, dtype=torch.int64).cuda(), torch.tensor(fblk, dtype=torch.int64).cuda()
    eff = torch.full((base_n,), float("nan"), device="cuda")
    sh16 = torch.zeros(base_n, dtype=torch.bfloat16, device="cuda")
    tws = torch.full((t_n,), float("nan"), device="cuda")
    based, pd = base.cuda(), p.cuda()
    L.call("uwu_adapter_conv_merge", L.ptr(based), L.ptr(pd), L.ptr(tab), host.data_ptr(), L.ptr(bl), L.ptr(fb), len(rows),
           blk[-1], fblk[-1], L.ptr(tws), t_n, L.ptr(eff), L.ptr(sh16), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(based.cpu(), base)  # the base is read only
    for kind, co, ci, cout, cin, shapes, offs, boff, scale in segs:
        V = [p[o:o + math.prod(s)].view(s).double() for o, s in zip(offs, shapes)]
        n = co * 9 * ci
        want = base[boff:boff + n].double().view(co, 9, ci).clone()
        want[:cout, :, :cin] += _delta64(kind, V, scale)
        got = eff[boff:boff + n].cpu().view(co, 9, ci)
        err = float((got.double() - want).abs().max() / want.abs().max())
        print(f"kind {kind} [{co}, 9, {ci}] true ({cout}, {cin}): max-rel {err:.2e}")
        assert err < 1e-6, (kind, co, ci)
        assert float(got[cout:].abs().max() if co > cout else 0) == 0 and float(got[:, :, cin:].abs().max() if ci > cin else 0) == 0
        cast = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        L.call("uwu_cast_f32_to_bf16", L.ptr(eff[boff:boff + n].contiguous()), L.ptr(cast), n, L.stream())
        assert torch.equal(sh16[boff:boff + n], cast), (kind, co, ci)
    # in place (fold): eff aliases base
    L.call("uwu_adapter_conv_merge", L.ptr(based), L.ptr(pd), L.ptr(tab), host.data_ptr(), L.ptr(bl), L.ptr(fb), len(rows),
           blk[-1], fblk[-1], L.ptr(tws), t_n, L.ptr(based), None, L.stream())
    torch.cuda.synchronize()
    used = torch.zeros(base_n, dtype=torch.bool)
    for kind, co, ci, cout, cin, shapes, offs, boff, scale in segs:
        used[boff:boff + co * 9 * ci] = True
    assert torch.equal(based[used.cuda()], eff[used.cuda()])


def test_conv_merge_refuses_a_bad_table():
    """every row is checked on the host before anything is launched"""
    from uwudiff_amd import lib as L

    good = [LORA, 8, 9 * 8, 0, 0, -1, 0, 64, 0, 4, 0, 0, 0, 4, 8, 8, 0]
    bufs = [torch.zeros(1024, device="cuda") for _ in range(3)]
    blk = torch.tensor([0, 1], dtype=torch.int64).cuda()
    for field, value in ((14, 9), (13, 9), (2, 9 * 8 + 1), (9, 129), (0, 1), (3, 32)):
        row = list(good)
        row[field] = value
        host = torch.tensor([row], dtype=torch.int64)
        with pytest.raises(L.UwuError, match="adapter_conv_merge"):
            L.call("uwu_adapter_conv_merge", L.ptr(bufs[0]), L.ptr(bufs[1]), L.ptr(host.cuda()), host.data_ptr(), L.ptr(blk),
                   None, 1, 1, 0, None, 0, L.ptr(bufs[2]), None, L.stream())
    row = list(good)
    row[0] = TUCKER  # T [4, 9, 8] does not fit a workspace of 64 floats
    host = torch.tensor([row], dtype=torch.int64)
    with pytest.raises(L.UwuError, match="workspace"):
        L.call("uwu_adapter_conv_merge", L.ptr(bufs[0]), L.ptr(bufs[1]), L.ptr(host.cuda()), host.data_ptr(), L.ptr(blk),
               L.ptr(blk), 1, 1, 2, L.ptr(bufs[2]), 64, L.ptr(bufs[2]), None, L.stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ model
def _public_delta(s, leaf):
    """dW [Cout, Cin, 3, 3] of one adapted convolution from its public tensors, by torch ops (autograd runs through it)"""
    if s.algo == "lora" and not s.tucker:
        return s.scale * torch.einsum("pi,ichw->pchw", leaf("lora_up.weight")[:, :, 0, 0], leaf("lora_down.weight"))
    if s.algo == "lora":
        return s.scale * torch.einsum("pi,ijhw,jc->pchw", leaf("lora_up.weight")[:, :, 0, 0], leaf("lora_mid.weight"),
                                      leaf("lora_down.weight")[:, :, 0, 0])
    w1 = leaf("lokr_w1")
    w2 = (leaf("lokr_w2_a") @ leaf("lokr_w2_b")).view(s.out_k, s.in_n, 3, 3) if s.lowrank else leaf("lokr_w2")
    return s.scale * torch.einsum("ab,cdhw->acbdhw", w1, w2).reshape(s.shape[0], s.shape[1], 3, 3)


def _oracle_adapted(ora, net, inp):
    """the oracle with W + dW built by torch ops from leaf adapter tensors: output and the adapter gradients"""
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()
              if not k.endswith(".alpha")}
    params = dict(ora.named_parameters())
    sub = {}
    for s in net.specs:
        leaf = lambda t, s=s: leaves[f"{s.key}.{t}"]
        if s.algo == "norm":
            sub[s.name + ".weight"] = params[s.name + ".weight"] + leaf("w_norm")
            sub[s.name + ".bias"] = params[s.name + ".bias"] + leaf("b_norm")
            continue
        w = params[s.name + ".weight"]
        if s.conv is not None:
            assert tuple(w.shape) == (*s.shape, 3, 3)
            d = _public_delta(s, leaf)
        elif s.algo == "lora":
            d = (leaf("lora_up.weight") @ leaf("lora_down.weight")) * s.scale
        elif s.lowrank:
            d = torch.kron(leaf("lokr_w1"), leaf("lokr_w2_a") @ leaf("lokr_w2_b")) * s.scale
        else:
            d = torch.kron(leaf("lokr_w1"), leaf("lokr_w2")) * s.scale
        sub[s.name + ".weight"] = w + d.view(w.shape)
    x, t, ctx, pooled, ids, dout = inp
    y = torch.func.functional_call(ora, sub, (x, t), dict(encoder_hidden_states=ctx,
                                                         added_cond_kwargs={"text_embeds": pooled, "time_ids": ids}),
                                   strict=False)[0]
    y.backward(dout)
    return y.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("cfg,lyc,dtype", [(TINY, CONV, "fp32"), (TINY, LOCON_LOKR, "fp32"), (TINY, LOKR_LOW, "fp32"),
                                           (TINY, CONV, "bf16"), (SDXL_W, CONV, "bf16")],
                         ids=["tiny_tucker", "tiny_locon_lokr", "tiny_lokr_lowrank", "tiny_tucker_bf16", "sdxl_width_bf16"])
def test_conv_adapted_unet_matches_oracle(cfg, lyc, dtype):
    from uwudiff_amd import ops

    ora, model, net = _models(cfg, dtype, lyc)
    convs = [s for s in net.specs if s.conv is not None]
    names = {s.name for s in convs}
    assert {"conv_in", "conv_out", "down_blocks.0.resnets.0.conv1", "down_blocks.0.downsamplers.0.conv",
            "up_blocks.0.upsamplers.0.conv", "mid_block.resnets.1.conv2"} <= names
    if lyc is LOCON_LOKR:
        assert {s.kind for s in convs} == {LORA, LOKR}
    elif lyc is LOKR_LOW:
        assert {s.kind for s in convs} == {LOWRANK}  # (every convolution of this UNet has out_k or in_n = 8)
    else:
        assert {s.kind for s in convs} == {TUCKER}
    inp = _inputs(cfg)
    if cfg is SDXL_W:  # the implicit-GEMM convolution (forward, dgrad, wgrad) is the path under test
        x = torch.empty(2 * 16 * 16, 320, device="cuda", dtype=torch.bfloat16)
        assert ops.conv3x3_implicit_ok(x, 2, 16, 16, 320, 320, 1) and ops.conv3x3_implicit_ok(x, 2, 16, 16, 320, 320, 2)
    flat0 = model.flat.detach().clone()
    y = _run(model, inp)
    yo, go = _oracle_adapted(ora, net, inp)
    ybar, gbar = (1e-3, 2e-3) if dtype == "fp32" else (4e-2, 0.12)  # the bounds of tests/test_lycoris_gpu.py for each mode
    print(f"output rel {rel(y, yo):.2e}")
    assert rel(y, yo) < ybar
    got = _adapter_grads(net)
    errs = {k: rel(got[k], go[k]) for k in go}
    print("worst gradients:", sorted(((round(v, 6), k) for k, v in errs.items()), reverse=True)[:6])
    if dtype == "fp32":
        bad = {k: v for k, v in errs.items() if v > gbar}
    else:
        cat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(go)])
        print(f"all gradients rel {rel(cat(got), cat(go)):.2e}")
        bad = {"all": rel(cat(got), cat(go))} if rel(cat(got), cat(go)) > ybar else {}
        bad.update({k: v for k, v in errs.items() if go[k].numel() >= 64 and v > gbar})
    assert not bad, bad
    assert model.flat.grad is None and not model.flat.requires_grad
    assert torch.equal(model.flat.detach(), flat0)  # the base is never written


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fresh_conv_adapters_and_merge_lycoris(dtype):
    ora, model, net = _models(TINY, dtype, CONV, random_adapters=False)
    inp = _inputs(TINY)
    convs = [s.name + ".weight" for s in net.specs if s.conv is not None]
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        # W + dW of a fresh network IS the base weight, bit for bit: the fp32 effective copies and the bf16 shadow
        assert dtype == "bf16" or set(convs) <= set(model.P.ad.eff_off)
        for nm in model.P.ad.eff_off:
            assert torch.equal(model.P.w32(nm), model.P.base32(nm)), nm
        shadow_ad = model.shadow.clone() if dtype == "bf16" else None
        net.restore()
        if dtype == "bf16":
            assert torch.equal(model.shadow, shadow_ad)
        y_bare = _run(model, inp, backward=False)
        y_bare2 = _run(model, inp, backward=False)
    # the same weights bit for bit; the forward itself repeats to its last bits only (GroupNorm statistics add with fp32
    # atomics), so the outputs are compared within the bare model's own run-to-run noise, as tests/test_lycoris_gpu.py does
    floor = 1e-5 if dtype == "fp32" else 1e-3
    assert rel(y_ad, y_bare) <= max(3 * rel(y_bare2, y_bare), floor)
    # merge_lycoris: the deltas folded into the base weights -> a plain UNet computing the adapted output
    ora, model, net = _models(TINY, dtype, LOCON_LOKR if dtype == "fp32" else CONV)
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        want = {s.name: model.P.base32(s.name + ".weight").double().cpu().view(s.conv[3], 9, s.conv[2])
                + net.conv_delta(s.name).cpu() for s in net.specs if s.conv is not None}
        net.restore()
        net.merge_to(model)
        assert model.P.ad is None
        for name, w in want.items():  # the folded base: W + dW, zeros where the channels are padding
            got = model.P.base32(name + ".weight").double().cpu().view(w.shape)
            assert float((got - w).abs().max()) <= 1e-6 * float(w.abs().max()), name
        cin, cout, ci, co = model._conv_meta["conv_in"]
        assert float(model.P.base32("conv_in.weight").view(co, 9, ci)[:, :, cin:].abs().max()) == 0
        cin, cout, ci, co = model._conv_meta["conv_out"]
        assert float(model.P.base32("conv_out.weight").view(co, 9, ci)[cout:].abs().max()) == 0
        y_merged = _run(model, inp, backward=False)
    print(f"merged vs adapted output rel {rel(y_merged, y_ad):.2e}")
    if dtype == "fp32":
        assert rel(y_merged, y_ad) < 1e-6


def test_two_micro_batches_accumulate():
    """The adapter-gradient writers ADD: the gradient after two backward passes is the sum of the two.  The bound is the
    plain path's own run-to-run noise (GroupNorm statistics and the norm gradients add with fp32 atomics: ~5e-6 in fp32,
    tests/test_lycoris_gpu.py), with the 2e-5 floor that file uses for the same comparison."""
    ora, model, net = _models(TINY, "fp32", CONV)
    a, b = _inputs(TINY, seed=1), _inputs(TINY, seed=2)

    def grad_of(*inps):
        if net.flat.grad is not None:
            net.flat.grad.zero_()
        for inp in inps:
            _run(model, inp)
        return net.flat.grad.clone()

    ga, ga2, gb = grad_of(a), grad_of(a), grad_of(b)
    gab = grad_of(a, b)
    noise = rel(ga2, ga)
    print(f"accumulated vs sum rel {rel(gab, ga + gb):.2e}, run-to-run {noise:.2e}")
    assert float(gb.abs().max()) > 0 and rel(ga, gb) > 0.1
    assert rel(gab, ga + gb) <= max(3 * noise, 2e-5)


def test_average_state_round_trip_in_public_shapes():
    """FlatAverage reads and writes the adapter network's entries in public shapes; lokr_w2_b of a convolution is no view of
    the buffer (its public column order is not a stride of the stored one), so the load must go through ``write``"""
    from uwudiff_amd.adapters import LycorisNetwork
    from uwudiff_amd.averaging import FlatAverage
    from uwudiff_amd.unet import UNet2DConditionModel

    unet = UNet2DConditionModel(TINY, init_weights=False, device="meta")
    net = LycorisNetwork(unet, LOKR_LOW).cuda()
    avg = FlatAverage(net)
    ref = net.state_dict()
    g = torch.Generator().manual_seed(4)
    sd = {k: torch.randn(v.shape, generator=g) for k, v in ref.items() if not k.endswith(".alpha")}
    assert any(k.endswith("conv1.lokr_w2_b") for k in sd)
    avg.load_averaged_state(sd)
    back = avg.averaged_state()
    assert all(torch.equal(back[k].cpu(), sd[k]) and back[k].is_contiguous() for k in sd)
    now = net.state_dict()
    assert all(torch.equal(now[k], ref[k]) for k in ref)  # the weights themselves are untouched
    avg.copy_to_current()  # the weights become the average
    torch.cuda.synchronize()
    now = net.state_dict()
    assert all(torch.equal(now[k].cpu(), sd[k]) for k in sd)


def test_launcher_one_step_with_the_locon_config(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "demo_training_locon.yaml")))
    assert cfg["trainer"]["lycoris_config"].endswith("configs/lycoris/sdxl-diffusers-conv.toml")
    assert cfg["unet_gradient_checkpointing"] is True  # (the recomputed segments hold adapted convolutions)
    cfg["lightning_config"].update(max_steps=1, log_every_n_steps=1, callbacks=[], default_root_dir=str(tmp_path))
    cfg["data"]["dataset_config"].update(sample_size=[3, 32, 32], n_samples=4)
    cfg["data"]["dataloader_config"].update(batch_size=4, num_workers=0)
    cfg["trainer"].update(lr=1e-3, lycoris_config=CONV)
    unet = cfg["trainer"]["model_config"]["unet"]
    unet["config"] = "tiny-unet"
    unet.pop("subfolder", None)
    path = tmp_path / "locon.yaml"
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_train.py"), "--configs", str(path)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(l.split('"loss": ')[1].split(",")[0]) for l in r.stdout.splitlines() if '"loss": ' in l]
    assert losses and all(math.isfinite(v) for v in losses)
    sd = torch.load(tmp_path / "lycoris_weight" / "epoch=0.pt", weights_only=True)
    q = "lycoris_down_blocks_0_resnets_0_conv1"  # tiny-unet: 64 -> 64 channels
    assert {k: tuple(sd[f"{q}.{k}"].shape) for k in ("lora_down.weight", "lora_mid.weight", "lora_up.weight")} == {
        "lora_down.weight": (4, 64, 1, 1), "lora_mid.weight": (4, 4, 3, 3), "lora_up.weight": (64, 4, 1, 1)}
    assert tuple(sd["lycoris_conv_in.lora_down.weight"].shape) == (4, 3, 1, 1)  # 3 true input channels of 8 stored
    assert tuple(sd["lycoris_conv_out.lora_up.weight"].shape) == (3, 4, 1, 1)
    for k in (q + ".lora_up.weight", "lycoris_conv_in.lora_up.weight", "lycoris_conv_out.lora_up.weight",
              "lycoris_up_blocks_1_resnets_1_conv2.lora_up.weight"):
        assert float(sd[k].abs().max()) > 0, k  # moved away from its zero start
