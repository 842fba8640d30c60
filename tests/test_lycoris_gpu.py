"""GPU: LyCORIS adapters on the UNet -- uwu_adapter_merge / uwu_adapter_grad against torch (fp64), zero-delta start,
output and adapter-gradient parity with the CPU oracle fed merged weights, frozen base under the Fitter, gradient
checkpointing, merge_lycoris, the launcher with a TOML path, resume, and two ranks."""
import gc
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")
TINY = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
            down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
            transformer_layers_per_block=(1, 2), attention_head_dim=(1, 1), cross_attention_dim=32,
            addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=16 + 48,
            norm_num_groups=8)
# SDXL widths (640-channel transformer stack, 64-dim heads, 2048-dim context) at reduced depth: the shipped preset's
# factor-64 / factor-6 LoKr shapes
SDXL_W = dict(TINY, block_out_channels=(320, 640), attention_head_dim=(5, 10), transformer_layers_per_block=(1, 1),
              cross_attention_dim=2048, norm_num_groups=32)
LOWRANK = {"config": {"algo": "lokr", "linear_dim": 2, "linear_alpha": 3, "factor": 4, "train_norm": True},
           "preset": {"target_module": ["Transformer2DModel"], "module_algo_map": {"FeedForward": {"algo": "lora", "linear_dim": 3}}}}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------------------ kernels
def _grad_case(kind, N, K, r=0, out_k=0, in_n=0, seed=0):
    """random adapter factors + dW; returns (p, pa, pb, pc, shapes)"""
    from uwudiff_amd import adapters as A

    g = torch.Generator().manual_seed(seed)
    if kind == A.KIND_LORA:
        shapes = [(N, r), (r, K)]
    elif kind == A.KIND_LOKR:
        shapes = [(N // out_k, K // in_n), (out_k, in_n)]
    else:
        shapes = [(N // out_k, K // in_n), (out_k, r), (r, in_n)]
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        n += (math.prod(s) + 63) // 64 * 64
    p = torch.randn(n, generator=g)
    dW = torch.randn(N, K, generator=g)
    return p, dW, offs + [0] * (3 - len(offs)), shapes


def _run_grad(kind, p, dW, offs, spec_r, out_k, in_n, scale, g0=None):
    from uwudiff_amd import lib as L
    from uwudiff_amd.adapters import Spec, grad_ws_elems

    N, K = dW.shape
    s = Spec.__new__(Spec)
    s.algo, s.r, s.out_k, s.in_n = ("lora" if kind == 1 else "lokr"), spec_r, out_k, in_n
    ws = torch.empty(grad_ws_elems(s, N, K), device="cuda")
    g = (g0.clone() if g0 is not None else torch.zeros_like(p)).cuda()
    dWd, pd = dW.cuda(), p.cuda()  # (held: the kernel runs after L.call returns)
    L.call("uwu_adapter_grad", L.ptr(dWd), N, K, kind, L.ptr(pd), L.ptr(g), offs[0], offs[1], offs[2], spec_r,
           out_k, in_n, float(scale), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return g.cpu()


@pytest.mark.parametrize("kind,N,K,r,out_k,in_n", [
    (1, 96, 300, 1, 0, 0), (1, 640, 640, 3, 0, 0), (1, 77, 1280, 4, 0, 0), (1, 200, 130, 64, 0, 0),
    (2, 5 * 2048, 5 * 256, 0, 2048, 256), (2, 10 * 64, 32 * 64, 0, 64, 64), (2, 3 * 13, 7 * 11, 0, 13, 11),
    (3, 8 * 16, 8 * 16, 3, 16, 16)])
def test_adapter_grad_matches_fp64(kind, N, K, r, out_k, in_n):
    p, dW, offs, shapes = _grad_case(kind, N, K, r, out_k, in_n)
    scale = 0.75
    g0 = torch.randn_like(p)  # accumulates into what is there
    g = _run_grad(kind, p, dW, offs, r, out_k, in_n, scale, g0)
    views = lambda t: [t[o:o + math.prod(s)].view(s).double() for o, s in zip(offs, shapes)]
    P, G, G0, D = views(p), views(g), views(g0), dW.double()
    if kind == 1:
        up, down = P
        want = [scale * D @ down.T, scale * up.T @ D]
    else:
        w1 = P[0]
        w2 = P[1] if kind == 2 else P[1] @ P[2]
        D4 = D.view(N // out_k, out_k, K // in_n, in_n)
        dw1 = scale * torch.einsum("ikjl,kl->ij", D4, w2)
        dw2 = scale * torch.einsum("ikjl,ij->kl", D4, w1)
        want = [dw1, dw2] if kind == 2 else [dw1, dw2 @ P[2].T, P[1].T @ dw2]
    for gi, g0i, w in zip(G, G0, want):
        assert rel(gi - g0i, w) < 1e-5
    g2 = _run_grad(kind, p, dW, offs, r, out_k, in_n, scale, g0)
    assert torch.equal(g, g2)  # no float atomics: bit-identical


def test_adapter_merge_matches_torch():
    from uwudiff_amd import lib as L

    g = torch.Generator().manual_seed(3)
    segs = [(0, (1, 640)), (1, (96, 300)), (2, (640, 2048)), (3, (39, 77)), (1, (130, 200))]  # kind, (rows, cols)
    base_n, p_n, rows, blk, want = 0, 0, [], [0], []
    p_parts, alloc = [], lambda n: (n + 63) // 64 * 64
    for kind, (R, C) in segs:
        if kind == 0:
            sh = [(R * C,)]
        elif kind == 1:
            sh = [(R, 4), (4, C)]
        elif kind == 2:
            sh = [(10, 32), (64, 64)]
        else:
            sh = [(3, 7), (13, 2), (2, 11)]
        offs = []
        for s in sh:
            offs.append(p_n)
            t = torch.randn(math.prod(s), generator=g)
            p_parts.append((p_n, t))
            p_n += alloc(t.numel())
        rows.append((kind, R, C, base_n, sh, offs))
        base_n += alloc(R * C)
    p = torch.zeros(p_n)
    for o, t in p_parts:
        p[o:o + t.numel()] = t
    base = torch.randn(base_n, generator=g)
    table = []
    for kind, R, C, boff, sh, offs in rows:
        scale = 0.5 if kind != 2 else 1.0
        V = [p[o:o + math.prod(s)].view(s).double() for o, s in zip(offs, sh)]
        if kind == 0:
            d = V[0].view(R, C)
        elif kind == 1:
            d = scale * V[0] @ V[1]
        elif kind == 2:
            d = scale * torch.kron(V[0], V[1])
        else:
            d = scale * torch.kron(V[0], V[1] @ V[2])
        want.append(base[boff:boff + R * C].double().view(R, C) + d)
        sbits = int.from_bytes(torch.tensor([scale], dtype=torch.float32).numpy().tobytes(), "little")
        out_k, in_n, r = {0: (0, 0, 0), 1: (0, 0, 4), 2: (64, 64, 0), 3: (13, 11, 2)}[kind]
        table.append([kind, R, C, boff, boff, boff, offs[0], offs[1] if len(offs) > 1 else 0,
                      offs[2] if len(offs) > 2 else 0, r, out_k, in_n, sbits])
        blk.append(blk[-1] + -(-(R * C) // 4096))
    tab = torch.tensor(table, dtype=torch.int64).cuda()
    bl = torch.tensor(blk, dtype=torch.int64).cuda()
    eff = torch.full((base_n,), float("nan"), device="cuda")
    sh16 = torch.zeros(base_n, dtype=torch.bfloat16, device="cuda")
    based, pd = base.cuda(), p.cuda()
    L.call("uwu_adapter_merge", L.ptr(based), L.ptr(pd), L.ptr(tab), L.ptr(bl), len(table), blk[-1], L.ptr(eff),
           L.ptr(sh16), L.stream())
    torch.cuda.synchronize()
    for (kind, R, C, boff, _, _), w in zip(rows, want):
        got = eff[boff:boff + R * C].cpu().view(R, C)
        assert float((got.double() - w).abs().max() / w.abs().max()) < 1e-6, kind
        cast = torch.empty(R * C, dtype=torch.bfloat16, device="cuda")
        L.call("uwu_cast_f32_to_bf16", L.ptr(eff[boff:boff + R * C].contiguous()), L.ptr(cast), R * C, L.stream())
        assert torch.equal(sh16[boff:boff + R * C], cast), kind


# ------------------------------------------------------------------------------------------------------------ model
def _models(cfg, dtype, lyc, seed=0, random_adapters=True):
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
        with torch.no_grad():
            net.flat.data.copy_(torch.randn(net.n, generator=torch.Generator().manual_seed(seed + 9)).cuda() * 0.1)
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


def _oracle_adapted(ora, net, inp):
    """the oracle with W + dW built by torch ops from leaf adapter tensors: output and the adapter gradients"""
    leaves = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()
              if not k.endswith(".alpha")}
    params = dict(ora.named_parameters())
    sub = {}
    for s in net.specs:
        L = lambda t: leaves[f"{s.key}.{t}"]
        if s.algo == "norm":
            sub[s.name + ".weight"] = params[s.name + ".weight"] + L("w_norm")
            sub[s.name + ".bias"] = params[s.name + ".bias"] + L("b_norm")
            continue
        if s.algo == "lora":
            d = (L("lora_up.weight") @ L("lora_down.weight")) * s.scale
        elif s.lowrank:
            d = torch.kron(L("lokr_w1"), L("lokr_w2_a") @ L("lokr_w2_b")) * s.scale
        else:
            d = torch.kron(L("lokr_w1"), L("lokr_w2")) * s.scale
        w = params[s.name + ".weight"]
        sub[s.name + ".weight"] = w + d.view(w.shape)
    x, t, ctx, pooled, ids, dout = inp
    y = torch.func.functional_call(ora, sub, (x, t), dict(encoder_hidden_states=ctx,
                                                         added_cond_kwargs={"text_embeds": pooled, "time_ids": ids}),
                                   strict=False)[0]
    y.backward(dout)
    return y.detach(), {k: v.grad for k, v in leaves.items()}


def _adapter_grads(net):
    return {f"{s.key}.{t}": net.view(s.name, t, buf=net.flat.grad).cpu() for s in net.specs for t, _ in s.tensors}


@pytest.mark.parametrize("cfg,lyc,dtype", [(TINY, TOML, "fp32"), (SDXL_W, TOML, "fp32"), (TINY, LOWRANK, "fp32"),
                                           (TINY, TOML, "bf16")], ids=["tiny", "sdxl_width", "tiny_lowrank", "tiny_bf16"])
def test_adapted_unet_matches_oracle(cfg, lyc, dtype):
    ora, model, net = _models(cfg, dtype, lyc)
    inp = _inputs(cfg)
    y = _run(model, inp)
    yo, go = _oracle_adapted(ora, net, inp)
    ybar, gbar = (1e-3, 2e-3) if dtype == "fp32" else (4e-2, 0.12)
    assert rel(y, yo) < ybar
    got = _adapter_grads(net)
    if dtype == "fp32":
        bad = {k: rel(got[k], go[k]) for k in go if rel(got[k], go[k]) > gbar}
    else:  # bf16 operands: the whole adapter gradient, and every tensor of >= 64 elements (a LoKr w1 of one element is
        # a single 4096-term dot product <dW, w2> that cancels down to the bf16 noise of dW)
        cat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(go)])
        bad = {"all": rel(cat(got), cat(go))} if rel(cat(got), cat(go)) > ybar else {}
        bad.update({k: rel(got[k], go[k]) for k in go if go[k].numel() >= 64 and rel(got[k], go[k]) > gbar})
    assert not bad, bad
    assert model.flat.grad is None and not model.flat.requires_grad


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fresh_adapters_leave_output_unchanged(dtype):
    from uwudiff_amd.adapters import LycorisNetwork

    ora, model, net = _models(TINY, dtype, TOML, random_adapters=False)
    inp = _inputs(TINY)
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        # the merged effective weights are the base weights, bit for bit
        for nm in model.P.ad.eff_off:
            assert torch.equal(model.P.w32(nm), model.P.base32(nm)), nm
        shadow_ad = model.shadow.clone() if dtype == "bf16" else None
        net.restore()
        if dtype == "bf16":
            assert torch.equal(model.shadow, shadow_ad)  # the re-cast base == the merged shadow
        y_bare = _run(model, inp, backward=False)
        y_bare2 = _run(model, inp, backward=False)
    # The effective weights are the base weights bit for bit (above).  The forward itself is reproducible to its last bits
    # only (GroupNorm statistics add with fp32 atomics, so two runs of the bare model may differ by a few 1e-7 in fp32 or an
    # occasional bf16 ulp): the outputs agree within that noise -- far below any effect of a non-zero adapter.
    floor = 1e-5 if dtype == "fp32" else 1e-3
    assert rel(y_ad, y_bare) <= max(3 * rel(y_bare2, y_bare), floor)
    # merge_lycoris: W + dW folded into the base weights -> a plain UNet computing the adapted output
    ora, model, net = _models(TINY, dtype, TOML)
    with torch.no_grad():
        y_ad = _run(model, inp, backward=False)
        net.restore()
        net.merge_to(model)
        assert model.P.ad is None
        y_merged = _run(model, inp, backward=False)
    if dtype == "fp32":
        assert rel(y_merged, y_ad) < 1e-6
    assert isinstance(net, LycorisNetwork)


@pytest.mark.parametrize("dtype,floor", [("fp32", 2e-5), ("bf16", 5e-3)])
def test_gradient_checkpointing_same_adapter_gradients(dtype, floor):
    """Recomputed segments give the adapter gradients of the plain path, to within the plain path's own run-to-run noise
    (GroupNorm statistics, norm dgamma / dbeta and the LayerNorm column sums add with fp32 atomics; in bf16 a last-bit
    difference of a statistic flips bf16 roundings downstream: ~2 % on the adapter gradients of this model, measured the
    same between two plain runs as between a plain and a recomputed run).  The fp32 case is the sharp one (~5e-6)."""
    ora, model, net = _models(SDXL_W, dtype, TOML)
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
    assert rel(g1, g0) <= max(3 * noise, floor), (rel(g1, g0), noise)


# ------------------------------------------------------------------------------------------------------------ training
def _fit_cfg(tmp_path, lyc, steps, extra=None):
    from uwudiff_amd.config import load_yaml, merge

    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1,
                                 "default_root_dir": str(tmp_path)},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8}, "dataloader_config": {"batch_size": 4}},
            "trainer": {"lr": 1e-3, "lycoris_config": lyc}}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over, extra or {})
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    return cfg, lc


def test_fitter_trains_adapters_only(tmp_path):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    peaks = {}
    for mode in ("full", "lycoris"):
        cfg, lc = _fit_cfg(tmp_path / mode, TOML if mode == "lycoris" else None, 3)
        seed_everything(cfg.seed)
        fit = Fitter(**lc)
        dm, tr = load_all(cfg)
        flat0 = tr.unet.flat.detach().clone()
        # the peak is measured from `base`: device memory that only a cycle still holds (a UNet and the network attached to it in the
        # tests above, the trainer and fitter of the first pass) goes now, not at some point inside the measured region
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        hist = fit.fit(tr, dm)
        peaks[mode] = torch.cuda.max_memory_allocated() - base
        assert fit.global_step == 3 and all(math.isfinite(h["loss"]) for h in hist)
        if mode == "lycoris":
            assert torch.equal(tr.unet.flat.detach().cpu(), flat0.cpu())
            assert tr.unet.flat.grad is None
            opt_params = [p for st in fit._fit_state[1].state for p in [st]]
            assert len(opt_params) == 1 and opt_params[0] is tr.lycoris_model.flat
            assert fit._fit_state[1].state[tr.lycoris_model.flat]["exp_avg"].numel() == tr.lycoris_model.n
            assert float(tr.lycoris_model.flat.detach().abs().sum()) > 0
        del tr, dm, fit
        torch.cuda.empty_cache()
    assert peaks["lycoris"] < peaks["full"], peaks


def test_launcher_with_toml_path_and_epoch_weights(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "demo_training.yaml")))
    cfg["lightning_config"].update(fast_dev_run=False, max_steps=2, log_every_n_steps=1, callbacks=[],
                                   default_root_dir=str(tmp_path))
    cfg["data"]["dataset_config"].update(n_samples=8)
    cfg["data"]["dataloader_config"].update(batch_size=4, num_workers=0)
    cfg["trainer"].update(lr=1e-3, lycoris_config=TOML)
    path = tmp_path / "lyc.yaml"
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_train.py"), "--configs", str(path)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(l.split('"loss": ')[1].split(",")[0]) for l in r.stdout.splitlines() if '"loss": ' in l]
    assert losses and all(math.isfinite(v) for v in losses)
    sd = torch.load(tmp_path / "lycoris_weight" / "epoch=0.pt", weights_only=True)
    q = "lycoris_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q"
    assert {q + ".lokr_w1", q + ".lokr_w2", q + ".alpha"} <= set(sd)
    assert "lycoris_down_blocks_1_attentions_0_proj_in.lora_up.weight" in sd
    assert float(sd[q + ".lokr_w2"].abs().max()) > 0  # moved away from its zero start


def test_resume_matches_uninterrupted_run(tmp_path):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    path = str(tmp_path / "step2.ckpt")

    def fresh(steps):
        cfg, lc = _fit_cfg(tmp_path, TOML, steps)
        seed_everything(cfg.seed)
        fit = Fitter(**lc)
        dm, tr = load_all(cfg)
        return fit, dm, tr

    def save_at_2(f):
        if f.global_step == 2:
            f.save_checkpoint(path)
            seed_everything(777)

    fit, dm, tr = fresh(4)
    fit.step_hooks.append(save_at_2)
    tail_a = [h["loss"] for h in fit.fit(tr, dm)][-2:]
    ad_a = tr.lycoris_model.flat.detach().clone()
    ck = torch.load(path, weights_only=True)
    assert any(k.startswith("lycoris_model.lycoris_") for k in ck["state_dict"])

    fit2, dm2, tr2 = fresh(4)
    orig = fit2.load_checkpoint

    def load_and_seed(p):
        out = orig(p)
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert [h["loss"] for h in hist_b] == pytest.approx(tail_a, rel=1e-4)
    assert rel(tr2.lycoris_model.flat.detach(), ad_a) < 1e-3


# ------------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from uwudiff_amd.gradsync import FlatGradSync
    from uwudiff_amd.optim import FusedAdamW

    torch.cuda.set_device(0)
    ora, model, net = _models(TINY, "bf16", TOML, seed=0)  # identical replicas (same seeds)
    inp = _inputs(TINY, seed=10 + rank)  # per-rank data
    _run(model, inp)
    mine = net.flat.grad.clone()
    sync = FlatGradSync(world)
    sync.all_reduce(net.flat.grad)
    sync.wait_all()
    torch.cuda.synchronize()
    both = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    fails = []
    avg = (both[0] + both[1]) * 0.5
    if rel(net.flat.grad * sync.pre_scale, avg) > 1e-6:
        fails.append("averaged gradient")
    opt = FusedAdamW([net.flat], lr=1e-3)
    opt.step(pre_scale=sync.pre_scale)
    torch.cuda.synchronize()
    after = net.flat.detach().clone()
    gathered = [torch.empty_like(after) for _ in range(world)]
    dist.all_gather(gathered, after)
    if not torch.equal(gathered[0], gathered[1]):
        fails.append("replicas differ")
    q.put((rank, fails))
    dist.destroy_process_group()


def test_two_ranks_average_adapter_gradients():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(not f for _, f in res), res
