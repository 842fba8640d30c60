"""GPU: ``uwudiff_amd.optim.FusedAdafactor`` (uwu_adafactor_stats / _norm / _apply) against the fp64 oracle
advanced from the device's previous state, its side effects, determinism under chunking, the launch count, the refusals, and the
fit loop on the DiT, on a bit-reproducible denoiser (checkpoint and resume) and on LyCORIS adapters.

Bars (the issue's): ``p`` at the project's optimizer bar rtol 1e-5 / atol 1e-6; ``row``, ``col``, ``v`` at rtol 1e-5; ``exp_avg``: the
issue's rtol 1e-5 is too tight for a sum of two rounded products of either sign -- where they cancel an element carries their 2^-24
roundings, not its own, and the PACKAGE itself is 0.60 away element-wise from the oracle (tests/test_adafactor_cpu.py prints it).  The
replacement the issue names: 4x the package-vs-oracle floor.  That floor, in the metric |diff| / max|exp_avg| of the tensor, is
9.057e-7 (``EXP_AVG_FLOOR``, measured by the CPU test), so the bar is |diff| <= 3.623e-6 * max|exp_avg| of the tensor, no rtol term.
The package sits 4.5e-7 (p) and 1.7e-7 (second moments) from the oracle, so the rtol 1e-5 bars of those hold with room."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import adafactor_oracle as AO
from tests.conftest import ROOT
from tests.test_adafactor_cpu import EXP_AVG_FLOOR, SETTINGS, SHAPES, exp_avg_dev, make_grads, make_params
from tests.test_optimizers_gpu import TOML, ElementwiseDenoiser

pytestmark = pytest.mark.gpu

ZERO, HOLES = SHAPES.index((64, 64)), SHAPES.index((33, 257))  # all-zero gradient; one zero row and one zero column
KEYS = (("row", "exp_avg_sq_row"), ("col", "exp_avg_sq_col"), ("v", "exp_avg_sq"))
CASES = dict(SETTINGS, pre_scale=dict(SETTINGS["kohya"]), pre_scale_clip=dict(SETTINGS["kohya"]),
             clip_threshold_4=dict(SETTINGS["kohya"], clip_threshold=4.0))


def pad64(n):
    return (n + 63) // 64 * 64


def layout(shapes):
    tensors, n = [], 0
    for s in shapes:
        tensors.append((n, tuple(s)))
        n += pad64(math.prod(s))
    return tensors, n


def grads_for(step, seed=0):
    gs = make_grads(SHAPES, step, seed)
    gs[ZERO][...] = 0.0
    gs[HOLES][5, :] = 0.0
    gs[HOLES][:, 100] = 0.0
    return gs


def flat_of(arrays, tensors, n, fill=0.0):
    out = np.full(n, fill, np.float32)
    for a, (off, shape) in zip(arrays, tensors):
        out[off:off + a.size] = a.reshape(-1)
    return out


def make(kw, shadow=False, gap=0.0, shapes=SHAPES):
    from uwudiff_amd.optim import FusedAdafactor

    tensors, n = layout(shapes)
    p = torch.nn.Parameter(torch.from_numpy(flat_of(make_params(shapes), tensors, n, gap)).cuda())
    if shadow:
        p._uwu_bf16_shadow = torch.full((n,), 7.0, dtype=torch.bfloat16, device="cuda")
    return FusedAdafactor([p], tensors=tensors, **kw), p, tensors, n


def set_grad(p, arrays, tensors, n, gap=0.0):
    p.grad = torch.from_numpy(flat_of(arrays, tensors, n, gap)).cuda()


def snapshot(opt, p, tensors, beta1=None):
    """the oracle's list of tensors from the device: p and the state in fp64, 2-D tensors in their [R, C] view"""
    flat = p.detach().cpu().numpy().astype(np.float64)
    st = {k: v.cpu().numpy().astype(np.float64) for k, v in opt.state[p].items() if torch.is_tensor(v)}
    out, o = [], dict(row=0, col=0, v=0)
    for off, shape in tensors:
        view = AO.view2d(shape)
        d = dict(p=flat[off:off + math.prod(shape)].reshape(view or shape))
        if not st:
            d.update(AO.new_state(d["p"], beta1))
        else:
            for a, k in KEYS:
                if (a == "v") == (view is None):
                    ln = d["p"].shape[0] if a != "col" else d["p"].shape[1]
                    d[a] = st[k][o[a]:o[a] + ln]
                    o[a] += ln
            if "exp_avg" in st:
                d["m"] = st["exp_avg"][off:off + math.prod(shape)].reshape(d["p"].shape)
        out.append(d)
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def all_bits(opt, p):
    return [bits(p)] + [bits(v) for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", list(CASES))
def test_steps_follow_the_oracle(case):
    kw = CASES[case]
    pre_scale = 0.25 if case.startswith("pre_scale") else 1.0
    clip = torch.tensor([0.0, 0.5], device="cuda") if case == "pre_scale_clip" else None
    gscale = float(np.float32(pre_scale) * np.float32(0.5 if clip is not None else 1.0))
    opt, p, tensors, n = make(kw)
    p0 = p.detach().clone()
    worst = dict(p=0.0, state=0.0, m=0.0, m_rel=0.0)
    for step in range(1, 11):
        gs = grads_for(step)
        set_grad(p, gs, tensors, n)
        prev = snapshot(opt, p, tensors, kw.get("beta1"))
        want = AO.adafactor_step([dict(d, g=g.astype(np.float64).reshape(d["p"].shape)) for d, g in zip(prev, gs)], step,
                                 gscale=gscale, **kw)
        opt.step(pre_scale=pre_scale, clip=clip)
        got = snapshot(opt, p, tensors, kw.get("beta1"))
        assert opt.state[p]["step"] == step
        for i, (a, w) in enumerate(zip(got, want)):
            assert all(np.isfinite(v).all() for v in a.values()), (step, i)
            np.testing.assert_allclose(a["p"], w["p"], rtol=1e-5, atol=1e-6, err_msg=f"p of tensor {i} at step {step}")
            worst["p"] = max(worst["p"], float(np.max(np.abs(a["p"] - w["p"]) / np.maximum(np.abs(w["p"]), 1e-3))))
            for k in ("row", "col", "v"):
                if k in w:
                    np.testing.assert_allclose(a[k], w[k], rtol=1e-5, atol=0, err_msg=f"{k} of tensor {i} at step {step}")
                    worst["state"] = max(worst["state"], float(np.max(np.abs(a[k] - w[k]) / np.abs(w[k]))))
            if "m" in w:
                scaled, rel = exp_avg_dev(a["m"], w["m"])
                worst["m"], worst["m_rel"] = max(worst["m"], scaled), max(worst["m_rel"], rel)
                assert scaled <= 4 * EXP_AVG_FLOOR, f"exp_avg of tensor {i} at step {step}: {scaled:.3e} of its largest value"
            # the clip does what the case is about, judged on the oracle's RMS(u)
            if i == ZERO:
                assert w["rms_u"] == 0.0
            elif kw.get("clip_threshold") == 0.5:
                assert w["rms_u"] > 0.5, (step, i, w["rms_u"])
            elif kw.get("clip_threshold") == 4.0:
                assert w["rms_u"] < 4.0, (step, i, w["rms_u"])
        if kw.get("scale_parameter", True):
            np.testing.assert_allclose(opt.state[p]["RMS"].cpu().numpy()[:len(want)], [w["rms_p"] for w in want], rtol=1e-5)
    print(f"\n{case}: largest relative deviation from the oracle over 10 steps  p {worst['p']:.3e}  second moments {worst['state']:.3e}")
    if "beta1" in kw:
        print(f"{case}: exp_avg  largest |diff| / max|exp_avg| of the tensor {worst['m']:.3e} (bar {4 * EXP_AVG_FLOOR:.3e})  "
              f"largest element-wise relative {worst['m_rel']:.3e}")
    off, shape = tensors[ZERO]
    moved = not torch.equal(bits(p)[off:off + 4096], bits(p0)[off:off + 4096])
    assert moved == bool(kw.get("weight_decay"))  # the tensor without gradient moves by the weight decay alone
    gaps = np.ones(n, bool)
    for o, s in tensors:
        gaps[o:o + math.prod(s)] = False
    assert not p.detach().cpu().numpy()[gaps].any()


# ------------------------------------------------------------------------------------------------------------ side effects
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_grad", "zero_grad"])
def test_side_effects(zero_grad):
    kw = dict(SETTINGS["beta1"])
    opt, p, tensors, n = make(kw, shadow=True, gap=123.0)
    inside = np.zeros(n, bool)
    for o, s in tensors:
        inside[o:o + math.prod(s)] = True
    for step in (1, 2):
        set_grad(p, grads_for(step), tensors, n, gap=float("nan"))  # nothing may read the gaps
        g0 = bits(p.grad)
        opt.step(zero_grad=zero_grad)
        g1 = p.grad.detach().cpu().numpy()
        if zero_grad:
            assert not g1[inside].any() and np.isnan(g1[~inside]).all()
        else:
            assert torch.equal(bits(p.grad), g0)
    flat, shadow = p.detach().cpu(), p._uwu_bf16_shadow.cpu()
    assert torch.isfinite(flat).all() and torch.isfinite(shadow.float()).all()
    assert all(torch.isfinite(v).all() for v in opt.state[p].values() if torch.is_tensor(v))
    m = torch.from_numpy(inside)
    assert torch.equal(shadow[m], flat[m].bfloat16())
    assert (flat[~m] == 123.0).all() and (shadow[~m].float() == 7.0).all()  # the gaps are never written
    assert not opt.state[p]["exp_avg"].cpu()[~m].any()


# ------------------------------------------------------------------------------------------------------------ determinism
def _run(kw, chunks=None, steps=3):
    opt, p, tensors, n = make(kw, shadow=True)
    for step in range(1, steps + 1):
        set_grad(p, grads_for(step), tensors, n)
        opt.step(chunks=chunks(n) if chunks else None, zero_grad=True)
    return all_bits(opt, p) + [p._uwu_bf16_shadow.cpu().view(torch.int16)]


@pytest.mark.parametrize("setting", ["defaults", "beta1"])
def test_runs_and_chunkings_agree_bit_for_bit(setting):
    kw = SETTINGS[setting]
    a, b = _run(kw), _run(kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))

    def chunks(n):  # cuts inside tensors (multiples of 4 elements, not of 64), handed over last chunk first
        cuts = [0, 100, 2500, 9000, 9004, 13000, 20000, n]
        return [(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])][::-1]

    c = _run(kw, chunks)
    assert len(a) == len(c) and all(torch.equal(x, y) for x, y in zip(a, c))


def test_state_dict_round_trips_every_key():
    """``state_dict()`` -> a fresh optimizer -> ``load_state_dict()`` -> two more steps equal the uninterrupted run bit for bit, on the
    parity layout with ``beta1`` and ``scale_parameter``: factored and 1-D tensors, a first moment and a written ``RMS``."""
    import copy

    kw = dict(SETTINGS["beta1"])  # (defaults otherwise: relative_step, scale_parameter)
    keys = {"step", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg", "RMS"}
    opt, p, tensors, n = make(kw, shadow=True)
    for step in (1, 2, 3):
        set_grad(p, grads_for(step), tensors, n)
        opt.step(zero_grad=True)
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == keys and sd["state"][0]["step"] == 3
    assert all(float(sd["state"][0][k].abs().max()) > 0 for k in keys - {"step"})  # every key carries something that moved
    assert sd["param_groups"][0]["lr"] is None and sd["param_groups"][0]["beta1"] == 0.9
    opt2, p2, _, _ = make(kw, shadow=True)
    with torch.no_grad():
        p2.copy_(p)
        p2._uwu_bf16_shadow.copy_(p._uwu_bf16_shadow)
    saved = {k: v.clone() for k, v in sd["state"][0].items() if torch.is_tensor(v)}  # (load_state_dict may adopt sd's tensors)
    opt2.load_state_dict(sd)
    st2 = opt2.state[p2]
    assert set(st2) == keys and st2["step"] == 3
    for k in keys - {"step"}:
        assert st2[k].dtype == torch.float32 and st2[k].is_cuda and torch.equal(bits(st2[k]), bits(saved[k])), k
    for step in (4, 5):
        for o, q in ((opt, p), (opt2, p2)):
            set_grad(q, grads_for(step), tensors, n)
            o.step(zero_grad=True)
    a, b = all_bits(opt, p), all_bits(opt2, p2)
    assert len(a) == len(b) == 6 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert opt.state[p]["step"] == opt2.state[p2]["step"] == 5
    assert all(not torch.equal(bits(st2[k]), bits(saved[k])) for k in saved)  # steps 4-5 did move every key
    assert torch.equal(p2._uwu_bf16_shadow, p._uwu_bf16_shadow)


def test_partly_covered_tensors_are_an_error():
    opt, p, tensors, n = make(SETTINGS["kohya"])
    set_grad(p, grads_for(1), tensors, n)
    with pytest.raises(ValueError, match="partly covered"):
        opt.step(chunks=[(0, 9000)])  # ends inside [33, 257]


def test_the_launch_count_does_not_depend_on_the_number_of_tensors(monkeypatch):
    from uwudiff_amd import lib

    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    counts = []
    for k in (3, 300):
        shapes = [(5, 9), (70,), (3, 130)] * (k // 3)
        opt, p, tensors, n = make(SETTINGS["defaults"], shapes=shapes)
        p.grad = torch.randn(n, device="cuda")
        opt.step()  # (the first step also allocates the state: fills, no adafactor launches)
        del calls[:]
        p.grad = torch.randn(n, device="cuda")
        opt.step()
        counts.append([c for c in calls if c.startswith("uwu_adafactor_")])
        assert torch.isfinite(p.detach()).all()
    assert counts[0] == counts[1] == ["uwu_adafactor_stats", "uwu_adafactor_norm", "uwu_adafactor_apply"]


def test_a_nan_gradient_shows_in_its_tensor_alone():
    opt, p, tensors, n = make(SETTINGS["defaults"])
    bad = SHAPES.index((130, 7))
    for step in (1, 2):
        gs = grads_for(step)
        if step == 2:
            gs[bad][17, 3] = np.nan
        set_grad(p, gs, tensors, n)
        opt.step()
    flat = p.detach().cpu()
    for i, (off, shape) in enumerate(tensors):
        part = flat[off:off + math.prod(shape)]
        assert torch.isnan(part).all() if i == bad else torch.isfinite(part).all(), i


# ------------------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_and_touch_nothing():
    from uwudiff_amd import lib as L

    kw = dict(SETTINGS["beta1"])
    opt, p, tensors, n = make(kw, shadow=True)
    set_grad(p, grads_for(1), tensors, n)
    opt.step()
    set_grad(p, grads_for(2), tensors, n)
    st, dev = opt.state[p], opt._dev
    host_list, dev_list = opt._launch_list(dev, list(range(len(tensors))))

    def desc(**over):
        d = L.AdafactorDesc()
        d.p, d.g, d.p_bf16 = L.ptr(p.data), L.ptr(p.grad), L.ptr(p._uwu_bf16_shadow)
        d.row, d.col, d.v = L.ptr(st["exp_avg_sq_row"]), L.ptr(st["exp_avg_sq_col"]), L.ptr(st["exp_avg_sq"])
        d.m, d.rms, d.fws, d.dws = L.ptr(st["exp_avg"]), L.ptr(st["RMS"]), L.ptr(dev["fws"]), L.ptr(dev["dws"])
        d.table_host, d.table, d.ntensors = dev["host"].data_ptr(), L.ptr(dev["table"]), len(tensors)
        d.n, d.n_row, d.n_col, d.n_v = n, st["exp_avg_sq_row"].numel(), st["exp_avg_sq_col"].numel(), st["exp_avg_sq"].numel()
        d.n_fws, d.n_dws = dev["fws"].numel(), dev["dws"].numel()
        for k, v in over.items():
            setattr(d, k, v)
        return d

    watched = [p.data, p.grad, p._uwu_bf16_shadow.view(torch.int16), st["exp_avg_sq_row"], st["exp_avg_sq_col"], st["exp_avg_sq"],
               st["exp_avg"], st["RMS"]]
    before = [w.clone() for w in watched]
    lib = L.load()
    nready = len(tensors)

    def calls(d, host=host_list, devl=dev_list, nr=nready, clip_threshold=1.0, beta1=0.9, apply_only=False):
        ref = ctypes.byref(d) if d is not None else None
        hp = host.data_ptr() if host is not None else None
        dp = L.ptr(devl) if devl is not None else None
        first = [] if apply_only else [lib.uwu_adafactor_stats(ref, hp, dp, nr, 0.3, 1e-30, 1, 1.0, None, L.stream()),
                                       lib.uwu_adafactor_norm(ref, hp, dp, nr, 1.0, None, L.stream())]
        return first + [lib.uwu_adafactor_apply(ref, hp, dp, nr, 1e-3, 1e-3, clip_threshold, 1, 1, beta1, 0.0, 1.0, None, 1,
                                                L.stream())]

    outside = dev["host"].clone()
    outside[-1, 0] = n - 4  # the last tensor (1000 elements) now leaves the buffer
    overlap = dev["host"].clone()
    overlap[3, 0] = overlap[2, 0]
    misaligned = dev["host"].clone()
    misaligned[-1, 0] += 2
    wrong_starts = host_list.clone()
    wrong_starts[nready + 1] += 1
    every = [
        ("null descriptor", calls(None), 3),
        ("null p", calls(desc(p=None)), 3),
        ("null gradient", calls(desc(g=None)), 3),
        ("null table", calls(desc(table=None)), 3),
        ("null launch list", calls(desc(), devl=None), 3),
        ("no tensors", calls(desc(), nr=0), 3),
        ("row outside the buffer", calls(desc(table_host=outside.data_ptr())), 3),
        ("shorter buffer", calls(desc(n=n - 64)), 3),
        ("shorter row state", calls(desc(n_row=5)), 3),
        ("shorter workspace", calls(desc(n_fws=10)), 3),
        ("overlap", calls(desc(table_host=overlap.data_ptr())), 3),
        ("misaligned offset", calls(desc(table_host=misaligned.data_ptr())), 3),
        ("wrong workgroup starts", calls(desc(), host=wrong_starts), 3),
    ]
    for what, rcs, n_bad in every:
        assert sum(rc != 0 for rc in rcs) == n_bad, (what, rcs)
        assert lib.uwu_last_error()
    # what only the apply pass is given (the two passes before it would run with these descriptors)
    assert calls(desc(), clip_threshold=0.0, apply_only=True) != [0] and b"clip_threshold" in lib.uwu_last_error()
    assert calls(desc(), clip_threshold=-1.0, apply_only=True) != [0]
    assert calls(desc(), beta1=1.0, apply_only=True) != [0] and b"beta1" in lib.uwu_last_error()
    assert calls(desc(), beta1=-0.1, apply_only=True) != [0]
    assert calls(desc(m=None), apply_only=True) != [0]
    torch.cuda.synchronize()
    for w, b in zip(watched, before):
        assert torch.equal(bits(w) if w.element_size() == 4 else w, bits(b) if b.element_size() == 4 else b)
    with pytest.raises(L.UwuError, match="bfloat16"):
        p._uwu_bf16_shadow = torch.zeros(n, dtype=torch.float16, device="cuda")
        opt.step()


# ------------------------------------------------------------------------------------------------------------ the fit loop
LR = 3e-4  # without the parameter scale every element moves by about lr per step (RMS(u) is clipped to 1): 1e-3 overshoots the DiT


def _fit_cfg(tmp_path, steps, clip=None, n_acc=1, lyc=False, unet=None, lr=LR, monitor=False, opt_config=None, trainer=None):
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import LearningRateMonitor

    node = load_yaml(os.path.join(ROOT, "configs", "demo_training_adafactor.yaml"))["trainer"]
    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1, "gradient_clip_val": clip,
                                 "default_root_dir": str(tmp_path), "accumulate_grad_batches": n_acc},
            "data": {"dataset_config": {"n_samples": 8}, "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": lr, "optimizer": node["optimizer"], "opt_config": dict(node["opt_config"])}}
    if lyc or unet is not None:  # the tiny UNet's config (adapters are the UNet's) with the optimizer node of the Adafactor config
        base = "demo_training.yaml"
        over["data"]["dataset_config"]["sample_size"] = [3, 32, 32]
        over["trainer"]["lycoris_config"] = TOML if lyc else None
        if unet is not None:
            over["trainer"]["model_config"] = {"unet": {"_target_": unet}}
    else:
        base = "demo_training_adafactor.yaml"
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", base)), over)
    cfg["trainer"]["opt_config"] = dict(node["opt_config"] if opt_config is None else opt_config)  # (merge would keep the betas)
    cfg["trainer"].update(trainer or {})
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    if monitor:
        lc["callbacks"] = [LearningRateMonitor(logging_interval="step")]
    return cfg, lc


def _fresh(tmp_path, steps, **kw):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, steps, **kw)
    seed_everything(cfg.seed)
    fit = Fitter(**lc)
    dm, tr = load_all(cfg)
    return fit, dm, tr


@pytest.mark.parametrize("clip, n_acc", [(None, 1), (1.0, 1), (None, 2)], ids=["noclip", "clip", "accumulate2"])
def test_fitter_trains_the_dit(tmp_path, clip, n_acc):
    from uwudiff_amd.dit import DiT
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdafactor, adafactor_state_elems, flat_tensors

    steps = 12
    fit, dm, tr = _fresh(tmp_path, steps, clip=clip, n_acc=n_acc, monitor=True)
    assert isinstance(tr.unet, DiT) and tr.unet.cfg.hidden == 384 and tr.unet.cfg.depth == 12  # DiT-S/2
    flat0 = tr.unet.flat.detach().clone()

    def after_step(f):
        assert not tr.unet.flat.grad.any()  # left zeroed by the apply pass

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert isinstance(optim, FlatFusedOptimizer) and type(optim) is FusedAdafactor
    assert fit.global_step == steps and len(hist) == steps and all(math.isfinite(h["loss"]) for h in hist)
    # (the config's cosine schedule has moved lr by parts in 1e9 after a dozen steps; lr_t is what the last step used)
    assert all(abs(h["lr"] - LR) < 1e-9 and abs(h["lr_t"] - LR) < 1e-9 for h in hist)
    flat = tr.unet.flat.detach()
    assert torch.isfinite(flat).all() and float((flat - flat0.to(flat.device)).abs().max()) > 0
    assert torch.equal(tr.unet.shadow, flat.bfloat16())
    st = optim.state[tr.unet.flat]
    elems = adafactor_state_elems(flat_tensors(tr.unet))
    assert set(st) == {"step", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "RMS"} and st["step"] == steps
    for k, v in elems.items():
        assert st[k].shape == (v,) and st[k].dtype == torch.float32 and torch.isfinite(st[k]).all()
    assert all(float(st[k].min()) > 0 for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"))
    losses = [h["loss"] for h in hist]
    print(f"\nlosses: {[round(x, 4) for x in losses]}")
    assert sum(losses[-4:]) < sum(losses[:4])  # the loss falls


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def test_fitter_runs_the_relative_step(tmp_path):
    """The package's defaults through ``Fitter.fit``: ``lr: null`` with no scheduler and no warm-up.  The None survives the loop, the
    log records and the checkpoint; ``lr_t`` is the host's step size of each step; a resumed run continues from the saved ``step``."""
    from uwudiff_amd.optim import FusedAdafactor

    null_lr = dict(lr=None, opt_config={}, trainer={"lr_scheduler": None, "use_warm_up": False})
    path = str(tmp_path / "step2.ckpt")
    fit, dm, tr = _fresh(tmp_path, 3, monitor=True, **null_lr)
    fit.step_hooks.append(lambda f: f.save_checkpoint(path) if f.global_step == 2 else None)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedAdafactor and fit._fit_state[2] is None  # no scheduler
    g = optim.param_groups[0]
    assert g["lr"] is None and g["relative_step"] and g["scale_parameter"]
    assert len(hist) == 3 and all(h["lr"] is None and math.isfinite(h["loss"]) for h in hist)
    assert [h["lr_t"] for h in hist] == [min(1e-2, 1.0 / math.sqrt(t)) for t in (1, 2, 3)]
    st = optim.state[tr.unet.flat]
    assert st["step"] == 3 and float(st["RMS"].max()) > 0 and torch.isfinite(tr.unet.flat.detach()).all()
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["lr_schedulers"] == [] and ck["optimizer_states"][0]["param_groups"][0]["lr"] is None
    assert ck["optimizer_states"][0]["state"][0]["step"] == 2
    fit2, dm2, tr2 = _fresh(tmp_path, 3, monitor=True, **null_lr)
    hist2 = fit2.fit(tr2, dm2, ckpt_path=path)
    opt2 = fit2._fit_state[1]
    assert fit2.global_step == 3 and len(hist2) == 1 and hist2[0]["lr"] is None and hist2[0]["lr_t"] == 1e-2
    assert opt2.param_groups[0]["lr"] is None and opt2.state[tr2.unet.flat]["step"] == 3
    assert torch.isfinite(tr2.unet.flat.detach()).all()


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after step 3, resume in fresh objects, steps 4-5: parameters and every state tensor equal the uninterrupted run's bit
    for bit (on the denoiser whose gradient is bit-reproducible; its (3, 1, 1) and (3, 32, 32) tensors are factored)."""
    from uwudiff_amd.engine import seed_everything

    path = str(tmp_path / "step3.ckpt")
    unet = f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser"
    keys = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "RMS")

    def save_at_3(f):
        if f.global_step == 3:
            f.save_checkpoint(path)
            seed_everything(777)

    fit, dm, tr = _fresh(tmp_path, 5, unet=unet)
    fit.step_hooks.append(save_at_3)
    fit.fit(tr, dm)
    fit2, dm2, tr2 = _fresh(tmp_path, 5, unet=unet)
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        st = fit2._fit_state[1].state[tr2.unet.flat]
        loaded.update({k: v.clone() if torch.is_tensor(v) else v for k, v in st.items()})
        loaded["flat"] = tr2.unet.flat.detach().clone()
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert fit.global_step == 5 and fit2.global_step == 5 and len(hist_b) == 2
    assert isinstance(tr.unet, ElementwiseDenoiser) and isinstance(tr2.unet, ElementwiseDenoiser)
    ck_st = torch.load(path, map_location="cpu", weights_only=True)["optimizer_states"][0]["state"][0]
    assert set(ck_st) == set(keys) | {"step"} and ck_st["step"] == loaded["step"] == 3
    for k in keys:
        assert ck_st[k].dtype == torch.float32 and _same_bits(loaded[k], ck_st[k]), k
    st_a, st_b = fit._fit_state[1].state[tr.unet.flat], fit2._fit_state[1].state[tr2.unet.flat]
    assert float((loaded["flat"] - tr2.unet.flat.detach()).abs().max()) > 0  # steps 4-5 did move them
    assert _same_bits(tr2.unet.flat.detach(), tr.unet.flat.detach())
    for k in keys:
        assert _same_bits(st_b[k], st_a[k]), k
    for k in keys[:2]:  # (every tensor of this denoiser is factored: there is no 1-D state to move)
        assert not _same_bits(st_b[k], loaded[k]), k
    assert st_b["step"] == st_a["step"] == 5
    assert torch.equal(tr2.unet.shadow, tr2.unet.flat.detach().bfloat16())


def test_adapters_train(tmp_path):
    from uwudiff_amd.optim import FusedAdafactor, flat_tensors

    fit, dm, tr = _fresh(tmp_path, 3, clip=1.0, lyc=True)
    base0 = tr.unet.flat.detach().clone()
    ad0 = tr.lycoris_model.flat.detach().clone()

    def after_step(f):
        assert not tr.lycoris_model.flat.grad.any()

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedAdafactor and list(optim.state) == [tr.lycoris_model.flat]
    assert len(optim.tensors) == len(flat_tensors(tr.lycoris_model)) and any(r for _, (r, c) in optim.tensors)
    assert fit.global_step == 3 and all(math.isfinite(h["loss"]) for h in hist)
    ad = tr.lycoris_model.flat.detach()
    assert torch.isfinite(ad).all() and float((ad - ad0.to(ad.device)).abs().max()) > 0
    assert torch.equal(tr.unet.flat.detach().cpu(), base0.cpu()) and tr.unet.flat.grad is None


def test_the_adafactor_config_loads_and_trains():
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything
    from uwudiff_amd.optim import FusedAdafactor

    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_adafactor.yaml")),
                {"lightning_config": {"fast_dev_run": False, "max_steps": 2, "log_every_n_steps": 1},
                 "data": {"dataloader_config": {"num_workers": 0}}})
    fit = Fitter(**cfg["lightning_config"])
    dm, tr = load_all(cfg)
    seed_everything(cfg.seed)
    hist = fit.fit(tr, dm)
    assert type(fit._fit_state[1]) is FusedAdafactor
    assert fit.global_step == 2 and all(math.isfinite(h["loss"]) for h in hist)
