"""GPU tests of weight averaging: ``uwu_ema_update`` against the float64 recurrence under a derived bound,
``uwu_ema_swap`` bit for bit (special values included), their refusals, and the callbacks of uwudiff_amd/averaging.py through
``Fitter``: the average over the optimizer steps, validation on the averaged weights, checkpoints and resume, adapters, the launcher."""
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

S_A, S_P, S_SH = 7.0, 3.0, 9.0  # sentinels around the launched range
SHAPES = [(0, 1), (0, 5), (0, 8), (0, 100_003), (4, 3), (4, 7), (4, 4 * 515 + 3)]  # the optimizer entry points' edge shapes
ULP = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _same_bits(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().cpu().contiguous().view(view), b.detach().cpu().contiguous().view(view))


def _outside(buf, r, sentinel):
    a = buf.detach().float().cpu().numpy()
    out = np.ones(a.size, bool)
    out[r] = False
    return bool((a[out] == sentinel).all())


# ---------------------------------------------------------------------------------------------------------- uwu_ema_update
def _run_updates(off, ln, coefs, seed):
    """K successive updates with a fresh p each; returns the largest |got - want| / (3 K 2^-24 M) over the elements, want = the same
    recurrence in float64 on the fp32-rounded coefficients, M = the largest magnitude any avg or p took over the run"""
    from uwudiff_amd import lib as L

    rng = np.random.default_rng(seed)
    N, r = off + ln + 9, slice(off, off + ln)
    avg = np.full(N, S_A, np.float32)
    avg[r] = rng.standard_normal(ln)
    d_avg = _dev(avg)
    want = avg[r].astype(np.float64)
    M = float(np.abs(want).max())
    for keep, take in coefs:
        p = np.full(N, S_P, np.float32)
        p[r] = rng.standard_normal(ln) * 2.0
        d_p = _dev(p)
        L.call("uwu_ema_update", d_avg.data_ptr() + 4 * off, d_p.data_ptr() + 4 * off, ln, keep, take, L.stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits32(d_p), p.view(np.uint32))  # p is only read
        want = float(np.float32(keep)) * want + float(np.float32(take)) * p[r].astype(np.float64)
        M = max(M, float(np.abs(p[r]).max()), float(np.abs(want).max()))
    got = d_avg.cpu().numpy()
    assert _outside(d_avg, r, S_A)
    bound = 3 * len(coefs) * ULP * M
    err = float(np.abs(got[r].astype(np.float64) - want).max())
    print(f"ema_update off {off} len {ln}: max |got - want| {err:.3e}, bound 3 K 2^-24 M = {bound:.3e} (K {len(coefs)}, M {M:.3f})")
    assert np.isfinite(got[r]).all() and err <= bound
    return err


@pytest.mark.parametrize("off,ln", SHAPES)
def test_ema_update_matches_the_float64_recurrence(off, ln):
    """A step rounds three times at most (keep * avg, take * p, their sum; the kernel's fused multiply-add makes it two) quantities no
    larger than M, and scales the inherited error by keep < 1: |got - want| <= 3 K 2^-24 M after K steps."""
    _run_updates(off, ln, [(0.9, 1 - 0.9)] * 4, seed=21)


@pytest.mark.parametrize("off,ln", SHAPES)
def test_ema_update_running_mean_coefficients(off, ln):
    _run_updates(off, ln, [(n / (n + 1), 1 / (n + 1)) for n in range(4)], seed=22)


# ---------------------------------------------------------------------------------------------------------- uwu_ema_swap
SPECIAL = np.array([0x7fc00000, 0x7fc00001, 0x7f800001, 0xffc12345, 0xff8abcde, 0x7fffffff, 0x00000000, 0x80000000, 0x7f800000,
                    0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x00800000, 0x3f800000, 0xbf808000, 0x3f808000, 0x3f818000,
                    0x7f7fffff, 0xff7fffff], dtype=np.uint32)  # NaNs with payloads, +-0, +-inf, subnormals, bf16 ties, the largest


def _swap_buffers(off, ln, seed):
    rng = np.random.default_rng(seed)
    N, r = off + ln + 9, slice(off, off + ln)
    a = np.full(N, S_A, np.float32)
    p = np.full(N, S_P, np.float32)
    a[r] = rng.standard_normal(ln)
    p[r] = rng.standard_normal(ln) * 1e-3
    ab, pb = a.view(np.uint32), p.view(np.uint32)
    k = min(ln, SPECIAL.size)
    ab[off:off + k] = SPECIAL[:k]  # (every special value meets an ordinary one and, shifted, another special one)
    pb[off + ln - k:off + ln] = SPECIAL[::-1][:k]
    return N, r, ab.copy(), pb.copy()


def _cast_bits(p_range):
    """what uwu_cast_f32_to_bf16 makes of a contiguous fp32 tensor"""
    from uwudiff_amd import lib as L

    src = p_range.contiguous().clone()
    dst = torch.empty(src.numel(), device="cuda", dtype=torch.bfloat16)
    L.call("uwu_cast_f32_to_bf16", L.ptr(src), L.ptr(dst), src.numel(), L.stream())
    return _bits16(dst)


@pytest.mark.parametrize("off,ln", SHAPES)
@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "null_shadow"])
def test_ema_swap_exchanges_bit_for_bit_and_is_its_own_inverse(off, ln, shadow):
    from uwudiff_amd import lib as L

    N, r, ab, pb = _swap_buffers(off, ln, 31)
    d_a, d_p = _dev(ab.view(np.int32)).view(torch.float32), _dev(pb.view(np.int32)).view(torch.float32)
    sh = torch.full((N,), S_SH, device="cuda", dtype=torch.bfloat16)
    shp = sh.data_ptr() + 2 * off if shadow else None
    L.call("uwu_ema_swap", d_a.data_ptr() + 4 * off, d_p.data_ptr() + 4 * off, shp, ln, 0, L.stream())
    torch.cuda.synchronize()
    got_a, got_p = _bits32(d_a), _bits32(d_p)
    assert np.array_equal(got_a[r], pb[r]) and np.array_equal(got_p[r], ab[r])
    out = np.ones(N, bool)
    out[r] = False
    assert np.array_equal(got_a[out], ab[out]) and np.array_equal(got_p[out], pb[out])
    if shadow:
        assert np.array_equal(_bits16(sh)[r], _cast_bits(d_p[r])) and _outside(sh, r, S_SH)
    else:
        assert bool((sh.float() == S_SH).all())
    L.call("uwu_ema_swap", d_a.data_ptr() + 4 * off, d_p.data_ptr() + 4 * off, shp, ln, 0, L.stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(d_a), ab) and np.array_equal(_bits32(d_p), pb)
    if shadow:
        assert np.array_equal(_bits16(sh)[r], _cast_bits(d_p[r])) and _outside(sh, r, S_SH)


@pytest.mark.parametrize("off,ln", SHAPES)
def test_ema_swap_mode_1_copies_the_average_into_the_weights(off, ln):
    from uwudiff_amd import lib as L

    N, r, ab, pb = _swap_buffers(off, ln, 32)
    d_a, d_p = _dev(ab.view(np.int32)).view(torch.float32), _dev(pb.view(np.int32)).view(torch.float32)
    sh = torch.full((N,), S_SH, device="cuda", dtype=torch.bfloat16)
    L.call("uwu_ema_swap", d_a.data_ptr() + 4 * off, d_p.data_ptr() + 4 * off, sh.data_ptr() + 2 * off, ln, 1, L.stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(d_a), ab)  # avg untouched
    got_p = _bits32(d_p)
    out = np.ones(N, bool)
    out[r] = False
    assert np.array_equal(got_p[r], ab[r]) and np.array_equal(got_p[out], pb[out])
    assert np.array_equal(_bits16(sh)[r], _cast_bits(d_a[r])) and _outside(sh, r, S_SH)
    d_p2 = _dev(pb.view(np.int32)).view(torch.float32)
    L.call("uwu_ema_swap", d_a.data_ptr() + 4 * off, d_p2.data_ptr() + 4 * off, None, ln, 1, L.stream())  # no shadow
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(d_p2), got_p) and np.array_equal(_bits32(d_a), ab)


def test_ema_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L

    a = torch.full((64,), S_A, device="cuda")
    p = torch.full((64,), S_P, device="cuda")
    sh = torch.full((64,), S_SH, device="cuda", dtype=torch.bfloat16)
    A, P, SH, s = a.data_ptr(), p.data_ptr(), sh.data_ptr(), L.stream()
    bad_update = [(None, P, 8), (A, None, 8), (A + 4, P, 8), (A, P + 8, 8), (A, P, -8), (A, P, 0)]
    for avg, pp, n in bad_update:
        with pytest.raises(L.UwuError, match="ema_update"):
            L.call("uwu_ema_update", avg, pp, n, 0.9, 0.1, s)
    bad_swap = [(None, P, SH, 8, 0), (A, None, SH, 8, 0), (A + 4, P, SH, 8, 0), (A, P + 12, SH, 8, 0), (A, P, SH + 2, 8, 0),
                (A, P, SH, -8, 0), (A, P, SH, 0, 1), (A, P, SH, 8, 2), (A, P, SH, 8, -1),
                (A, A, SH, 8, 0), (A, A, None, 8, 1),  # avg == p
                (A, A + 16, SH, 8, 0), (A + 32, A, SH, 16, 0), (A + 16, A, None, 5, 1)]  # overlapping ranges
    for avg, pp, shp, n, mode in bad_swap:
        with pytest.raises(L.UwuError, match="ema_swap"):
            L.call("uwu_ema_swap", avg, pp, shp, n, mode, s)
    torch.cuda.synchronize()
    assert bool((a == S_A).all()) and bool((p == S_P).all()) and bool((sh.float() == S_SH).all())
    L.call("uwu_ema_swap", A, A + 32, None, 8, 0, s)  # adjacent ranges of one buffer do not overlap
    L.call("uwu_ema_swap", A, A + 32, None, 8, 0, s)
    torch.cuda.synchronize()
    assert bool((a == S_A).all())


# ---------------------------------------------------------------------------------------------------------- FlatAverage
def test_flat_average_on_a_flat_module():
    from tests.test_optimizers_gpu import ElementwiseDenoiser
    from uwudiff_amd.averaging import FlatAverage

    m = ElementwiseDenoiser().cuda()
    avg = FlatAverage(m)
    assert avg.avg.dtype == torch.float32 and avg.avg.numel() == m.flat.numel() and avg.avg.device == m.flat.device
    assert _same_bits(avg.avg, m.flat.data) and avg.n_averaged == 0
    w0 = m.flat.detach().clone()
    ptrs = (m.flat.data_ptr(), m.shadow.data_ptr())
    with torch.no_grad():
        m.flat.mul_(2.0)
    m.refresh_shadow()
    w1 = m.flat.detach().clone()
    avg.update(0.25, 0.75)  # the first update is a copy, whatever the coefficients
    assert _same_bits(avg.avg, w1) and avg.n_averaged == 1
    with torch.no_grad():
        m.flat.copy_(w0)
    m.refresh_shadow()
    avg.update(0.25, 0.75)
    torch.testing.assert_close(avg.avg, 0.25 * w1 + 0.75 * w0, rtol=0, atol=4 * ULP * float(w1.abs().max()))
    held = avg.avg.clone()
    st = avg.averaged_state()
    assert list(st) == list(m.state_dict()) and all(_same_bits(v, dict(m._public_views(held))[k]) for k, v in st.items())
    avg.swap()
    assert _same_bits(m.flat.data, held) and _same_bits(avg.avg, w0) and _same_bits(m.shadow, held.bfloat16())
    assert (m.flat.data_ptr(), m.shadow.data_ptr()) == ptrs  # no pointer moved
    avg.swap()
    assert _same_bits(m.flat.data, w0) and _same_bits(avg.avg, held) and _same_bits(m.shadow, w0.bfloat16())
    avg.copy_to_current()
    assert _same_bits(m.flat.data, held) and _same_bits(avg.avg, held) and _same_bits(m.shadow, held.bfloat16())
    avg.load_averaged_state({k: v.cpu() * 3 for k, v in st.items()})
    assert all(torch.equal(v, st[k] * 3) for k, v in avg.averaged_state().items()) and _same_bits(m.flat.data, held)
    with pytest.raises(RuntimeError, match="missing"):
        avg.load_averaged_state({k: v for k, v in st.items() if k != "gate"})
    avg.reset()
    assert _same_bits(avg.avg, m.flat.data) and avg.n_averaged == 0


# ---------------------------------------------------------------------------------------------------------- the fit loop
def _latent_fit(root, callbacks, steps=4, n_acc=1, with_val=False, step_hook=None, wrap=None):
    """the DiT of configs/demo_training_latent.yaml at 4x32x32, batch 16, lr 1e-3 (the set-up of the validation and accumulation tests)"""
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    extra = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1, "accumulate_grad_batches": n_acc},
             "data": {"dataloader_config": {"num_workers": 0}}, "trainer": {"lr": 1e-3}}
    if with_val:
        extra["lightning_config"].update({"val_check_interval": 2, "check_val_every_n_epoch": None, "num_sanity_val_steps": 1})
        extra["data"]["val_dataset_config"] = {"_target_": "duwu.data.DummyDataset", "sample_size": [4, 32, 32], "n_samples": 40}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml")), extra)
    seed_everything(cfg.seed)
    fit = Fitter(callbacks=callbacks, default_root_dir=str(root), **cfg["lightning_config"])
    dm, tr = load_all(cfg)
    if step_hook is not None:
        fit.step_hooks.append(lambda f: step_hook(f, tr))
    if wrap is not None:
        wrap(fit, tr)
    hist = fit.fit(tr, dm)
    return fit, tr, hist


def _recurrence(clones, keep, take):
    """first update = copy, then the float64 recurrence on the fp32-rounded coefficients; (want, K kernel updates, M)"""
    want = clones[0].double()
    M = float(want.abs().max())
    for c in clones[1:]:
        want = float(np.float32(keep)) * want + float(np.float32(take)) * c.double()
        M = max(M, float(c.abs().max()), float(want.abs().max()))
    return want, len(clones) - 1, M


def _check_average(cb, clones, keep, take, what):
    want, K, M = _recurrence(clones, keep, take)
    err = float((cb.average.avg.double() - want).abs().max())
    print(f"{what}: max |average - float64 recurrence| {err:.3e}, bound 3 K 2^-24 M = {3 * K * ULP * M:.3e} (K {K}, M {M:.3f})")
    assert err <= 3 * K * ULP * M
    assert cb.average.n_averaged == len(clones)


def test_ema_over_four_optimizer_steps(tmp_path):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb, clones = EMAWeightAveraging(decay=0.5), []
    fit, tr, hist = _latent_fit(tmp_path, [cb], step_hook=lambda f, tr: clones.append(tr.unet.flat.detach().clone()))
    assert fit.global_step == 4 and len(clones) == 4 and cb.latest_update_step == 4
    assert float((clones[3] - clones[0]).abs().max()) > 0
    _check_average(cb, clones, 0.5, 0.5, "decay 0.5, 4 steps")
    assert cb.average.owner is tr.unet
    # the module fit returns holds the average, with a matching shadow
    assert _same_bits(tr.unet.flat.data, cb.average.avg) and not _same_bits(tr.unet.flat.data, clones[3])
    assert torch.equal(tr.unet.shadow, tr.unet.flat.detach().bfloat16())


@pytest.mark.parametrize("kw,n_acc,steps_updated", [({"update_every_n_steps": 2}, 1, [1, 3]), ({}, 2, [1, 2, 3, 4])],
                         ids=["every_2_steps", "accumulate_2"])
def test_updates_happen_at_the_optimizer_steps_the_rule_names(tmp_path, kw, n_acc, steps_updated):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb, clones, at = EMAWeightAveraging(decay=0.5, **kw), {}, []
    inner = cb._update

    def update():
        at.append((holder["fit"].global_step, holder["fit"].train_batches))
        return inner()

    cb._update = update
    holder = {}
    fit, tr, hist = _latent_fit(tmp_path, [cb], n_acc=n_acc, wrap=lambda f, tr: holder.update(fit=f),
                                step_hook=lambda f, tr: clones.update({f.global_step: tr.unet.flat.detach().clone()}))
    assert fit.global_step == 4 and fit.train_batches == 4 * n_acc and sorted(clones) == [1, 2, 3, 4]
    assert [g for g, _ in at] == steps_updated
    assert [b for _, b in at] == [g * n_acc for g in steps_updated]  # on the window's boundary batch, once
    _check_average(cb, [clones[g] for g in steps_updated], 0.5, 0.5, f"{kw} accumulate {n_acc}")
    assert _same_bits(tr.unet.flat.data, cb.average.avg) and torch.equal(tr.unet.shadow, tr.unet.flat.detach().bfloat16())


class _PassRecorder:
    """listed after the averaging callback: what the weights are inside a validation pass"""

    def __init__(self):
        self.inside = []

    def on_validation_epoch_start(self, trainer, pl_module):
        self.inside.append({"flat": pl_module.unet.flat.detach().clone(), "shadow": pl_module.unet.shadow.detach().clone(),
                            "sanity": trainer.sanity_checking, "step": trainer.global_step})


def _val_run(root, with_ema):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb, rec, around = EMAWeightAveraging(decay=0.9), _PassRecorder(), []

    def wrap(fit, tr):
        inner = fit.validate

        def snapshot():
            _, opt, _ = fit._fit_state
            gen = torch.cuda.default_generators[torch.cuda.current_device()]
            flat = tr.unet.flat
            return {"cuda_rng": (gen.initial_seed(), gen.get_offset()), "cpu_rng": torch.get_rng_state(), "flat": flat.detach().clone(),
                    "shadow": tr.unet.shadow.detach().clone(), "grad": None if flat.grad is None else flat.grad.detach().clone(),
                    "ema_loss": tr.ema_loss.detach().clone(), "opt_step": int(opt.state_dict()["state"][0]["step"]) if opt.state_dict()["state"] else 0,
                    "avg": cb.average.avg.detach().clone() if with_ema else None}

        def validate(module, loader, **kw):
            before = snapshot()
            out = inner(module, loader, **kw)
            around.append((before, snapshot()))
            return out

        fit.validate = validate

    fit, tr, hist = _latent_fit(root, [cb, rec] if with_ema else [rec], steps=5, with_val=True, wrap=wrap)
    return {"fit": fit, "tr": tr, "hist": hist, "rec": rec, "around": around, "cb": cb}


@pytest.fixture(scope="module")
def val_runs(tmp_path_factory):
    return {"ema": _val_run(tmp_path_factory.mktemp("ema"), True), "plain": _val_run(tmp_path_factory.mktemp("plain"), False)}


def test_validation_runs_on_the_averaged_weights(val_runs):
    r = val_runs["ema"]
    assert [(p["step"], p["sanity"]) for p in r["rec"].inside] == [(0, True), (2, False), (4, False)] and len(r["around"]) == 3
    for p, (before, _) in zip(r["rec"].inside, r["around"]):
        assert _same_bits(p["flat"], before["avg"]) and _same_bits(p["shadow"], before["avg"].bfloat16())
    for p, (before, _) in list(zip(r["rec"].inside, r["around"]))[1:]:
        assert not _same_bits(p["flat"], before["flat"])  # (the average is not the iterate once steps were taken)


def test_a_pass_on_the_average_leaves_training_where_it_was(val_runs):
    for before, after in val_runs["ema"]["around"]:
        assert before["cuda_rng"] == after["cuda_rng"] and torch.equal(before["cpu_rng"], after["cpu_rng"])
        for k in ("flat", "shadow", "avg", "ema_loss"):
            assert _same_bits(before[k], after[k]), k
        assert (before["grad"] is None) == (after["grad"] is None)
        if before["grad"] is not None:
            assert _same_bits(before["grad"], after["grad"])
        assert before["opt_step"] == after["opt_step"]


def test_training_losses_equal_the_run_without_the_callback(val_runs):
    a = [h["loss"] for h in val_runs["ema"]["hist"]]
    b = [h["loss"] for h in val_runs["plain"]["hist"]]
    print("max relative difference of the training losses:", max(abs(x - y) / abs(y) for x, y in zip(a, b)))
    # rel 1e-4: the project's bound on this config and lr for run-to-run differences from fp32 atomics (tests/test_validation_gpu.py)
    assert len(a) == len(b) == 5 and a == pytest.approx(b, rel=1e-4)
    va = [h["val/loss"] for h in val_runs["ema"]["fit"].val_history]
    vb = [h["val/loss"] for h in val_runs["plain"]["fit"].val_history]
    print("val/loss on the average:", va, "on the iterate:", vb)
    assert len(va) == len(vb) == 2 and all(x != y for x, y in zip(va, vb))


def test_a_pass_that_raises_still_swaps_back(tmp_path):
    from uwudiff_amd.averaging import EMAWeightAveraging

    class Boom:
        def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
            if not trainer.sanity_checking:
                self.inside = pl_module.unet.flat.detach().clone()
                raise RuntimeError("boom")

    cb, boom, clones = EMAWeightAveraging(decay=0.5), Boom(), []
    holder = {}
    with pytest.raises(RuntimeError, match="boom"):
        _latent_fit(tmp_path, [cb, boom], with_val=True, wrap=lambda f, tr: holder.update(tr=tr),
                    step_hook=lambda f, tr: clones.append(tr.unet.flat.detach().clone()))
    tr = holder["tr"]
    assert len(clones) == 2 and not cb._swapped
    assert _same_bits(tr.unet.flat.data, clones[1]) and _same_bits(boom.inside, cb.average.avg)
    assert torch.equal(tr.unet.shadow, clones[1].bfloat16())


# ---------------------------------------------------------------------------------------------------------- checkpoints
def _elementwise(tmp_path, callbacks, steps):
    from duwu.loader import load_all
    from tests.test_optimizers_gpu import ElementwiseDenoiser, _fit_cfg
    from uwudiff_amd.config import merge
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, "lion", steps)
    cfg = merge(cfg, {"trainer": {"model_config": {"unet": {"_target_": f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser"}}},
                      "data": {"dataloader_config": {"num_workers": 0}}})
    seed_everything(cfg.seed)
    fit = Fitter(callbacks=callbacks, **lc)
    dm, tr = load_all(cfg)
    assert isinstance(tr.unet, ElementwiseDenoiser)
    return fit, dm, tr


@pytest.fixture(scope="module")
def resumed(tmp_path_factory):
    """run A: 5 uninterrupted steps with the callback, a checkpoint written after step 3; run B: fresh objects resumed from that file
    (the RNG re-seeded at the same point of both, the pattern of tests/test_optimizers_gpu.py)"""
    from uwudiff_amd.averaging import EMAWeightAveraging
    from uwudiff_amd.engine import seed_everything

    tmp = tmp_path_factory.mktemp("resume")
    path = str(tmp / "step3.ckpt")
    at3, end = {}, {}

    def run(ckpt_path):
        cb = EMAWeightAveraging(decay=0.5)
        fit, dm, tr = _elementwise(tmp, [cb], 5)
        key = "b" if ckpt_path else "a"

        def hook(f):
            if f.global_step == 3 and not ckpt_path:
                at3["avg"] = cb.average.averaged_state()
                at3["weights"] = tr.unet.state_dict()
                at3["ptrs"] = (tr.unet.flat.data_ptr(), cb.average.avg.data_ptr())
                f.save_checkpoint(path)
                at3["ptrs_after"] = (tr.unet.flat.data_ptr(), cb.average.avg.data_ptr())
                at3["weights_after"] = tr.unet.state_dict()
                seed_everything(777)
            if f.global_step == 5:
                end[key] = tr.unet.flat.detach().clone()

        fit.step_hooks.append(hook)
        if ckpt_path:
            orig = fit.load_checkpoint

            def load_and_seed(p):
                out = orig(p)
                seed_everything(777)
                return out

            fit.load_checkpoint = load_and_seed
        hist = fit.fit(tr, dm, ckpt_path=ckpt_path)
        return {"fit": fit, "tr": tr, "cb": cb, "hist": hist}

    a = run(None)
    b = run(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    return {"a": a, "b": b, "ck": ck, "at3": at3, "end": end, "path": path, "tmp": tmp}


def test_checkpoint_carries_both_sets_of_weights_and_both_counters(resumed):
    ck, at3 = resumed["ck"], resumed["at3"]
    assert ck["averaging_state"] == {"n_averaged": 3} and ck["callbacks"]["WeightAveraging"] == {"latest_update_step": 3}
    assert ck["global_step"] == 3 and list(ck["state_dict"]) == list(ck["current_model_state"])
    unet_keys = [k for k in ck["state_dict"] if k.startswith("unet.")]
    assert [k[5:] for k in unet_keys] == list(at3["avg"])
    for k in unet_keys:
        assert _same_bits(ck["state_dict"][k], at3["avg"][k[5:]]), k
        assert _same_bits(ck["current_model_state"][k], at3["weights"][k[5:]]), k
    assert any(not _same_bits(ck["state_dict"][k], ck["current_model_state"][k]) for k in unet_keys)
    for k in ck["state_dict"]:
        if not k.startswith("unet."):  # buffers and the other sub-modules as they are
            assert _same_bits(ck["state_dict"][k], ck["current_model_state"][k]), k
    # no pointer swap and no weight write while saving
    assert at3["ptrs"] == at3["ptrs_after"] and all(_same_bits(v, at3["weights_after"][k]) for k, v in at3["weights"].items())


def test_resume_is_bit_identical_to_the_uninterrupted_run(resumed):
    a, b, end = resumed["a"], resumed["b"], resumed["end"]
    assert a["fit"].global_step == b["fit"].global_step == 5 and len(b["hist"]) == 2
    assert _same_bits(end["a"], end["b"])  # the trained weights after step 5
    assert _same_bits(a["cb"].average.avg, b["cb"].average.avg) and not _same_bits(end["a"], a["cb"].average.avg)
    assert a["cb"].latest_update_step == b["cb"].latest_update_step == 5
    assert a["cb"].average.n_averaged == b["cb"].average.n_averaged == 5
    for r in (a, b):  # fit returns the module holding the average
        assert _same_bits(r["tr"].unet.flat.data, r["cb"].average.avg)
        assert torch.equal(r["tr"].unet.shadow, r["tr"].unet.flat.detach().bfloat16())


def test_a_checkpoint_without_current_model_state_starts_the_average_from_the_loaded_weights(resumed, capsys):
    from uwudiff_amd.averaging import EMAWeightAveraging

    ck = dict(resumed["ck"])
    ck["state_dict"] = ck.pop("current_model_state")  # what a run without the callback writes
    del ck["averaging_state"]
    ck["callbacks"] = {}
    path = str(resumed["tmp"] / "plain.ckpt")
    torch.save(ck, path)

    class AtSetup:
        def setup(self, fitter, module, stage):
            self.flat, self.avg, self.n = module.unet.flat.detach().clone(), cb.average.avg.detach().clone(), cb.average.n_averaged

    cb, seen = EMAWeightAveraging(decay=0.5), AtSetup()
    fit, dm, tr = _elementwise(resumed["tmp"], [cb, seen], 3)  # (max_steps = the checkpoint's step: nothing is trained)
    capsys.readouterr()
    fit.fit(tr, dm, ckpt_path=path)
    out = capsys.readouterr().out
    assert "copy of the loaded weights" in out
    assert _same_bits(seen.flat, seen.avg) and seen.n == 0 and cb.latest_update_step == 0
    for k, v in tr.unet.state_dict().items():
        assert _same_bits(v, ck["state_dict"]["unet." + k]), k


def test_load_any_picks_up_the_averaged_denoiser(resumed):
    from duwu.loader import load_any
    from tests.test_optimizers_gpu import ElementwiseDenoiser

    model = load_any({"_target_": f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser",
                      "_load_config_": {"ckpt_path": resumed["path"], "state_dict_key": "state_dict", "state_dict_prefix": "unet."}})
    sd = model.state_dict()
    assert list(sd) == list(resumed["at3"]["avg"])
    for k, v in sd.items():
        assert _same_bits(v, resumed["at3"]["avg"][k]), k


# ---------------------------------------------------------------------------------------------------------- adapters
def test_adapters_are_what_is_averaged(tmp_path):
    """The UNet's forward is not reproducible to the bit on unchanged weights (its GroupNorm statistics add with fp32 atomics: see
    tests/test_lycoris_gpu.py::test_fresh_adapters_leave_output_unchanged), so "the second swap restores the output bit for bit" is
    asserted on everything the forward reads -- the adapter buffer, the merged effective fp32 weights, the whole bf16 shadow -- and the
    output is held to the forward's own run-to-run noise, measured in the same test on the same weights."""
    from duwu.loader import load_all
    from tests.test_optimizers_gpu import TOML, _fit_cfg
    from uwudiff_amd.averaging import EMAWeightAveraging
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, "lion", 2, clip=1.0, lyc=TOML)
    seed_everything(cfg.seed)
    cb = EMAWeightAveraging(decay=0.5)
    fit = Fitter(callbacks=[cb], **lc)
    dm, tr = load_all(cfg)
    base0 = tr.unet.flat.detach().clone()
    call, seen, clones = {}, {}, []

    def remember(mod, args, kwargs):
        if torch.is_grad_enabled():  # (the training forward's inputs, to run again below)
            call["args"], call["kwargs"] = args, kwargs

    tr.unet.register_forward_pre_hook(remember, with_kwargs=True)

    def forward():
        with torch.no_grad():
            out = tr.unet(*call["args"], **call["kwargs"])
        return (out[0] if isinstance(out, (tuple, list)) else getattr(out, "sample", out)).detach().clone()

    def merged():
        """what the last forward ran on: the fp32 buffer of merged effective weights and the whole bf16 shadow"""
        return {"eff": tr.unet.P.ad.eff.detach().clone(), "shadow": tr.unet.shadow.detach().clone()}

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def after_step(f):
        clones.append(tr.lycoris_model.flat.detach().clone())
        if f.global_step != 2:
            return
        lyc, avg = tr.lycoris_model, cb.average
        seen["w"], seen["avg"] = lyc.flat.detach().clone(), avg.avg.detach().clone()
        seen["y0"], seen["m0"] = forward(), merged()
        seen["y0b"] = forward()  # (the same weights again: the forward's own run-to-run noise)
        avg.swap()
        seen["swapped"] = (lyc.flat.detach().clone(), avg.avg.detach().clone())
        seen["y1"], seen["m1"] = forward(), merged()  # merges from the averaged adapters
        avg.swap()
        seen["y2"], seen["m2"] = forward(), merged()
        seen["base"] = tr.unet.flat.detach().clone()
        with torch.no_grad():  # the average written into the adapters by hand: what a merge from it gives
            lyc.flat.copy_(seen["avg"])
        lyc.mark_dirty()
        forward()
        seen["m_avg"] = merged()
        with torch.no_grad():
            lyc.flat.copy_(seen["w"])
        lyc.mark_dirty()

    fit.step_hooks.append(after_step)
    fit.fit(tr, dm)
    lyc = tr.lycoris_model
    assert cb.average.owner is lyc and cb.average.avg.numel() == lyc.flat.numel() != tr.unet.flat.numel()
    _check_average(cb, clones, 0.5, 0.5, "adapters, 2 steps")
    assert _same_bits(seen["swapped"][0], seen["avg"]) and _same_bits(seen["swapped"][1], seen["w"])
    assert not _same_bits(seen["w"], seen["avg"])
    # after a swap the forward ran on the adapters merged from the average; after the second on what it ran on before, bit for bit
    for nm in ("eff", "shadow"):
        assert _same_bits(seen["m1"][nm], seen["m_avg"][nm]), nm
        assert _same_bits(seen["m2"][nm], seen["m0"][nm]), nm
    assert any(not _same_bits(seen["m1"][nm], seen["m0"][nm]) for nm in ("eff", "shadow"))
    noise, moved, back = rel(seen["y0b"], seen["y0"]), rel(seen["y1"], seen["y0"]), rel(seen["y2"], seen["y0"])
    print(f"UNet output, relative L2 against the first forward: the same weights again {noise:.3e}, on the average {moved:.3e}, "
          f"swapped back {back:.3e}; bit-equal: again {torch.equal(seen['y0b'], seen['y0'])}, back {torch.equal(seen['y2'], seen['y0'])}")
    assert torch.isfinite(seen["y0"]).all() and not torch.equal(seen["y1"], seen["y0"])
    # the output itself comes back to the forward's own noise (bound: tests/test_lycoris_gpu.py, the bf16 floor 1e-3)
    assert back <= max(3 * noise, 1e-3)
    assert _same_bits(seen["base"], base0) and _same_bits(tr.unet.flat.data, base0) and tr.unet.flat.grad is None  # the frozen base
    assert _same_bits(lyc.flat.data, cb.average.avg)  # fit returns the averaged adapters
    st = cb.average.averaged_state()
    assert list(st) == list(lyc.state_dict()) and all(_same_bits(v, lyc.state_dict()[k]) for k, v in st.items())


# ---------------------------------------------------------------------------------------------------------- the launcher
def test_launcher_runs_the_ema_config(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_train.py"), "--configs",
                        os.path.join(ROOT, "configs", "demo_training_ema.yaml")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = sorted(glob.glob(str(tmp_path / "checkpoints" / "*.ckpt")))
    assert len(files) == 2, files  # the best two by val/loss of the two passes
    for f in files:
        ck = torch.load(f, map_location="cpu", weights_only=True)
        assert "current_model_state" in ck and list(ck["current_model_state"]) == list(ck["state_dict"])
        assert ck["averaging_state"]["n_averaged"] == ck["global_step"] == ck["callbacks"]["WeightAveraging"]["latest_update_step"]
        assert any(not _same_bits(ck["state_dict"][k], ck["current_model_state"][k]) for k in ck["state_dict"] if k.startswith("unet."))
        assert "ModelCheckpoint" in ck["callbacks"] and math.isfinite(float(ck["state_dict"]["ema_loss"]))
