"""GPU: the fused Prodigy optimizer (uwu_prodigy_stats / _finalize / _apply, csrc/optimizer_prodigy.hip; uwudiff_amd.optim.FusedProdigy)
against the fp64 restatement of tests/test_prodigy_cpu.py, one step at a time from the device's own previous state; the early
return, the shadow and the zeroed gradient, chunked launches and run-to-run determinism, argument refusals, the fit loop
(clip, accumulation, checkpoint resume), LyCORIS adapters and two ranks."""
import math
import os
import socket

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_optimizers_gpu import TOML, ElementwiseDenoiser, _same_bits
from tests.test_prodigy_cpu import DEFAULTS, Generator, fresh_scalars, prodigy_step

pytestmark = pytest.mark.gpu

D0 = 1e-6


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _state(opt, flat):
    """the device's state after a step: fp32 tensors as numpy and the scalar block as a dict (a host synchronisation)"""
    st = opt.state[flat]
    return {k: _np(st[k]) for k in ("exp_avg", "exp_avg_sq", "s", "p0")}, opt.scalars()


def _recurrence(prev, num, den, hp):
    """d, d_max, d_hat from the step's d_numerator and d_denom"""
    d_hat = hp["d_coef"] * num / den
    d = prev["d"]
    if d == hp["d0"]:
        d = max(d, d_hat)
    d_max = max(prev["d_max"], d_hat)
    return min(d_max, d * hp["growth_rate"]), d_max, d_hat


def _check_step(got_p, got, got_sc, prev_p, prev, prev_sc, g_eff, hp, conditioned=True):
    """the device's step against the restatement advanced from the device's previous state.  Bars: p as Lion's (rtol 1e-5,
    atol 1e-6); exp_avg and s rtol 1e-5 with Lion's atol 1e-7 scaled by the step's d, exp_avg_sq by d^2; the sums 1e-12."""
    hp = {**DEFAULTS, **hp}
    b3 = hp["beta3"] if hp["beta3"] is not None else math.sqrt(hp["betas"][1])
    want_p, want_m, want_v, want_s, want_sc, info = prodigy_step(prev_p, g_eff, prev["p0"], prev["exp_avg"], prev["exp_avg_sq"],
                                                                  prev["s"], prev_sc, **hp)
    d = info["d_used"]
    assert want_sc["skipped"] == 0.0 and got_sc["skipped"] == 0.0 and got_sc["k"] == prev_sc["k"] + 1
    np.testing.assert_allclose(got_p, want_p, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["exp_avg"], want_m, rtol=1e-5, atol=1e-7 * d)
    np.testing.assert_allclose(got["s"], want_s, rtol=1e-5, atol=1e-7 * d)
    np.testing.assert_allclose(got["exp_avg_sq"], want_v, rtol=1e-5, atol=1e-7 * d * d)
    assert np.array_equal(got["p0"], prev["p0"])
    # d_denom: a double sum of the fp32 values the kernel stored
    den = float(np.abs(got["s"].astype(np.float64)).sum())
    assert got_sc["d_denom"] == pytest.approx(den, rel=1e-12, abs=0)
    # d_numerator's increment: the fp64 dot of the gradient the kernel formed with p0 - p
    assert got_sc["dlr"] == pytest.approx(want_sc["dlr"], rel=1e-14, abs=0)
    scale = (d / hp["d0"]) * want_sc["dlr"]
    inc = got_sc["d_numerator"] - b3 * prev_sc["d_numerator"]
    ratio = info["abs"] / abs(info["dot"]) if info["dot"] else float("inf")
    print(f"k={int(got_sc['k'])} d={got_sc['d']:.6e} d_hat={got_sc['d_hat']:.6e} inc err/bar="
          f"{abs(inc - scale * info['dot']) / (1e-12 * scale * info['abs'] + 1e-300):.3f} sum|terms|/|sum|={ratio:.3f}")
    assert abs(inc - scale * info["dot"]) <= 1e-12 * scale * info["abs"]
    if conditioned:
        assert ratio <= 10  # the dot is not a cancellation: 1e-12 of the terms is 1e-11 of the sum at most
        # against the restatement's own sums: its d_denom adds the unrounded s, the kernel's the fp32 values it stored, each
        # within 2^-24 of those (6e-8 of the sum at most); the dot adds 1e-11
        assert got_sc["d"] == pytest.approx(want_sc["d"], rel=2.0 ** -24 + 1e-11, abs=0)
    # d, d_max, d_hat follow from the device's own sums by the recurrence
    d_new, d_max, d_hat = _recurrence(prev_sc, got_sc["d_numerator"], got_sc["d_denom"], hp)
    assert got_sc["d_hat"] == pytest.approx(d_hat, rel=1e-12, abs=0)
    assert got_sc["d"] == pytest.approx(d_new, rel=1e-12, abs=0) and got_sc["d_max"] == pytest.approx(d_max, rel=1e-12, abs=0)
    return want_sc


def _fresh_state(p):
    z = np.zeros(p.size, np.float32)
    return {"exp_avg": z, "exp_avg_sq": z, "s": z, "p0": p.copy()}, fresh_scalars(D0)


# the rule holds d at d0 for three steps under the bias correction: over 12 steps the fp64 simulation of the rule itself grows d by
# 37.06 (tests/test_prodigy_cpu.py asserts the figure), so that set can only be asked for the rule's own growth; all others 1e3
SETS = {
    "defaults": ({}, 1.0, False, 1e3),
    "bias_correction": (dict(use_bias_correction=True), 1.0, False, 30.0),
    "growth_rate_2": (dict(growth_rate=2.0), 1.0, False, 1e3),
    "safeguard_coupled_wd": (dict(safeguard_warmup=True, weight_decay=0.01, decouple=False), 1.0, False, 1e3),
    "safeguard_decoupled_wd": (dict(safeguard_warmup=True, weight_decay=0.01), 1.0, False, 1e3),
    "pre_scale": ({}, 0.25, False, 1e3),
    "pre_scale_clip": ({}, 0.25, True, 1e3),
}


@pytest.mark.parametrize("name", list(SETS))
def test_prodigy_follows_fp64_step_by_step(name):
    from uwudiff_amd.optim import FusedProdigy

    hp, pre, clipped, growth = SETS[name]
    gen = Generator()
    flat = torch.nn.Parameter(_dev(gen.p_init.astype(np.float32)))
    flat._uwu_bf16_shadow = torch.zeros(flat.numel(), device="cuda", dtype=torch.bfloat16)
    opt = FusedProdigy([flat], **hp)
    prev_p = _np(flat)
    prev, prev_sc = _fresh_state(prev_p)
    want_sc = prev_sc
    for t in range(12):
        g = gen.grad(prev_p).astype(np.float32)
        flat.grad = _dev(g)
        coef = np.float32(1.0)
        if clipped:
            clip = opt.grad_norm_clip(1.0, pre_scale=pre)
            opt.step(clip=clip, pre_scale=pre, zero_grad=True)
            coef = np.float32(float(clip.cpu()[1]))
            norm = math.sqrt(float((g.astype(np.float64) ** 2).sum())) * pre
            assert float(coef) == pytest.approx(min(1.0, 1.0 / (norm + 1e-6)), rel=1e-5) and coef < 0.1
        else:
            opt.step(pre_scale=pre, zero_grad=True)
        torch.cuda.synchronize()
        g_eff = g.astype(np.float64) * float(np.float32(pre) * coef)  # the fp32 factor the kernel multiplies by, the product exact
        got_p = _np(flat)
        got, got_sc = _state(opt, flat)
        want_sc = _check_step(got_p, got, got_sc, prev_p, prev, prev_sc, g_eff, hp, conditioned=t > 0)
        if t == 0:
            assert got_sc["d"] == D0 and got_sc["d_numerator"] == 0.0  # p0 == p
        assert got_sc["d"] >= prev_sc["d"]
        assert torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16()) and not flat.grad.any()
        prev_p, prev, prev_sc = got_p, got, got_sc
    assert want_sc["d"] / D0 > growth and opt.d == prev_sc["d"]
    if "growth_rate" in hp:
        assert prev_sc["d"] <= D0 * 2.0 ** 12


def test_prodigy_early_return_then_first_step():
    from uwudiff_amd.optim import FusedProdigy

    gen = Generator()
    p_init = gen.p_init.astype(np.float32)
    flat = torch.nn.Parameter(_dev(p_init))
    flat._uwu_bf16_shadow = torch.full((flat.numel(),), 9.0, device="cuda", dtype=torch.bfloat16)
    opt = FusedProdigy([flat])
    flat.grad = torch.zeros_like(flat)
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    got, sc = _state(opt, flat)
    assert np.array_equal(_np(flat).view(np.uint32), p_init.view(np.uint32))
    assert (flat._uwu_bf16_shadow == 9.0).all()  # not refreshed: the step returned before the update
    assert sc == dict(fresh_scalars(D0), skipped=1.0, dlr=D0)
    assert not got["exp_avg"].any() and not got["exp_avg_sq"].any() and not got["s"].any()
    g = gen.grad(p_init).astype(np.float32)
    flat.grad = _dev(g)
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    got2, sc2 = _state(opt, flat)
    prev, prev_sc = _fresh_state(p_init)
    _check_step(_np(flat), got2, sc2, p_init, prev, prev_sc, g.astype(np.float64), {}, conditioned=False)
    assert sc2["k"] == 1.0 and sc2["d"] == D0 and torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16())


def test_prodigy_zero_lr_skips_the_statistics():
    from uwudiff_amd.optim import FusedProdigy

    gen = Generator()
    p_init = gen.p_init.astype(np.float32)
    flat = torch.nn.Parameter(_dev(p_init))
    opt = FusedProdigy([flat])
    opt.param_groups[0]["lr"] = 0.0  # (a scheduler's doing: the constructor refuses it)
    flat.grad = _dev(gen.grad(p_init).astype(np.float32))
    opt.step(zero_grad=True)
    torch.cuda.synchronize()
    got, sc = _state(opt, flat)
    assert sc == dict(fresh_scalars(D0), skipped=1.0) and np.array_equal(_np(flat), p_init) and not flat.grad.any()
    assert not got["exp_avg"].any() and not got["exp_avg_sq"].any() and not got["s"].any()


@pytest.mark.parametrize("zero_grad", [False, True])
def test_prodigy_shadow_and_zeroed_gradient(zero_grad):
    from uwudiff_amd.optim import FusedProdigy

    rng = np.random.default_rng(3)
    n = 4 * 515 + 3
    flat = torch.nn.Parameter(_dev(rng.standard_normal(n).astype(np.float32)))
    flat._uwu_bf16_shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    opt = FusedProdigy([flat], d0=1e-2)
    for _ in range(2):  # (the second step moves p: after the first d_numerator is 0 but the update is not)
        g = rng.standard_normal(n).astype(np.float32)
        flat.grad = _dev(g)
        before = flat.detach().clone()
        opt.step(zero_grad=zero_grad)
        torch.cuda.synchronize()
        assert float((flat.detach() - before).abs().max()) > 0
        assert torch.equal(flat._uwu_bf16_shadow, flat.detach().to(torch.bfloat16))
        assert np.array_equal(_np(flat.grad), np.zeros(n, np.float32) if zero_grad else g)


# ------------------------------------------------------------------------------------------------------------ chunks
N_CH = 4096 * 5 + 12
CHUNKS = [(0, 8192), (8192, 4100), (12292, N_CH - 12292)]
GUARD = 8  # elements before and after every buffer
S_P, S_G, S_M, S_V, S_S, S_P0, S_SH = 7.0, 3.0, 5.0, 2.5, -4.0, 6.0, 9.0


class _Guarded:
    """FusedProdigy on the inside of buffers with sentinel elements on both sides (the state is put in place by hand)"""

    def __init__(self, n, seed=21, steps_of_history=True):
        from uwudiff_amd.optim import FusedProdigy

        rng = np.random.default_rng(seed)
        self.n, self.rng = n, rng
        self.inner = slice(GUARD, GUARD + n)

        def buf(sentinel, values, dtype=torch.float32):
            t = torch.full((n + 2 * GUARD,), sentinel, device="cuda", dtype=dtype)
            t[self.inner] = _dev(values.astype(np.float32)).to(dtype)
            return t

        p0 = rng.standard_normal(n)
        self.bufs = {"p": (buf(S_P, p0 + 0.1 * rng.standard_normal(n)), S_P), "g": (buf(S_G, np.zeros(n)), S_G),
                     "exp_avg": (buf(S_M, 1e-3 * rng.standard_normal(n)), S_M),
                     "exp_avg_sq": (buf(S_V, 1e-6 * rng.standard_normal(n) ** 2), S_V),
                     "s": (buf(S_S, 1e-3 * rng.standard_normal(n)), S_S), "p0": (buf(S_P0, p0), S_P0),
                     "shadow": (buf(S_SH, np.zeros(n), torch.bfloat16), S_SH)}
        self.flat = torch.nn.Parameter(self.bufs["p"][0][self.inner])
        self.flat.grad = self.bufs["g"][0][self.inner]
        self.flat._uwu_bf16_shadow = self.bufs["shadow"][0][self.inner]
        self.opt = FusedProdigy([self.flat], d0=1e-3)
        st = self.opt.state[self.flat]
        self.opt._init_state(self.flat, st)
        for k in ("exp_avg", "exp_avg_sq", "s", "p0"):
            st[k] = self.bufs[k][0][self.inner]
        block = torch.tensor([2e-3, 2e-3, 0.5, 0.0, 0.0, 3.0, 0.0, 0.0], dtype=torch.float64)  # a run three steps in
        st["scalars"] = block.view(torch.float32).cuda()

    def step(self, chunks, g):
        self.flat.grad.copy_(_dev(g))
        self.opt.step(chunks=chunks, zero_grad=True)
        torch.cuda.synchronize()

    def snapshot(self):
        out = {k: _np(t[self.inner].float()) for k, (t, _) in self.bufs.items()}
        out["scalars"] = self.opt.scalars()
        return out

    def guards_intact(self):
        for name, (t, sentinel) in self.bufs.items():
            a = t.float().cpu().numpy()
            assert (a[:GUARD] == sentinel).all() and (a[GUARD + self.n:] == sentinel).all(), name


def _bits_equal(a, b):
    assert a["scalars"] == b["scalars"]
    for k in a:
        if k != "scalars":
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_prodigy_chunked_launches_are_deterministic_and_agree_with_one_launch():
    assert GUARD % 4 == 0 and all(o % 4 == 0 for o, _ in CHUNKS) and sum(ln for _, ln in CHUNKS) == N_CH
    g1, g2 = (np.random.default_rng(22 + i).standard_normal(N_CH).astype(np.float32) for i in range(2))
    runs = []
    for chunks in (CHUNKS, CHUNKS, None):
        r = _Guarded(N_CH)
        start = r.snapshot()
        r.step(chunks, g1)
        mid = r.snapshot()
        r.step(chunks, g2)
        r.guards_intact()
        runs.append((start, mid, r.snapshot()))
    _bits_equal(runs[0][1], runs[1][1])
    _bits_equal(runs[0][2], runs[1][2])  # the same chunking: the same bits in p, state and scalars
    (start, mid3, end3), (_, mid1, end1) = runs[0], runs[2]
    assert mid3["scalars"]["k"] == 4.0 and end3["scalars"]["k"] == 5.0 and not end3["g"].any()
    hp = dict(d0=1e-3)
    for before, after, g in ((start, mid3, g1), (mid3, end3, g2), (start, mid1, g1), (mid1, end1, g2)):  # each within the bars
        _check_step(after["p"], after, after["scalars"], before["p"], before, before["scalars"], g.astype(np.float64), hp,
                    conditioned=False)  # (random p0 - p: the dot cancels, which the bar on its increment allows for)
        assert np.array_equal(after["shadow"], _np(_dev(after["p"]).bfloat16().float()))
    # one launch adds the same partials' terms in another order: the sums agree to double rounding, the tensors within the bars
    for k in ("d", "d_numerator", "d_denom"):
        assert end1["scalars"][k] == pytest.approx(end3["scalars"][k], rel=1e-12, abs=0)
    np.testing.assert_allclose(end1["p"], end3["p"], rtol=1e-5, atol=1e-6)


def test_prodigy_four_element_chunk():
    g = np.random.default_rng(23).standard_normal(4).astype(np.float32)
    a, b = _Guarded(4), _Guarded(4)
    start = a.snapshot()
    a.step([(0, 4)], g)
    b.step([(0, 4)], g)
    a.guards_intact()
    end = a.snapshot()
    _bits_equal(end, b.snapshot())
    _check_step(end["p"], end, end["scalars"], start["p"], start, start["scalars"], g.astype(np.float64), dict(d0=1e-3),
                conditioned=False)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_prodigy_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L
    from uwudiff_amd.optim import FusedProdigy

    n = 64
    t = {k: torch.full((n,), float(i + 1), device="cuda") for i, k in enumerate(("p", "g", "p0", "m", "v", "s"))}
    sc = torch.tensor([D0, D0, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device="cuda")
    ws = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    hyper = (1.0, 0.9, 0.999, math.sqrt(0.999), 0.0, 1, D0, 0, 0, 1.0, None, 1)

    def stats(p=None, g=None, p0=0, m=None, ln=n, scal=None, w=None, ws_slots=4, slot0=0):
        ptr = lambda x, k: t[k].data_ptr() if x is None else x  # noqa: E731
        L.call("uwu_prodigy_stats", ptr(p, "p"), ptr(g, "g"), t["p0"].data_ptr() if p0 == 0 else p0, ptr(m, "m"),
               t["v"].data_ptr(), t["s"].data_ptr(), ln, sc.data_ptr() if scal is None else scal,
               ws.data_ptr() if w is None else w, ws_slots, slot0, *hyper, L.stream())

    for kw in (dict(p=t["p"].data_ptr() + 4), dict(m=t["m"].data_ptr() + 8), dict(ln=0), dict(p0=None), dict(slot0=4),
               dict(ws_slots=0), dict(slot0=-1), dict(scal=sc.data_ptr() + 4), dict(w=ws.data_ptr() + 4)):
        with pytest.raises(L.UwuError, match="prodigy_stats"):
            stats(**kw)
    fin = (1.0, 0.9, 0.999, math.sqrt(0.999), D0, 1.0, float("inf"), 0)
    for args in ((None, ws.data_ptr(), 1), (sc.data_ptr(), None, 1), (sc.data_ptr(), ws.data_ptr(), 0),
                 (sc.data_ptr() + 4, ws.data_ptr(), 1)):
        with pytest.raises(L.UwuError, match="prodigy_finalize"):
            L.call("uwu_prodigy_finalize", *args, *fin, L.stream())
    sh = torch.full((n,), 9.0, device="cuda", dtype=torch.bfloat16)
    for args in ((t["p"].data_ptr() + 4, t["m"].data_ptr(), t["v"].data_ptr(), None, 8, sc.data_ptr()),
                 (t["p"].data_ptr(), None, t["v"].data_ptr(), None, n, sc.data_ptr()),
                 (t["p"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), None, 0, sc.data_ptr()),
                 (t["p"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), sh.data_ptr() + 2, 8, sc.data_ptr()),
                 (t["p"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), None, n, None)):
        with pytest.raises(L.UwuError, match="prodigy_apply"):
            L.call("uwu_prodigy_apply", *args, 1e-8, 0.0, 1, L.stream())
    # the shadow's dtype is the host's to check: the optimizer refuses it by the entry point's name before the update is launched
    flat = torch.nn.Parameter(t["p"])
    flat.grad = t["g"]
    flat._uwu_bf16_shadow = torch.full((n,), 9.0, device="cuda", dtype=torch.float16)
    opt = FusedProdigy([flat])
    with pytest.raises(L.UwuError, match="uwu_prodigy_apply.*bfloat16"):
        opt.step()
    torch.cuda.synchronize()
    assert not opt.state[flat]
    # nothing was launched by a refused call: every buffer the entry points were given still holds its fill
    for i, k in enumerate(("p", "g", "p0", "m", "v", "s")):
        assert (t[k] == float(i + 1)).all(), k
    assert (sh == 9.0).all() and (flat._uwu_bf16_shadow == 9.0).all() and (ws == -1.0).all()
    assert sc.tolist() == [D0, D0, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ fit loop
OPT_CONFIG = {"weight_decay": 0.01, "use_bias_correction": False, "safeguard_warmup": True}


def _fit_cfg(tmp_path, steps, clip=None, accumulate=1, lyc=None, unet=None, monitor=False):
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import LearningRateMonitor

    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 2, "gradient_clip_val": clip,
                                 "accumulate_grad_batches": accumulate, "default_root_dir": str(tmp_path)},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8},
                     "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": 1.0, "optimizer": "prodigyopt.Prodigy", "opt_config": OPT_CONFIG, "lycoris_config": lyc}}
    if unet is not None:
        over["trainer"]["model_config"] = {"unet": {"_target_": unet}}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over)
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


@pytest.mark.parametrize("clip,accumulate", [(None, 1), (1.0, 1), (None, 2)], ids=["noclip", "clip", "accumulate2"])
def test_fitter_takes_the_fused_branch_under_prodigy(tmp_path, clip, accumulate):
    from uwudiff_amd.optim import FusedProdigy

    fit, dm, tr = _fresh(tmp_path, 6, clip=clip, accumulate=accumulate, monitor=True)
    flat0 = tr.unet.flat.detach().clone()
    calls = {"refresh": 0, "at_step": []}
    inner = tr.unet.refresh_shadow

    def counted():
        calls["refresh"] += 1
        return inner()

    tr.unet.refresh_shadow = counted

    def after_step(f):
        calls["at_step"].append(calls["refresh"])
        assert not tr.unet.flat.grad.any()  # left zeroed by the statistics kernel

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedProdigy and fit.global_step == 6
    assert [h["step"] for h in hist] == [2, 4, 6] and all(math.isfinite(h["loss"]) for h in hist)
    assert len(set(calls["at_step"])) == 1, calls  # no refresh_shadow() once the steps have begun: the kernel wrote the shadow
    sc = optim.scalars()
    print(f"d after 6 steps: {sc['d']:.6e}", [h["d"] for h in hist])
    assert sc["k"] == 6.0 and sc["skipped"] == 0.0 and optim.d == sc["d"] > optim.param_groups[0]["d0"]
    assert hist[-1]["d"] == sc["d"] and [h["d"] for h in hist] == sorted(h["d"] for h in hist)  # logged next to lr
    flat = tr.unet.flat.detach()
    assert torch.isfinite(flat).all() and float((flat - flat0.to(flat.device)).abs().max()) > 0
    assert torch.equal(tr.unet.shadow, flat.bfloat16())
    st = optim.state[tr.unet.flat]
    assert set(st) == {"exp_avg", "exp_avg_sq", "s", "p0", "scalars"} and all(v.dtype == torch.float32 for v in st.values())
    assert torch.equal(st["p0"], flat0.to(flat.device))


def test_prodigy_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after step 3, resume in fresh objects, steps 4-6: parameters, moments, s, p0 and the scalar block equal the
    uninterrupted run's bit for bit (on the denoiser whose gradient is bit-reproducible: see ElementwiseDenoiser)."""
    from uwudiff_amd.engine import seed_everything

    path = str(tmp_path / "step3.ckpt")
    unet = f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser"

    def save_at_3(f):
        if f.global_step == 3:
            f.save_checkpoint(path)
            seed_everything(777)

    fit, dm, tr = _fresh(tmp_path, 6, unet=unet)
    fit.step_hooks.append(save_at_3)
    fit.fit(tr, dm)
    fit2, dm2, tr2 = _fresh(tmp_path, 6, unet=unet)
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        loaded.update({k: v.clone() for k, v in fit2._fit_state[1].state[tr2.unet.flat].items()})
        loaded["d"] = fit2._fit_state[1].d
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert isinstance(tr.unet, ElementwiseDenoiser) and isinstance(tr2.unet, ElementwiseDenoiser)
    assert fit.global_step == 6 and fit2.global_step == 6 and all(math.isfinite(h["loss"]) for h in hist_b)
    opt_a, opt_b = fit._fit_state[1], fit2._fit_state[1]
    st_a, st_b = opt_a.state[tr.unet.flat], opt_b.state[tr2.unet.flat]
    # what the resumed run started from is the file's content: the scalar block, p0 and s came from the checkpoint
    ck = torch.load(path, map_location="cpu", weights_only=True)["optimizer_states"][0]["state"][0]
    assert set(ck) == {"exp_avg", "exp_avg_sq", "s", "p0", "scalars"}
    for k, v in ck.items():
        assert _same_bits(loaded[k], v), k
    ck_sc = dict(zip(opt_a.SCALARS, ck["scalars"].view(torch.float64).tolist()))
    assert ck_sc["k"] == 3.0 and loaded["d"] == ck_sc["d"] and ck["s"].abs().max() > 0
    print(f"d at the checkpoint {ck_sc['d']:.6e}, at step 6 {opt_b.d:.6e}")
    assert opt_a.scalars()["k"] == 6.0 and opt_a.scalars() == opt_b.scalars()
    assert _same_bits(tr2.unet.flat.detach(), tr.unet.flat.detach())
    for k in ("exp_avg", "exp_avg_sq", "s", "p0", "scalars"):
        assert st_b[k].dtype == torch.float32 and _same_bits(st_b[k], st_a[k]), k
    assert not _same_bits(st_b["s"], loaded["s"])  # steps 4-6 did move it
    assert torch.equal(tr2.unet.shadow, tr2.unet.flat.detach().bfloat16())


def test_lycoris_adapters_train_under_prodigy(tmp_path):
    from uwudiff_amd.optim import FusedProdigy

    fit, dm, tr = _fresh(tmp_path, 3, clip=1.0, lyc=TOML)
    base0 = tr.unet.flat.detach().clone()
    ad0 = tr.lycoris_model.flat.detach().clone()

    def after_step(f):
        assert not tr.lycoris_model.flat.grad.any()

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedProdigy and list(optim.state) == [tr.lycoris_model.flat]
    assert fit.global_step == 3 and all(math.isfinite(h["loss"]) for h in hist)
    assert optim.scalars()["k"] == 3.0 and optim.d >= D0
    assert float((tr.lycoris_model.flat.detach() - ad0.to(tr.lycoris_model.flat.device)).abs().max()) > 0
    assert torch.equal(optim.state[tr.lycoris_model.flat]["p0"].cpu(), ad0.cpu())
    assert torch.equal(tr.unet.flat.detach().cpu(), base0.cpu()) and tr.unet.flat.grad is None


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
    from uwudiff_amd.optim import FusedProdigy

    torch.cuda.set_device(0)
    gen = Generator(N_CH)  # identical replicas (the same seed)
    flat = torch.nn.Parameter(_dev(gen.p_init.astype(np.float32)))
    flat.grad = torch.zeros_like(flat)
    opt = FusedProdigy([flat])
    sync = FlatGradSync(world, chunk_elems=8192)
    noise = np.random.default_rng(100 + rank)  # per-rank data
    fails = []
    for _ in range(3):
        g = gen.grad(_np(flat)) + 0.5 * noise.standard_normal(N_CH)
        flat.grad.copy_(_dev(g.astype(np.float32)))
        chunks = sync.all_reduce(flat.grad)
        if len(chunks) != 3:
            fails.append(f"chunks {chunks}")
        opt.step(pre_scale=sync.pre_scale, chunks=chunks, before_chunk=sync.wait_chunk, zero_grad=True)
    torch.cuda.synchronize()
    mine = torch.cat([flat.detach(), opt.state[flat]["scalars"]])
    both = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    if not _same_bits(both[0], both[1]):
        fails.append("replicas differ")
    sc = opt.scalars()
    if not (sc["k"] == 3.0 and sc["d"] > D0):
        fails.append(f"scalars {sc}")
    q.put((rank, fails))
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_d_and_parameters():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=30)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert all(not f for _, f in res), res
