"""CPU: the host side of the fused schedule-free AdamW (uwudiff_amd.optim.FusedAdamWScheduleFree) -- target
resolution, the constructor, the per-step scalars -- and the fp64 restatement of ``schedulefree.AdamWScheduleFree.step`` that
tests/test_schedulefree_gpu.py and tests/test_schedulefree_trainer_gpu.py hold the kernels against.  The package is not installed, so
the restatement is checked on properties of the rule: hand-computed scalars, the first step, and the average beating the base
iterate on a noisy quadratic."""
import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

TARGET = "schedulefree.AdamWScheduleFree"
DEFAULTS = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, warmup_steps=0, r=0.0, weight_lr_power=2.0)
GROUP_KEYS = {"k", "r", "warmup_steps", "weight_sum", "lr_max", "scheduled_lr", "weight_lr_power", "train_mode", "lr", "betas", "eps",
              "weight_decay"}


# ------------------------------------------------------------------------------------------------------------ restatement
def fresh_scalars():
    return {"k": 0, "weight_sum": 0.0, "lr_max": -1.0, "scheduled_lr": 0.0}


def sf_scalars(sc, **hp):
    """The host side of one step: (the scalars after it, the step's constants {lr_t, c, bc2})."""
    hp = {**DEFAULTS, **hp}
    k, warmup = sc["k"], hp["warmup_steps"]
    sched = (k + 1) / warmup if k < warmup else 1.0
    bc2 = 1 - hp["betas"][1] ** (k + 1)
    lr_t = hp["lr"] * sched
    lr_max = max(lr_t, sc["lr_max"])
    weight = ((k + 1) ** hp["r"]) * (lr_max ** hp["weight_lr_power"])
    weight_sum = sc["weight_sum"] + weight
    c = weight / weight_sum if weight_sum != 0 else 0.0
    return {"k": k + 1, "weight_sum": weight_sum, "lr_max": lr_max, "scheduled_lr": lr_t}, {"lr_t": lr_t, "c": c, "bc2": bc2}


def lerp(start, end, w):
    """torch.lerp: start + w (end - start) for w < 0.5, else end - (end - start)(1 - w)"""
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    return start + w * (end - start) if w < 0.5 else end - (end - start) * (1 - w)


def sf_step(y, g, z, v, sc, **hp):
    """One ``AdamWScheduleFree.step`` in fp64 from the given state.  ``g`` is the gradient the rule sees (pre-scale and clip
    coefficient applied).  Returns (y, z, v, scalars, info); info: the step's constants and ``gn``, for the tests' bounds."""
    hp = {**DEFAULTS, **hp}
    b1, b2 = hp["betas"]
    y, g, z, v = (np.asarray(a, dtype=np.float64) for a in (y, g, z, v))
    out, now = sf_scalars(sc, **hp)
    lr_t, c, bc2 = now["lr_t"], now["c"], now["bc2"]
    v = b2 * v + (1 - b2) * g * g
    gn = g / (np.sqrt(v / bc2) + hp["eps"]) + hp["weight_decay"] * y  # y BEFORE the interpolation
    y = lerp(y, z, c)
    y = y + lr_t * (b1 * (1 - c) - 1) * gn
    z = z - lr_t * gn
    return y, z, v, out, dict(now, gn=gn)


def sf_average(y, z, beta1=0.9):
    """x, the weights to evaluate"""
    return lerp(y, z, 1 - 1 / beta1)


# ------------------------------------------------------------------------------------------------------------ the class, host side
def test_the_alias_resolves():
    from uwudiff_amd.config import instantiate_any
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamWScheduleFree

    assert instantiate_any(TARGET) is FusedAdamWScheduleFree
    assert issubclass(FusedAdamWScheduleFree, FlatFusedOptimizer)


def test_the_entry_points_are_bound():
    from uwudiff_amd import lib

    assert len(lib._SIGS["uwu_sfadamw_step"][1]) == 17 and len(lib._SIGS["uwu_sf_average"][1]) == 6
    head = open(os.path.join(ROOT, "include", "uwu_hip.h")).read()
    assert "AdamWScheduleFree" in head and "uwu_sfadamw_step(" in head and "uwu_sf_average(" in head


def test_constructor_defaults_group_keys_and_refusals():
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    p = torch.zeros(8, requires_grad=True)
    opt = FusedAdamWScheduleFree([p])
    g = opt.param_groups[0]
    assert GROUP_KEYS <= set(g)
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["warmup_steps"], g["r"], g["weight_lr_power"]) == \
        (0.0025, (0.9, 0.999), 1e-8, 0, 0, 0.0, 2.0)
    assert (g["k"], g["weight_sum"], g["lr_max"], g["train_mode"]) == (0, 0.0, -1.0, False)
    assert not opt.state  # z and exp_avg_sq appear at the first step
    FusedAdamWScheduleFree([p], foreach=True)  # accepted and ignored
    for kw in ({"betas": (0.0, 0.999)}, {"betas": (1.0, 0.999)}, {"betas": (0.9, 1.0)}, {"lr": -1e-3}, {"eps": -1e-8},
               {"weight_decay": -0.1}):
        with pytest.raises(ValueError):
            FusedAdamWScheduleFree([p], **kw)


def test_step_outside_train_mode_is_refused_and_the_modes_are_idempotent():
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    p = torch.zeros(8, requires_grad=True)
    opt = FusedAdamWScheduleFree([p])
    with pytest.raises(RuntimeError, match="train mode"):
        opt.step()
    assert opt.param_groups[0]["k"] == 0  # (a refused step advances nothing)
    opt.train()
    opt.train()
    assert opt.param_groups[0]["train_mode"] is True
    opt.eval()  # before the first step x = y = z: nothing to launch, also without a GPU
    opt.eval()
    assert opt.param_groups[0]["train_mode"] is False and opt.held_weights(p) is None
    sd = opt.state_dict()
    assert GROUP_KEYS <= set(sd["param_groups"][0])


def _advance(opt, steps):
    """optimizer steps without a gradient: no launch (the base class skips such a parameter), the scalars advance as the package's do"""
    seen = []
    for _ in range(steps):
        now = opt.step_scalars(opt.param_groups[0])
        opt.step()
        seen.append((now, dict(opt.param_groups[0])))
    return seen


def test_host_scalars_over_ten_steps():
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    lr, b2 = 0.01, 0.999
    p = torch.zeros(8, requires_grad=True)
    opt = FusedAdamWScheduleFree([p], lr=lr, betas=(0.9, b2), warmup_steps=4, r=0.5)
    opt.train()
    seen = _advance(opt, 10)
    sched = [0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # weight_k = sqrt(k + 1) * lr_max^2 with lr_max = lr * sched (it never falls); c = weight / running sum
    weights = [math.sqrt(k + 1) * (lr * s) ** 2 for k, s in enumerate(sched)]
    sc = fresh_scalars()
    for k, ((lr_t, lr_max, weight_sum, c, bc2), g) in enumerate(seen):
        assert lr_t == pytest.approx(lr * sched[k], rel=1e-15) and lr_max == pytest.approx(lr * sched[k], rel=1e-15)
        assert c == pytest.approx(weights[k] / sum(weights[:k + 1]), rel=1e-14)
        assert bc2 == pytest.approx(1 - b2 ** (k + 1), rel=1e-15)
        assert weight_sum == pytest.approx(sum(weights[:k + 1]), rel=1e-14)
        assert (g["k"], g["scheduled_lr"], g["lr_max"], g["weight_sum"]) == (k + 1, lr_t, lr_max, weight_sum)
        sc, now = sf_scalars(sc, lr=lr, betas=(0.9, b2), warmup_steps=4, r=0.5)  # the restatement agrees to the bit
        assert (now["lr_t"], now["c"], now["bc2"]) == (lr_t, c, bc2) and sc["weight_sum"] == weight_sum
    assert seen[0][0][3] == 1.0  # the first step: c = 1, lerp(y, z, 1) is z
    state = opt.state_dict()["param_groups"][0]
    assert state["k"] == 10 and state["train_mode"] is True and state["weight_sum"] == seen[-1][0][2]
    fresh = FusedAdamWScheduleFree([p], lr=lr, betas=(0.9, b2), warmup_steps=4, r=0.5)
    fresh.load_state_dict(opt.state_dict())  # the scalars and the mode travel with the state dict
    assert {k: fresh.param_groups[0][k] for k in GROUP_KEYS} == {k: opt.param_groups[0][k] for k in GROUP_KEYS}


def test_lr_zero_gives_weight_sum_zero_and_c_zero():
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    p = torch.zeros(8, requires_grad=True)
    opt = FusedAdamWScheduleFree([p], lr=0.0, warmup_steps=4, r=0.5)
    opt.train()
    for (lr_t, lr_max, weight_sum, c, _), g in _advance(opt, 3):
        assert (lr_t, lr_max, weight_sum, c) == (0.0, 0.0, 0.0, 0.0)
    assert opt.param_groups[0]["k"] == 3
    _, now = sf_scalars(fresh_scalars(), lr=0.0)
    assert now["c"] == 0.0


# ------------------------------------------------------------------------------------------------------------ the rule
def test_first_step_of_the_rule_lands_on_z():
    rng = np.random.default_rng(0)
    y, z, g = rng.standard_normal(16), rng.standard_normal(16), rng.standard_normal(16)
    y1, z1, v1, sc, info = sf_step(y, g, z, np.zeros(16), fresh_scalars(), lr=1e-2, weight_decay=0.1)
    assert info["c"] == 1.0 and sc["k"] == 1
    assert np.array_equal(y1, z - 1e-2 * info["gn"]) and np.array_equal(y1, z1)  # a = -lr_t at c = 1
    assert np.array_equal(lerp(y, z, 1.0), z) and np.array_equal(lerp(y, z, 0.0), y)
    np.testing.assert_allclose(info["gn"], g / (np.sqrt((1 - 0.999) * g * g / (1 - 0.999)) + 1e-8) + 0.1 * y, rtol=1e-12)


def test_the_average_beats_the_base_iterate_on_a_noisy_quadratic():
    """f(w) = 1/2 sum h_i (w_i - t_i)^2 on 64 coordinates, the gradient taken at y with unit noise: after 1000 steps the average x is
    closer to the target than the base iterate z, which carries the last steps' noise."""
    rng = np.random.default_rng(0)
    n = 64
    h, target = np.logspace(-1, 1, n), rng.standard_normal(n)
    y = z = rng.standard_normal(n)
    v, sc = np.zeros(n), fresh_scalars()
    for _ in range(1000):
        g = h * (y - target) + rng.standard_normal(n)
        y, z, v, sc, _ = sf_step(y, g, z, v, sc, lr=0.05, warmup_steps=50)
    x = sf_average(y, z)
    ex, ez = float(np.abs(x - target).mean()), float(np.abs(z - target).mean())
    print(f"mean |x - target| {ex:.4f}, mean |z - target| {ez:.4f}")
    assert sc["k"] == 1000 and ex < ez and ex < 0.1


# ------------------------------------------------------------------------------------------------------------ the config
def test_the_schedulefree_yaml_names_the_alias():
    from uwudiff_amd.config import instantiate_any, load_yaml
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_schedulefree.yaml"))
    tr = cfg["trainer"]
    assert tr["optimizer"] == TARGET and instantiate_any(tr["optimizer"]) is FusedAdamWScheduleFree
    assert tr["lr_scheduler"] is None and tr["use_warm_up"] is False
    assert set(tr["opt_config"]) >= {"warmup_steps", "weight_decay"}
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    assert tr["model_config"] == base["trainer"]["model_config"] and cfg["data"]["dataset_config"] == base["data"]["dataset_config"]
