"""CPU: the fused Prodigy optimizer's host side -- exported symbols, target resolution, argument validation -- and the fp64
restatement of ``prodigyopt.Prodigy.step`` that tests/test_prodigy_gpu.py holds the kernels against.  The package is not installed,
so the restatement is checked on properties of the rule (the recorded growth of d on a fixed generator, monotonicity, the first
step, growth_rate, the bias correction's hold)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

SYMBOLS = {"uwu_prodigy_stats_blocks": 1, "uwu_prodigy_stats": 24, "uwu_prodigy_finalize": 12, "uwu_prodigy_apply": 10}
DEFAULTS = dict(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True, use_bias_correction=False,
                safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"))
N_GEN = 4096


# ------------------------------------------------------------------------------------------------------------ restatement
def fresh_scalars(d0=1e-6):
    return {"d": d0, "d_max": d0, "d_numerator": 0.0, "d_denom": 0.0, "d_hat": 0.0, "k": 0.0, "skipped": 0.0, "dlr": 0.0}


def prodigy_step(p, g, p0, m, v, s, sc, **hp):
    """One ``prodigyopt.Prodigy.step`` in fp64 from the given state.  ``g`` is the gradient the rule sees (pre-scale and clip
    coefficient applied, coupled decay not yet); ``sc`` the scalars (``fresh_scalars``).  Returns (p, m, v, s, scalars, info);
    info: the d_numerator increment's dot, the sum of its terms' magnitudes, and the d this step used."""
    hp = {**DEFAULTS, **hp}
    b1, b2 = hp["betas"]
    b3 = hp["beta3"] if hp["beta3"] is not None else math.sqrt(b2)
    lr, wd, d0 = hp["lr"], hp["weight_decay"], hp["d0"]
    p, g, p0, m, v, s = (np.asarray(a, dtype=np.float64) for a in (p, g, p0, m, v, s))
    d, k = sc["d"], sc["k"]
    bc = math.sqrt(1 - b2 ** (k + 1)) / (1 - b1 ** (k + 1)) if hp["use_bias_correction"] else 1.0
    dlr = d * lr * bc
    out = dict(sc, dlr=dlr)
    if wd != 0 and not hp["decouple"]:
        g = g + wd * p
    terms = g * (p0 - p)
    info = {"dot": float(terms.sum()), "abs": float(np.abs(terms).sum()), "d_used": d}
    out["d_numerator"] = b3 * sc["d_numerator"]
    if lr > 0:  # (a group lr of 0 skips the statistics)
        out["d_numerator"] += (d / d0) * dlr * info["dot"]
        m = b1 * m + d * (1 - b1) * g
        v = b2 * v + d * d * (1 - b2) * g * g
        s = b3 * s + (d / d0) * (d if hp["safeguard_warmup"] else dlr) * g
        out["d_denom"] = float(np.abs(s).sum())
    else:
        out["d_denom"] = 0.0
    if out["d_denom"] == 0:
        out["skipped"] = 1.0
        return p, m, v, s, out, info
    d_hat = hp["d_coef"] * out["d_numerator"] / out["d_denom"]
    if d == d0:
        d = max(d, d_hat)
    d_max = max(sc["d_max"], d_hat)
    d = min(d_max, d * hp["growth_rate"])
    if wd != 0 and hp["decouple"]:
        p = p * (1 - wd * dlr)
    p = p - dlr * m / (np.sqrt(v) + d * hp["eps"])
    out.update(d=d, d_max=d_max, d_hat=d_hat, k=k + 1, skipped=0.0)
    return p, m, v, s, out, info


class Generator:
    """The tests' gradient source: ``target ~ N(0,1)``, ``p ~ N(0,1)``, then per step ``g = (p - target) + 0.1 N(0,1)``"""

    def __init__(self, n=N_GEN, seed=0):
        self.rng = np.random.default_rng(seed)
        self.target = self.rng.standard_normal(n)
        self.p_init = self.rng.standard_normal(n)

    def grad(self, p):
        return (np.asarray(p, dtype=np.float64) - self.target) + 0.1 * self.rng.standard_normal(self.target.size)


def simulate(steps, n=N_GEN, **hp):
    """the rule free-running in fp64 on the generator; returns d after every step"""
    gen = Generator(n)
    p = gen.p_init.copy()
    p0, m, v, s = p.copy(), np.zeros(n), np.zeros(n), np.zeros(n)
    sc, ds = fresh_scalars(hp.get("d0", 1e-6)), []
    for _ in range(steps):
        p, m, v, s, sc, _ = prodigy_step(p, gen.grad(p), p0, m, v, s, sc, **hp)
        ds.append(sc["d"])
    assert sc["k"] == steps
    return ds


# ------------------------------------------------------------------------------------------------------------ tests
def test_restatement_grows_d_as_recorded():
    ds = simulate(12)
    print(" ".join(f"{d:.3e}" for d in ds))
    assert [f"{d:.3e}" for d in ds[:4]] == ["1.000e-06", "1.578e-06", "4.797e-06", "1.338e-05"]
    assert f"{ds[-1]:.3e}" == "2.515e-02"
    assert all(b >= a for a, b in zip(ds, ds[1:]))  # d never decreases
    assert ds[0] == 1e-6  # step 1: p0 == p, the numerator is 0


def test_restatement_growth_rate_caps_every_ratio():
    ds = simulate(12, growth_rate=2.0)
    ratios = [b / a for a, b in zip([1e-6] + ds, ds)]
    assert max(ratios) <= 2.0 and ratios.count(2.0) >= 6 and all(r >= 1.0 for r in ratios)


def test_restatement_bias_correction_holds_d_at_first():
    ds = simulate(12, use_bias_correction=True)
    assert ds[:3] == [1e-6] * 3 and ds[3] > 1e-6 and all(b >= a for a, b in zip(ds, ds[1:]))
    assert f"{ds[-1] / 1e-6:.3e}" == "3.706e+01"  # the rule's own growth over 12 steps: what the GPU test can ask of this set


def test_restatement_early_return_and_zero_lr():
    gen = Generator(64)
    p = gen.p_init
    z = np.zeros(64)
    sc = dict(fresh_scalars(), d_numerator=3.0)
    out = prodigy_step(p, z, p, z, z, z, sc)
    assert out[4]["skipped"] == 1.0 and out[4]["k"] == 0 and out[4]["d"] == 1e-6 and np.array_equal(out[0], p)
    assert out[4]["d_numerator"] == 3.0 * math.sqrt(0.999)  # keeps its decayed value
    out = prodigy_step(p, gen.grad(p), p, z, z, z, fresh_scalars(), lr=0.0)
    assert out[4]["skipped"] == 1.0 and not out[1].any() and not out[3].any() and np.array_equal(out[0], p)


def test_library_exports_the_prodigy_entry_points():
    from uwudiff_amd import build, lib

    build.build(verbose=False)
    cd = ctypes.CDLL(lib.LIB_PATH)
    for s, arity in SYMBOLS.items():
        assert hasattr(cd, s), s
        assert s in lib.exported_symbols() and len(lib._SIGS[s][1]) == arity
    cd.uwu_prodigy_stats_blocks.argtypes = [ctypes.c_int64]
    blocks = [cd.uwu_prodigy_stats_blocks(n) for n in (0, 1, 4, 1024, 1028, 4096 * 5 + 12, 2_570_000_000)]
    assert blocks == [0, 1, 1, 1, 2, 21, 2048]  # a function of n alone (host only: nothing is launched)
    with open(os.path.join(ROOT, "include", "uwu_hip.h")) as f:
        header = f.read()
    assert all(f"int {s}(" in header for s in SYMBOLS)
    from uwudiff_amd.optim import FusedProdigy

    assert f"#define UWU_PRODIGY_SCALARS {len(FusedProdigy.SCALARS)}\n" in header
    for i, name in enumerate(FusedProdigy.SCALARS):
        assert re.search(rf"#define UWU_PRODIGY_{name.upper()} {i}\s", header), name
    assert tuple(fresh_scalars()) == FusedProdigy.SCALARS


def test_prodigy_target_resolves_to_the_fused_class():
    from duwu.utils import instantiate_any
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedProdigy

    assert instantiate_any("prodigyopt.Prodigy") is FusedProdigy and issubclass(FusedProdigy, FlatFusedOptimizer)
    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_prodigy.yaml"))
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_lycoris.yaml"))
    assert instantiate_any(cfg["trainer"]["optimizer"]) is FusedProdigy
    assert cfg["trainer"]["lr"] == 1.0 and cfg["trainer"]["use_warm_up"] is False
    assert cfg["trainer"]["opt_config"] == {"weight_decay": 0.01, "use_bias_correction": True, "safeguard_warmup": True}
    a, b = dict(cfg["trainer"]), dict(base["trainer"])
    for k in ("optimizer", "opt_config", "lr"):
        a.pop(k), b.pop(k)
    assert a == b and {k: v for k, v in cfg.items() if k != "trainer"} == {k: v for k, v in base.items() if k != "trainer"}


def test_prodigy_validates_its_arguments():
    from uwudiff_amd import lib as L
    from uwudiff_amd.optim import FusedProdigy

    def p():
        return [torch.nn.Parameter(torch.zeros(16))]

    for kw, msg in ((dict(d0=0.0), "Invalid d0 value: 0.0"), (dict(lr=0.0), "Invalid learning rate: 0.0"),
                    (dict(lr=-1.0), "Invalid learning rate: -1.0"), (dict(eps=0.0), "Invalid epsilon value: 0.0"),
                    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1")):
        with pytest.raises(ValueError, match=msg):
            FusedProdigy(p(), **kw)
    with pytest.raises(NotImplementedError, match="one flat parameter buffer"):
        FusedProdigy(p() + p())
    opt = FusedProdigy(p(), fsdp_in_use=True)  # accepted and ignored
    g = opt.param_groups[0]
    assert {k: g[k] for k in DEFAULTS} == DEFAULTS and opt.d == 1e-6 and opt.scalars() == fresh_scalars()
    opt.param_groups[0]["params"][0].grad = torch.ones(16)
    with pytest.raises(L.UwuError, match="CPU tensor"):
        opt.step()  # a CPU parameter: there is no CPU path
    assert not opt.state[opt.param_groups[0]["params"][0]]


def test_learning_rate_monitor_reports_d_only_when_the_optimizer_has_one():
    from uwudiff_amd.engine import LearningRateMonitor
    from uwudiff_amd.optim import FusedLion, FusedProdigy

    mon = LearningRateMonitor(logging_interval="step")
    q = [torch.nn.Parameter(torch.zeros(16))]
    assert mon.extra(FusedProdigy(q, d0=1e-5)) == {"d": 1e-5} and mon.extra(FusedLion(q)) == {}
