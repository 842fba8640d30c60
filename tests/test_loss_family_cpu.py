"""CPU: the element-loss argument of the loss classes -- construction, refusals, the demo config's node -- and the
conditions under which tests/loss_family_oracle.py is a fit reference for tests/test_loss_family_gpu.py (no kernel runs here)."""
import os

import pytest
import torch
import torch.nn as nn

from tests import loss_family_oracle as FO
from tests.conftest import ROOT

CLASSES = ("DiffusionLoss", "RectifiedFlowLoss", "NNWeightedRFLoss")


def _sched():
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    return EulerDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder="scheduler")


def _build(cls, loss):
    from uwudiff_amd import objective

    kw = dict(scheduler=_sched(), loss=loss)
    if cls == "NNWeightedRFLoss":
        kw["loss_pred_module"] = nn.Identity()
    return getattr(objective, cls)(**kw)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", FO.KIND_NAMES)
def test_every_class_accepts_every_module(cls, name):
    loss = FO.module(name)
    mod = _build(cls, loss)
    assert mod.loss is loss
    kind, param = FO.kind_param(name)
    assert (mod.loss_kind, mod.loss_param) == (kind, param)
    assert isinstance(mod.loss_kind, int) and isinstance(mod.loss_param, float)


@pytest.mark.parametrize("cls", CLASSES)
def test_default_is_mse_and_beta_zero_is_l1(cls):
    from uwudiff_amd import lib as L

    mod = _build(cls, None)
    assert isinstance(mod.loss, nn.MSELoss) and mod.loss.reduction == "none"  # the reference's default (diffusion.py:27)
    assert (mod.loss_kind, mod.loss_param) == (L.LOSS_MSE, 0.0)
    mod = _build(cls, nn.SmoothL1Loss(reduction="none", beta=0.0))
    assert isinstance(mod.loss, nn.SmoothL1Loss) and (mod.loss_kind, mod.loss_param) == (L.LOSS_L1, 0.0)
    assert (L.LOSS_MSE, L.LOSS_L1, L.LOSS_HUBER, L.LOSS_SMOOTH_L1) == (0, 1, 2, 3)  # UWU_LOSS_* of include/uwu_hip.h


def test_header_declares_the_kinds():
    import re

    src = open(os.path.join(ROOT, "include", "uwu_hip.h")).read()
    got = dict(re.findall(r"#define (UWU_LOSS_[A-Z0-9_]+) (\d+)", src))
    assert got == {"UWU_LOSS_MSE": "0", "UWU_LOSS_L1": "1", "UWU_LOSS_HUBER": "2", "UWU_LOSS_SMOOTH_L1": "3"}


@pytest.mark.parametrize("cls", CLASSES)
def test_refusals_name_what_was_given(cls):
    for red in ("mean", "sum"):
        for make in (nn.MSELoss, nn.L1Loss, nn.HuberLoss, nn.SmoothL1Loss):
            with pytest.raises(NotImplementedError, match=f"{make.__name__}.*{red}"):
                _build(cls, make(reduction=red))
    with pytest.raises(NotImplementedError, match="BCELoss"):
        _build(cls, nn.BCELoss(reduction="none"))
    with pytest.raises(NotImplementedError, match="mse_loss"):
        _build(cls, torch.nn.functional.mse_loss)
    # (1e-50 is 0 and 1e39 is inf as the float the kernel takes; 1e-40 is subnormal there: 1 / beta would be inf)
    for delta in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, 1e-40):
        with pytest.raises(ValueError, match="HuberLoss.*delta"):
            _build(cls, nn.HuberLoss(reduction="none", delta=delta))
    for beta in (-0.5, float("nan"), float("inf"), 1e-50, 1e39, 1e-40):
        with pytest.raises(ValueError, match="SmoothL1Loss.*beta"):
            _build(cls, nn.SmoothL1Loss(reduction="none", beta=beta))


def test_demo_config_node_builds_a_huber_diffusion_loss():
    from uwudiff_amd.config import instantiate_any, load_yaml
    from uwudiff_amd.objective import DiffusionLoss

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_huber.yaml"))
    assert cfg.trainer["_recursive_"] is False  # the trainer node is built flat: loss_config reaches DMTrainer as a node ...
    node = cfg.trainer.loss_config
    assert node["_target_"] == "duwu.loss.DiffusionLoss" and node["loss"]["_target_"] == "torch.nn.HuberLoss"
    mod = instantiate_any(node)  # ... and DMTrainer builds it with recursion on (duwu/trainer/trainer.py)
    assert type(mod) is DiffusionLoss
    assert type(mod.loss) is nn.HuberLoss and mod.loss.delta == 0.1 and mod.loss.reduction == "none"
    assert (mod.loss_kind, mod.loss_param) == (2, 0.1)
    # apart from the loss_config node the config is demo_training_latent.yaml
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    rest = {k: v for k, v in cfg.trainer.items() if k != "loss_config"}
    assert rest == dict(base.trainer) and cfg.data == base.data and cfg.lightning_config == base.lightning_config


# ---- the oracle: its analytic statements against autograd through torch's modules, fp64 ----------------------------------------
@pytest.mark.parametrize("name", FO.KIND_NAMES)
@pytest.mark.parametrize("case", [c.name for c in FO.CASES])
def test_oracle_analytic_statements_agree_with_autograd(case, name):
    for B in FO.BATCHES:
        inp = FO.make_inputs(case, B, FO.SHAPES[1])
        # random (not solved-for) outputs as well: d of any scale
        for out in (None, torch.randn(inp.x.shape, generator=torch.Generator().manual_seed(B))):
            ref = FO.reference(case, name, inp, out)
            losses, g = FO.analytic(name, ref)
            torch.testing.assert_close(losses, ref.losses, rtol=1e-12, atol=1e-14)
            torch.testing.assert_close(g, ref.dloss_dout, rtol=1e-10, atol=1e-16)
            assert ref.losses.shape == (B,) and ref.loss.shape == ()


def test_oracle_at_zero_nan_and_inf():
    for name in FO.KIND_NAMES:
        kind, param = FO.kind_param(name)
        d = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
        r, g = FO.rho(kind, param, d), FO.drho(kind, param, d)
        assert r[0] == 0 and r[1] == 0 and g[0] == 0 and g[1] == 0
        assert r[2].isnan() and g[2].isnan()
        assert r[3] == float("inf") and r[4] == float("inf")
        lim = {0: float("inf"), 1: 1.0, 2: param, 3: 1.0}[kind]
        assert g[3] == lim and g[4] == -lim
        # torch's own forward at the same points; its backward agrees except at the NaN for L1 (0 there, which hides it)
        dd = d.clone().requires_grad_(True)
        t = FO.module(name)(dd, torch.zeros_like(dd))
        torch.testing.assert_close(t.detach(), r, rtol=0, atol=0, equal_nan=True)
        (tg,) = torch.autograd.grad(t.sum(), dd)
        keep = torch.tensor([True, True, kind != 1, True, True])
        torch.testing.assert_close(tg[keep], g[keep], rtol=0, atol=0, equal_nan=True)


# ---- the GPU test's seeded inputs meet the conditions its caps assume -------------------------------------------------------------
def test_input_conditions_of_the_gpu_cases():
    """The share of each Huber / SmoothL1 branch is established on the largest shape, [4, 16, 20] at B = 3 (3840 elements), for
    every case: the smaller shapes draw d from the same law (make_inputs), and a share of 4 or 256 elements says little.  The
    sign band is counted on every shape and batch the GPU test runs."""
    worst_branch, worst_band = 1.0, 0.0
    for case in FO.CASES:
        inp = FO.make_inputs(case, 3, FO.SHAPES[2])
        ref = FO.reference(case, "mse", inp)
        a = ref.d.abs()
        for thr in (1.0, 0.1):
            quad = float((a < thr).double().mean())
            worst_branch = min(worst_branch, quad, 1 - quad)
            assert quad >= 0.02 and 1 - quad >= 0.02, (case.name, thr, quad)
        for B in FO.BATCHES:
            for shape in FO.SHAPES:
                r = FO.reference(case, "l1", FO.make_inputs(case, B, shape))
                band = float(FO.sign_band(r).double().mean())
                worst_band = max(worst_band, band)
                assert band <= 1e-3, (case.name, B, shape, band)
                for name in FO.KIND_NAMES:
                    assert float(FO.grad_exclusion(name, r).double().mean()) <= band
    print(f"smallest branch share {worst_branch:.4f}, largest sign-band share {worst_band:.5f}")
