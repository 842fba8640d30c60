"""Specification of the fused objective's element losses: torch's own loss modules in fp64 on the CPU, composed
with what oracle/loss.py provides for the MSE objective.

    pred, target   x0_eps_from_pred / get_target                      (diffusion.py:84-125, rectified_flow.py:79-82)
    w              snr_weight, debias_weight                           (diffusion.py:141-167)
    losses         w * loss_module(pred, target).flatten(1).mean(1)    (diffusion.py:186-191)
    loss           losses.mean()
    dloss_dout     autograd

TEST INFRASTRUCTURE: tests import this module, product code does not.  Everything runs in fp64; the tests cast the results to
fp32 (or bf16) to compare.  ``rho`` / ``drho`` restate the four element functions analytically (checked against autograd in
tests/test_loss_family_cpu.py); the one place where the specification is NOT torch's backward is a NaN: the expected gradient is
NaN at a NaN element for every kind, where torch's L1Loss / SmoothL1Loss(beta=0) give 0.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from oracle import loss as OL
from oracle.scheduler import EulerDiscreteScheduler as OracleScheduler

# (name, torch module factory, UWU_LOSS_* kind, parameter): the kinds and thresholds every test of the family runs
KINDS = (
    ("mse", lambda: nn.MSELoss(reduction="none"), 0, 0.0),
    ("l1", lambda: nn.L1Loss(reduction="none"), 1, 0.0),
    ("huber_1.0", lambda: nn.HuberLoss(reduction="none", delta=1.0), 2, 1.0),
    ("huber_0.1", lambda: nn.HuberLoss(reduction="none", delta=0.1), 2, 0.1),
    ("smoothl1_1.0", lambda: nn.SmoothL1Loss(reduction="none", beta=1.0), 3, 1.0),
    ("smoothl1_0.1", lambda: nn.SmoothL1Loss(reduction="none", beta=0.1), 3, 0.1),
)
KIND_NAMES = tuple(k[0] for k in KINDS)
SHAPES = ((1, 2, 2), (4, 8, 8), (4, 16, 20))  # n = 4 (one active lane), 256 (one partial pass), 1280 (a full pass + a quarter)
BATCHES = (1, 3)
SIGN_BAND = 1e-4  # |d| <= SIGN_BAND * rms_b(d): where an fp32 d may take the other sign than the fp64 d


def module(name):
    return {k[0]: k[1] for k in KINDS}[name]()


def kind_param(name):
    return {k[0]: (k[2], k[3]) for k in KINDS}[name]


_SCHED = None


def scheduler():
    global _SCHED
    if _SCHED is None:
        _SCHED = OracleScheduler.sdxl()
    return _SCHED


# ---- the element functions, analytically ------------------------------------------------------------------------------------------
def _sign(d):
    """+-1, 0 at 0, NaN at NaN"""
    return torch.where(d > 0, torch.ones_like(d), torch.where(d < 0, -torch.ones_like(d), d))


def rho(kind, param, d):
    a = d.abs()
    if kind == 0:
        return d * d
    if kind == 1:
        return a
    if kind == 2:
        return torch.where(a < param, 0.5 * d * d, param * (a - 0.5 * param))
    return torch.where(a < param, 0.5 * d * d / param, a - 0.5 * param)


def drho(kind, param, d):
    a = d.abs()
    if kind == 0:
        return 2 * d
    if kind == 1:
        return _sign(d)
    if kind == 2:
        return torch.where(a < param, d, param * _sign(d))
    return torch.where(a < param, d / param, _sign(d))


# ---- one case: which loss class, which conversion, which weights --------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cls: str  # "diffusion" | "rf"
    prediction_type: str
    target_type: str
    use_snr_weight: bool = False
    use_debiased_estimation: bool = False
    time_sampling_type: str = "uniform_time"


CASES = (
    Case("eps", "diffusion", "epsilon", "epsilon"),
    Case("v", "diffusion", "v_prediction", "v_prediction"),
    Case("sample", "diffusion", "sample", "sample"),
    Case("rf", "diffusion", "rectified_flow", "rectified_flow"),
    Case("eps_to_v", "diffusion", "epsilon", "v_prediction"),
    Case("sample_to_eps", "diffusion", "sample", "epsilon"),
    Case("v_to_rf", "diffusion", "v_prediction", "rectified_flow"),
    Case("eps_snr", "diffusion", "epsilon", "epsilon", use_snr_weight=True),
    Case("v_snr", "diffusion", "v_prediction", "v_prediction", use_snr_weight=True),
    Case("eps_debias", "diffusion", "epsilon", "epsilon", use_debiased_estimation=True),
    Case("rfloss_time", "rf", "rectified_flow", "rectified_flow"),
    Case("rfloss_timestep", "rf", "epsilon", "rectified_flow", time_sampling_type="uniform_timestep"),
)
CASE_BY_NAME = {c.name: c for c in CASES}


class Inputs(NamedTuple):
    x: torch.Tensor  # fp32 [B, C, H, W]
    noise: torch.Tensor
    timesteps: Optional[torch.Tensor]  # int64 [B] (None: uniform_time)
    u01: Optional[torch.Tensor]  # fp32 [B] (uniform_time only)
    sigmas: torch.Tensor  # fp64 [B]
    model_output: torch.Tensor  # fp32


class Out(NamedTuple):
    loss: torch.Tensor
    losses: torch.Tensor
    pred: torch.Tensor
    target: torch.Tensor
    d: torch.Tensor
    w: torch.Tensor
    c: torch.Tensor  # d pred / d model_output, [B]
    dloss_dout: torch.Tensor


def _pred_target(case, x, noise, sigmas, timesteps, out):
    sch = scheduler()
    if case.cls == "rf":  # rectified_flow.py:71-82: always converts, from the noisy latent
        noisy = OL.q_sample(x, noise, sigmas)
        x0h, epsh = OL.x0_eps_from_pred(case.prediction_type, noisy, out, sigmas)
        return epsh - x0h, noise - x
    if case.prediction_type == case.target_type:
        pred = out
    else:  # diffusion.py:177: the clean x goes in as `xt`
        x0h, epsh = OL.x0_eps_from_pred(case.prediction_type, x, out, sigmas)
        pred = OL.get_target(case.target_type, sch, x0h, epsh, timesteps)
    return pred, OL.get_target(case.target_type, sch, x, noise, timesteps)


def _weights(case, timesteps, B):
    w = torch.ones(B, dtype=torch.float64)
    if case.use_snr_weight:
        w = w * OL.snr_weight(scheduler(), case.prediction_type, timesteps, 5.0).double()  # min_snr_gamma's default
    if case.use_debiased_estimation:
        w = w * OL.debias_weight(scheduler(), timesteps).double()
    return w


def make_inputs(case, B, shape, seed=0):
    """Seeded inputs of one case: x, noise ~ N(0, 1), and a model output whose prediction misses the target by e ~ N(0, 2)
    elementwise (every conversion is affine in the output, so the output is solved for): d = pred - target then has the same
    law in every case, and both branches of Huber / SmoothL1 are populated at thresholds 1.0 and 0.1."""
    if isinstance(case, str):
        case = CASE_BY_NAME[case]
    g = torch.Generator().manual_seed(1000 * seed + 10 * SHAPES.index(tuple(shape)) + B)
    x = torch.randn(B, *shape, generator=g)
    noise = torch.randn(B, *shape, generator=g)
    e = torch.randn(B, *shape, generator=g, dtype=torch.float64) * 2 ** 0.5
    timesteps = u01 = None
    if case.cls == "rf" and case.time_sampling_type == "uniform_time":
        u01 = torch.rand(B, generator=g) * 0.9 + 0.05
        sigmas = OL.rf_time_to_sigma(scheduler(), u01.double())
    else:
        timesteps = torch.randint(0, 1000, (B,), generator=g)
        sigmas = OL.sigmas_for_timesteps(scheduler(), timesteps).double()
    xd, nd = x.double(), noise.double()
    p0, target = _pred_target(case, xd, nd, sigmas, timesteps, torch.zeros_like(xd))
    p1, _ = _pred_target(case, xd, nd, sigmas, timesteps, torch.ones_like(xd))
    out = ((target + e - p0) / (p1 - p0)).float()
    return Inputs(x, noise, timesteps, u01, sigmas, out)


def reference(case, kind_name, inp, model_output=None):
    """fp64 loss, losses, pred, target and d loss / d model_output of one case under one element loss."""
    if isinstance(case, str):
        case = CASE_BY_NAME[case]
    kind, param = kind_param(kind_name)
    out = (inp.model_output if model_output is None else model_output).double().detach().requires_grad_(True)
    x, noise = inp.x.double(), inp.noise.double()
    B, n = x.shape[0], x[0].numel()
    pred, target = _pred_target(case, x, noise, inp.sigmas, inp.timesteps, out)
    w = _weights(case, inp.timesteps, B)
    losses = w * module(kind_name)(pred, target).flatten(1).mean(1)
    loss = losses.mean()
    (g,) = torch.autograd.grad(loss, out)
    d = (pred - target).detach()
    ones = torch.ones_like(x)
    c = (_pred_target(case, x, noise, inp.sigmas, inp.timesteps, ones)[0]
         - _pred_target(case, x, noise, inp.sigmas, inp.timesteps, 0 * ones)[0]).flatten(1)[:, 0]
    # the specification's one departure from torch's backward: a NaN in d is a NaN in the gradient, for every kind
    g = torch.where(d.isnan(), torch.full_like(g, float("nan")), g)
    return Out(loss.detach(), losses.detach(), pred.detach(), target, d, w, c, g)


def analytic(kind_name, ref):
    """(losses, dloss_dout) from rho / drho and the per-sample scalars of ``ref``: what the kernel states it computes."""
    kind, param = kind_param(kind_name)
    B, n = ref.d.shape[0], ref.d[0].numel()
    losses = ref.w * rho(kind, param, ref.d).flatten(1).mean(1)
    g = OL._bcast(ref.w * ref.c / (n * B), ref.d) * drho(kind, param, ref.d)
    return losses, g


def sign_band(ref):
    """elements with |d| <= SIGN_BAND * rms_b(d) (per sample): there the sign of an fp32 d is not pinned by the fp64 d"""
    rms = ref.d.flatten(1).square().mean(1).sqrt()
    return ref.d.abs() <= SIGN_BAND * OL._bcast(rms, ref.d)


def grad_exclusion(kind_name, ref):
    """The elements the gradient comparison leaves out: the sign band where rho' = sign(d), i.e. all of L1 and the linear branch
    of SmoothL1 (Huber's rho' and the quadratic branches are continuous there)."""
    kind, param = kind_param(kind_name)
    band = sign_band(ref)
    if kind == 1:
        return band
    if kind == 3:
        return band & (ref.d.abs() >= param)
    return torch.zeros_like(band)
