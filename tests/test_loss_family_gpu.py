"""GPU: the fused objective under each element loss (MSE, L1, Huber, SmoothL1) against torch's own modules in fp64
(tests/loss_family_oracle.py), through the loss classes with injected draws and a leaf "UNet", as tests/test_objective_gpu.py.

Shapes: [1, 2, 2] (n = 4: one active lane), [4, 8, 8] (n = 256: one partial pass of the 256-thread, 4-wide loop) and [4, 16, 20]
(n = 1280: a full pass plus a quarter), each at B = 1 and 3.  Tolerances are those of tests/test_objective_gpu.py for the same
quantities.  Where rho' = sign(d) the gradient comparison leaves out |d| <= 1e-4 rms_b(d) of the fp64 reference (an fp32 d may
carry the other sign there); tests/test_loss_family_cpu.py shows that this is at most 0.1 % of the seeded inputs."""
import math
import os

import pytest
import torch
import torch.nn as nn

from tests import loss_family_oracle as FO
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# (pred, target, losses / loss, gradient) as (rtol, atol): tests/test_objective_gpu.py's for DiffusionLoss and for RF
TOL = {"diffusion": dict(pred=(1e-4, 1e-4), target=(2e-5, 2e-6), losses=(1e-4, 1e-7), grad=(2e-4, 1e-7)),
       "rf": dict(pred=(2e-4, 2e-4), target=(1e-4, 1e-5), losses=(2e-4, 1e-7), grad=(5e-4, 1e-7))}
_SCHED = {}


class LeafUNet(nn.Module):
    """a "UNet" that returns a given tensor: the leaf the gradient is read from"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, noisy, timesteps, **kw):
        return (self.out,)


def _sched(prediction_type="epsilon"):
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    if prediction_type not in _SCHED:
        _SCHED[prediction_type] = EulerDiscreteScheduler.from_pretrained(
            "stabilityai/stable-diffusion-xl-base-1.0", subfolder="scheduler", prediction_type=prediction_type)
    return _SCHED[prediction_type]


def close(a, b, tol, **kw):
    torch.testing.assert_close(a.detach().float().cpu(), b.float(), rtol=tol[0], atol=tol[1], **kw)


def build(case, loss):
    from uwudiff_amd.objective import DiffusionLoss, RectifiedFlowLoss

    case = FO.CASE_BY_NAME[case] if isinstance(case, str) else case
    if case.cls == "rf":
        return RectifiedFlowLoss(scheduler=_sched(case.prediction_type), time_sampling_type=case.time_sampling_type, loss=loss)
    return DiffusionLoss(_sched(), prediction_type=case.prediction_type, target_type=case.target_type,
                         use_snr_weight=case.use_snr_weight, use_debiased_estimation=case.use_debiased_estimation, loss=loss)


def run(case, loss, inp, model_output=None, upstream=None):
    """(loss, aux, d loss / d model_output) of one forward + backward on the device"""
    case = FO.CASE_BY_NAME[case] if isinstance(case, str) else case
    mod = build(case, loss)
    out = (inp.model_output if model_output is None else model_output).cuda().requires_grad_(True)
    if case.cls == "rf":
        mod.inject(u01=None if inp.u01 is None else inp.u01.cuda(), timesteps=None if inp.timesteps is None else inp.timesteps.cuda())
        x = torch.stack([inp.x, inp.noise], dim=1).cuda()  # [B, 2, C, H, W]: the latent and its injected noise
    else:
        mod.inject(noise=inp.noise.cuda(), timesteps=inp.timesteps.cuda())
        x = inp.x.cuda()
    loss_v, aux = mod(x, LeafUNet(out))
    (loss_v if upstream is None else loss_v * upstream).backward()
    return loss_v, aux, out.grad


def grad_close(name, ref, got, tol, want=None, among=None):
    """the gradient against the reference's, over the elements ``among`` (default: all) outside the sign band"""
    want = ref.dloss_dout if want is None else want
    among = torch.ones_like(want, dtype=torch.bool) if among is None else among
    skip = FO.grad_exclusion(name, ref) & among
    share = float(skip.sum()) / float(among.sum())
    print(f"{name}: sign-band share left out of the gradient comparison {share:.5f}")
    assert share <= 1e-3
    close(got.cpu()[among & ~skip], want[among & ~skip], tol, equal_nan=True)


@pytest.mark.parametrize("name", FO.KIND_NAMES)
@pytest.mark.parametrize("case", [c.name for c in FO.CASES])
def test_parity_with_torch_modules_fp64(case, name):
    tol = TOL[FO.CASE_BY_NAME[case].cls]
    for shape in FO.SHAPES:
        for B in FO.BATCHES:
            inp = FO.make_inputs(case, B, shape)
            ref = FO.reference(case, name, inp)
            loss, aux, g = run(case, FO.module(name), inp)
            assert aux.losses.shape == (B,) and g.dtype == torch.float32
            close(aux.pred, ref.pred, tol["pred"])
            close(aux.target, ref.target, tol["target"])
            close(aux.losses, ref.losses, tol["losses"])
            close(loss, ref.loss, tol["losses"])
            grad_close(name, ref, g, tol["grad"])


@pytest.mark.parametrize("name", ["l1", "huber_1.0", "huber_0.1"])
def test_bf16_model_output_and_upstream_scale(name):
    for shape in FO.SHAPES:
        for B in FO.BATCHES:
            inp = FO.make_inputs("eps", B, shape)
            out_bf = inp.model_output.bfloat16()
            ref = FO.reference("eps", name, inp, out_bf.float())
            loss, aux, g = run("eps", FO.module(name), inp, out_bf, upstream=3.0)
            assert g.dtype == torch.bfloat16
            close(loss, ref.loss, (1e-5, 1e-7))
            grad_close(name, ref, g, (1.6e-2, 1e-6), want=(3.0 * ref.dloss_dout).bfloat16().double())


@pytest.mark.parametrize("name", FO.KIND_NAMES)
def test_exact_zeros(name):
    """model_output == noise (epsilon -> epsilon): d is exactly 0 there, and so are the gradient and the loss contribution."""
    B, shape = 3, FO.SHAPES[2]
    inp = FO.make_inputs("eps", B, shape)
    loss, aux, g = run("eps", FO.module(name), inp, inp.noise.clone())
    assert (aux.losses == 0).all() and loss.item() == 0.0 and (g == 0).all()
    half = torch.zeros(B, *shape, dtype=torch.bool)
    half.flatten(1)[:, ::2] = True
    out = torch.where(half, inp.noise, inp.model_output)
    ref = FO.reference("eps", name, inp, out)
    loss, aux, g = run("eps", FO.module(name), inp, out)
    assert (g.cpu()[half] == 0).all() and (g.cpu()[~half] != 0).all()
    close(aux.losses, ref.losses, TOL["diffusion"]["losses"])  # the zeros' share of the mean is exactly none
    assert (ref.dloss_dout[half] == 0).all()
    grad_close(name, ref, g, TOL["diffusion"]["grad"], among=~half)  # (the exact zeros are compared exactly, above)


def test_exact_zeros_at_the_smallest_threshold():
    """SmoothL1 multiplies by 1 / beta: at the smallest beta the library takes (FLT_MIN) that is finite, and d == 0 stays 0."""
    B, shape = 3, FO.SHAPES[2]
    inp = FO.make_inputs("eps", B, shape)
    half = torch.zeros(B, *shape, dtype=torch.bool)
    half.flatten(1)[:, ::2] = True
    out = torch.where(half, inp.noise, inp.model_output)
    for loss in (nn.SmoothL1Loss(reduction="none", beta=1.1754943508222875e-38), nn.HuberLoss(reduction="none", delta=1.1754943508222875e-38)):
        loss_v, aux, g = run("eps", loss, inp, out)
        assert loss_v.isfinite() and aux.losses.isfinite().all() and g.isfinite().all()
        assert (g.cpu()[half] == 0).all()


@pytest.mark.parametrize("name", FO.KIND_NAMES)
def test_nan_and_inf_stay_visible_and_local(name):
    B, shape = 3, FO.SHAPES[2]
    n = math.prod(shape)
    inp = FO.make_inputs("eps", B, shape)
    out = inp.model_output.clone()
    i_nan, i_inf = 5, 777  # (a first-pass lane and a quarter-pass one)
    out[1].view(-1)[i_nan] = float("nan")
    out[1].view(-1)[i_inf] = float("inf")
    ref = FO.reference("eps", name, inp, out)
    loss, aux, g = run("eps", FO.module(name), inp, out)
    g, losses = g.cpu().flatten(1), aux.losses.cpu()
    assert losses[1].isnan() and loss.isnan() and losses[[0, 2]].isfinite().all()
    close(losses[[0, 2]], ref.losses[[0, 2]], TOL["diffusion"]["losses"])
    assert g[1, i_nan].isnan()  # every kind, L1 included (torch's L1Loss gives 0 here)
    kind, param = FO.kind_param(name)
    lim = {0: float("inf"), 1: 1.0, 2: param, 3: 1.0}[kind]
    if kind == 0:
        assert g[1, i_inf] == float("inf")
    else:  # w = c = 1: rho'(+inf) / (n B)
        torch.testing.assert_close(g[1, i_inf].double(), torch.tensor(lim / (n * B), dtype=torch.float64), rtol=1e-6, atol=0)
    rest = torch.ones(B, n, dtype=torch.bool)
    rest[1, i_nan] = rest[1, i_inf] = False
    assert g[rest].isfinite().all()
    grad_close(name, ref, g.view(B, *shape), TOL["diffusion"]["grad"])


def _direct_mse(case, inp, out):
    """the five outputs of a direct uwu_loss_fwd_bwd call on the coefficients the module gathers"""
    from uwudiff_amd import lib as L

    mod = build(case, None)
    x, noise, mo = inp.x.cuda(), inp.noise.cuda(), out.cuda()
    mod.inject(timesteps=inp.timesteps.cuda())
    _, coef = mod.sample_timesteps_and_sigmas(x)
    B, n = x.shape[0], x[0].numel()
    losses, loss = torch.empty(B, device="cuda"), torch.empty((), device="cuda")
    grad, pred, target = torch.empty_like(mo), torch.empty_like(x), torch.empty_like(x)
    L.call("uwu_loss_fwd_bwd", L.ptr(x), L.ptr(noise), L.ptr(x), L.ptr(mo), L.dt(mo), L.ptr(coef), L.PT[mod.prediction_type],
           L.PT[mod.target_type], 0, B, n, L.ptr(losses), L.ptr(loss), L.ptr(grad), L.ptr(pred), L.ptr(target), L.stream())
    return loss, losses, pred, target, grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["eps", "eps_to_v", "eps_snr"])
def test_mse_routes_give_the_same_bits(case, dtype):
    """loss=None, loss=nn.MSELoss(reduction="none") and the unchanged entry point uwu_loss_fwd_bwd are one instantiation."""
    inp = FO.make_inputs(case, 3, FO.SHAPES[2])
    out = inp.model_output.to(dtype)
    routes = []
    for loss_arg in (None, nn.MSELoss(reduction="none")):
        loss, aux, g = run(case, loss_arg, inp, out)
        routes.append((loss, aux.losses, aux.pred, aux.target, g))
    routes.append(_direct_mse(case, inp, out))
    for other in routes[1:]:
        for a, b in zip(routes[0], other):
            assert a.dtype == b.dtype and torch.equal(a, b)
    assert routes[0][4].dtype == dtype


@pytest.mark.parametrize("name", FO.KIND_NAMES)
def test_two_calls_give_equal_bits(name):
    inp = FO.make_inputs("v_to_rf", 3, FO.SHAPES[2])
    a, b = (run("v_to_rf", FO.module(name), inp) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].losses, b[1].losses) and torch.equal(a[2], b[2])
    assert torch.equal(a[1].pred, b[1].pred) and torch.equal(a[1].target, b[1].target)


@pytest.mark.parametrize("kind,param", [(4, 1.0), (-1, 1.0), (17, 0.0)]
                         + [(k, p) for k in (2, 3) for p in (0.0, -1.0, float("nan"), float("inf"), 1e-40)])  # (1e-40: subnormal as a float)
def test_c_abi_refuses_without_launching(kind, param):
    from uwudiff_amd import lib as L

    B, n = 2, 256
    x, noise, mo = (torch.randn(B, n, device="cuda") for _ in range(3))
    coef = torch.tensor([[1.0, 1.0, 0.5, 0.5]] * B, device="cuda")
    losses, loss = torch.full((B,), -7.0, device="cuda"), torch.full((), -7.0, device="cuda")
    grad, pred, target = (torch.full((B, n), -7.0, device="cuda") for _ in range(3))
    rc = L.load().uwu_loss_elem_fwd_bwd(L.ptr(x), L.ptr(noise), L.ptr(x), L.ptr(mo), L.F32, L.ptr(coef), 0, 0, 0, kind, param, B, n,
                                        L.ptr(losses), L.ptr(loss), L.ptr(grad), L.ptr(pred), L.ptr(target), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"loss_fwd_bwd" in L.load().uwu_last_error()
    for t in (losses, loss, grad, pred, target):
        assert (t == -7.0).all()
    with pytest.raises(L.UwuError):
        L.call("uwu_loss_elem_fwd_bwd", L.ptr(x), L.ptr(noise), L.ptr(x), L.ptr(mo), L.F32, L.ptr(coef), 0, 0, 0, kind, param, B, n,
               L.ptr(losses), L.ptr(loss), L.ptr(grad), L.ptr(pred), L.ptr(target), L.stream())


class OneParamLossPred(nn.Module):
    """loss_pred_module with one parameter: the same predicted log-loss for every sample"""

    def __init__(self):
        super().__init__()
        self.s = nn.Parameter(torch.tensor(-0.4))

    def forward(self, noisy, sigmas, **kw):
        return self.s.expand(noisy.shape[0])


@pytest.mark.parametrize("name", ["huber_1.0", "huber_0.1"])
def test_nn_weighted_rf_loss_with_huber(name):
    """The element loss replaces the squared error inside rf (reference rectified_flow.py:186): rescaled * pred_loss is the
    oracle's Huber RF loss, and the tail's gradient into loss_pred_module is autograd's on the oracle's [B] values."""
    from uwudiff_amd.objective import NNWeightedRFLoss

    case, B, shape = "rfloss_time", 3, FO.SHAPES[2]
    inp = FO.make_inputs(case, B, shape)
    ref = FO.reference(case, name, inp)  # (w = 1: ref.losses are the per-sample RF losses)
    lp = OneParamLossPred().cuda()
    mod = NNWeightedRFLoss(loss_pred_module=lp, scheduler=_sched("rectified_flow"), loss=FO.module(name))
    out = inp.model_output.cuda().requires_grad_(True)
    mod.inject(u01=inp.u01.cuda())
    loss, aux = mod(torch.stack([inp.x, inp.noise], dim=1).cuda(), LeafUNet(out))
    loss.backward()
    tol = TOL["rf"]
    close(aux.rescaled_losses * aux.pred_losses, ref.losses, tol["losses"])
    close(aux.losses, ref.losses, tol["losses"])
    s = torch.tensor(-0.4, dtype=torch.float64, requires_grad=True)
    pred_loss = s.detach().exp().clamp(min=1e-4)
    tail = (ref.losses / pred_loss).mean() + (ref.losses.log() - s).square().mean()
    (gs,) = torch.autograd.grad(tail, s)
    close(loss, tail, (3e-4, 1e-7))
    close(lp.s.grad, gs, (2e-3, 1e-5))
    grad_close(name, ref, out.grad, tol["grad"], want=ref.dloss_dout / pred_loss)


def test_trainer_takes_two_steps_under_the_huber_config(tmp_path):
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    def fit(loss_node):
        over = {"lightning_config": {"fast_dev_run": False, "max_steps": 2, "log_every_n_steps": 1, "default_root_dir": str(tmp_path)},
                "data": {"dataloader_config": {"num_workers": 0}}}
        cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_huber.yaml")), over)
        if loss_node is None:
            cfg.trainer.loss_config.loss = None  # the default: MSELoss
        seed_everything(cfg.seed)
        fitter = Fitter(**cfg["lightning_config"])
        dm, tr = load_all(cfg)
        shapes = []
        tr.loss.register_forward_hook(lambda m, a, o: shapes.append((tuple(o[1].losses.shape), a[0].shape[0])))
        hist = fitter.fit(tr, dm)
        assert fitter.global_step == 2 and len(shapes) == 2 and all(s == (b,) for s, b in shapes)
        return tr, [h["loss"] for h in hist]

    tr, huber = fit("huber")
    assert type(tr.loss.loss) is nn.HuberLoss and tr.loss.loss.delta == 0.1 and tr.loss.loss_kind == 2
    tr_mse, mse = fit(None)
    assert type(tr_mse.loss.loss) is nn.MSELoss
    assert all(math.isfinite(v) for v in huber + mse)
    assert all(h != m and h < m for h, m in zip(huber, mse))  # same seed, same draws: rho_0.1(d) < d^2 wherever d != 0
