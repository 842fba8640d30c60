"""GPU: ``schedulefree.AdamWScheduleFree`` (uwudiff_amd.optim.FusedAdamWScheduleFree) through DMTrainer / Fitter: the fused branch,
the two modes round validation passes and at the end of ``fit``, both sets of weights in a checkpoint, resume, accumulation,
adapters, the refusal of a weight-averaging callback and configs/demo_training_schedulefree.yaml.  The pattern of
tests/test_optim8bit_trainer_gpu.py and of the callback tests of tests/test_averaging_gpu.py; bit-equality is asserted on the
denoiser whose gradient is bit-reproducible (ElementwiseDenoiser).  DESIGN.md section 4.42."""
import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_optimizers_gpu import TOML, ElementwiseDenoiser
from tests.test_schedulefree_cpu import GROUP_KEYS, sf_average

pytestmark = pytest.mark.gpu

TARGET = "schedulefree.AdamWScheduleFree"
ELEMENTWISE = f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser"
ULP = 2.0 ** -24
SCALARS = ("k", "weight_sum", "lr_max", "scheduled_lr", "train_mode")


def _same_bits(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().cpu().contiguous().view(view),
                                                                     b.detach().cpu().contiguous().view(view))


def _check_x(x, y, z, what):
    """x against the oracle's lerp(y, z, 1 - 1/beta1) under the bound of tests/test_schedulefree_gpu.py: z - y rounds once (on
    |y| + |z|, times |w|), w once, the fused multiply-add once (on |x|)"""
    want = sf_average(y.double().cpu().numpy(), z.double().cpu().numpy(), 0.9)
    w = abs(1 - 1 / 0.9)
    bound = ULP * (2 * w * (y.double().abs() + z.double().abs()).cpu().numpy() + np.abs(want))
    err = np.abs(x.double().cpu().numpy() - want)
    print(f"{what}: x against the oracle, largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


def _fit_cfg(tmp_path, steps, clip=None, unet=None, lyc=None, val=False, n_acc=1):
    from uwudiff_amd.config import load_yaml, merge

    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1, "gradient_clip_val": clip,
                                 "default_root_dir": str(tmp_path), "accumulate_grad_batches": n_acc},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8},
                     "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": 1e-3, "optimizer": TARGET, "lr_scheduler": None, "use_warm_up": False,
                        "opt_config": {"weight_decay": 0.01, "betas": [0.9, 0.999], "warmup_steps": 2}, "lycoris_config": lyc}}
    if val:
        over["lightning_config"].update({"val_check_interval": 2, "check_val_every_n_epoch": None, "num_sanity_val_steps": 1})
        over["data"]["val_dataset_config"] = {"_target_": "duwu.data.DummyDataset", "sample_size": [3, 32, 32], "n_samples": 8}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over)
    if unet is not None:
        cfg = merge(cfg, {"trainer": {"model_config": {"unet": {"_target_": unet}}}})
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    return cfg, lc


def _fresh(tmp_path, steps, callbacks=(), **kw):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, steps, **kw)
    seed_everything(cfg.seed)
    fit = Fitter(callbacks=list(callbacks), **lc)
    dm, tr = load_all(cfg)
    return fit, dm, tr


def _snapshot(fit, p):
    """y, z, v and the scalars wherever they are right now (y: the parameter while training, the buffer kept aside otherwise)"""
    opt = fit._fit_state[1]
    st, g = opt.state[p], opt.param_groups[0]
    held = opt.held_weights(p)
    return {"y": (p.data if held is None else held).detach().clone(), "z": st["z"].detach().clone(),
            "v": st["exp_avg_sq"].detach().clone(), "flat": p.data.detach().clone(), **{k: g[k] for k in SCALARS}}


# ------------------------------------------------------------------------------------------------------------ the fused branch
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
def test_fitter_takes_the_fused_branch(tmp_path, clip):
    from uwudiff_amd.averaging import ScheduleFreeMode
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamWScheduleFree

    fit, dm, tr = _fresh(tmp_path, 3, clip=clip)
    flat0 = tr.unet.flat.detach().clone()
    inside = []

    def after_step(f):
        g = f._fit_state[1].param_groups[0]
        inside.append((g["k"], f.global_step, g["train_mode"], tr.unet.flat.detach().clone()))
        assert not tr.unet.flat.grad.any()  # left zeroed by the update kernel

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert isinstance(optim, FlatFusedOptimizer) and type(optim) is FusedAdamWScheduleFree
    assert sum(isinstance(cb, ScheduleFreeMode) for cb in fit.callbacks) == 1
    assert fit.global_step == 3 and len(hist) == 3 and all(math.isfinite(h["loss"]) for h in hist)
    assert [(k, s, m) for k, s, m, _ in inside] == [(1, 1, True), (2, 2, True), (3, 3, True)]  # k counts optimizer steps
    p = tr.unet.flat
    st, g = optim.state[p], optim.param_groups[0]
    assert set(st) == {"z", "exp_avg_sq"} and GROUP_KEYS <= set(g)
    for k in ("z", "exp_avg_sq"):
        assert st[k].dtype == torch.float32 and st[k].shape == p.shape and st[k].is_cuda and torch.isfinite(st[k]).all()
    assert g["k"] == 3 and g["scheduled_lr"] == 1e-3 and g["lr_max"] == 1e-3 and g["weight_sum"] > 0
    # fit returns the module holding x; y sits in the buffer that restores it
    assert g["train_mode"] is False
    y = optim.held_weights(p)
    assert y is not None and _same_bits(y, inside[-1][3]) and not _same_bits(p.data, y)
    _check_x(p.data, y, st["z"], f"after fit, clip {clip}")
    assert torch.isfinite(p.data).all() and float((p.data - flat0.to(p.device)).abs().max()) > 0
    assert torch.equal(tr.unet.shadow, p.detach().bfloat16())  # written by the exchange


# ------------------------------------------------------------------------------------------------------------ validation
class _PassRecorder:
    """listed by the user, so after the mode handling Fitter installs: what the weights are inside a validation pass"""

    def __init__(self, save_at=None, path=None):
        self.inside, self.save_at, self.path = [], save_at, path

    def on_validation_epoch_start(self, fitter, module):
        p = module.unet.flat
        opt = fitter._fit_state[1]
        held = opt.held_weights(p)
        self.inside.append({"flat": p.detach().clone(), "shadow": module.unet.shadow.detach().clone(), "sanity": fitter.sanity_checking,
                            "step": fitter.global_step, "held": None if held is None else held.detach().clone(),
                            "z": opt.state[p]["z"].detach().clone() if p in opt.state else None,
                            "train_mode": opt.param_groups[0]["train_mode"]})
        if self.save_at is not None and fitter.global_step == self.save_at and not fitter.sanity_checking:
            ptrs = (p.data_ptr(), held.data_ptr())
            fitter.save_checkpoint(self.path)
            assert ptrs == (p.data_ptr(), opt.held_weights(p).data_ptr())
            assert _same_bits(p.data, self.inside[-1]["flat"]) and _same_bits(opt.held_weights(p), self.inside[-1]["held"])


def _seed_at(step):
    from uwudiff_amd.engine import seed_everything

    def hook(f):
        if f.global_step == step:
            seed_everything(777)

    return hook


@pytest.fixture(scope="module")
def val_runs(tmp_path_factory):
    """run A validates after every 2 batches (and writes a checkpoint from inside the pass at step 2), run B never validates; both
    re-seed after step 2, where run C resumes from A's file"""
    from uwudiff_amd.engine import seed_everything

    tmp = tmp_path_factory.mktemp("sf_val")
    path = str(tmp / "inside_val.ckpt")
    out = {"path": path}
    for name, val in (("a", True), ("b", False)):
        rec = _PassRecorder(save_at=2, path=path)
        fit, dm, tr = _fresh(tmp, 4, callbacks=[rec] if val else [], unet=ELEMENTWISE, val=val)
        steps = []
        fit.step_hooks.append(lambda f, tr=tr, steps=steps: steps.append(_snapshot(f, tr.unet.flat)))
        fit.step_hooks.append(_seed_at(2))
        hist = fit.fit(tr, dm)
        out[name] = {"fit": fit, "tr": tr, "rec": rec, "steps": steps, "hist": hist, "end": _snapshot(fit, tr.unet.flat)}
    rec = _PassRecorder()
    fit, dm, tr = _fresh(tmp, 4, callbacks=[rec], unet=ELEMENTWISE, val=True)
    orig = fit.load_checkpoint

    def load_and_seed(p):
        res = orig(p)
        out["c_loaded"] = _snapshot(fit, tr.unet.flat)
        seed_everything(777)
        return res

    fit.load_checkpoint = load_and_seed
    hist = fit.fit(tr, dm, ckpt_path=path)
    out["c"] = {"fit": fit, "tr": tr, "rec": rec, "hist": hist, "end": _snapshot(fit, tr.unet.flat)}
    out["ck"] = torch.load(path, map_location="cpu", weights_only=True)
    return out


def test_validation_does_not_disturb_training(val_runs):
    a, b = val_runs["a"], val_runs["b"]
    assert a["fit"].global_step == b["fit"].global_step == 4 and len(a["fit"].val_history) == 2 and not b["fit"].val_history
    assert isinstance(a["tr"].unet, ElementwiseDenoiser)
    for sa, sb in zip(a["steps"] + [a["end"]], b["steps"] + [b["end"]]):
        for k in ("y", "z", "v", "flat"):
            assert _same_bits(sa[k], sb[k]), k
        assert all(sa[k] == sb[k] for k in SCALARS)
    assert a["end"]["k"] == 4 and a["end"]["train_mode"] is False and all(s["train_mode"] is True for s in a["steps"])
    assert not _same_bits(a["steps"][3]["y"], a["steps"][1]["y"])


def test_validation_runs_on_x(val_runs):
    a = val_runs["a"]
    seen = a["rec"].inside
    assert [(p["step"], p["sanity"]) for p in seen] == [(0, True), (2, False), (4, False)]
    assert all(p["train_mode"] is False for p in seen)
    assert seen[0]["held"] is None  # the sanity check at step 0: x = y = z, nothing is exchanged
    for p, step in zip(seen[1:], (a["steps"][1], a["steps"][3])):
        assert _same_bits(p["held"], step["y"]) and _same_bits(p["z"], step["z"])  # y is kept aside, bit for bit
        _check_x(p["flat"], step["y"], step["z"], f"inside the pass at step {p['step']}")
        assert not _same_bits(p["flat"], step["y"]) and _same_bits(p["shadow"], p["flat"].bfloat16())


def test_checkpoint_from_inside_a_validation_pass_resumes_bit_for_bit(val_runs):
    a, c, ck = val_runs["a"], val_runs["c"], val_runs["ck"]
    at2, inside = a["steps"][1], a["rec"].inside[1]
    assert ck["global_step"] == 2 and list(ck["state_dict"]) == list(ck["current_model_state"])
    sd = {k[5:]: v for k, v in ck["state_dict"].items() if k.startswith("unet.")}
    cur = {k[5:]: v for k, v in ck["current_model_state"].items() if k.startswith("unet.")}
    unet = a["tr"].unet
    for k, v in unet._public_views(inside["flat"]):
        assert _same_bits(sd[k], v), k  # state_dict holds x
    for k, v in unet._public_views(at2["y"]):
        assert _same_bits(cur[k], v), k  # current_model_state holds y
    opt_ck = ck["optimizer_states"][0]
    assert opt_ck["param_groups"][0]["k"] == 2 and _same_bits(opt_ck["state"][0]["z"], at2["z"])
    loaded = val_runs["c_loaded"]
    assert _same_bits(loaded["flat"], at2["y"]) and _same_bits(loaded["z"], at2["z"]) and _same_bits(loaded["v"], at2["v"])
    assert c["fit"].global_step == 4 and len(c["hist"]) == 2
    for k in ("y", "z", "v", "flat"):
        assert _same_bits(c["end"][k], a["end"][k]), k
    assert all(c["end"][k] == a["end"][k] for k in SCALARS)
    assert [(p["step"], p["sanity"]) for p in c["rec"].inside] == [(4, False)]
    assert _same_bits(c["rec"].inside[0]["flat"], a["rec"].inside[2]["flat"])


# ------------------------------------------------------------------------------------------------------------ checkpoints
@pytest.fixture(scope="module")
def resumed(tmp_path_factory):
    """run A: 5 uninterrupted steps, a checkpoint written after step 3; run B: fresh objects resumed from that file (the RNG re-seeded
    at the same point of both, the pattern of tests/test_optimizers_gpu.py)"""
    from uwudiff_amd.engine import seed_everything

    tmp = tmp_path_factory.mktemp("sf_resume")
    path = str(tmp / "step3.ckpt")
    at3 = {}
    fit, dm, tr = _fresh(tmp, 5, unet=ELEMENTWISE)

    def save_at_3(f):
        if f.global_step == 3:
            p = tr.unet.flat
            at3.update(_snapshot(f, p))
            at3["weights"] = {k: v.detach().clone() for k, v in tr.unet.state_dict().items()}
            at3["ptr"] = p.data_ptr()
            f.save_checkpoint(path)
            at3["after"] = _snapshot(f, p)
            at3["ptr_after"] = p.data_ptr()
            seed_everything(777)

    fit.step_hooks.append(save_at_3)
    fit.fit(tr, dm)
    fit2, dm2, tr2 = _fresh(tmp, 5, unet=ELEMENTWISE)
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        loaded.update(_snapshot(fit2, tr2.unet.flat))
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    return {"a": (fit, tr), "b": (fit2, tr2), "hist_b": hist_b, "at3": at3, "loaded": loaded, "path": path, "tmp": tmp,
            "ck": torch.load(path, map_location="cpu", weights_only=True)}


def test_checkpoint_holds_x_and_y(resumed):
    ck, at3 = resumed["ck"], resumed["at3"]
    tr = resumed["a"][1]
    assert ck["global_step"] == 3 and list(ck["state_dict"]) == list(ck["current_model_state"])
    keys = [k for k in ck["state_dict"] if k.startswith("unet.")]
    assert [k[5:] for k in keys] == list(at3["weights"])
    for k in keys:
        assert _same_bits(ck["current_model_state"][k], at3["weights"][k[5:]]), k  # y, as training had it
    x = at3["y"].clone()  # (every tensor of the buffer is overwritten from the file)
    for k, v in tr.unet._public_views(x):
        v.copy_(ck["state_dict"]["unet." + k])
    _check_x(x, at3["y"], at3["z"], "state_dict of the checkpoint after step 3")
    assert not _same_bits(x, at3["y"])
    for k in ck["state_dict"]:
        if not k.startswith("unet."):  # buffers and the other sub-modules as they are
            assert _same_bits(ck["state_dict"][k], ck["current_model_state"][k]), k
    # no weight was written and no pointer moved while saving, and training stayed in train mode
    assert at3["ptr"] == at3["ptr_after"] and at3["after"]["train_mode"] is True
    for k in ("y", "z", "v", "flat"):
        assert _same_bits(at3[k], at3["after"][k]), k
    g = ck["optimizer_states"][0]["param_groups"][0]
    assert GROUP_KEYS <= set(g) and g["k"] == 3 and g["train_mode"] is True and g["weight_sum"] == at3["weight_sum"]
    st = ck["optimizer_states"][0]["state"][0]
    assert set(st) == {"z", "exp_avg_sq"} and _same_bits(st["z"], at3["z"]) and _same_bits(st["exp_avg_sq"], at3["v"])


def test_the_prefix_loader_reads_x(resumed):
    from duwu.loader import load_any

    ck = resumed["ck"]
    model = load_any({"_target_": ELEMENTWISE,
                      "_load_config_": {"ckpt_path": resumed["path"], "state_dict_key": "state_dict", "state_dict_prefix": "unet."}})
    for k, v in model.state_dict().items():
        assert _same_bits(v, ck["state_dict"]["unet." + k]), k


def test_resume_is_bit_identical_to_the_uninterrupted_run(resumed):
    (fit, tr), (fit2, tr2), loaded, at3 = resumed["a"], resumed["b"], resumed["loaded"], resumed["at3"]
    assert fit.global_step == fit2.global_step == 5 and len(resumed["hist_b"]) == 2
    for k in ("y", "z", "v"):  # the resumed run starts from y and the file's state
        assert _same_bits(loaded[k], at3[k]), k
    assert _same_bits(loaded["flat"], at3["y"])
    a, b = _snapshot(fit, tr.unet.flat), _snapshot(fit2, tr2.unet.flat)
    for k in ("y", "z", "v", "flat"):
        assert _same_bits(a[k], b[k]), k
        assert not _same_bits(b[k], loaded[k]), k  # steps 4-5 did move them
    assert all(a[k] == b[k] for k in SCALARS) and b["k"] == 5 and b["train_mode"] is False
    assert torch.equal(tr2.unet.shadow, tr2.unet.flat.detach().bfloat16())


def test_a_checkpoint_without_current_model_state_starts_from_the_loaded_weights(resumed, capsys):
    ck = dict(resumed["ck"])
    ck["state_dict"] = ck.pop("current_model_state")  # (what a loader that knows one set of weights would keep)
    path = str(resumed["tmp"] / "plain.ckpt")
    torch.save(ck, path)
    fit, dm, tr = _fresh(resumed["tmp"], 3, unet=ELEMENTWISE)  # (max_steps = the checkpoint's step: nothing is trained)
    capsys.readouterr()
    fit.fit(tr, dm, ckpt_path=path)
    out = capsys.readouterr().out
    assert out.count("no current_model_state") == 1 and "y = the loaded weights" in out
    end = _snapshot(fit, tr.unet.flat)
    assert _same_bits(end["y"], resumed["at3"]["y"]) and _same_bits(end["z"], resumed["at3"]["z"]) and end["k"] == 3


# ------------------------------------------------------------------------------------------------------------ accumulation
def test_accumulation_counts_optimizer_steps(tmp_path):
    fit, dm, tr = _fresh(tmp_path, 2, clip=1.0, n_acc=2)
    hist = fit.fit(tr, dm)
    g = fit._fit_state[1].param_groups[0]
    assert fit.global_step == 2 and fit.train_batches == 4 and g["k"] == 2
    assert len(hist) == 2 and all(math.isfinite(h["loss"]) for h in hist)
    assert torch.isfinite(tr.unet.flat.detach()).all()


# ------------------------------------------------------------------------------------------------------------ adapters
def test_adapters_train_and_the_checkpoint_holds_the_averaged_adapters(tmp_path):
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    fit, dm, tr = _fresh(tmp_path, 2, clip=1.0, lyc=TOML)
    base0 = tr.unet.flat.detach().clone()
    ad0 = tr.lycoris_model.flat.detach().clone()
    call = {}

    def remember(mod, args, kwargs):
        if torch.is_grad_enabled():  # (the training forward's inputs, to run again below)
            call["args"], call["kwargs"] = args, kwargs

    tr.unet.register_forward_pre_hook(remember, with_kwargs=True)

    def forward(unet):
        with torch.no_grad():
            out = unet(*call["args"], **call["kwargs"])
        return (out[0] if isinstance(out, (tuple, list)) else getattr(out, "sample", out)).detach().float().clone()

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def after_step(f):
        assert not tr.lycoris_model.flat.grad.any()

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    lyc = tr.lycoris_model
    assert type(optim) is FusedAdamWScheduleFree and list(optim.state) == [lyc.flat]
    assert fit.global_step == 2 and all(math.isfinite(h["loss"]) for h in hist) and optim.param_groups[0]["k"] == 2
    assert float((lyc.flat.detach() - ad0.to(lyc.flat.device)).abs().max()) > 0
    assert _same_bits(tr.unet.flat.detach(), base0) and tr.unet.flat.grad is None  # the frozen base
    y = optim.held_weights(lyc.flat)
    assert y is not None and not _same_bits(lyc.flat.data, y)
    _check_x(lyc.flat.data, y, optim.state[lyc.flat]["z"], "adapters after fit")
    path = str(tmp_path / "end.ckpt")
    ck = fit.save_checkpoint(path)
    held = {k[len("lycoris_model."):]: v for k, v in ck["state_dict"].items() if k.startswith("lycoris_model.")}
    assert list(held) == list(lyc.state_dict()) and all(_same_bits(v, lyc.state_dict()[k]) for k, v in held.items())
    assert any(not _same_bits(ck["state_dict"][k], ck["current_model_state"][k]) for k in ck["state_dict"] if k.startswith("lycoris_model."))
    y_a, y_a2 = forward(tr.unet), forward(tr.unet)  # (the UNet merges the averaged adapters; the same weights again: its own noise)
    # a fresh UNet with the adapters of the checkpoint's state_dict
    fit2, dm2, tr2 = _fresh(tmp_path, 2, clip=1.0, lyc=TOML)
    assert _same_bits(tr2.unet.flat.detach(), base0)
    if hasattr(tr.unet, "cfg"):  # (what fit sets before it moves the module)
        tr2.unet.cfg.compute_dtype = tr.unet.cfg.compute_dtype
    tr2.unet.P.bf16 = tr.unet.P.bf16
    tr2.to(tr.unet.flat.device)
    from_file = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
    tr2.lycoris_model.load_state_dict({k[len("lycoris_model."):]: v for k, v in from_file.items() if k.startswith("lycoris_model.")})
    for k, v in tr2.lycoris_model.state_dict().items():
        assert _same_bits(v, held[k]), k
    tr2.unet.refresh_shadow()
    y_b = forward(tr2.unet)
    noise, moved = rel(y_a2, y_a), rel(y_b, y_a)
    print(f"UNet output: the same weights again {noise:.3e}, a fresh UNet with the checkpoint's adapters {moved:.3e}")
    # the bound of the adapter tests of tests/test_averaging_gpu.py: the forward's own run-to-run noise, the bf16 floor 1e-3
    assert torch.isfinite(y_a).all() and moved <= max(3 * noise, 1e-3)


# ------------------------------------------------------------------------------------------------------------ refusals, the config
def test_a_weight_averaging_callback_is_refused(tmp_path):
    from uwudiff_amd.averaging import EMAWeightAveraging

    fit, dm, tr = _fresh(tmp_path, 2, callbacks=[EMAWeightAveraging(decay=0.9)], unet=ELEMENTWISE)
    flat0 = tr.unet.flat.detach().clone()
    seen = []
    fit.step_hooks.append(lambda f: seen.append(f.global_step))
    with pytest.raises(ValueError, match="EMAWeightAveraging.*FusedAdamWScheduleFree"):
        fit.fit(tr, dm)
    assert not seen and fit.global_step == 0 and _same_bits(tr.unet.flat.detach().cpu(), flat0.cpu())  # before the first batch


def test_learning_rate_monitor_logs_scheduled_lr(tmp_path):
    from uwudiff_amd.engine import LearningRateMonitor

    fit, dm, tr = _fresh(tmp_path, 3, callbacks=[LearningRateMonitor()], unet=ELEMENTWISE)
    hist = fit.fit(tr, dm)
    assert [h["scheduled_lr"] for h in hist] == [0.5e-3, 1e-3, 1e-3] and all(h["lr"] == 1e-3 for h in hist)  # warmup_steps = 2


def test_the_schedulefree_config_loads_and_trains():
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_schedulefree.yaml")),
                {"lightning_config": {"fast_dev_run": False, "max_steps": 2, "log_every_n_steps": 1, "limit_val_batches": 0},
                 "data": {"dataloader_config": {"num_workers": 0}}})
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    fit = Fitter(**lc)
    dm, tr = load_all(cfg)
    seed_everything(cfg.seed)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedAdamWScheduleFree and fit._fit_state[2] is None  # no scheduler
    g = optim.param_groups[0]
    assert fit.global_step == 2 and g["k"] == 2 and g["warmup_steps"] == 4 and g["scheduled_lr"] == 1e-4 * 2 / 4
    assert all(math.isfinite(h["loss"]) for h in hist) and g["train_mode"] is False


def test_launcher_runs_the_schedulefree_config(tmp_path):
    """the launcher trains, validates on x and writes checkpoints whose state_dict (x) the unet node's loader picks up"""
    import glob
    import subprocess
    import sys

    from duwu.loader import load_any
    from uwudiff_amd.config import load_yaml

    yaml = os.path.join(ROOT, "configs", "demo_training_schedulefree.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_train.py"), "--configs", yaml], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count('"val/loss"') == 2
    files = sorted(glob.glob(str(tmp_path / "checkpoints" / "*.ckpt")))
    assert len(files) == 2, files  # the best two by val/loss of the two passes
    for f in files:
        ck = torch.load(f, map_location="cpu", weights_only=True)
        assert list(ck["current_model_state"]) == list(ck["state_dict"])
        g = ck["optimizer_states"][0]["param_groups"][0]
        assert g["k"] == ck["global_step"] and g["train_mode"] is True and g["warmup_steps"] == 4
        assert any(not _same_bits(ck["state_dict"][k], ck["current_model_state"][k]) for k in ck["state_dict"] if k.startswith("unet."))
        assert math.isfinite(float(ck["state_dict"]["ema_loss"]))
    node = dict(load_yaml(yaml)["trainer"]["model_config"]["unet"])
    node["_load_config_"] = {"ckpt_path": files[-1], "state_dict_key": "state_dict", "state_dict_prefix": "unet."}
    for k, v in load_any(node).state_dict().items():
        assert _same_bits(v, ck["state_dict"]["unet." + k]), k
