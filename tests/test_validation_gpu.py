"""GPU tests of the validation loop: ``uwu_timestep_stats_accum`` against an ordered loop in numpy float64
(exact equality: the product of two floats is exact in double, and the additions happen in the same order), its refusals, a fit
with a validation set -- what a pass records, that every pass draws the same timesteps and noise, and that it leaves training where it
was -- the plot callback, and float timesteps through ``Fitter.validate``."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


def numpy_stats(losses, timesteps, n_steps, stats=None):
    """the reference: samples in ascending b, float64 throughout, bucket = trunc toward zero"""
    st = np.zeros((3, n_steps), dtype=np.float64) if stats is None else stats
    for l, t in zip(np.asarray(losses, dtype=np.float32), np.asarray(timesteps)):
        if np.isnan(t) or not (-1 < t < n_steps):
            continue
        k = int(np.trunc(t))
        l = np.float64(l)
        st[0, k] += 1.0
        st[1, k] += l
        st[2, k] += l * l
    return st


def run_kernel(losses, timesteps, n_steps, state=None, loss=None):
    from uwudiff_amd.validation import TimestepLossStats

    st = state or TimestepLossStats(n_steps, "cuda")
    st.update(losses.cuda(), timesteps.cuda(), None if loss is None else loss.cuda())
    return st


def draws(B, n_steps, kind, seed):
    g = torch.Generator().manual_seed(seed)
    losses = torch.randn(B, generator=g).abs() * 0.3
    if kind == "int64":
        t = torch.randint(0, n_steps, (B,), generator=g)
    else:  # fractions, and what lies just outside: (-1, 0) truncates to bucket 0
        t = torch.rand(B, generator=g) * (n_steps + 1.5) - 0.75
    return losses, t


@pytest.mark.parametrize("kind", ["int64", "fp32"])
@pytest.mark.parametrize("B,n_steps", [(1, 1), (7, 10), (64, 10), (257, 1000), (1000, 10), (1000, 1000)])
def test_kernel_matches_the_ordered_float64_loop(B, n_steps, kind):
    losses, t = draws(B, n_steps, kind, seed=B * 7 + n_steps)
    st = run_kernel(losses, t, n_steps)
    got = st.state.cpu().numpy()
    want = numpy_stats(losses.numpy(), t.numpy(), n_steps)
    assert np.array_equal(got[:3 * n_steps].reshape(3, n_steps), want)
    assert got[3 * n_steps:].tolist() == [0.0, 0.0]  # no scalar loss was passed: totals untouched
    if kind == "int64":
        assert want[0].sum() == B


def test_out_of_range_and_fractional_timesteps():
    n = 10
    losses = torch.arange(1, 9, dtype=torch.float32) / 8
    for t in (torch.tensor([-1, n, n + 5, 0, 9, 3, -7, 2 ** 40]),
              torch.tensor([-1.0, float(n), n + 5.0, -0.5, 9.99, 3.9, float("nan"), float("inf")])):
        got = run_kernel(losses, t, n).state.cpu().numpy()[:3 * n].reshape(3, n)
        want = np.zeros((3, n))
        for b, k in ((3, 0), (4, 9), (5, 3)):
            l = float(losses[b])
            want[:, k] += (1.0, l, l * l)
        assert np.array_equal(got, want)


def test_nan_and_inf_losses_stay_in_their_buckets():
    n = 10
    losses, t = draws(64, n, "int64", seed=5)
    t[10], t[20] = 4, 6
    t[(t == 4) & (torch.arange(64) != 10)] = 5
    t[(t == 6) & (torch.arange(64) != 20)] = 7
    losses[10], losses[20] = float("nan"), float("inf")
    got = run_kernel(losses, t, n).state.cpu().numpy()[:3 * n].reshape(3, n)
    want = numpy_stats(losses.numpy(), t.numpy(), n)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[1:, 4]).all() and np.isinf(got[1:, 6]).all() and got[0, 4] == got[0, 6] == 1
    assert np.isfinite(np.delete(got, [4, 6], axis=1)).all()


def test_two_calls_equal_one_call_on_the_concatenation_and_totals():
    n = 1000
    a, ta = draws(257, n, "int64", seed=1)
    b, tb = draws(1000, n, "int64", seed=2)
    st = run_kernel(a, ta, n, loss=a.mean())
    run_kernel(b, tb, n, state=st, loss=b.mean())
    one = run_kernel(torch.cat([a, b]), torch.cat([ta, tb]), n)
    got = st.state.cpu().numpy()
    assert np.array_equal(got[:3 * n], one.state.cpu().numpy()[:3 * n])
    assert got[3 * n:].tolist() == [sum([257 * float(a.mean()), 1000 * float(b.mean())]), 1257.0]
    res = st.compute()
    assert res["loss"] == got[3 * n] / 1257.0 and res["n_samples"] == 1257
    st.reset()
    assert float(st.state.abs().sum()) == 0.0


def test_refusals_leave_the_accumulator_untouched():
    from uwudiff_amd import lib as L

    n, B = 10, 8
    losses = torch.rand(B, device="cuda")
    t = torch.randint(0, n, (B,), device="cuda")
    lm = losses.mean().reshape(1)
    stats = torch.full((3 * n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    tot = stats[3 * n:].data_ptr()
    ok = dict(losses=L.ptr(losses), timesteps=L.ptr(t), t_dtype=L.I64, loss_mean=L.ptr(lm), B=B, n_steps=n, stats=L.ptr(stats), totals=tot)
    bad = [dict(B=0), dict(B=-3), dict(n_steps=0), dict(n_steps=65537), dict(losses=None), dict(timesteps=None), dict(stats=None),
           dict(totals=None), dict(t_dtype=L.BF16), dict(t_dtype=7)]
    for change in bad:
        args = {**ok, **change}
        with pytest.raises(L.UwuError, match="timestep_stats_accum"):
            L.call("uwu_timestep_stats_accum", *args.values(), L.stream())
    torch.cuda.synchronize()
    assert bool((stats == SENTINEL).all())
    # the same call with nothing wrong goes through; without a scalar loss totals may be NULL
    stats.zero_()
    L.call("uwu_timestep_stats_accum", *ok.values(), L.stream())
    L.call("uwu_timestep_stats_accum", *{**ok, "loss_mean": None, "totals": None}.values(), L.stream())
    got = stats.cpu().numpy()
    assert got[:n].sum() == 2 * B and got[3 * n + 1] == B
    big = torch.zeros(3 * 65536, dtype=torch.float64, device="cuda")  # the upper bound itself is in range
    L.call("uwu_timestep_stats_accum", *{**ok, "n_steps": 65536, "stats": L.ptr(big), "loss_mean": None, "totals": None}.values(), L.stream())
    assert float(big[:65536].sum()) == B and float(big[n:65536].sum()) == 0.0


# ---------------------------------------------------------------------- fit with a validation set
class _Recorder:
    """what the callbacks see of every pass, and -- wrapped round Fitter.validate -- the training state before and after it"""

    def __init__(self):
        self.passes, self.around = [], []

    def on_validation_epoch_start(self, trainer, pl_module):
        self.cur = {"step": trainer.global_step, "sanity": trainer.sanity_checking, "B": [], "loss": [], "losses": [], "timesteps": [],
                    "noisy": [], "eval": not pl_module.training and not pl_module.unet.training, "grad": torch.is_grad_enabled()}

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        loss, aux = outputs
        c = self.cur
        c["B"].append(batch[0].shape[0])
        c["loss"].append(loss.detach().clone())
        c["losses"].append(aux.losses.detach().clone())
        c["timesteps"].append(aux.timesteps.detach().clone())
        c["noisy"].append(aux.noisy_latent.detach().clone())

    def on_validation_epoch_end(self, trainer, pl_module):
        self.passes.append(self.cur)

    def wrap(self, fit):
        inner = fit.validate

        def snapshot(module):
            _, opt, _ = fit._fit_state
            gen = torch.cuda.default_generators[torch.cuda.current_device()]
            flat = module.unet.flat
            return {"cuda_rng": (gen.initial_seed(), gen.get_offset()), "cpu_rng": torch.get_rng_state(), "flat": flat.detach().clone(),
                    "grad": None if flat.grad is None else flat.grad.detach().clone(), "ema": module.ema_loss.detach().clone(),
                    "opt_step": int(opt.state_dict()["state"][0]["step"]) if opt.state_dict()["state"] else 0,
                    "training": [m.training for m in module.modules()], "global_step": fit.global_step}

        def validate(module, loader, **kw):
            before = snapshot(module)
            rec = inner(module, loader, **kw)
            self.around.append((before, snapshot(module)))
            return rec

        fit.validate = validate


def _fit(root, with_val):
    from duwu.loader import load_all
    from duwu.trainer.callbacks import PlotValLossPerTimestep
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    extra = {"lightning_config": {"fast_dev_run": False, "max_steps": 5, "log_every_n_steps": 1, "val_check_interval": 2,
                                  "check_val_every_n_epoch": None, "num_sanity_val_steps": 1},
             "trainer": {"lr": 1e-3}}
    if with_val:
        extra["data"] = {"val_dataset_config": {"_target_": "duwu.data.DummyDataset", "sample_size": [4, 32, 32], "n_samples": 40}}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml")), extra)
    seed_everything(cfg.seed)
    rec, plot = _Recorder(), PlotValLossPerTimestep()
    fit = Fitter(callbacks=[rec, plot], default_root_dir=str(root), **cfg["lightning_config"])
    dm, tr = load_all(cfg)
    rec.wrap(fit)
    hist = fit.fit(tr, dm)
    return {"fit": fit, "rec": rec, "plot": plot, "hist": hist, "tr": tr, "root": str(root)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return {"val": _fit(tmp_path_factory.mktemp("val"), True), "plain": _fit(tmp_path_factory.mktemp("plain"), False)}


def test_fit_records_the_scheduled_passes(runs):
    r = runs["val"]
    fit, passes = r["fit"], r["rec"].passes
    assert [(p["step"], p["sanity"], p["B"]) for p in passes] == [(0, True, [16]), (2, False, [16, 16, 8]), (4, False, [16, 16, 8])]
    assert all(p["eval"] and not p["grad"] for p in passes)
    assert [(h["step"], h["val_samples"]) for h in fit.val_history] == [(2, 40), (4, 40)]  # the sanity pass is absent
    assert fit.global_step == 5 and len(r["hist"]) == 5
    for h, p in zip(fit.val_history, passes[1:]):
        want = sum([B * float(l) for B, l in zip(p["B"], p["loss"])]) / 40  # the sample-weighted mean, not the mean of three means
        print(f"step {h['step']}: val/loss {h['val/loss']!r}, from the batches' scalars {want!r}")
        assert h["val/loss"] == want
    assert runs["plain"]["fit"].val_history == [] and runs["plain"]["rec"].passes == []


def test_every_pass_draws_the_same_timesteps_and_noise(runs):
    r = runs["val"]
    _, p2, p4 = r["rec"].passes
    for a, b in zip(p2["timesteps"], p4["timesteps"]):
        assert torch.equal(a, b)
    for a, b in zip(p2["noisy"], p4["noisy"]):
        assert torch.equal(a, b)
    assert torch.equal(r["rec"].passes[0]["timesteps"][0], p2["timesteps"][0])  # (the sanity pass too)
    v2, v4 = (h["val/loss"] for h in r["fit"].val_history)
    assert v2 != v4  # two AdamW steps at lr 1e-3 lie between them


def test_a_pass_leaves_training_where_it_was(runs):
    r = runs["val"]
    assert len(r["rec"].around) == 3
    for before, after in r["rec"].around:
        assert before["cuda_rng"] == after["cuda_rng"]
        assert torch.equal(before["cpu_rng"], after["cpu_rng"])
        assert torch.equal(before["flat"].view(torch.int32), after["flat"].view(torch.int32))
        assert (before["grad"] is None) == (after["grad"] is None)
        if before["grad"] is not None:
            assert torch.equal(before["grad"].view(torch.int32), after["grad"].view(torch.int32))
        assert torch.equal(before["ema"], after["ema"])
        assert before["opt_step"] == after["opt_step"] and before["global_step"] == after["global_step"]
        assert before["training"] == after["training"]
    assert r["tr"].training and r["tr"].unet.training


def test_training_losses_equal_the_run_without_a_validation_set(runs):
    a = [h["loss"] for h in runs["val"]["hist"]]
    b = [h["loss"] for h in runs["plain"]["hist"]]
    print("max relative difference of the training losses:", max(abs(x - y) / abs(y) for x, y in zip(a, b)))
    # rel 1e-4: the project's bound on this config and lr for run-to-run differences from fp32 atomics (tests/test_train_gpu.py)
    assert len(a) == len(b) == 5 and a == pytest.approx(b, rel=1e-4)


def test_plot_callback_matches_the_captured_losses(runs):
    r = runs["val"]
    plot, passes = r["plot"], r["rec"].passes
    for p in passes:
        losses = torch.cat(p["losses"]).cpu().numpy()
        t = torch.cat(p["timesteps"]).cpu().numpy()
        st = numpy_stats(losses, t, 1000)
        seen = st[0] > 0
        mean = st[1][seen] / st[0][seen]
        std = np.sqrt(np.maximum(st[2][seen] / st[0][seen] - mean * mean, 0.0))
        want = {"timesteps": np.nonzero(seen)[0], "count": st[0][seen], "mean": mean, "std": std}
        stem = os.path.join(r["root"], "plots", f"losses_per_timestep-training_step-{p['step']}")
        with np.load(stem + ".npz") as z:
            for k, v in want.items():
                assert np.array_equal(z[k], v), (p["step"], k)
        if p is passes[-1]:
            for k, v in want.items():
                assert np.array_equal(plot.last[k], v), k
    assert int(plot.last["count"].sum()) == 40


def test_plot_callback_writes_the_png(runs):
    pytest.importorskip("matplotlib")
    png = os.path.join(runs["val"]["root"], "plots", "losses_per_timestep-training_step-4.png")
    assert open(png, "rb").read(4) == b"\x89PNG"


def test_float_timesteps_fall_into_their_truncated_buckets(tmp_path):
    """RectifiedFlowLoss(time_sampling_type="uniform_time") hands out fp32 timesteps with fractions (rectified_flow.py:37-47)"""
    from duwu.trainer.callbacks import PlotValLossPerTimestep
    from duwu.trainer.trainer import DMTrainer
    from uwudiff_amd.engine import Fitter

    torch.manual_seed(3)
    mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config",
                   "config": dict(depth=2, hidden=128, heads=2, patch=2, sample_size=16, in_channels=4, out_channels=4, cond_dim=0)}}
    loss = {"_target_": "duwu.loss.RectifiedFlowLoss", "time_sampling_type": "uniform_time",
            "scheduler": {"_target_": "uwudiff_amd.scheduler.EulerDiscreteScheduler.from_pretrained", "pretrained_model_name_or_path": "sdxl"}}
    tr = DMTrainer(mc, loss_config=loss, use_warm_up=False, lr_scheduler=None).cuda()
    rec, plot = _Recorder(), PlotValLossPerTimestep()
    fit = Fitter(callbacks=[rec, plot], default_root_dir=str(tmp_path))
    batches = [(torch.randn(n, 4, 16, 16), [""] * n, [], {}, {}) for n in (16, 16, 8)]
    out = fit.validate(tr, batches)
    t = torch.cat(rec.passes[0]["timesteps"]).cpu()
    losses = torch.cat(rec.passes[0]["losses"]).cpu()
    assert t.dtype == torch.float32 and bool((t != t.trunc()).any()) and out["val_samples"] == 40
    res = plot.last
    want = numpy_stats(losses.numpy(), t.numpy(), 1000)
    assert np.array_equal(res["timesteps"], np.unique(t.trunc().long().numpy()))
    assert res["count"].sum() == 40 and np.array_equal(res["count"], want[0][want[0] > 0])
    assert np.array_equal(fit.val_stats.state.cpu().numpy()[:3000].reshape(3, 1000), want)
