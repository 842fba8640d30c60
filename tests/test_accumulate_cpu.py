"""CPU tests of gradient accumulation in the fit loop (``Fitter(accumulate_grad_batches=N)``): when an
optimizer step is taken, what the optimizer is handed, which counters count optimizer steps and which count batches, validation
inside a window, checkpoints at and inside a window, and the data-parallel exchange over two gloo ranks (one exchange per
optimizer step, none inside a window).  The device path is tested in tests/test_accumulate_gpu.py."""
import os
import socket
from typing import NamedTuple

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAM = 12


class _Aux(NamedTuple):
    losses: torch.Tensor
    timesteps: torch.Tensor


class _FakeUnet(nn.Module):
    """One flat parameter + the DiT's `set_grad_ready_hook` contract (slices reported from inside every backward)."""

    def __init__(self, n=N_PARAM, dtype=torch.float32):
        super().__init__()
        self.flat = nn.Parameter(torch.arange(n, dtype=dtype) / n)
        self._hook = None
        self.fired = 0
        self.flat.register_post_accumulate_grad_hook(self._fire)

    def _fire(self, p):
        self.fired += 1
        if self._hook is not None:
            n = p.numel()
            self._hook(p.grad, [(n // 2, n - n // 2, None)])

    def set_grad_ready_hook(self, hook, group_layers=4):
        self._hook = hook


class _CountingScheduler:
    def __init__(self):
        self.n = 0

    def step(self):
        self.n += 1


class _Linear(nn.Module):
    """the trainer of tests/test_engine_cpu.py: the gradient of a batch is mean(x) in every element, whatever the parameters"""

    n_diffusion_time_steps = 10

    def __init__(self, opt_cls=torch.optim.SGD, lr=0.1):
        super().__init__()
        self.unet = _FakeUnet()
        self.register_buffer("ema_loss", torch.tensor(0.0))
        self.opt_cls, self.lr = opt_cls, lr
        self.sched = _CountingScheduler()
        self.spied, self.seen, self.grad_at_entry = [], [], []

    def configure_optimizers(self):
        opt = self.opt_cls(self.unet.parameters(), lr=self.lr)
        inner = opt.step

        def step(*a, **kw):  # what the optimizer is handed
            self.spied.append(self.unet.flat.grad.detach().clone())
            return inner(*a, **kw)

        opt.step = step
        self.opt = opt
        return {"optimizer": opt, "lr_scheduler": {"scheduler": self.sched}}

    def training_step(self, batch, idx):
        g = self.unet.flat.grad
        self.seen.append(float(batch[0].flatten()[0]))
        self.grad_at_entry.append(None if g is None else g.detach().clone())
        return {"loss": (self.unet.flat * batch[0].mean()).sum()}

    def validation_step(self, batch, idx):
        x = batch[0]
        losses = (x * self.unet.flat.detach()[: x.numel()]).float()
        return losses.mean(), _Aux(losses=losses, timesteps=torch.arange(x.numel()) % self.n_diffusion_time_steps)


class _Regress(_Linear):
    """a loss that is a per-sample mean and whose gradient depends on the parameters: mean_i 0.5 (w . x_i - sum(x_i))^2"""

    def __init__(self, dtype=torch.float64, **kw):
        super().__init__(**kw)
        self.unet = _FakeUnet(dtype=dtype)

    def training_step(self, batch, idx):
        x = batch[0]
        self.seen.append(float(x.flatten()[0]))
        g = self.unet.flat.grad
        self.grad_at_entry.append(None if g is None else g.detach().clone())
        r = x @ self.unet.flat - x.sum(dim=1)
        return {"loss": 0.5 * (r * r).mean()}

    def validation_step(self, batch, idx):
        x = batch[0]
        r = (x @ self.unet.flat.detach() - x.sum(dim=1)).float()
        return (r * r).mean(), _Aux(losses=r * r, timesteps=torch.arange(x.shape[0]) % self.n_diffusion_time_steps)


def _batch(x):
    return (x, [""] * x.shape[0], [], {}, {})


class _DM:
    """`n` batches per epoch; batch i (1-based) is filled with i"""

    def __init__(self, n=4, val=False):
        self.n, self.val = n, val

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [_batch(torch.full((4,), float(i + 1))) for i in range(self.n)]

    def val_dataloader(self):
        return [_batch(torch.full((4,), 1.0)), _batch(torch.full((2,), 2.0))] if self.val else None


def _samples(n_batches, B, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N_PARAM, generator=g, dtype=torch.float64).to(dtype) for _ in range(n_batches)]


class _DMX(_DM):
    """batches of given sample matrices (for `_Regress`)"""

    def __init__(self, xs, val=False):
        self.xs, self.val = xs, val

    def train_dataloader(self):
        return [_batch(x) for x in self.xs]

    def val_dataloader(self):
        return [_batch(self.xs[0][:3]), _batch(self.xs[1][:2])] if self.val else None


def _fitter(**kw):
    from uwudiff_amd.engine import Fitter

    kw.setdefault("log_every_n_steps", 1)
    return Fitter(accelerator="cpu", **kw)


# ---------------------------------------------------------------------- the schedule
def test_steps_follow_every_third_batch_and_the_last_batch_of_each_epoch():
    tr = _Linear()
    fit = _fitter(accumulate_grad_batches=3, max_epochs=2)
    hooks = []
    fit.step_hooks.append(lambda f: hooks.append((f.global_step, f.train_batches, f.accum_pending)))
    hist = fit.fit(tr, _DM(4))
    assert fit.global_step == 4 and tr.sched.n == 4 and len(tr.spied) == 4
    assert fit.train_batches == 8 and tr.seen == [1.0, 2.0, 3.0, 4.0] * 2
    assert hooks == [(1, 3, 0), (2, 4, 0), (3, 7, 0), (4, 8, 0)]  # the step hooks run once per optimizer step, after batches 3 and 4
    assert [h["step"] for h in hist] == [1, 2, 3, 4] and [h["accum"] for h in hist] == [3, 1, 3, 1]
    # sum / 3 in both kinds of window: (1 + 2 + 3) / 3 and 4 / 3 (the short last window is divided by N too)
    for got, want in zip(tr.spied, [2.0, 4.0 / 3.0] * 2):
        assert torch.allclose(got, torch.full((N_PARAM,), want), rtol=1e-6, atol=0)
    # no zeroing on the batches that only accumulate: batch 2 and 3 of an epoch start on the running sum
    assert [None if g is None else float(g[0]) for g in tr.grad_at_entry[:4]] == [None, 1.0, 3.0, 0.0]
    assert tr.unet.fired == 8 and fit.accum_pending == 0
    assert hist[0]["loss"] == pytest.approx(float((torch.arange(N_PARAM) / N_PARAM).sum()) * 3.0)  # the last micro-batch's


def test_max_steps_counts_optimizer_steps():
    class _EpochEnds(_Linear):
        ends = 0

        def on_train_epoch_end(self):
            self.ends += 1

    tr = _EpochEnds()
    fit = _fitter(accumulate_grad_batches=2, max_steps=5, max_epochs=100)
    fit.fit(tr, _DM(4))
    assert fit.global_step == 5 and fit.train_batches == 10 and len(tr.seen) == 10
    assert fit.current_epoch == 2 and fit.batches_in_epoch == 2 and tr.ends == 2  # no epoch-end hook for the partial epoch
    assert tr.sched.n == 5 and len(tr.spied) == 5


def test_log_every_n_steps_and_every_n_train_steps_count_optimizer_steps(tmp_path):
    from uwudiff_amd.engine import ModelCheckpoint

    cb = ModelCheckpoint(dirpath=str(tmp_path), filename="step={step}", every_n_train_steps=2, save_top_k=-1)
    fit = _fitter(accumulate_grad_batches=2, max_epochs=3, log_every_n_steps=2, callbacks=[cb])
    hist = fit.fit(_Linear(), _DM(4))
    assert fit.global_step == 6 and [h["step"] for h in hist] == [2, 4, 6]
    assert sorted(os.listdir(tmp_path)) == ["step=2.ckpt", "step=4.ckpt", "step=6.ckpt"]
    ck = torch.load(tmp_path / "step=4.ckpt", weights_only=True)
    assert (ck["global_step"], ck["train_batches"], ck["batches_in_epoch"], ck["accum_pending"], ck["epoch"]) == (4, 8, 4, 0, 1)


def test_fast_dev_run_is_one_batch_and_one_step():
    tr = _Linear()
    fit = _fitter(accumulate_grad_batches=3, fast_dev_run=True)
    hist = fit.fit(tr, _DM(4))
    assert fit.global_step == 1 and tr.seen == [1.0] and len(tr.spied) == 1 and hist[0]["accum"] == 1
    assert torch.allclose(tr.spied[0], torch.full((N_PARAM,), 1.0 / 3.0))


# ---------------------------------------------------------------------- equivalence with the concatenated batch
def runs_noclip_norms():
    """the gradients of the unclipped 2B run of the test below (what gradient_clip_val is compared with)"""
    xs = _samples(4, 5, torch.float64)
    tr = _Regress(lr=0.05)
    _fitter(max_epochs=3).fit(tr, _DMX([torch.cat(xs[0:2]), torch.cat(xs[2:4])]))
    return tr.spied


@pytest.mark.parametrize("clip", [None, 0.05], ids=["noclip", "clip"])
def test_two_batches_of_B_equal_one_batch_of_2B(clip):
    xs = _samples(4, 5, torch.float64)
    runs = []
    for n_acc, batches in ((2, xs), (1, [torch.cat(xs[0:2]), torch.cat(xs[2:4])])):
        tr = _Regress(lr=0.05)
        fit = _fitter(accumulate_grad_batches=n_acc, max_epochs=3, gradient_clip_val=clip)
        after = []
        fit.step_hooks.append(lambda f, tr=tr, after=after: after.append(tr.unet.flat.detach().clone()))
        fit.fit(tr, _DMX(batches))
        assert fit.global_step == 6 and len(after) == 6
        runs.append((after, tr.spied))
    if clip is not None:  # low enough to bite on every step: what the optimizer got was scaled down to the bound
        unclipped = [float(g.norm()) for g in runs_noclip_norms()]
        assert min(unclipped) > 2 * clip
        for r in runs:
            assert all(float(g.norm()) == pytest.approx(clip, rel=1e-5) for g in r[1])
    for a, b in zip(*[r[0] for r in runs]):
        assert a.dtype == torch.float64
        torch.testing.assert_close(a, b, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------- N = 1 is the loop as it was
def _tree_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_tree_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_tree_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("clip", [None, 0.05], ids=["noclip", "clip"])
def test_n1_equals_a_run_that_does_not_pass_the_option(tmp_path, clip):
    from uwudiff_amd.engine import ModelCheckpoint

    xs = _samples(4, 5, torch.float32)
    outs = []
    for name, kw in (("plain", {}), ("n1", {"accumulate_grad_batches": 1})):
        d = tmp_path / name
        cb = ModelCheckpoint(dirpath=str(d), filename="step={step}", every_n_train_steps=3, save_top_k=-1, save_last=True)
        tr = _Regress(dtype=torch.float32, lr=0.05)
        fit = _fitter(max_steps=7, max_epochs=100, callbacks=[cb], gradient_clip_val=clip, val_check_interval=3,
                      check_val_every_n_epoch=None, **kw)
        hist = fit.fit(tr, _DMX(xs, val=True))
        files = sorted(os.listdir(d))
        outs.append({"hist": [{k: v for k, v in h.items() if k != "elapsed_s"} for h in hist],  # (elapsed_s is the wall clock)
                     "val": [{k: v for k, v in h.items() if k != "elapsed_s"} for h in fit.val_history],
                     "files": files, "ckpt": [torch.load(d / f, weights_only=True) for f in files],
                     "flat": tr.unet.flat.detach().clone(), "spied": tr.spied, "seen": tr.seen})
    a, b = outs
    assert a["files"] == b["files"] == ["last.ckpt", "step=3.ckpt", "step=6.ckpt"]
    assert a["hist"] == b["hist"] and len(a["hist"]) == 7 and all("accum" not in h for h in b["hist"])
    assert a["val"] == b["val"] and [h["step"] for h in b["val"]] == [3, 6]
    assert torch.equal(a["flat"], b["flat"]) and a["seen"] == b["seen"]
    assert all(torch.equal(x, y) for x, y in zip(a["spied"], b["spied"]))
    for x, y in zip(a["ckpt"], b["ckpt"]):
        for ck in (x, y):  # (the callback's state lists its files by path: the two runs wrote into two folders)
            st = ck["callbacks"].get("ModelCheckpoint", {})
            st["saved"] = [os.path.basename(f) for f in st.get("saved", [])]
        assert _tree_equal(x, y)
        assert x["train_batches"] == x["global_step"] and x["accum_pending"] == 0


# ---------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [0, -1, True, 2.0, {0: 2}, "4", None], ids=repr)
def test_refusals(bad):
    with pytest.raises(TypeError, match="accumulate_grad_batches") as e:
        _fitter(accumulate_grad_batches=bad)
    assert ("GradientAccumulationScheduler" in str(e.value)) == isinstance(bad, dict)


def test_accepted_values():
    for ok in (1, 2, 7):
        assert _fitter(accumulate_grad_batches=ok).accumulate_grad_batches == ok
    assert _fitter().accumulate_grad_batches == 1


# ---------------------------------------------------------------------- validation inside a window
def test_validation_inside_a_window_leaves_the_partial_gradient():
    tr = _Linear()
    fit = _fitter(accumulate_grad_batches=2, max_epochs=2, val_check_interval=3, check_val_every_n_epoch=None, num_sanity_val_steps=0)
    inner, around = fit.validate, []

    def validate(module, loader, **kw):
        before = module.unet.flat.grad.detach().clone()
        state = (fit.train_batches, fit.global_step, fit.accum_pending)
        rec = inner(module, loader, **kw)
        around.append((state, before, module.unet.flat.grad.detach().clone()))
        return rec

    fit.validate = validate
    fit.fit(tr, _DM(4, val=True))
    # after batches 3 and 6: the first inside the window of batches 3-4 (one micro-batch summed), the second on a boundary
    assert [s for s, _, _ in around] == [(3, 1, 1), (6, 3, 0)]
    for _, before, after in around:
        assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert torch.equal(around[0][1], torch.full((N_PARAM,), 3.0))  # batch 3's gradient, unscaled, waiting for batch 4
    assert [h["step"] for h in fit.val_history] == [1, 3]
    assert torch.allclose(tr.spied[1], torch.full((N_PARAM,), 3.5))  # and batch 4 was added to it: (3 + 4) / 2
    assert fit.global_step == 4


# ---------------------------------------------------------------------- checkpoints and resume
def test_resume_at_a_boundary_continues_the_uninterrupted_run(tmp_path):
    from uwudiff_amd.engine import ModelCheckpoint

    xs = _samples(4, 5, torch.float64, seed=1)

    def run(max_steps, d=None, ckpt=None):
        cbs = [ModelCheckpoint(dirpath=str(d), save_last=True, save_top_k=0)] if d is not None else []
        tr = _Regress(lr=0.05)
        fit = _fitter(accumulate_grad_batches=2, max_steps=max_steps, max_epochs=100, callbacks=cbs)
        fit.fit(tr, _DMX(xs), ckpt_path=ckpt)
        return fit, tr

    full, tr_full = run(6)
    first, tr1 = run(3, d=tmp_path)
    assert (first.global_step, first.current_epoch, first.batches_in_epoch, first.train_batches) == (3, 1, 2, 6)
    last = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert (last["global_step"], last["epoch"], last["batches_in_epoch"], last["train_batches"], last["accum_pending"]) == (3, 1, 2, 6, 0)
    second, tr2 = run(6, ckpt=str(tmp_path / "last.ckpt"))
    assert (second.global_step, second.current_epoch, second.batches_in_epoch, second.train_batches) == (6, 3, 0, 12)
    assert (full.global_step, full.current_epoch, full.batches_in_epoch, full.train_batches) == (6, 3, 0, 12)
    assert tr1.seen + tr2.seen == tr_full.seen and len(tr2.seen) == 6  # skipped two batches of epoch 1, not three and not one
    assert torch.equal(tr2.unet.flat.detach(), tr_full.unet.flat.detach())
    assert not torch.equal(tr1.unet.flat.detach(), tr_full.unet.flat.detach())


def test_resume_inside_a_window_starts_the_window_again(tmp_path, capsys):
    from uwudiff_amd.engine import ModelCheckpoint

    xs = _samples(4, 5, torch.float64, seed=2)

    def run(max_steps, ckpt=None, save=False):
        cbs = [ModelCheckpoint(dirpath=str(tmp_path), filename="b{step}", monitor="val/loss", save_top_k=-1)] if save else []
        tr = _Regress(lr=0.05)
        fit = _fitter(accumulate_grad_batches=2, max_steps=max_steps, max_epochs=100, callbacks=cbs, val_check_interval=3,
                      num_sanity_val_steps=0)
        fit.fit(tr, _DMX(xs, val=True), ckpt_path=ckpt)
        return fit, tr

    full, tr_full = run(4)
    first, tr1 = run(2, save=True)  # validates after batch 3 of epoch 0: one micro-batch into the window of batches 3-4
    ck = torch.load(tmp_path / "b1.ckpt", weights_only=True)
    assert (ck["global_step"], ck["batches_in_epoch"], ck["train_batches"], ck["accum_pending"]) == (1, 3, 3, 1)
    capsys.readouterr()
    second, tr2 = run(4, ckpt=str(tmp_path / "b1.ckpt"))
    out = capsys.readouterr().out
    assert out.count("replaying") == 1 and "1 batch(es)" in out
    # the skip moved back by one: batch 3 (index 2) is the first one run, on a zero gradient
    assert tr2.seen[0] == float(xs[2].flatten()[0]) and len(tr2.seen) == 6
    g0 = tr2.grad_at_entry[0]
    assert g0 is None or not bool(g0.any())
    assert (second.global_step, second.train_batches, second.current_epoch) == (4, 8, 2)
    # (this fake has no random draws and no ema_loss, so here even the mid-window resume reproduces the uninterrupted run)
    assert torch.equal(tr2.unet.flat.detach(), tr_full.unet.flat.detach())


def test_a_checkpoint_without_a_batch_count_is_refused_when_n_is_above_one(tmp_path):
    from uwudiff_amd.engine import ModelCheckpoint

    cb = ModelCheckpoint(dirpath=str(tmp_path), save_last=True, save_top_k=0)
    _fitter(max_steps=2, max_epochs=100, callbacks=[cb]).fit(_Linear(), _DM(4))
    ck = torch.load(tmp_path / "last.ckpt", weights_only=True)
    for k in ("batches_in_epoch", "train_batches", "accum_pending"):
        del ck[k]
    torch.save(ck, tmp_path / "old.ckpt")
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        _fitter(accumulate_grad_batches=2, max_steps=4, max_epochs=100).fit(_Linear(), _DM(4), ckpt_path=str(tmp_path / "old.ckpt"))
    fit = _fitter(max_steps=4, max_epochs=100)  # at N = 1 the fallback global_step % n_batches holds
    tr = _Linear()
    fit.fit(tr, _DM(4), ckpt_path=str(tmp_path / "old.ckpt"))
    assert tr.seen == [3.0, 4.0] and fit.train_batches == 4


# ---------------------------------------------------------------------- FlatGradSync.defer
def test_deferred_sync_reduces_nothing_and_refuses_all_reduce():
    from uwudiff_amd.gradsync import FlatGradSync

    sync = FlatGradSync(world_size=2)  # (no process group: any collective here would raise)
    g = torch.ones(8)
    assert sync.defer(True) is sync and sync.deferred
    sync._on_ready(g, [(4, 4, None)])
    assert sync._early == [] and torch.equal(g, torch.ones(8))
    with pytest.raises(RuntimeError, match="deferred"):
        sync.all_reduce(g)
    sync.defer(False)
    assert not sync.deferred and FlatGradSync(world_size=1).deferred is False


# ---------------------------------------------------------------------- world 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_fused_sgd():
    """a FlatFusedOptimizer (so the Fitter takes the fused path and attaches the early reduction) whose update is plain SGD on the
    CPU, chunk by chunk, with the arguments the HIP optimizers take"""
    from uwudiff_amd.optim import FlatFusedOptimizer

    class _CpuFusedSGD(FlatFusedOptimizer):
        def __init__(self, params, lr=0.05):
            super().__init__(params, dict(lr=lr))
            self.steps = 0

        @torch.no_grad()
        def step(self, closure=None, clip=None, pre_scale=1.0, chunks=None, before_chunk=None, zero_grad=False):
            self.steps += 1
            for group in self.param_groups:
                for p in group["params"]:
                    for i, (off, ln) in enumerate(chunks or [(0, p.numel())]):
                        if before_chunk is not None:
                            before_chunk(i)
                        p.data[off:off + ln].add_(p.grad[off:off + ln], alpha=-group["lr"] * pre_scale)
                        if zero_grad:
                            p.grad[off:off + ln].zero_()

    return _CpuFusedSGD


class _RegressFused(_Regress):
    def configure_optimizers(self):
        self.opt = _cpu_fused_sgd()(self.unet.parameters(), lr=self.lr)
        return self.opt


def _shards(world, n_batches=4, B=3):
    return [_samples(n_batches, B, torch.float32, seed=10 + r) for r in range(world)]


def _accum_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from uwudiff_amd.engine import Fitter

    calls = []
    inner = dist.all_reduce
    state = {"tr": None}

    def counted(t, *a, **kw):
        calls.append((len(state["tr"].seen), t.numel()))  # (how many training batches had started when it was issued)
        return inner(t, *a, **kw)

    dist.all_reduce = counted
    out = {}
    for n_acc in (3, 1):
        calls.clear()
        tr = state["tr"] = _RegressFused(dtype=torch.float32, lr=0.05)
        fit = Fitter(accelerator="cpu", accumulate_grad_batches=n_acc, max_epochs=2, log_every_n_steps=1)
        fit.fit(tr, _DMX(_shards(world)[rank]))
        out[n_acc] = {"calls": list(calls), "steps": fit.global_step, "opt_steps": tr.opt.steps, "fired": tr.unet.fired,
                      "hooked": tr.unet._hook is not None, "flat": tr.unet.flat.detach().tolist()}  # (plain data through the queue)
    q.put((rank, out))
    dist.destroy_process_group()


def test_world2_gloo_exchanges_once_per_optimizer_step():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_accum_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        for n_acc in (3, 1):
            res[r][n_acc]["flat"] = torch.tensor(res[r][n_acc]["flat"], dtype=torch.float32)
        a, b = res[r][3], res[r][1]
        assert a["hooked"] and b["hooked"] and a["fired"] == b["fired"] == 8  # the model reported its slices on every backward
        assert (a["steps"], a["opt_steps"], b["steps"], b["opt_steps"]) == (4, 4, 8, 8)
        # all_reduce calls per optimizer step: the same at N = 3 as at N = 1 (one early slice + one remainder), not N times it
        assert len(b["calls"]) % b["steps"] == 0 and len(a["calls"]) // a["steps"] == len(b["calls"]) // b["steps"] == 2
        assert len(a["calls"]) == 2 * a["steps"]
        # and none of them on a batch that only accumulates: batches 3, 4, 7, 8 end the windows
        assert sorted({k for k, _ in a["calls"]}) == [3, 4, 7, 8]
        assert sum(n for _, n in a["calls"]) == 4 * N_PARAM  # every element reduced exactly once per optimizer step
    assert torch.equal(res[0][3]["flat"], res[1][3]["flat"])
    # one process on the union of the shards: batch k is both ranks' batch k, the loss is a per-sample mean
    sh = _shards(world)
    union = [torch.cat([sh[0][k], sh[1][k]]) for k in range(4)]
    tr = _Regress(dtype=torch.float32, lr=0.05)
    _fitter(accumulate_grad_batches=3, max_epochs=2).fit(tr, _DMX(union))
    torch.testing.assert_close(res[0][3]["flat"], tr.unet.flat.detach(), rtol=1e-6, atol=0)
    assert not torch.allclose(res[0][3]["flat"], res[0][1]["flat"], rtol=1e-3, atol=0)  # (N = 1 is another trajectory)


# ---------------------------------------------------------------------- the YAML
def test_accum_yaml_is_the_latent_demo_with_the_option():
    from uwudiff_amd.config import load_yaml

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_accum.yaml"))
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    lc = dict(cfg["lightning_config"])
    assert lc["accumulate_grad_batches"] == 4 and lc["fast_dev_run"] is False and 0 < lc["max_steps"] <= 8
    fit = _fitter(**{k: v for k, v in lc.items() if k != "log_every_n_steps"})
    assert fit.accumulate_grad_batches == 4
    assert cfg["trainer"] == base["trainer"] and cfg["data"] == base["data"] and cfg["seed"] == base["seed"]
