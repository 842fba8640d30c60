"""CPU tests of the validation loop: the schedule of ``Fitter`` (Lightning's rules), the CPU path of
``TimestepLossStats`` against numpy, its reduction over two gloo ranks, ``ModelCheckpoint(monitor=...)``, the data module's validation
loader, the YAML and the plot callback.  The kernel itself is tested in tests/test_validation_gpu.py."""
import os
import socket
from typing import NamedTuple

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Aux(NamedTuple):
    losses: torch.Tensor
    timesteps: torch.Tensor


class _Unet(nn.Module):
    def __init__(self, n=16):
        super().__init__()
        self.flat = nn.Parameter(torch.arange(n, dtype=torch.float32) / n)


class _TrainOnly(nn.Module):
    """the trainer of tests/test_engine_cpu.py: no validation_step"""

    n_diffusion_time_steps = 10

    def __init__(self):
        super().__init__()
        self.unet = _Unet()
        self.register_buffer("ema_loss", torch.tensor(0.0))

    def configure_optimizers(self):
        return torch.optim.SGD(self.unet.parameters(), lr=0.1)

    def training_step(self, batch, idx):
        return {"loss": (self.unet.flat * batch[0].mean()).sum()}


class _Trainer(_TrainOnly):
    def validation_step(self, batch, idx):
        x = batch[0]
        assert not self.training and not torch.is_grad_enabled()
        losses = (x * self.unet.flat.detach()[: x.numel()]).float()
        return losses.mean(), _Aux(losses=losses, timesteps=torch.arange(x.numel()) % self.n_diffusion_time_steps)


def _batch(n, v):
    return (torch.full((n,), float(v)), [""] * n, [], {}, {})


class _DMTrainOnly:
    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [_batch(4, i + 1) for i in range(4)]


class _DM(_DMTrainOnly):
    def val_dataloader(self):
        return [_batch(4, 1), _batch(4, 2), _batch(2, 3)]  # (a ragged last batch)


class _Recorder:
    """the sequence of passes as the callbacks see it: (global_step, batches, sanity)"""

    def __init__(self):
        self.passes = []

    def on_validation_epoch_start(self, trainer, pl_module):
        self.n = 0

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        assert batch_idx == self.n
        self.n += 1

    def on_validation_epoch_end(self, trainer, pl_module):
        self.passes.append((trainer.global_step, self.n, trainer.sanity_checking))


def _run(trainer=None, dm=None, **kw):
    from uwudiff_amd.engine import Fitter

    rec = _Recorder()
    kw.setdefault("max_epochs", 2)
    fit = Fitter(accelerator="cpu", callbacks=[rec], **kw)
    hist = fit.fit(trainer or _Trainer(), dm or _DM())
    real = [(s, n) for s, n, sanity in rec.passes if not sanity]
    assert [r["step"] for r in fit.val_history] == [s for s, _ in real]
    return fit, rec, real, hist


def test_default_schedule_validates_at_each_epoch_end_after_a_two_batch_sanity_pass():
    fit, rec, real, _ = _run()
    assert rec.passes == [(0, 2, True), (4, 3, False), (8, 3, False)]
    assert fit.global_step == 8 and not fit.sanity_checking
    assert [r["val_samples"] for r in fit.val_history] == [10, 10]
    assert [r["epoch"] for r in fit.val_history] == [0, 1]
    assert set(fit.val_history[0]) == {"step", "epoch", "val/loss", "val_samples", "elapsed_s"}


@pytest.mark.parametrize("kw,want", [
    (dict(val_check_interval=0.5), [2, 4, 6, 8]),
    (dict(val_check_interval=3), [3, 7]),
    (dict(val_check_interval=3, check_val_every_n_epoch=None), [3, 6]),
    (dict(check_val_every_n_epoch=2), [8]),
], ids=["half_epoch", "int_within_epoch", "int_global", "every_second_epoch"])
def test_val_check_interval(kw, want):
    _, _, real, _ = _run(**kw)
    assert real == [(s, 3) for s in want]


def test_int_interval_beyond_the_epoch_is_refused():
    with pytest.raises(ValueError, match=r"5.*4"):
        _run(val_check_interval=5)


@pytest.mark.parametrize("limit,n", [(2, 2), (0.34, 1)])
def test_limit_val_batches(limit, n):
    _, rec, real, _ = _run(limit_val_batches=limit)
    assert real == [(4, n), (8, n)]
    assert rec.passes[0] == (0, min(2, n), True)


def test_limit_val_batches_zero_switches_validation_off():
    fit, rec, real, _ = _run(limit_val_batches=0)
    assert rec.passes == [] and fit.val_history == []
    fit, rec, real, _ = _run(limit_val_batches=0.0)
    assert rec.passes == [] and fit.val_history == []


def test_sanity_steps():
    assert _run(num_sanity_val_steps=0)[1].passes[0] == (4, 3, False)
    assert _run(num_sanity_val_steps=-1)[1].passes[0] == (0, 3, True)


def test_fast_dev_run_is_one_training_batch_and_one_validation_batch():
    fit, rec, real, _ = _run(fast_dev_run=True)
    assert rec.passes == [(1, 1, False)] and fit.global_step == 1


def test_no_validation_without_a_loader_or_a_validation_step():
    for tr, dm in ((_Trainer(), _DMTrainOnly()), (_TrainOnly(), _DM())):
        fit, rec, real, hist = _run(trainer=tr, dm=dm)
        assert fit.val_history == [] and rec.passes == [] and fit.global_step == 8


def test_validation_leaves_training_where_it_was():
    """same parameters, training records and CPU generator state with and without the validation passes"""
    outs = []
    for dm in (_DM(), _DMTrainOnly()):
        torch.manual_seed(5)
        tr = _Trainer()
        fit, _, _, hist = _run(trainer=tr, dm=dm, val_check_interval=0.5, log_every_n_steps=1)
        outs.append((tr.unet.flat.detach().clone(), [h["loss"] for h in hist], torch.get_rng_state(), tr.training, len(hist)))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    assert outs[0][3] and outs[0][4] == outs[1][4]  # train mode restored; fit.history keeps its length


def test_val_loss_is_the_sample_weighted_mean_and_every_pass_sees_the_same_draws():
    from uwudiff_amd.engine import Fitter

    tr = _Trainer()
    fit = Fitter(accelerator="cpu")
    rec = fit.validate(tr, _DM().val_dataloader())
    f = tr.unet.flat.detach()
    per = [float((torch.full((n,), float(v)) * f[:n]).float().mean()) for n, v in ((4, 1), (4, 2), (2, 3))]
    want = (4 * per[0] + 4 * per[1] + 2 * per[2]) / 10
    assert rec["val/loss"] == want and rec["val_samples"] == 10
    assert rec["val/loss"] != pytest.approx(sum(per) / 3, rel=1e-3)  # (the mean of the batch means is another number)
    assert fit.val_history == [rec]


# ---------------------------------------------------------------------- TimestepLossStats on CPU
def _numpy_stats(losses, timesteps, n):
    st = np.zeros((3, n), dtype=np.float64)
    for l, t in zip(np.asarray(losses, dtype=np.float32), np.asarray(timesteps)):
        if np.isnan(t):
            continue
        k = int(np.trunc(t))
        if 0 <= k < n and t > -1:
            l = np.float64(l)
            st[0, k] += 1.0
            st[1, k] += l
            st[2, k] += l * l
    return st


def test_timestep_loss_stats_cpu_matches_numpy():
    from uwudiff_amd.validation import TimestepLossStats

    g = torch.Generator().manual_seed(3)
    n = 10
    st = TimestepLossStats(n, "cpu")
    all_l, all_t, tot = [], [], [0.0, 0.0]
    for B, as_float in ((7, False), (64, True), (5, True)):
        losses = torch.randn(B, generator=g).abs()
        t = torch.rand(B, generator=g) * (n + 4) - 2 if as_float else torch.randint(-1, n + 2, (B,), generator=g)
        if as_float:
            t[0], t[1] = -0.5, float("nan")
        st.update(losses, t, losses.mean())
        all_l += losses.tolist()
        all_t += t.tolist()
        tot[0] += B * float(losses.mean())
        tot[1] += B
    want = _numpy_stats(all_l, all_t, n)
    assert np.array_equal(st.state[:3 * n].numpy().reshape(3, n), want)
    res = st.compute()
    seen = want[0] > 0
    assert np.array_equal(res["timesteps"], np.nonzero(seen)[0]) and np.array_equal(res["count"], want[0][seen])
    mean = want[1][seen] / want[0][seen]
    assert np.array_equal(res["mean"], mean)
    assert np.array_equal(res["std"], np.sqrt(np.maximum(want[2][seen] / want[0][seen] - mean * mean, 0.0)))
    assert res["loss"] == tot[0] / tot[1] and res["n_samples"] == 76
    st.reset()
    assert float(st.state.abs().sum()) == 0.0


def test_constant_loss_has_zero_std_and_empty_buckets_are_omitted():
    from uwudiff_amd.validation import TimestepLossStats

    c = np.float32(0.123456)
    # the reference's formula on its fp32 sums (callbacks.py:115-125) leaves a residue at this constant from 131 samples on -- a
    # negative one there, whose square root is NaN -- where the same formula on float64 sums gives exactly 0
    s32, q32 = np.float32(0), np.float32(0)
    for _ in range(131):
        s32, q32 = np.float32(s32 + c), np.float32(q32 + np.float32(c * c))
    m32 = np.float32(s32 / np.float32(131))
    assert float(np.float32(np.float32(q32 / np.float32(131)) - np.float32(m32 * m32))) != 0.0
    st = TimestepLossStats(1000, "cpu")
    st.update(torch.full((134,), float(c)), torch.tensor([3] * 131 + [999] * 3))
    res = st.compute()
    assert res["timesteps"].tolist() == [3, 999] and res["count"].tolist() == [131.0, 3.0]
    assert res["std"].tolist() == [0.0, 0.0] and res["mean"].tolist() == [float(c), float(c)]
    assert np.isnan(res["loss"])  # no batch passed its scalar loss


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_data(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(33, generator=g).abs(), torch.randint(0, 10, (33,), generator=g)


def _reduce_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from uwudiff_amd.validation import TimestepLossStats

    st = TimestepLossStats(10, "cpu")
    losses, t = _rank_data(rank)
    st.update(losses, t, losses.mean())
    st.reduce()
    q.put((rank, st.state.tolist()))
    dist.destroy_process_group()


def test_reduce_sums_the_state_over_two_gloo_ranks():
    from uwudiff_amd.validation import TimestepLossStats

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    parts = []
    for r in range(world):
        st = TimestepLossStats(10, "cpu")
        losses, t = _rank_data(r)
        st.update(losses, t, losses.mean())
        parts.append(st.state.clone())
    want = (parts[0] + parts[1]).tolist()  # (a sum of two doubles: exact in either order)
    assert res[0] == want and res[1] == want


# ---------------------------------------------------------------------- ModelCheckpoint(monitor=...)
class _ScoreFitter:
    """what ModelCheckpoint reads of a Fitter"""

    global_rank, fast_dev_run, sanity_checking, current_epoch = 0, False, False, 0

    def __init__(self):
        self.global_step, self.val_history, self.written = 0, [], []

    def save_checkpoint(self, path, callbacks=None):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"callbacks": callbacks or {}}, path)
        self.written.append(path)


@pytest.mark.parametrize("mode,kept", [("min", [1.0, 0.5]), ("max", [3.0, 2.0])])
def test_model_checkpoint_keeps_the_best_k_by_the_monitored_value(tmp_path, mode, kept):
    from uwudiff_amd.engine import ModelCheckpoint

    cb = ModelCheckpoint(dirpath=str(tmp_path), filename="s{step}", monitor="val/loss", mode=mode, save_top_k=2)
    f = _ScoreFitter()
    names = {}
    for i, score in enumerate([3.0, 1.0, 2.0, 0.5]):
        f.global_step = i + 1
        f.val_history.append({"step": i + 1, "val/loss": score})
        names[score] = f"s{i + 1}.ckpt"
        cb.on_step(f)  # the periodic triggers are off with a monitor
        cb.on_validation_end(f, None)
    assert sorted(os.listdir(tmp_path)) == sorted(names[s] for s in kept)
    assert sorted(s for _, s in cb.best) == sorted(kept)
    f.sanity_checking = True  # a sanity pass writes nothing
    f.val_history.append({"step": 9, "val/loss": -1.0 if mode == "min" else 99.0})
    f.global_step = 9
    cb.on_validation_end(f, None)
    assert "s9.ckpt" not in os.listdir(tmp_path)
    with pytest.raises(KeyError):
        f.sanity_checking = False
        ModelCheckpoint(dirpath=str(tmp_path), monitor="val/nope").on_validation_end(f, None)


def test_monitored_checkpoints_through_fit_and_the_score_list_survives_a_resume(tmp_path):
    from uwudiff_amd.engine import Fitter, ModelCheckpoint

    def cb():
        return ModelCheckpoint(dirpath=str(tmp_path), filename="s{step}", monitor="val/loss", mode="min", save_top_k=2)

    c1 = cb()
    fit = Fitter(accelerator="cpu", callbacks=[c1], max_epochs=1, val_check_interval=1, num_sanity_val_steps=0)
    fit.fit(_Trainer(), _DM())
    scores = {r["step"]: r["val/loss"] for r in fit.val_history}
    assert len(scores) == 4
    best2 = sorted(scores, key=scores.get)[:2]
    assert sorted(os.listdir(tmp_path)) == sorted(f"s{s}.ckpt" for s in best2)
    last = os.path.join(tmp_path, f"s{max(best2)}.ckpt")
    ck = torch.load(last, weights_only=True)
    assert sorted(s for _, s in ck["callbacks"]["ModelCheckpoint"]["best"]) == sorted(scores[s] for s in best2)
    c2 = cb()
    fit2 = Fitter(accelerator="cpu", callbacks=[c2], max_epochs=2, val_check_interval=1, num_sanity_val_steps=0)
    fit2.fit(_Trainer(), _DM(), ckpt_path=last)  # a resumed run goes on pruning over the files of the interrupted one
    assert fit2.global_step == 8 and len(c2.best) == 2
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p, _ in c2.best)
    both = {**scores, **{r["step"]: r["val/loss"] for r in fit2.val_history}}
    assert sorted(s for _, s in c2.best) == sorted(both.values())[:2]


def test_monitor_step_or_none_behaves_as_before(tmp_path):
    from uwudiff_amd.engine import Fitter, ModelCheckpoint

    cb = ModelCheckpoint(dirpath=str(tmp_path), filename="step={step}", every_n_train_steps=2, save_top_k=2, monitor="step", mode="max")
    Fitter(max_steps=7, accelerator="cpu", callbacks=[cb], max_epochs=100).fit(_Trainer(), _DM())
    assert sorted(os.listdir(tmp_path)) == ["step=4.ckpt", "step=6.ckpt"]


# ---------------------------------------------------------------------- data module, YAML, callback
def test_validation_loader_does_not_shuffle_and_gets_the_tokenizers():
    from duwu.data import TrainDataModule

    node = {"_target_": "duwu.data.DummyDataset", "sample_size": [1, 2, 2], "n_samples": 5}
    dm = TrainDataModule(node, {"batch_size": 2, "shuffle": True, "drop_last": True, "num_workers": 3},
                         val_dataset_config={**node, "n_samples": 5})
    toks = [lambda c, **kw: {"input_ids": torch.zeros(1, 3, dtype=torch.long), "attention_mask": torch.ones(1, 3, dtype=torch.long)}]
    dm.set_tokenizers(toks)
    torch.manual_seed(11)
    dm.setup("fit")
    state = torch.get_rng_state()
    torch.manual_seed(11)
    plain = TrainDataModule(node, {"batch_size": 2})
    plain.set_tokenizers(toks)
    plain.setup("fit")
    assert torch.equal(state, torch.get_rng_state())  # building the validation set left the CPU generator where it was
    assert plain.val_dataloader() is None
    assert dm.val_dataset.tokenizers is toks and dm.dataset.tokenizers is toks
    vl = dm.val_dataloader()
    assert isinstance(vl.sampler, torch.utils.data.SequentialSampler) and not vl.drop_last and len(vl) == 3
    got = torch.cat([b[0] for b in vl])
    assert torch.equal(got, torch.stack(dm.val_dataset.samples))
    assert len(dm.train_dataloader()) == 2  # the training loader keeps its own settings
    own = TrainDataModule(node, {"batch_size": 2}, val_dataset_config=node, val_dataloader_config={"batch_size": 5})
    own.setup("fit")
    assert len(own.val_dataloader()) == 1


def test_validation_yaml_instantiates():
    from duwu.trainer.callbacks import PlotValLossPerTimestep
    from duwu.utils import instantiate_any
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.engine import Fitter, ModelCheckpoint

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_val.yaml"))
    lc = dict(cfg["lightning_config"])
    lc["callbacks"] = [instantiate_any(c) for c in lc["callbacks"]]
    fit = Fitter(accelerator="cpu", **{k: v for k, v in lc.items() if k != "accelerator"})
    assert isinstance(lc["callbacks"][0], PlotValLossPerTimestep)
    ck = lc["callbacks"][1]
    assert isinstance(ck, ModelCheckpoint) and ck.monitor == "val/loss" and ck.mode == "min" and ck.save_top_k == 2
    assert fit.val_check_interval == 4 and fit.check_val_every_n_epoch is None
    dm = instantiate_any(cfg["data"])
    dm.set_tokenizers([])
    dm.setup("fit")
    assert len(dm.val_dataset) == 40 and [b[0].shape[0] for b in dm.val_dataloader()] == [16, 16, 8]
    # everything else is configs/demo_training_latent.yaml
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    assert cfg["trainer"] == base["trainer"] and cfg["seed"] == base["seed"]
    assert cfg["data"]["dataset_config"] == base["data"]["dataset_config"]


def test_plot_callback_writes_the_arrays_and_the_png(tmp_path):
    from duwu.trainer.callbacks import PlotValLossPerTimestep
    from uwudiff_amd.engine import Fitter

    cb = PlotValLossPerTimestep()
    tr = _Trainer()
    fit = Fitter(accelerator="cpu", callbacks=[cb], default_root_dir=str(tmp_path))
    fit.global_step = 12
    fit.validate(tr, _DM().val_dataloader())
    f = tr.unet.flat.detach()
    losses = torch.cat([torch.full((n,), float(v)) * f[:n] for n, v in ((4, 1), (4, 2), (2, 3))])
    want = _numpy_stats(losses.numpy(), [0, 1, 2, 3, 0, 1, 2, 3, 0, 1], 10)
    seen = want[0] > 0
    mean = want[1][seen] / want[0][seen]
    std = np.sqrt(np.maximum(want[2][seen] / want[0][seen] - mean * mean, 0.0))
    stem = tmp_path / "plots" / "losses_per_timestep-training_step-12"
    with np.load(str(stem) + ".npz") as z:
        for got in (cb.last, z):
            assert np.array_equal(got["timesteps"], [0, 1, 2, 3]) and np.array_equal(got["count"], want[0][seen])
            assert np.array_equal(got["mean"], mean) and np.array_equal(got["std"], std)
    # the next epoch starts from zero
    fit.validate(tr, _DM().val_dataloader())
    assert np.array_equal(cb.last["count"], want[0][seen])
    pytest.importorskip("matplotlib")
    png = str(stem) + ".png"
    assert os.path.getsize(png) > 1000 and open(png, "rb").read(4) == b"\x89PNG"
