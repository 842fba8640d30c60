"""CPU: the weight-averaging callbacks (uwudiff_amd/averaging.py) as far as they go without a device: the
aliases and the YAML, the ``should_update`` tables, the batch-end rule under gradient accumulation, the refusals, the fp32 coefficients,
and the checkpoint bookkeeping of the callback on plain dicts."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


class _StubAverage:
    """stands in for FlatAverage: records the coefficients of every update"""

    def __init__(self):
        self.n_averaged, self.updates = 0, []

    def update(self, keep, take):
        self.updates.append((keep, take))
        self.n_averaged += 1


class _FakeFitter:
    global_rank = 0

    def __init__(self):
        self.global_step, self.current_epoch = 0, 0


# ---------------------------------------------------------------------- surface
def test_aliases_resolve():
    from uwudiff_amd import averaging
    from uwudiff_amd.config import ALIASES, get_obj_from_str

    assert get_obj_from_str("lightning.pytorch.callbacks.WeightAveraging") is averaging.WeightAveraging
    assert get_obj_from_str("lightning.pytorch.callbacks.EMAWeightAveraging") is averaging.EMAWeightAveraging
    assert ALIASES["lightning.pytorch.callbacks.ModelCheckpoint"] == "uwudiff_amd.engine.ModelCheckpoint"  # (kept)


def test_ema_yaml_instantiates_through_the_launchers_path():
    from duwu.trainer.callbacks import PlotValLossPerTimestep
    from duwu.utils import instantiate_any
    from uwudiff_amd.averaging import EMAWeightAveraging
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.engine import Fitter, ModelCheckpoint

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_ema.yaml"))
    lc = dict(cfg["lightning_config"])
    lc["callbacks"] = [instantiate_any(c) for c in lc["callbacks"]]
    fit = Fitter(accelerator="cpu", **{k: v for k, v in lc.items() if k != "accelerator"})
    ema, plot, ck = fit.callbacks
    assert type(ema) is EMAWeightAveraging and ema.decay == 0.9 and ema.update_every_n_steps == 1
    assert isinstance(plot, PlotValLossPerTimestep) and isinstance(ck, ModelCheckpoint) and ck.monitor == "val/loss"
    # everything else is configs/demo_training_val.yaml
    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_val.yaml"))
    assert cfg["trainer"] == base["trainer"] and cfg["data"] == base["data"] and cfg["seed"] == base["seed"]
    rest = {k: v for k, v in cfg["lightning_config"].items() if k != "callbacks"}
    assert rest == {k: v for k, v in base["lightning_config"].items() if k != "callbacks"}
    assert cfg["lightning_config"]["callbacks"][1:] == base["lightning_config"]["callbacks"]


# ---------------------------------------------------------------------- should_update
@pytest.mark.parametrize("start", [None, 4])
@pytest.mark.parametrize("every", [1, 3])
def test_ema_should_update_table_over_steps(every, start):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb = EMAWeightAveraging(update_every_n_steps=every, update_starting_at_step=start)
    by_hand = {(1, None): [1, 1, 1, 1, 1, 1, 1, 1, 1, 1], (3, None): [1, 0, 0, 1, 0, 0, 1, 0, 0, 1],
               (1, 4): [0, 0, 0, 0, 1, 1, 1, 1, 1, 1], (3, 4): [0, 0, 0, 0, 0, 0, 1, 0, 0, 1]}[(every, start)]
    assert [cb.should_update(step_idx=s) for s in range(10)] == [bool(v) for v in by_hand]
    assert not any(cb.should_update(epoch_idx=e) for e in range(4))  # no update_starting_at_epoch: never at an epoch's end


def test_ema_should_update_epochs_and_degenerate_period():
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb = EMAWeightAveraging(update_starting_at_epoch=2)
    assert [cb.should_update(epoch_idx=e) for e in range(5)] == [False, False, True, True, True]
    assert cb.should_update(step_idx=0) and not cb.should_update()
    off = EMAWeightAveraging(update_every_n_steps=0)
    assert not any(off.should_update(step_idx=s) for s in range(5))


def test_base_class_updates_at_every_step_and_no_epoch():
    from uwudiff_amd.averaging import WeightAveraging

    cb = WeightAveraging()
    assert all(cb.should_update(step_idx=s) for s in range(10))
    assert not any(cb.should_update(epoch_idx=e) for e in range(10))
    assert [cb.coefficients(n) for n in range(3)] == [(0.0, 1.0), (0.5, 0.5), (2 / 3, 1 / 3)]


# ---------------------------------------------------------------------- the batch-end rule
@pytest.mark.parametrize("n_acc", [1, 2, 4])
def test_one_update_per_optimizer_step_under_accumulation(n_acc):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb, fit = EMAWeightAveraging(decay=0.75), _FakeFitter()
    cb.average = _StubAverage()
    seen = []
    for b in range(5 * n_acc):  # global_step stays put for N - 1 of N batches
        if (b + 1) % n_acc == 0:
            fit.global_step += 1
        cb.on_train_batch_end(fit, None, None, None, b)
        seen.append(cb.average.n_averaged)
    assert cb.average.n_averaged == 5 and cb.latest_update_step == 5
    assert seen == [(b + 1) // n_acc for b in range(5 * n_acc)]
    assert cb.average.updates == [(0.75, 0.25)] * 5


def test_update_every_k_steps_updates_after_steps_1_k_plus_1():
    from uwudiff_amd.averaging import EMAWeightAveraging, WeightAveraging

    cb, fit = EMAWeightAveraging(update_every_n_steps=3), _FakeFitter()
    cb.average = _StubAverage()
    at = []
    for _ in range(8):
        fit.global_step += 1
        before = cb.average.n_averaged
        cb.on_train_batch_end(fit, None, None, None, 0)
        cb.on_train_batch_end(fit, None, None, None, 0)  # (the same global_step again: nothing)
        if cb.average.n_averaged != before:
            at.append(fit.global_step)
    assert at == [1, 4, 7]
    mean = WeightAveraging()
    mean.average = _StubAverage()
    for _ in range(3):
        fit.global_step += 1
        mean.on_train_batch_end(fit, None, None, None, 0)
    assert mean.average.updates == [(0.0, 1.0), (0.5, 0.5), (2 / 3, 1 / 3)]
    fit.current_epoch = 1
    cb2 = EMAWeightAveraging(update_starting_at_epoch=1)
    cb2.average = _StubAverage()
    cb2.on_train_epoch_end(fit, None)
    mean.on_train_epoch_end(fit, None)
    assert cb2.average.n_averaged == 1 and mean.average.n_averaged == 3


# ---------------------------------------------------------------------- refusals
@pytest.mark.parametrize("decay", [-0.1, 1.0001, float("nan"), "0.9", True])
def test_decay_outside_the_unit_interval_is_refused(decay):
    from uwudiff_amd.averaging import EMAWeightAveraging

    with pytest.raises(ValueError, match="decay"):
        EMAWeightAveraging(decay=decay)


def test_decay_bounds_are_accepted():
    from uwudiff_amd.averaging import EMAWeightAveraging

    assert EMAWeightAveraging(decay=0).coefficients(3) == (0.0, 1.0) and EMAWeightAveraging(decay=1).coefficients(3) == (1.0, 0.0)


@pytest.mark.parametrize("cls", ["WeightAveraging", "EMAWeightAveraging"])
def test_cpu_device_and_avg_fn_are_refused(cls):
    from uwudiff_amd import averaging

    C = getattr(averaging, cls)
    with pytest.raises(ValueError, match="next to the weights"):
        C(device="cpu")
    with pytest.raises(ValueError, match="next to the weights"):
        C(device=torch.device("cpu"))
    with pytest.raises(TypeError, match="avg_fn"):
        C(avg_fn=lambda a, p, n: a)
    with pytest.raises(TypeError, match="multi_avg_fn"):
        C(multi_avg_fn=lambda a, p, n: None)
    with pytest.raises(TypeError, match="bogus"):
        C(bogus=1)
    cb = C(device=None, use_buffers=False, avg_fn=None)  # (use_buffers is accepted and has no effect)
    assert cb.average is None and cb.state_dict() == {"latest_update_step": 0}
    assert C(device="cuda").device == torch.device("cuda")


def test_a_second_averaging_callback_is_refused():
    from uwudiff_amd.averaging import EMAWeightAveraging, WeightAveraging
    from uwudiff_amd.engine import Fitter

    with pytest.raises(ValueError, match="averaging"):
        Fitter(accelerator="cpu", callbacks=[WeightAveraging(), EMAWeightAveraging()])
    fit = Fitter(accelerator="cpu", callbacks=[EMAWeightAveraging()], fast_dev_run=True)
    assert len(fit.callbacks) == 1  # fast_dev_run keeps it: it is no checkpoint callback


def test_cpu_tensors_are_refused():
    from uwudiff_amd.averaging import EMAWeightAveraging, FlatAverage
    from uwudiff_amd.lib import UwuError

    class Owner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.flat = torch.nn.Parameter(torch.zeros(64))

    with pytest.raises(UwuError, match="CPU"):
        FlatAverage(Owner())
    with pytest.raises(TypeError):
        FlatAverage(torch.nn.Linear(2, 2))

    class Module:
        lycoris_model = None
        unet = Owner()

    with pytest.raises(UwuError, match="CPU"):
        EMAWeightAveraging().setup(_FakeFitter(), Module(), "fit")


# ---------------------------------------------------------------------- coefficients
def test_coefficient_pairs_sum_to_one_within_an_ulp():
    """keep and take are formed in double and rounded once to fp32 each: their sum, taken exactly, is within 2^-23 (one ulp of 1) of 1"""
    from uwudiff_amd.averaging import EMAWeightAveraging, WeightAveraging

    pairs = [EMAWeightAveraging(decay=d).coefficients(5) for d in (0.0, 1e-3, 0.1, 0.5, 0.9, 0.99, 0.999, 0.9999, 0.99999, 1.0 - 2.0 ** -30, 1.0)]
    rng = np.random.default_rng(0)
    pairs += [EMAWeightAveraging(decay=float(d)).coefficients(1) for d in rng.random(2000)]
    mean = WeightAveraging()
    pairs += [mean.coefficients(n) for n in list(range(0, 5000)) + [10 ** 6, 2 ** 24 - 1, 2 ** 24, 2 ** 31, 10 ** 12]]
    worst = 0.0
    for keep, take in pairs:
        assert type(keep) is float and type(take) is float and 0.0 <= keep <= 1.0 and 0.0 <= take <= 1.0
        s = float(np.float32(keep)) + float(np.float32(take))  # (exact in double: both are fp32 values in [0, 1])
        worst = max(worst, abs(s - 1.0))
    print(f"max |fp32(keep) + fp32(take) - 1| over {len(pairs)} pairs: {worst:.3e} (one ulp of 1: {2.0 ** -23:.3e})")
    assert worst <= 2.0 ** -23


# ---------------------------------------------------------------------- checkpoint bookkeeping on plain dicts
class _DictAverage:
    n_averaged = 7

    def averaged_state(self):
        return {"w": torch.full((2,), 5.0)}


class _Mod:
    lycoris_model = None
    unet = object()


def test_save_puts_the_average_under_state_dict_and_the_weights_under_current_model_state():
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb = EMAWeightAveraging()
    cb.average, cb.latest_update_step = _DictAverage(), 9
    ckpt = {"state_dict": {"unet.w": torch.full((2,), 1.0), "ema_loss": torch.tensor(0.25)}, "callbacks": {}}
    cb.on_save_checkpoint(_FakeFitter(), _Mod(), ckpt)
    assert ckpt["state_dict"]["unet.w"].tolist() == [5.0, 5.0] and ckpt["current_model_state"]["unet.w"].tolist() == [1.0, 1.0]
    assert float(ckpt["state_dict"]["ema_loss"]) == float(ckpt["current_model_state"]["ema_loss"]) == 0.25  # buffers as they are
    assert list(ckpt["state_dict"]) == list(ckpt["current_model_state"]) == ["unet.w", "ema_loss"]
    assert ckpt["averaging_state"] == {"n_averaged": 7} and cb.state_dict() == {"latest_update_step": 9}
    # and the way back: the module is pointed at the weights it trained on, the averaged entries wait for setup
    cb2 = EMAWeightAveraging()
    cb2.on_load_checkpoint(_FakeFitter(), _Mod(), ckpt)
    cb2.load_state_dict(cb.state_dict())
    assert ckpt["state_dict"]["unet.w"].tolist() == [1.0, 1.0]
    sd, n = cb2._resumed
    assert list(sd) == ["w"] and sd["w"].tolist() == [5.0, 5.0] and n == 7 and cb2.latest_update_step == 9


def test_a_checkpoint_without_current_model_state_says_so_in_one_line(capsys):
    from uwudiff_amd.averaging import EMAWeightAveraging

    cb = EMAWeightAveraging()
    ckpt = {"state_dict": {"unet.w": torch.ones(2)}}
    cb.on_load_checkpoint(_FakeFitter(), _Mod(), ckpt)
    out = capsys.readouterr().out
    assert cb._resumed is None and len(out.strip().splitlines()) == 1 and "copy of the loaded weights" in out
    assert ckpt["state_dict"]["unet.w"].tolist() == [1.0, 1.0]


def test_fitter_round_trips_callback_state_and_keeps_the_modelcheckpoint_entry(tmp_path, capsys):
    """save_checkpoint / load_checkpoint on a CPU stand-in: the generic ``callbacks`` entry next to ModelCheckpoint's, the
    on_save / on_load hooks, and the one line of a Fitter without the callback that meets ``current_model_state``."""
    from uwudiff_amd.averaging import EMAWeightAveraging
    from uwudiff_amd.engine import Fitter, ModelCheckpoint

    class Unet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(2))

    class Mod(torch.nn.Module):
        lycoris_model = None

        def __init__(self):
            super().__init__()
            self.unet = Unet()

    def fitter(cbs):
        m = Mod()
        f = Fitter(accelerator="cpu", callbacks=cbs)
        f._fit_state = (m, torch.optim.SGD(m.parameters(), lr=0.1), None)
        return f, m

    cb = EMAWeightAveraging()
    cb.average, cb.latest_update_step = _DictAverage(), 4
    f, m = fitter([cb, ModelCheckpoint(dirpath=str(tmp_path))])
    path = str(tmp_path / "a.ckpt")
    mc_state = {"saved": ["x.ckpt"]}
    ck = f.save_checkpoint(path, callbacks={"ModelCheckpoint": mc_state})
    assert ck["callbacks"] == {"ModelCheckpoint": {"saved": ["x.ckpt"]}, "WeightAveraging": {"latest_update_step": 4}}
    assert mc_state == {"saved": ["x.ckpt"]}
    assert ck["state_dict"]["unet.w"].tolist() == [5.0, 5.0] and ck["current_model_state"]["unet.w"].tolist() == [1.0, 1.0]
    assert torch.equal(m.unet.w.detach(), torch.ones(2))  # nothing was written while saving
    # resumed with the callback: the module gets the weights it trained on
    cb2 = EMAWeightAveraging()
    f2, m2 = fitter([ModelCheckpoint(dirpath=str(tmp_path)), cb2])
    with torch.no_grad():
        m2.unet.w.zero_()
    f2.load_checkpoint(path)
    assert m2.unet.w.tolist() == [1.0, 1.0] and cb2.latest_update_step == 4 and cb2._resumed[1] == 7
    assert f2.callbacks[0].saved == ["x.ckpt"]
    capsys.readouterr()
    # resumed without it: state_dict as before (the average), and one line about current_model_state
    f3, m3 = fitter([])
    f3.load_checkpoint(path)
    out = capsys.readouterr().out
    assert m3.unet.w.tolist() == [5.0, 5.0]
    assert len(out.strip().splitlines()) == 1 and "current_model_state" in out and "not used" in out
