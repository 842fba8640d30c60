"""reference src/duwu/trainer/callbacks.py: ``PlotValLossPerTimestep`` (:48-158) on the fit loop's validation hooks, without Lightning.

The reference fills three fp32 vectors with a Python loop over all timesteps, three masked reductions each, every batch; here a batch is
one ``uwu_timestep_stats_accum`` launch into a float64 accumulator on the device (``uwudiff_amd.validation.TimestepLossStats``), the
ranks are summed by one all-reduce, and the standard deviation is the reference's formula in double with the clamp that fp32 needs there.
``LogAdditionalLosses`` (:10-45) is not built: it exists for per-step ``.item()`` logging into a logger, and there is no logger here.
"""
import os

import numpy as np

from uwudiff_amd.validation import TimestepLossStats


class PlotValLossPerTimestep:
    # Note (reference :49): this also runs for the sanity pass at the beginning of training

    def __init__(self, n_diffusion_time_steps: int | None = None, loss_key: str = "losses"):
        self.n_diffusion_time_steps = n_diffusion_time_steps
        self.loss_key = loss_key
        self.stats = None
        self.last = None  # the arrays of the last validation epoch (rank 0)

    def on_validation_epoch_start(self, trainer, pl_module):
        if self.stats is not None:
            self.stats.reset()

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        _, aux_output = outputs
        losses = getattr(aux_output, self.loss_key)
        n = int(self.n_diffusion_time_steps or pl_module.n_diffusion_time_steps)
        if self.stats is None or self.stats.n_steps != n or self.stats.device != losses.device:
            self.stats = TimestepLossStats(n, losses.device)
        self.stats.update(losses, aux_output.timesteps)  # timesteps may be float (:83-84): the kernel truncates like .long()

    def on_validation_epoch_end(self, trainer, pl_module):
        if self.stats is None:
            return
        res = self.stats.reduce().compute()
        if getattr(trainer, "global_rank", 0) != 0:
            return
        self.last = {k: res[k] for k in ("timesteps", "count", "mean", "std")}
        # no logger here: <default_root_dir>/plots/ instead of the logger's experiment directory (:143-148)
        stem = os.path.join(getattr(trainer, "default_root_dir", None) or ".", "plots",
                            f"{self.loss_key}_per_timestep-training_step-{trainer.global_step}")
        os.makedirs(os.path.dirname(stem), exist_ok=True)
        np.savez(stem + ".npz", **self.last)
        try:
            import matplotlib
        except ImportError:
            return
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        t, mean, std = self.last["timesteps"], self.last["mean"], self.last["std"]
        fig = plt.figure(figsize=(12, 8))
        plt.plot(t, mean)
        plt.fill_between(t, mean - std, mean + std, alpha=0.2)
        plt.xlabel("Timestep")
        plt.ylabel("Loss")
        plt.savefig(stem + ".png")
        plt.close(fig)
