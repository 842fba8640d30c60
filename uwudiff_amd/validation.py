"""Per-timestep loss statistics of a validation pass.

Reference: ``PlotValLossPerTimestep`` (src/duwu/trainer/callbacks.py:58-125) keeps three fp32 vectors of length ``n_steps`` -- count,
sum of the per-sample losses, sum of their squares, per ``timesteps.long()`` -- and fills them with a Python loop over all timesteps,
three masked reductions each, every batch.  Here the three vectors and the two numbers behind the epoch's ``val/loss``
(``self.log(..., on_epoch=True, batch_size=B)``: the sample-weighted mean of the batches' scalar losses) are ONE float64 tensor on the
device, and a batch is one ``uwu_timestep_stats_accum`` launch: ``update`` never waits for the device, ``reduce`` is one all-reduce,
``compute`` reads the tensor once.
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from . import lib as L


class TimestepLossStats:
    def __init__(self, n_steps, device="cpu"):
        self.n_steps = int(n_steps)
        if not 1 <= self.n_steps <= 65536:
            raise ValueError(f"TimestepLossStats: n_steps = {n_steps} outside 1..65536")
        self.device = torch.device(device)
        # [count | sum | sum of squares] of n_steps each, then (sum of B * loss, sum of B)
        self.state = torch.zeros(3 * self.n_steps + 2, dtype=torch.float64, device=self.device)

    def reset(self):
        self.state.zero_()

    @torch.no_grad()
    def update(self, losses, timesteps, loss=None):
        """losses [B] (fp32), timesteps [B] (int64, or float: truncated toward zero), loss: the batch's scalar loss or None."""
        B = losses.numel()
        if timesteps.numel() != B or B == 0:
            raise ValueError(f"TimestepLossStats.update: {B} losses and {timesteps.numel()} timesteps")
        if losses.device != self.state.device or timesteps.device != self.state.device:
            raise ValueError(f"TimestepLossStats.update: the state is on {self.state.device}, losses on {losses.device}, timesteps on "
                             f"{timesteps.device}")
        n = self.n_steps
        if losses.is_cuda:
            losses = losses.detach().reshape(-1).float().contiguous()
            if timesteps.dtype not in (torch.int64, torch.float32):
                timesteps = timesteps.float() if timesteps.is_floating_point() else timesteps.long()
            timesteps = timesteps.detach().reshape(-1).contiguous()
            lm = None
            if loss is not None:
                lm = loss.detach().reshape(-1).float().contiguous()
                if lm.numel() != 1 or lm.device != losses.device:
                    raise ValueError("TimestepLossStats.update: loss must be one number on the device of the losses")
            L.call("uwu_timestep_stats_accum", L.ptr(losses), L.ptr(timesteps), L.I64 if timesteps.dtype == torch.int64 else L.F32,
                   L.ptr(lm), B, n, L.ptr(self.state), self.state[3 * n:].data_ptr() if lm is not None else None, L.stream())
            return
        # CPU tensors (the accelerator="cpu" driver of the host-logic tests): the same sums in float64, a bucket's samples in ascending b
        ls = losses.detach().reshape(-1).to(torch.float32).double()
        t = timesteps.detach().reshape(-1)
        if t.is_floating_point():
            ok = (t > -1) & (t < n)  # (NaN fails both)
            bucket = torch.where(ok, t, torch.zeros_like(t)).long()  # .long() truncates toward zero
        else:
            bucket = t.long()
            ok = (bucket >= 0) & (bucket < n)
        st = self.state
        for b in torch.nonzero(ok).flatten().tolist():
            k = int(bucket[b])
            st[k] += 1.0
            st[n + k] += ls[b]
            st[2 * n + k] += ls[b] * ls[b]
        if loss is not None:
            st[3 * n] += float(B) * float(loss.detach().float())
            st[3 * n + 1] += float(B)

    def reduce(self):
        """Sum the state over the ranks of the default process group (reference: three all_gathers and a sum each); no-op without one."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.state, op=dist.ReduceOp.SUM)
        return self

    def compute(self):
        """-> dict of numpy float64 arrays over the timesteps that were seen -- ``timesteps`` (int64), ``count``, ``mean``, ``std`` =
        sqrt(max(E[l^2] - mean^2, 0)) -- and ``loss``, ``n_samples`` (floats; loss is NaN when no batch passed its scalar loss).
        The one device-to-host read."""
        n = self.n_steps
        st = self.state.cpu().numpy()
        count, s, sq = st[:n], st[n:2 * n], st[2 * n:3 * n]
        seen = count > 0
        c = count[seen]
        mean = s[seen] / c
        with np.errstate(invalid="ignore"):
            std = np.sqrt(np.maximum(sq[seen] / c - mean * mean, 0.0))
        tot, nb = float(st[3 * n]), float(st[3 * n + 1])
        return {"timesteps": np.nonzero(seen)[0].astype(np.int64), "count": c.copy(), "mean": mean, "std": std,
                "loss": tot / nb if nb > 0 else math.nan, "n_samples": nb}
