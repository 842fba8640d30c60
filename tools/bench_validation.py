"""Time the validation path (uwudiff_amd/validation.py, Fitter.validate) on one GPU.

    python tools/bench_validation.py                   # both measurements below
    python tools/bench_validation.py --only kernel
    python tools/bench_validation.py --only pass

1. The per-timestep statistics of one validation batch at B = 768 and B = 3072, n_steps = 1000: ``uwu_timestep_stats_accum`` (through
   ``TimestepLossStats.update``) against the formulation of the reference's callback (src/duwu/trainer/callbacks.py:85-91: a Python loop
   over all timesteps with a boolean mask and three masked reductions each) on the same device tensors -- what a user without the kernel
   has to write.  Device events around each call, median of --calls after --warmup; each side runs in a process of its own (this
   script starts them one after the other and collects their JSON lines).
2. A DiT-S/2 validation pass (``Fitter.validate``: forward, loss, statistics; --val-batches batches of 768 latents of 4x32x32, already
   on the device) in images/s, next to the training step (forward, loss, backward, fused AdamW) of the same module at the same batch,
   from the same process.  The pass is timed by the host clock round ``validate``, which ends in its device-to-host read; the training
   step by device events.  No text encoder: the conditioning vector is zeros, as in bench.py.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_text import time_calls  # noqa: E402

N_STEPS = 1000


def reference_update(counts, sums, squares, losses, timesteps, n_steps):
    """callbacks.py:84-91, line for line"""
    timesteps = timesteps.long()
    for timestep in range(n_steps):
        relevant_indices = timesteps == timestep
        counts[timestep] += relevant_indices.sum()
        sums[timestep] += losses[relevant_indices].sum()
        squares[timestep] += (losses[relevant_indices] ** 2).sum()


def bench_side(side, batches, warmup, calls):
    import torch

    from uwudiff_amd.validation import TimestepLossStats

    rows = []
    for B in batches:
        g = torch.Generator().manual_seed(B)
        losses = (torch.randn(B, generator=g).abs() * 0.3).cuda()
        timesteps = torch.randint(0, N_STEPS, (B,), generator=g).cuda()
        if side == "kernel":
            stats = TimestepLossStats(N_STEPS, "cuda")
            loss = losses.mean()
            run = lambda: stats.update(losses, timesteps, loss)  # noqa: E731
        else:
            vec = [torch.zeros(N_STEPS, device="cuda") for _ in range(3)]
            run = lambda: reference_update(*vec, losses, timesteps, N_STEPS)  # noqa: E731
        times = time_calls(run, warmup, calls)
        rows.append(dict(side=side, B=B, n_steps=N_STEPS, ms=statistics.median(times), ms_min=min(times), ms_max=max(times)))
    return rows


def bench_pass(args):
    import torch

    from duwu.trainer.trainer import DMTrainer
    from uwudiff_amd.engine import Fitter

    torch.manual_seed(0)
    B = args.batch
    mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": "DiT-S/2", "cond_dim": 1280, "init": "random"}}
    tr = DMTrainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-4).cuda()
    fit = Fitter(precision="bf16-mixed")  # (the DiT's default compute type is bf16)
    opt = tr.configure_optimizers()
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(B, 4, 32, 32, generator=g).cuda(), [""] * B, [], {}, {}) for _ in range(args.val_batches)]
    one = torch.ones((), device="cuda")

    def train_step():
        tr.training_step(batches[0], 0)["loss"].backward(one)
        opt.step(zero_grad=True)

    def val_pass():
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):  # (the JSON line of every pass)
            fit.validate(tr, batches)  # ends in the device-to-host read of the statistics
        return (time.perf_counter() - t0) * 1e3

    rows = []
    for rep in range(args.repeats):  # the two alternate, so that a drift of the machine shows in both
        step_ms = statistics.median(time_calls(train_step, args.warmup, args.calls))
        for _ in range(args.warmup):
            val_pass()
        pass_ms = statistics.median([val_pass() for _ in range(args.calls)])
        rows.append(dict(repeat=rep, batch=B, val_batches=args.val_batches, train_step_ms=step_ms, train_images_per_s=B / step_ms * 1e3,
                         val_pass_ms=pass_ms, val_images_per_s=B * args.val_batches / pass_ms * 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "pass"))
    ap.add_argument("--side", choices=("kernel", "reference"), help="one side of measurement 1 in this process (used by the script itself)")
    ap.add_argument("--batches", type=int, nargs="+", default=[768, 3072])
    ap.add_argument("--batch", type=int, default=768)
    ap.add_argument("--val-batches", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.side:
        print(json.dumps(bench_side(args.side, args.batches, args.warmup, args.calls)))
        return
    out = {}
    if args.only != "pass":
        out["kernel"] = []
        for rep in range(args.repeats):
            for side in ("kernel", "reference"):  # a fresh process per side, one at a time
                cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--calls", str(args.calls), "--warmup", str(args.warmup),
                       "--batches", *map(str, args.batches)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                for row in json.loads(r.stdout.strip().splitlines()[-1]):
                    out["kernel"].append(dict(repeat=rep, **row))
    if args.only != "kernel":
        out["pass"] = bench_pass(args)
    if args.json:
        print(json.dumps(out))
        return
    for r in out.get("kernel", []):
        name = "uwu_timestep_stats_accum" if r["side"] == "kernel" else "reference loop (callbacks.py:85-91)"
        print(f"run {r['repeat']}: B = {r['B']}, n_steps = {r['n_steps']}: {name} {r['ms']:.3f} ms per batch (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})")
    for r in out.get("pass", []):
        print(f"run {r['repeat']}: DiT-S/2 bf16, batch {r['batch']}: training step {r['train_step_ms']:.2f} ms = {r['train_images_per_s']:.0f} images/s; "
              f"validation pass of {r['val_batches']} batches {r['val_pass_ms']:.2f} ms = {r['val_images_per_s']:.0f} images/s")


if __name__ == "__main__":
    main()
