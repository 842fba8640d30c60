"""What gradient accumulation costs or saves per micro-batch (``Fitter(accumulate_grad_batches=N)``), one GPU.

    python tools/bench_accumulate.py                         # every configuration below, N = 1 and N = 4
    python tools/bench_accumulate.py --only dit-s2-b16 --n 1 4 8

Configurations: DiT-S/2 bf16 at per-GPU batch 768 and 16 (4x32x32 latents, pooled-text conditioning), and the SDXL-shape UNet bf16 at
batch 12 (4x128x128 latents, 77 x 2048 context).  Each (configuration, N) runs in a process of its own under its own time limit; this
script starts them one after the other, N = 1 and N > 1 alternating over --repeats, and collects their JSON lines.

What is timed is the fit loop itself: ``Fitter.fit`` over --batches micro-batches that are already on the device (fused AdamW, no
clipping, no text encoder, one log record at the end), by the host clock round the call, which ends in a device synchronisation; a
shorter fit before it warms the kernels and the allocator up.  Per window of N micro-batches, N - 1 optimizer launches (which also
zero the gradient and refresh the bf16 shadow of the parameters) are not issued; the backward passes are the same.
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

CONFIGS = {
    # name: (model, per-GPU batch, latent side, timed micro-batches, warm-up micro-batches, time limit of one process in seconds)
    "dit-s2-b768": ("DiT-S/2", 768, 32, 48, 16, 300),
    "dit-s2-b16": ("DiT-S/2", 16, 32, 192, 48, 300),
    "sdxl-unet-b12": ("SDXL-UNet", 12, 128, 8, 4, 600),
}


class _ListDM:
    def __init__(self, batches):
        self.batches = batches

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return self.batches


def run_one(name, n_acc, batches, warmup):
    import torch

    from duwu.trainer.trainer import DMTrainer
    from uwudiff_amd.engine import Fitter

    model, B, S, _, _, _ = CONFIGS[name]

    class _Trainer(DMTrainer):
        """no text encoder: the context and the pooled embedding travel in the batch's `added` dict"""

        def get_latent_and_conditioning(self, batch):
            x, _, _, added, ca = batch
            added = dict(added)
            return x, added.pop("ctx", None), None, added, ca

    torch.manual_seed(0)
    if model == "SDXL-UNet":
        mc = {"unet": {"_target_": "uwudiff_amd.unet.UNet2DConditionModel.from_config", "config": "sdxl", "compute_dtype": "bf16",
                       "device": "cuda"}}
    else:
        mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": model, "cond_dim": 1280, "init": "random"}}
    tr = _Trainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-6).cuda()
    g = torch.Generator().manual_seed(1)

    def batch():
        added = {"text_embeds": torch.randn(B, 1280, generator=g).cuda()}
        if model == "SDXL-UNet":
            added["ctx"] = torch.randn(B, 77, 2048, generator=g).cuda()
            added["time_ids"] = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B).cuda()
        return (torch.randn(B, 4, S, S, generator=g).cuda(), [""] * B, [], added, {})

    pool = [batch() for _ in range(4)]  # (the loop walks them round and round: the data is not what is measured)

    def fit(n_batches):
        f = Fitter(precision="bf16-mixed", accumulate_grad_batches=n_acc, log_every_n_steps=1 << 30, max_epochs=1)
        dm = _ListDM([pool[i % len(pool)] for i in range(n_batches)])
        tr.train_params = tr.unet.parameters()  # (the trainer keeps a generator, which a fit uses up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            f.fit(tr, dm)  # (ends in torch.cuda.synchronize())
        dt = time.perf_counter() - t0
        assert f.train_batches == n_batches and f.global_step == -(-n_batches // n_acc)
        return dt

    fit(warmup)
    dt = fit(batches)
    return dict(config=name, model=model, batch=B, latent=S, n=n_acc, micro_batches=batches, optimizer_steps=-(-batches // n_acc),
                ms_per_micro_batch=dt / batches * 1e3, images_per_s=B * batches / dt,
                peak_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=sorted(CONFIGS))
    ap.add_argument("--n", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", nargs=2, metavar=("CONFIG", "N"), help="one configuration in this process (used by the script itself)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.one:
        name, n_acc = args.one[0], int(args.one[1])
        _, _, _, batches, warmup, _ = CONFIGS[name]
        print(json.dumps(run_one(name, n_acc, batches, warmup)))
        return
    rows = []
    for name in args.only or list(CONFIGS):
        limit = CONFIGS[name][5]
        for rep in range(args.repeats):
            for n_acc in args.n:  # the values of N alternate, so that a drift of the machine shows in all of them
                cmd = [sys.executable, os.path.abspath(__file__), "--one", name, str(n_acc)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                if r.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                row = dict(repeat=rep, **json.loads(r.stdout.strip().splitlines()[-1]))
                rows.append(row)
                if not args.json:
                    print(f"run {rep}: {row['model']} bf16, batch {row['batch']}, N = {row['n']}: {row['ms_per_micro_batch']:.3f} ms per "
                          f"micro-batch = {row['images_per_s']:.1f} images/s ({row['micro_batches']} micro-batches, "
                          f"{row['optimizer_steps']} optimizer steps, peak {row['peak_gb']:.1f} GB)", flush=True)
    if args.json:
        print(json.dumps(rows))
        return
    for name in args.only or list(CONFIGS):
        for n_acc in args.n:
            ms = [r["ms_per_micro_batch"] for r in rows if r["config"] == name and r["n"] == n_acc]
            ips = [r["images_per_s"] for r in rows if r["config"] == name and r["n"] == n_acc]
            print(f"{name} N = {n_acc}: median {statistics.median(ms):.3f} ms per micro-batch (min {min(ms):.3f}, max {max(ms):.3f}), "
                  f"median {statistics.median(ips):.1f} images/s")


if __name__ == "__main__":
    main()
