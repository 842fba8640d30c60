"""Step time of DiT-S/2 (bf16, per-GPU batch 768) through ``Fitter.fit`` under schedule-free AdamW and under ``FusedAdamW``
(DESIGN.md section 4.42), one GPU: the set-up of the step measurement of tools/bench_averaging.py with the optimizer changed.

    python tools/bench_schedulefree.py [--repeats 3]

Each case runs in a process of its own, the two alternating, so that a drift of the machine shows in both; the kernels alone are
rows of tools/bench_optim.py.  A fit under the schedule-free optimizer ends with one ``eval()`` (the average written and exchanged
with the weights): it is inside the timed window, once per 48 steps.  One JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_averaging import STEP, _ListDM  # noqa: E402

CASES = {"schedulefree": "schedulefree.AdamWScheduleFree", "adamw": "torch.optim.AdamW"}


def run_step(case):
    import torch

    from duwu.trainer.trainer import DMTrainer
    from uwudiff_amd.engine import Fitter
    from uwudiff_amd.optim import FusedAdamW, FusedAdamWScheduleFree

    B, S = STEP["batch"], STEP["latent"]

    class _Trainer(DMTrainer):
        """no text encoder: the pooled embedding travels in the batch's `added` dict"""

        def get_latent_and_conditioning(self, batch):
            x, _, _, added, ca = batch
            return x, None, None, dict(added), ca

    torch.manual_seed(0)
    mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": STEP["model"], "cond_dim": 1280, "init": "random"}}
    tr = _Trainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-6, optimizer=CASES[case],
                  opt_config={"weight_decay": 0.01, "betas": (0.9, 0.999)}).cuda()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.randn(B, 4, S, S, generator=g).cuda(), [""] * B, [], {"text_embeds": torch.randn(B, 1280, generator=g).cuda()}, {})
            for _ in range(4)]

    def fit(n_batches):
        f = Fitter(precision="bf16-mixed", log_every_n_steps=1 << 30, max_epochs=1)
        dm = _ListDM([pool[i % len(pool)] for i in range(n_batches)])
        tr.train_params = tr.unet.parameters()  # (the trainer keeps a generator, which a fit uses up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            f.fit(tr, dm)  # (ends in torch.cuda.synchronize())
        dt = time.perf_counter() - t0
        assert f.global_step == n_batches
        assert type(f._fit_state[1]) is {"schedulefree": FusedAdamWScheduleFree, "adamw": FusedAdamW}[case]
        return dt

    fit(STEP["warmup"])
    dt = fit(STEP["batches"])
    return dict(model=STEP["model"], batch=B, optimizer=case, steps=STEP["batches"], ms_per_step=dt / STEP["batches"] * 1e3,
                images_per_s=B * STEP["batches"] / dt, params=tr.unet.flat.numel(), peak_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one", choices=sorted(CASES), help="one measurement in this process (used by the script itself)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_schedulefree.py measures on the GPU; there is no CPU path")
    if a.one:
        print(json.dumps(run_step(a.one)))
        return
    rows = []
    for rep in range(a.repeats):
        for case in ("adamw", "schedulefree"):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", case]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP["limit"])
            if r.returncode != 0:
                raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            row = dict(repeat=rep, **json.loads(r.stdout.strip().splitlines()[-1]))
            rows.append(row)
            print(f"run {rep}: {row['model']} bf16, batch {row['batch']}, {case}: {row['ms_per_step']:.3f} ms per step = "
                  f"{row['images_per_s']:.1f} images/s ({row['steps']} steps, peak {row['peak_gb']:.2f} GB)", flush=True)
    med = {}
    for case in CASES:
        ms = [r["ms_per_step"] for r in rows if r["optimizer"] == case]
        med[case] = statistics.median(ms)
        print(f"DiT-S/2 batch 768 under {case}: median {med[case]:.3f} ms per step (min {min(ms):.3f}, max {max(ms):.3f})")
    d = med["schedulefree"] - med["adamw"]
    print(f"schedule-free AdamW against FusedAdamW: {d:+.3f} ms per step = {100 * d / med['adamw']:+.2f} %")
    print(json.dumps({"step": rows, "median_ms": med}))


if __name__ == "__main__":
    main()
