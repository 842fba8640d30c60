"""What keeping a weight average costs (uwudiff_amd/averaging.py), one GPU.

    python tools/bench_averaging.py [--sizes 32966464,2570000000] [--reps 5] [--warmup 3] [--repeats 3] [--skip-step]

1. The two averaging kernels alone (``uwu_ema_update``, ``uwu_ema_swap`` in both modes, with the bf16 shadow) at DiT-S/2's parameter
   count and at the SDXL-shape UNet's 2.57 G: ms per launch, bytes moved per parameter and GB/s, with ``uwu_adamw_step`` (shadow and
   ``zero_grad`` on) measured in the same process at the same sizes as the yardstick.  Device events round a window of launches, the
   kernels alternating inside every repetition; the spread over the repetitions is printed with every median.
2. The DiT-S/2 bf16 training step at per-GPU batch 768 through ``Fitter.fit`` with and without ``EMAWeightAveraging`` (an update after
   every optimizer step), each in a process of its own, the two alternating over --repeats (the fit loop of tools/bench_accumulate.py:
   batches already on the device, fused AdamW, no clipping, no text encoder, the host clock round a fit that ends in a device
   synchronisation, a shorter fit before it as warm-up).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIT_S2, SDXL_UNET = 32_966_464, 2_570_000_000
# bytes per parameter, from the rule: avg and p read, avg written | both read and written, shadow written | avg read, p and shadow
# written | AdamW's p, g, m, v read, p, m, v written, + shadow + zeroed gradient (tools/bench_optim.py)
BYTES = {"ema_update": 8 + 4, "ema_swap": 8 + 8 + 2, "ema_copy": 4 + 4 + 2, "adamw": 16 + 12 + 2 + 4}
STEP = {"model": "DiT-S/2", "batch": 768, "latent": 32, "batches": 48, "warmup": 16, "limit": 300}


def bench_size(n, reps, warmup):
    import torch

    from uwudiff_amd import lib as L

    dev = torch.device("cuda", 0)
    f32 = lambda: torch.empty(n, device=dev, dtype=torch.float32)  # noqa: E731
    p, g, avg = f32().normal_(), f32().normal_().mul_(1e-3), f32().normal_()
    m, v = f32().zero_(), f32().zero_()
    shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    s = L.stream()
    launch = {
        "ema_update": lambda k: L.call("uwu_ema_update", L.ptr(avg), L.ptr(p), n, 0.999, 1.0 - 0.999, s),
        "ema_swap": lambda k: L.call("uwu_ema_swap", L.ptr(avg), L.ptr(p), L.ptr(shadow), n, 0, s),
        "ema_copy": lambda k: L.call("uwu_ema_swap", L.ptr(avg), L.ptr(p), L.ptr(shadow), n, 1, s),
        "adamw": lambda k: L.call("uwu_adamw_step", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(shadow), n, 1e-6, 0.9, 0.999, 1e-8,
                                  0.01, k, 1.0, None, 1, s),
    }
    iters = max(4, min(200, int(2e11 / (34 * n))))  # (an even count: the window's swaps leave both buffers where they were)
    iters += iters % 2
    for k in range(1, warmup + 1 + warmup % 2):
        for fn in launch.values():
            fn(k)
    torch.cuda.synchronize()
    ms = {name: [] for name in launch}
    for _ in range(reps):
        for name, fn in launch.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(iters):
                fn(warmup + 2 + k)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    out = {}
    for name, times in ms.items():
        times = sorted(times)
        med, bpp = times[len(times) // 2], BYTES[name]
        out[name] = {"ms": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "bytes_per_param": bpp,
                     "GBps": round(bpp * n / med / 1e6, 1), "GBps_min": round(bpp * n / times[-1] / 1e6, 1),
                     "GBps_max": round(bpp * n / times[0] / 1e6, 1)}
    return {"n": n, "launches_per_window": iters, "reps": reps, "kernels": out}


class _ListDM:
    def __init__(self, batches):
        self.batches = batches

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return self.batches


def run_step(with_ema):
    import torch

    from duwu.trainer.trainer import DMTrainer
    from uwudiff_amd.averaging import EMAWeightAveraging
    from uwudiff_amd.engine import Fitter

    B, S = STEP["batch"], STEP["latent"]

    class _Trainer(DMTrainer):
        """no text encoder: the pooled embedding travels in the batch's `added` dict"""

        def get_latent_and_conditioning(self, batch):
            x, _, _, added, ca = batch
            return x, None, None, dict(added), ca

    torch.manual_seed(0)
    mc = {"unet": {"_target_": "uwudiff_amd.dit.DiT.from_config", "config": STEP["model"], "cond_dim": 1280, "init": "random"}}
    tr = _Trainer(mc, use_warm_up=False, lr_scheduler=None, lr=1e-6).cuda()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.randn(B, 4, S, S, generator=g).cuda(), [""] * B, [], {"text_embeds": torch.randn(B, 1280, generator=g).cuda()}, {})
            for _ in range(4)]
    updates = []

    def fit(n_batches):
        cbs = [EMAWeightAveraging(decay=0.999)] if with_ema else []
        f = Fitter(precision="bf16-mixed", log_every_n_steps=1 << 30, max_epochs=1, callbacks=cbs)
        dm = _ListDM([pool[i % len(pool)] for i in range(n_batches)])
        tr.train_params = tr.unet.parameters()  # (the trainer keeps a generator, which a fit uses up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            f.fit(tr, dm)  # (ends in torch.cuda.synchronize())
        dt = time.perf_counter() - t0
        assert f.global_step == n_batches
        updates.append(cbs[0].average.n_averaged if with_ema else 0)
        return dt

    fit(STEP["warmup"])
    dt = fit(STEP["batches"])
    assert updates[-1] == (STEP["batches"] if with_ema else 0)
    return dict(model=STEP["model"], batch=B, ema=bool(with_ema), steps=STEP["batches"], updates=updates[-1],
                ms_per_step=dt / STEP["batches"] * 1e3, images_per_s=B * STEP["batches"] / dt, params=tr.unet.flat.numel(),
                peak_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{DIT_S2},{SDXL_UNET}")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--one", choices=["ema", "plain"], help="one step measurement in this process (used by the script itself)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_averaging.py measures on the GPU; there is no CPU path")
    if a.one:
        print(json.dumps(run_step(a.one == "ema")))
        return
    res = {"sizes": [bench_size(int(n), a.reps, a.warmup) for n in a.sizes.split(",")], "step": []}
    for r in res["sizes"]:
        for name, k in r["kernels"].items():
            print(f"n = {r['n']:>13,}  {name:<10} {k['ms']:9.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f})  "
                  f"{k['bytes_per_param']:>2} B/param  {k['GBps']:8.1f} GB/s ({k['GBps_min']:.1f} .. {k['GBps_max']:.1f})", flush=True)
        u, w = r["kernels"]["ema_update"], r["kernels"]["adamw"]
        print(f"n = {r['n']:>13,}  ema_update / adamw achieved bandwidth: {u['GBps'] / w['GBps']:.3f} (spread of ema_update over "
              f"{r['reps']} repetitions {100 * (u['GBps_max'] - u['GBps_min']) / u['GBps']:.1f} %, of adamw "
              f"{100 * (w['GBps_max'] - w['GBps_min']) / w['GBps']:.1f} %)", flush=True)
    if not a.skip_step:
        for rep in range(a.repeats):
            for which in ("plain", "ema"):  # alternating, so that a drift of the machine shows in both
                cmd = [sys.executable, os.path.abspath(__file__), "--one", which]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP["limit"])
                if r.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                row = dict(repeat=rep, **json.loads(r.stdout.strip().splitlines()[-1]))
                res["step"].append(row)
                print(f"run {rep}: {row['model']} bf16, batch {row['batch']}, {'with' if row['ema'] else 'without'} the average: "
                      f"{row['ms_per_step']:.3f} ms per step = {row['images_per_s']:.1f} images/s ({row['steps']} steps, "
                      f"{row['updates']} updates, peak {row['peak_gb']:.2f} GB)", flush=True)
        med = {}
        for ema in (False, True):
            ms = [r["ms_per_step"] for r in res["step"] if r["ema"] == ema]
            med[ema] = statistics.median(ms)
            print(f"DiT-S/2 batch 768 {'with' if ema else 'without'} the average: median {med[ema]:.3f} ms per step "
                  f"(min {min(ms):.3f}, max {max(ms):.3f})")
        print(f"cost of the average: {med[True] - med[False]:+.3f} ms per step = {100 * (med[True] - med[False]) / med[False]:+.2f} %")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
