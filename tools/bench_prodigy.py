"""Step time of the LyCORIS demo under Prodigy and under AdamW, one GPU.

    python tools/bench_prodigy.py [--steps 8] [--warmup 3] [--repeats 1]

``configs/demo_training_prodigy.yaml`` and ``configs/demo_training_lycoris.yaml`` differ in the optimizer alone.  Each case runs
``Fitter.fit`` on its config in a process of its own under its own time limit (as tools/bench_accumulate.py runs its cases), the two
alternating over --repeats; the step time is the median difference of the fit loop's ``elapsed_s`` between consecutive logged
steps after the warm-up steps (every step is logged, and a log record reads the loss back: the host clock then follows the device).
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"prodigy": "demo_training_prodigy.yaml", "adamw": "demo_training_lycoris.yaml"}
LIMIT_S = 540  # one process: building the SDXL-shape UNet and the text encoders, then a dozen steps


def run_one(case, steps, warmup):
    from duwu.loader import load_all
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything

    os.chdir(ROOT)  # (lycoris_config is a path relative to the repository root)
    with tempfile.TemporaryDirectory() as tmp:
        cfg = merge(load_yaml(os.path.join(ROOT, "configs", CASES[case])),
                    {"lightning_config": {"max_steps": steps + warmup, "log_every_n_steps": 1, "default_root_dir": tmp}})
        lc = dict(cfg["lightning_config"])
        lc.pop("callbacks", None)
        seed_everything(cfg.seed)
        fit = Fitter(**lc)
        dm, tr = load_all(cfg)
        hist = fit.fit(tr, dm)
    opt = fit._fit_state[1]
    t = [h["elapsed_s"] for h in hist]
    dt = sorted(b - a for a, b in zip(t[warmup - 1:], t[warmup:]))
    n_train = sum(p.numel() for g in opt.param_groups for p in g["params"])
    out = {"case": case, "optimizer": type(opt).__name__, "trained_parameters": n_train, "steps": len(dt),
           "step_ms": round(1e3 * statistics.median(dt), 2), "step_ms_min": round(1e3 * dt[0], 2),
           "step_ms_max": round(1e3 * dt[-1], 2), "last_loss": hist[-1]["loss"]}
    if hasattr(opt, "d"):
        out["d"] = opt.d
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    if a.warmup < 1:
        raise SystemExit("--warmup must be at least 1 (the first step pays for every kernel's first launch)")
    if a.case:
        return run_one(a.case, a.steps, a.warmup)
    results = []
    for _ in range(a.repeats):
        for case in CASES:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--steps", str(a.steps), "--warmup", str(a.warmup)]
            lines = []
            with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as proc:
                limit = threading.Timer(LIMIT_S, proc.kill)
                limit.start()
                for ln in proc.stdout:  # passed on as it comes: the fit loop's log records show the run is alive
                    print(ln, end="", flush=True)
                    lines.append(ln)
                proc.wait()
                limit.cancel()
            if proc.returncode != 0:  # nothing more is started on the GPU after a process that failed or ran out of time
                raise SystemExit(f"bench_prodigy.py: the {case} process ended with status {proc.returncode}")
            line = [ln for ln in lines if ln.startswith("RESULT ")][-1]
            results.append(json.loads(line[len("RESULT "):]))
            print(f"{case:<8} {results[-1]['optimizer']:<13} {results[-1]['step_ms']:9.2f} ms/step "
                  f"({results[-1]['step_ms_min']:.2f} .. {results[-1]['step_ms_max']:.2f}), "
                  f"{results[-1]['trained_parameters']:,} trained parameters", flush=True)
    print(json.dumps({"cases": results}))


if __name__ == "__main__":
    main()
