"""Time of the fused objective kernel alone (``loss_fwd_bwd_kernel``) under each element loss, one GPU.

    python tools/bench_objective.py [--repeats 3] [--against OTHER/libuwu_hip.so] [--bits]

Shapes: B = 768, n = 4096 (the headline's 4x32x32 latents) and B = 16, n = 65536 (the reference YAML's batch on SDXL's 4x128x128
latents), model output and gradient in fp32 and in bf16, epsilon -> epsilon (no conversion: x, noise and the output are read,
the gradient, pred and target written).  The call is ``uwu_loss_elem_fwd_bwd`` without the batch mean (``loss_mean = NULL``), so one
kernel per call.  Each (library, kind) is measured in a process of its own, the kinds alternating per repeat; a measurement is
the median over windows of back-to-back calls between two device events, after a warm-up, and the calls of a window walk a ring
of buffer sets larger than the last-level cache, so GB/s is traffic to memory: x and noise read, pred and target written (4 fp32)
plus the output read and the gradient written in their dtype, per element, over the time: 24 B (fp32) or 20 B (bf16).  Without a
conversion the kernel does not read xt.

``--against`` times ``uwu_loss_fwd_bwd`` (MSE) of another build's library in the same alternation: the yardstick.  ``--bits`` (with
``--against``) instead runs both libraries' MSE on the same seeded inputs at [3, 4, 16, 20], fp32 and bf16, same-type and
converting, and reports whether loss, losses, pred, target and gradient are bit-equal.  One JSON line at the end."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"mse": (0, 0.0), "l1": (1, 0.0), "huber": (2, 0.1), "smooth_l1": (3, 0.1)}
SHAPES = ((768, 4096), (16, 65536))
RING_BYTES = 512 << 20  # twice the 256 MiB last-level cache
WINDOWS, CALLS, WARMUP = 21, 50, 100
LIMIT = 300


def _bind(path):
    """uwu_loss_fwd_bwd and, where the library has it, uwu_loss_elem_fwd_bwd of the library at ``path`` (signatures of lib.py)"""
    from uwudiff_amd import lib as L

    cd = ctypes.CDLL(path)
    fns = {}
    for name in ("uwu_loss_fwd_bwd", "uwu_loss_elem_fwd_bwd"):
        if hasattr(cd, name):
            fn = getattr(cd, name)
            fn.restype, fn.argtypes = L._SIGS[name]
            fns[name] = fn
    return fns


def _call(fns, kind, t, pt, tt, with_mean=False):
    from uwudiff_amd import lib as L

    B, n = t["x"].shape[0], t["x"][0].numel()
    head = (L.ptr(t["x"]), L.ptr(t["noise"]), L.ptr(t["x"]), L.ptr(t["mo"]), L.dt(t["mo"]), L.ptr(t["coef"]), pt, tt, 0)
    tail = (B, n, L.ptr(t["losses"]), L.ptr(t["loss"]) if with_mean else None, L.ptr(t["grad"]), L.ptr(t["pred"]), L.ptr(t["target"]),
            L.stream())
    if kind == "parent_mse":
        rc = fns["uwu_loss_fwd_bwd"](*head, *tail)
    else:
        rc = fns["uwu_loss_elem_fwd_bwd"](*head, *KINDS[kind], *tail)
    if rc != 0:
        raise SystemExit(f"{kind}: the library refused the call (code {rc})")


def _buffers(B, n, dtype, gen):
    import torch

    t = {k: torch.randn(B, n, generator=gen, device="cuda") for k in ("x", "noise")}
    t["mo"] = torch.randn(B, n, generator=gen, device="cuda").to(dtype)
    sig = torch.rand(B, generator=gen, device="cuda") * 10 + 0.05
    abar = 1 / (1 + sig * sig)
    t["coef"] = torch.stack([sig, torch.ones_like(sig), abar.sqrt(), (1 - abar).sqrt()], dim=1).contiguous()
    t["losses"], t["loss"] = torch.empty(B, device="cuda"), torch.empty((), device="cuda")
    t["grad"], t["pred"], t["target"] = torch.empty_like(t["mo"]), torch.empty_like(t["x"]), torch.empty_like(t["x"])
    return t


def run_one(kind, path):
    import torch

    fns = _bind(path)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, n in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            per_elem = 4 * 4 + 2 * (4 if dtype == torch.float32 else 2)  # x, noise, pred, target + output, gradient
            nbytes = B * n * per_elem
            ring = [_buffers(B, n, dtype, gen) for _ in range(-(-RING_BYTES // nbytes))]
            for i in range(WARMUP):
                _call(fns, kind, ring[i % len(ring)], 0, 0)
            torch.cuda.synchronize()
            ms, k = [], 0
            for _ in range(WINDOWS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    _call(fns, kind, ring[k % len(ring)], 0, 0)
                    k += 1
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / CALLS)
            med = statistics.median(ms)
            rows.append(dict(kind=kind, B=B, n=n, dtype=str(dtype).split(".")[-1], ms=med, ms_min=min(ms), ms_max=max(ms),
                             gb_per_s=nbytes / (med * 1e-3) / 1e9, ring=len(ring)))
            del ring
            torch.cuda.empty_cache()
    return rows


def compare_bits(path_new, path_old):
    import torch

    new, old = _bind(path_new), _bind(path_old)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        for pt, tt in ((0, 0), (0, 1), (2, 0), (1, 3)):  # epsilon, epsilon -> v, sample -> epsilon, v -> rectified flow
            t = _buffers(3, 4 * 16 * 20, dtype, gen)
            outs = []
            for fns, kind in ((new, "mse"), (old, "parent_mse"), (new, "parent_mse")):
                for k in ("losses", "loss", "grad", "pred", "target"):
                    t[k].fill_(-7.0)
                _call(fns, kind, t, pt, tt, with_mean=True)
                torch.cuda.synchronize()
                outs.append({k: t[k].clone() for k in ("loss", "losses", "pred", "target", "grad")})
            res[f"{str(dtype).split('.')[-1]} pred {pt} target {tt}"] = all(
                torch.equal(outs[0][k], o[k]) for o in outs[1:] for k in outs[0]) and bool(outs[0]["loss"].isfinite())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--against", help="another build's libuwu_hip.so: its uwu_loss_fwd_bwd is timed in the same alternation")
    ap.add_argument("--bits", action="store_true", help="with --against: compare the two libraries' MSE outputs bit for bit instead")
    ap.add_argument("--one", help="one measurement in this process (used by the script itself)")
    ap.add_argument("--lib", help="the library --one measures")
    a = ap.parse_args()
    import torch

    from uwudiff_amd import lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_objective.py measures on the GPU; there is no CPU path")
    if a.one:
        print(json.dumps(run_one(a.one, a.lib)))
        return
    if a.bits:
        if not a.against:
            raise SystemExit("--bits compares against another library: give --against")
        res = compare_bits(L.LIB_PATH, os.path.abspath(a.against))
        for k, v in res.items():
            print(f"MSE, {k}: loss, losses, pred, target, grad {'bit-equal' if v else 'DIFFER'}")
        print(json.dumps({"bit_equal": res, "all": all(res.values())}))
        raise SystemExit(0 if all(res.values()) else 1)
    cases = [(k, L.LIB_PATH) for k in KINDS]
    if a.against:
        cases.insert(0, ("parent_mse", os.path.abspath(a.against)))
    rows = []
    for rep in range(a.repeats):
        for kind, path in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--lib", path]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
            if r.returncode != 0:
                raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            for row in json.loads(r.stdout.strip().splitlines()[-1]):
                rows.append(dict(repeat=rep, **row))
                print(f"run {rep}: {kind:10s} B={row['B']:4d} n={row['n']:6d} {row['dtype']:8s} {row['ms'] * 1e3:8.2f} us "
                      f"(min {row['ms_min'] * 1e3:.2f}, max {row['ms_max'] * 1e3:.2f})  {row['gb_per_s']:7.1f} GB/s", flush=True)
    med = []
    for kind, _ in cases:
        for B, n in SHAPES:
            for dt in ("float32", "bfloat16"):
                sel = [r for r in rows if (r["kind"], r["B"], r["n"], r["dtype"]) == (kind, B, n, dt)]
                ms = [r["ms"] for r in sel]
                m = dict(kind=kind, B=B, n=n, dtype=dt, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
                         gb_per_s=statistics.median(r["gb_per_s"] for r in sel))
                med.append(m)
                print(f"median of {len(ms)}: {kind:10s} B={B:4d} n={n:6d} {dt:8s} {m['ms'] * 1e3:8.2f} us "
                      f"(runs {m['ms_min'] * 1e3:.2f} .. {m['ms_max'] * 1e3:.2f})  {m['gb_per_s']:7.1f} GB/s")
    print(json.dumps({"runs": rows, "median": med}))


if __name__ == "__main__":
    main()
