"""The flat-buffer update kernels (AdamW, Lion, AdamWFP16, the 8-bit block-wise AdamW and Lion, Prodigy's three, and schedule-free
AdamW's step and its out-of-place average: uwudiff_amd/csrc/optimizer*.hip) alone, with the bf16
shadow and ``zero_grad`` on, at DiT-S/2's parameter count and at the SDXL-shape UNet's 2.57 G: ms per launch, bytes moved per
parameter and GB/s, and the optimizer-state bytes of the SDXL-shape UNet under each optimizer.  Prodigy is shown as its statistics
pass, its one-workgroup finalize and its apply pass separately, and as the whole step (the three on one stream), next to the AdamW
kernel of the same run.  One JSON line.  DESIGN.md sections 4.28, 4.36, 4.40 and 4.42.

    python tools/bench_optim.py [--sizes 32966464,2570000000] [--reps 5] [--warmup 3]

Bytes per parameter are derived from the update rule (reads + writes of p, g and the state, + 2 for the shadow, + 4 for the zeroed
gradient); the times are device events around a window of launches, the kernels alternating inside every repetition.

Adafactor is per tensor, so it is timed on the real tensor tables of DiT-S/2 and of the SDXL-shape UNet (their flat
registries, no weights needed): its three passes alone and the whole step, in the kohya setting (no parameter scale, no first
moment), next to the AdamW kernel over the same buffer in the same run.  ``--only adafactor`` / ``--only flat`` runs one half."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIT_S2, SDXL_UNET = 32_966_464, 2_570_000_000
# bytes per parameter: (read + written by the update rule, optimizer state held)
KERNELS = {"adamw": (16 + 12, 8), "lion": (12 + 8, 4), "adamw_fp16": (12 + 8, 4),
           # 8-bit codes + one fp32 scale per 256 elements and moment (the scales' traffic, 1/32 B per parameter, is left out)
           "adamw8": (10 + 6, 2 + 8 / 256), "lion8": (9 + 5, 1 + 4 / 256),
           # schedule-free AdamW: y, g, z, v read, y, z, v written; z and v held, and the spare buffer x is written into (4 B)
           "sfadamw": (16 + 12, 8 + 4)}
SF_AVERAGE = 8 + 4  # uwu_sf_average: y and z read, x written out of place (no shadow, no gradient)
EXTRA = 2 + 4  # bf16 shadow written, consumed gradient zeroed
# Prodigy's passes: bytes per parameter with the extras (statistics: p, g, p0, exp_avg, exp_avg_sq, s read, the three moments
# written, + 4 for the zeroed gradient; apply: p, exp_avg, exp_avg_sq read, p written, + 2 for the shadow); 16 B of state
PRODIGY = {"prodigy_stats": 24 + 12 + 4, "prodigy_finalize": 0, "prodigy_apply": 12 + 4 + 2}
PRODIGY["prodigy_step"] = sum(PRODIGY.values())
PRODIGY_STATE = 16  # exp_avg, exp_avg_sq, s, p0
# Adafactor's passes in the kohya setting: g read; g read; g and p read, p written, + 2 for the shadow, + 4 for the zeroed gradient.
# (The tile partials written by the first pass and read by its second launch are 1/64 of that and left out.)
ADAFACTOR = {"adafactor_stats": 4, "adafactor_norm": 4, "adafactor_apply": 8 + 4 + 2 + 4}
ADAFACTOR["adafactor_step"] = sum(ADAFACTOR.values())


def adafactor_models():
    """name -> the flat-buffer model whose registry is the tensor table (the UNet on the meta device: only its layout is used)"""
    from uwudiff_amd.dit import DiT, DiTConfig
    from uwudiff_amd.unet import SDXL_UNET_CONFIG, UNet2DConditionModel

    return {"dit_s2": lambda: DiT(DiTConfig(depth=12, hidden=384, heads=6, patch=2, cond_dim=1280)),
            "unet_sdxl": lambda: UNet2DConditionModel(SDXL_UNET_CONFIG, init_weights=False, device="meta")}


def bench_adafactor(name, reps, warmup):
    import torch

    from uwudiff_amd import lib as L
    from uwudiff_amd.optim import FusedAdafactor, adafactor_state_elems, flat_tensors

    model = adafactor_models()[name]()
    tensors, n = flat_tensors(model), model.flat.numel()
    del model
    dev = torch.device("cuda", 0)
    p = torch.nn.Parameter(torch.empty(n, device=dev, dtype=torch.float32).normal_())
    p.grad = torch.empty(n, device=dev, dtype=torch.float32).normal_().mul_(1e-3)
    p._uwu_bf16_shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    opt = FusedAdafactor([p], lr=1e-6, relative_step=False, scale_parameter=False, warmup_init=False, tensors=tensors)
    opt.step(zero_grad=False)  # allocates the state, the table and the workspaces; the moments are those of a real gradient
    st, group = opt.state[p], opt.param_groups[0]
    desc = opt.descriptor(p, st, L.ptr(p.data), L.ptr(p.grad), L.ptr(p._uwu_bf16_shadow))
    ids = list(range(len(tensors)))
    m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
    s = L.stream()
    calls = dict(opt.pass_calls(group, 2, desc, ids, 1.0, None, 1))
    launch = {"adafactor_" + k[len("uwu_adafactor_"):]: (lambda k=k: L.call(k, *calls[k])) for k in calls}
    launch["adafactor_step"] = lambda: [L.call(k, *a) for k, a in calls.items()]
    launch["adamw"] = lambda: L.call("uwu_adamw_step", L.ptr(p.data), L.ptr(p.grad), L.ptr(m), L.ptr(v), L.ptr(p._uwu_bf16_shadow),
                                     n, 1e-6, 0.9, 0.999, 1e-8, 0.01, 2, 1.0, None, 1, s)
    iters = max(4, min(200, int(2e11 / (34 * n))))
    for _ in range(warmup):
        for fn in launch.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in launch}
    for _ in range(reps):
        for k, fn in launch.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    out = {}
    for k, times in ms.items():
        times = sorted(times)
        med = times[len(times) // 2]
        bpp = ADAFACTOR[k] if k in ADAFACTOR else KERNELS["adamw"][0] + EXTRA
        out[k] = {"ms": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "bytes_per_param": bpp,
                  "GBps": round(bpp * n / med / 1e6, 1)}
    out["adafactor_step"]["ms_vs_adamw"] = round(out["adafactor_step"]["ms"] / out["adamw"]["ms"], 3)
    if not torch.isfinite(p.detach()).all():
        raise SystemExit("bench_optim.py: Adafactor left non-finite parameters")
    elems = adafactor_state_elems(tensors)
    return {"model": name, "n": n, "tensors": len(tensors), "launches_per_window": iters, "reps": reps, "kernels": out,
            "state_bytes": 4 * sum(elems.values()), "workspace_bytes": 4 * opt._dev["fws"].numel() + 8 * opt._dev["dws"].numel()}


def bench_size(n, reps, warmup):
    import math

    import torch

    from uwudiff_amd import lib as L

    dev = torch.device("cuda", 0)
    f32 = lambda: torch.empty(n, device=dev, dtype=torch.float32)  # noqa: E731
    p, g = f32().normal_(), f32().normal_().mul_(1e-3)
    shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    st = {"adamw": (f32().zero_(), f32().zero_()), "lion": (f32().zero_(),),
          "adamw_fp16": (torch.zeros(n, device=dev, dtype=torch.float16), torch.zeros(n, device=dev, dtype=torch.float16))}
    s = L.stream()
    from uwudiff_amd.optim import dynamic_map

    nb = (n + 255) // 256
    q1, q2 = dynamic_map(True).to(dev), dynamic_map(False).to(dev)
    c8 = lambda: torch.zeros(n, device=dev, dtype=torch.uint8)  # noqa: E731
    am = lambda: torch.zeros(nb, device=dev, dtype=torch.float32)  # noqa: E731
    st["adamw8"] = (c8(), c8(), am(), am())
    st["lion8"] = (c8(), am())

    def spread(name):
        """codes drawn uniformly over the table and unit scales, put there before every timed window: every kernel leaves g zeroed,
        and the zero state would send all 64 lanes of a wave down the same path of the table search (no LDS bank conflicts).  With
        g = 0 a block's moments shrink by one factor, so the ratios and the codes stay as spread as they were drawn."""
        for t in st[name]:
            if t.dtype == torch.uint8:
                t.random_(0, 256)
            else:
                t.fill_(1.0)
    launch = {
        "adamw": lambda k: L.call("uwu_adamw_step", L.ptr(p), L.ptr(g), L.ptr(st["adamw"][0]), L.ptr(st["adamw"][1]),
                                  L.ptr(shadow), n, 1e-6, 0.9, 0.999, 1e-8, 0.01, k, 1.0, None, 1, s),
        "lion": lambda k: L.call("uwu_lion_step", L.ptr(p), L.ptr(g), L.ptr(st["lion"][0]), L.ptr(shadow), n, 1e-6, 0.9, 0.99,
                                 0.01, 1.0, None, 1, s),
        "adamw_fp16": lambda k: L.call("uwu_adamw_fp16_step", L.ptr(p), L.ptr(g), L.ptr(st["adamw_fp16"][0]),
                                       L.ptr(st["adamw_fp16"][1]), L.ptr(shadow), n, 1e-6, 0.9, 0.999, 1e-8, k, 1.0, None, 1, s),
        "adamw8": lambda k: L.call("uwu_adamw8_step", L.ptr(p), L.ptr(g), *(L.ptr(t) for t in st["adamw8"]), L.ptr(q1), L.ptr(q2),
                                   L.ptr(shadow), n, 0, n, 1e-6, 0.9, 0.999, 1e-8, 0.01, k, 1.0, None, 1, s),
        "lion8": lambda k: L.call("uwu_lion8_step", L.ptr(p), L.ptr(g), *(L.ptr(t) for t in st["lion8"]), L.ptr(q1),
                                  L.ptr(shadow), n, 0, n, 1e-6, 0.9, 0.99, 0.01, 1.0, None, 1, s),
    }
    # Prodigy on moments of its own, with the demo config's options (bias correction, safeguard, decoupled decay)
    pm, pv, ps, p0 = f32().zero_(), f32().zero_(), f32().zero_(), p.clone()
    scal = torch.tensor([1e-6, 1e-6, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=dev)
    blocks = L.load().uwu_prodigy_stats_blocks(n)
    ws = torch.zeros(2 * blocks, dtype=torch.float64, device=dev)
    b3 = math.sqrt(0.999)
    launch["prodigy_stats"] = lambda k: L.call(
        "uwu_prodigy_stats", L.ptr(p), L.ptr(g), L.ptr(p0), L.ptr(pm), L.ptr(pv), L.ptr(ps), n, L.ptr(scal), L.ptr(ws), blocks, 0,
        1.0, 0.9, 0.999, b3, 0.01, 1, 1e-6, 1, 1, 1.0, None, 1, s)
    launch["prodigy_finalize"] = lambda k: L.call("uwu_prodigy_finalize", L.ptr(scal), L.ptr(ws), blocks, 1.0, 0.9, 0.999, b3,
                                                  1e-6, 1.0, float("inf"), 1, s)
    launch["prodigy_apply"] = lambda k: L.call("uwu_prodigy_apply", L.ptr(p), L.ptr(pm), L.ptr(pv), L.ptr(shadow), n, L.ptr(scal),
                                               1e-8, 0.01, 1, s)
    launch["prodigy_step"] = lambda k: (launch["prodigy_stats"](k), launch["prodigy_finalize"](k), launch["prodigy_apply"](k))
    # one whole Prodigy step while g is still nonzero (every kernel leaves it zeroed): s is nonzero from here on, so no later step
    # returns early and the apply pass does its full work in every window (checked below)
    launch["prodigy_step"](0)
    # schedule-free AdamW on a z and v of its own, past its warm-up (0 < c < 1: the first branch of the lerp, as in a long run)
    sz, sv, sx = p.clone(), f32().zero_(), f32()
    launch["sfadamw"] = lambda k: L.call("uwu_sfadamw_step", L.ptr(p), L.ptr(g), L.ptr(sz), L.ptr(sv), L.ptr(shadow), n, 1e-6, 0.9,
                                         0.999, 1e-8, 0.01, 1.0 / (k + 1), 1.0 - 0.999 ** (k + 1), 1.0, None, 1, s)
    launch["sf_average"] = lambda k: L.call("uwu_sf_average", L.ptr(p), L.ptr(sz), L.ptr(sx), n, 1.0 - 1.0 / 0.9, s)
    iters = max(4, min(200, int(2e11 / (34 * n))))  # a window of roughly 0.2 GB/param-byte: tens of ms at either size
    for k in range(1, warmup + 1):
        for fn in launch.values():
            fn(k)
    torch.cuda.synchronize()
    ms = {name: [] for name in launch}
    for _ in range(reps):
        for name, fn in launch.items():
            if name in ("adamw8", "lion8"):
                spread(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(iters):
                fn(warmup + 1 + k)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    out = {}
    for name, times in ms.items():
        times = sorted(times)
        med = times[len(times) // 2]
        bpp = KERNELS[name][0] + EXTRA if name in KERNELS else SF_AVERAGE if name == "sf_average" else PRODIGY[name]
        out[name] = {"ms": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
                     "bytes_per_param": bpp, "GBps": round(bpp * n / med / 1e6, 1),
                     "GBps_min": round(bpp * n / times[-1] / 1e6, 1), "GBps_max": round(bpp * n / times[0] / 1e6, 1)}
    if scal.tolist()[6] != 0.0:
        raise SystemExit("bench_optim.py: Prodigy's last step returned early (d_denom == 0): its apply pass did no work")
    for name in ("prodigy_stats", "prodigy_apply"):  # plain streams: to be judged against the AdamW kernel of this run
        out[name]["GBps_vs_adamw"] = round(out[name]["GBps"] / out["adamw"]["GBps"], 3)
    # the 8-bit step against the fp32 step of the same run; schedule-free AdamW moves AdamW's bytes and is judged against its time
    for name, ref in (("adamw8", "adamw"), ("lion8", "lion"), ("sfadamw", "adamw")):
        out[name]["ms_vs_" + ref] = round(out[name]["ms"] / out[ref]["ms"], 3)
    return {"n": n, "launches_per_window": iters, "reps": reps, "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{DIT_S2},{SDXL_UNET}")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["flat", "adafactor"], default=None, help="run one half of the tool")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU; there is no CPU path")
    res = {"sizes": [bench_size(int(n), a.reps, a.warmup) for n in a.sizes.split(",")] if a.only != "adafactor" else [],
           "adafactor": [bench_adafactor(m, a.reps, a.warmup) for m in adafactor_models()] if a.only != "flat" else [],
           "state_bytes_sdxl_unet": {**{name: int(state * SDXL_UNET) for name, (_, state) in KERNELS.items()},
                                     "prodigy": PRODIGY_STATE * SDXL_UNET},
           "weights_bytes_sdxl_unet": 4 * SDXL_UNET}
    for r in res["sizes"]:
        for name, k in r["kernels"].items():
            print(f"n = {r['n']:>13,}  {name:<16} {k['ms']:9.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f})  "
                  f"{k['bytes_per_param']} B/param  {k['GBps']:8.1f} GB/s ({k['GBps_min']:.1f} .. {k['GBps_max']:.1f})")
    for r in res["adafactor"]:
        for name, k in r["kernels"].items():
            print(f"{r['model']:<9} n = {r['n']:>13,}  {name:<16} {k['ms']:9.4f} ms ({k['ms_min']:.4f} .. {k['ms_max']:.4f})  "
                  f"{k['bytes_per_param']} B/param  {k['GBps']:8.1f} GB/s")
        print(f"{r['model']:<9} {r['tensors']} tensors; Adafactor state {r['state_bytes'] / 1e6:.2f} MB, workspace "
              f"{r['workspace_bytes'] / 1e6:.2f} MB; the step takes {r['kernels']['adafactor_step']['ms_vs_adamw']} of AdamW's time")
    for name, b in res["state_bytes_sdxl_unet"].items():
        print(f"SDXL-shape UNet optimizer state under {name:<11}: {b / 1e9:6.2f} GB (weights {4 * SDXL_UNET / 1e9:.2f} GB)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
