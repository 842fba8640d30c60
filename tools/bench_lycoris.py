"""LyCORIS adapter training vs full fine-tuning of the SDXL UNet at BASELINE config 4's shape (4x128x128 latents, batch 12,
bf16, fused AdamW): ms/step and peak memory of each mode, and the two adapter kernels alone (merge of every adapted
tensor, adapter gradient of every adapted Linear) with the bytes they move.  One JSON line.  DESIGN.md section 4.21.
With a weight-decomposed config (--lycoris configs/lycoris/sdxl-diffusers-dora.toml, section 4.39) the merge figure covers
its three launches and the summed time of uwu_adapter_dora_grad is reported on its own.  With a convolution preset
(--lycoris configs/lycoris/sdxl-diffusers-conv.toml, section 4.41) the convolution merge (uwu_adapter_conv_merge alone) and the
adapter gradients of the adapted convolutions (uwu_adapter_conv_grad from an fp32 dW of each stored shape) are reported too.

    python tools/bench_lycoris.py [--batch 12] [--steps 5] [--warmup 2] [--mode both|full|lycoris] [--lycoris PATH]

Each mode runs in a child process of its own (peak memory of one mode is not polluted by the other)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")


def run_mode(mode, B, steps, warmup, toml=TOML):
    import torch

    from duwu.loss import DiffusionLoss
    from uwudiff_amd.optim import FusedAdamW
    from uwudiff_amd.scheduler import EulerDiscreteScheduler
    from uwudiff_amd.unet import UNet2DConditionModel

    dev = torch.device("cuda", 0)
    torch.manual_seed(1215)
    model = UNet2DConditionModel.from_config("sdxl", compute_dtype="bf16", device=dev)
    net = None
    if mode == "lycoris":
        from uwudiff_amd.adapters import LycorisNetwork

        model.requires_grad_(False)
        net = LycorisNetwork(model, toml).to(dev)
        with torch.no_grad():  # non-zero adapters (a zero LoKr w2 computes the same, but the timing should not rely on it)
            keep = {s.name: net.view(s.name, "dora_scale").clone() for s in net.specs if s.dora}
            net.flat.data.normal_(0, 1e-3)
            for name, m in keep.items():  # (the magnitudes keep their start: the norms of the base weights)
                net.view(name, "dora_scale").copy_(m)
        net.apply_to(model)
        params = list(net.parameters())
    else:
        params = list(model.parameters())
    loss_fn = DiffusionLoss(EulerDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0",
                                                                   subfolder="scheduler"))
    opt = FusedAdamW(params, lr=1e-6, weight_decay=0.01)
    pool = torch.randn(2 * B, 4, 128, 128).to(dev)
    pooled = torch.randn(2 * B, 1280).to(dev)
    ctx = torch.randn(B, 77, 2048).to(dev)
    time_ids = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B).to(dev)
    one = torch.ones((), dtype=torch.float32).to(dev)

    def step(i):
        off = (i * B) % (B + 1)
        loss, _ = loss_fn(pool[off:off + B], model, encoder_hidden_states=ctx,
                          added_cond_kwargs={"text_embeds": pooled[off:off + B], "time_ids": time_ids})
        loss.backward(one)
        opt.step(zero_grad=True)
        if net is not None:
            net.mark_dirty()
        return loss

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = step(warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"ms_per_step": round(ms, 1), "images_per_s": round(B / ms * 1e3, 2),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2), "loss": float(loss)}
    if net is None:
        out["trainable_params"] = model.flat.numel()
        return out
    out["trainable_params"] = net.num_adapter_params()
    ad = model.P.ad
    n_el = sum(int(torch.tensor(model.P.registry[n][1]).prod()) for n in ad.names)
    # merge: one launch over every adapted tensor (reads the fp32 base, writes the bf16 shadow (+ fp32 for the norms))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 5
    ad.merge(model.P)
    ev[0].record()
    for _ in range(reps):
        ad.merge(model.P)
    ev[1].record()
    torch.cuda.synchronize()
    t_merge = ev[0].elapsed_time(ev[1]) / reps
    n_eff = sum(int(torch.tensor(model.P.registry[n][1]).prod()) for n in ad.eff_off)
    merge_bytes = n_el * (4 + 2) + n_eff * 4 + net.n * 4
    n_dora = sum(int(torch.tensor(model.P.registry[n][1]).prod()) for n in ad.dora)
    merge_bytes += n_dora * 4  # the norm pass reads the decomposed base elements once more
    # adapter gradients of every adapted Linear from an fp32 dW of its shape (reads dW once + the factors + small partials)
    grads_names = [n for n in ad.names if ad.seg[n][1] != 0 and n not in ad.convs]
    dws = {}
    for n in grads_names:
        shape = tuple(model.P.registry[n][1])
        if shape not in dws:
            dws[shape] = torch.randn(shape, device=dev)
    if net.flat.grad is None:
        net.flat.grad = torch.zeros_like(net.flat.data)
    t_grad = 0.0
    if grads_names:
        ad.grad_rows(model.P, grads_names[:1], dws[tuple(model.P.registry[grads_names[0]][1])])
        ev[0].record()
        for n in grads_names:
            ad.grad_rows(model.P, [n], dws[tuple(model.P.registry[n][1])])
        ev[1].record()
        torch.cuda.synchronize()
        t_grad = ev[0].elapsed_time(ev[1])
    grad_bytes = sum(int(torch.tensor(model.P.registry[n][1]).prod()) * 4 for n in grads_names)
    if ad.dora:  # the stage in front of uwu_adapter_grad alone: G read twice, base read once, G written once
        ev[0].record()
        for n in ad.dora:
            ad.dora_grad(model.P, n, dws[tuple(model.P.registry[n][1])])
        ev[1].record()
        torch.cuda.synchronize()
        t_dora = ev[0].elapsed_time(ev[1])
        out.update({"decomposed_elements": n_dora, "dora_grad_ms_per_step": round(t_dora, 3),
                    "dora_grad_bytes": n_dora * 16, "dora_grad_GBps": round(n_dora * 16 / t_dora / 1e6, 1)})
    if ad.convs:  # section 4.41: the convolution merge (T of the Tucker segments + merge) and the convolution adapter
        # gradients alone, from an fp32 dW of each stored shape (read once)
        n_conv = sum(int(torch.tensor(model.P.registry[n][1]).prod()) for n in ad.convs)
        shadow = model.P.shadow
        ad._launch_merge(model.P, None, None, ad.eff, shadow, ad.ctab)
        ev[0].record()
        for _ in range(reps):
            ad._launch_merge(model.P, None, None, ad.eff, shadow, ad.ctab)
        ev[1].record()
        torch.cuda.synchronize()
        t_cm = ev[0].elapsed_time(ev[1]) / reps
        for n in ad.convs:
            shape = tuple(model.P.registry[n][1])
            if shape not in dws:
                dws[shape] = torch.randn(shape, device=dev)
        ad.conv_grad_rows(model.P, ad.convs[0], dws[tuple(model.P.registry[ad.convs[0]][1])])
        ev[0].record()
        for n in ad.convs:
            ad.conv_grad_rows(model.P, n, dws[tuple(model.P.registry[n][1])])
        ev[1].record()
        torch.cuda.synchronize()
        t_cg = ev[0].elapsed_time(ev[1])
        out.update({"adapted_convs": len(ad.convs), "conv_elements": n_conv, "conv_merge_ms": round(t_cm, 3),
                    "conv_merge_GBps": round(n_conv * 6 / t_cm / 1e6, 1), "conv_adapter_grad_ms_per_step": round(t_cg, 3),
                    "conv_adapter_grad_dW_bytes": n_conv * 4, "conv_adapter_grad_GBps": round(n_conv * 4 / t_cg / 1e6, 1)})
    out.update({"adapted_elements": n_el, "merge_ms": round(t_merge, 3), "merge_bytes": merge_bytes,
                "merge_GBps": round(merge_bytes / t_merge / 1e6, 1), "adapter_grad_ms_per_step": round(t_grad, 3),
                "adapted_linears": len(grads_names), "adapter_grad_dW_bytes": grad_bytes,
                "adapter_grad_GBps": round(grad_bytes / t_grad / 1e6, 1) if t_grad else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="both", choices=["both", "full", "lycoris"])
    ap.add_argument("--lycoris", default=TOML, help="LyCORIS TOML of the adapter mode (default: the shipped preset)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run_mode(a.mode, a.batch, a.steps, a.warmup, a.lycoris)), flush=True)
        return
    res = {}
    for mode in (["full", "lycoris"] if a.mode == "both" else [a.mode]):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--mode", mode, "--batch", str(a.batch),
                            "--steps", str(a.steps), "--warmup", str(a.warmup), "--lycoris", os.path.abspath(a.lycoris)],
                           capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            res[mode] = {"error": f"exit {r.returncode}", "tail": (r.stdout + r.stderr)[-1500:]}
            break  # (nothing more on the device after a failed run)
        res[mode] = json.loads(line[0][len("RESULT "):])
    print(json.dumps({"tool": "bench_lycoris", "shape": f"SDXL UNet bf16, 4x128x128, batch {a.batch}",
                      "lycoris": os.path.relpath(os.path.abspath(a.lycoris), ROOT), **res}))


if __name__ == "__main__":
    main()
