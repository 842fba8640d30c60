"""Time the CLIP score (uwudiff_amd/metrics.py) in bf16 on one GPU.

    python tools/bench_metrics.py [--calls 20] [--warmup 3] [--json]
    python tools/bench_metrics.py --attention bidir      # uwu_attention_bidir_fwd alone at the ViT-L/14 shape
    python tools/bench_metrics.py --attention generic    # uwu_attention_fwd at the same shape: the path that existed before

Case: the openai/clip-vit-large-patch14 pair (image tower 1024 / 16 heads / 24 layers, 257 tokens; text tower 768 / 12 / 12, 77
tokens) at batches of 64 and 256 (image, caption) pairs.  One call = what ``CLIPScore.update`` does on the device: the text tower,
the image tower on [0, 255] images (preprocessing fused into the patch kernel) and ``uwu_clip_score_accum``.  Per case: call time
from device events around each call (median of --calls, after --warmup), images/s, algorithmic FLOP/s from the shape-derived
counts below (and that rate over the dense bf16 MFMA peak), and the time per kernel family from the library's live profiler
(uwu_prof_*), taken in separate calls.  The weights are drawn on the device (N(0, 0.02), norms 1: the time of a call does not
depend on their values).  `--counts` prints the FLOP counts alone (no GPU).

`--attention`: ONE of the two kernels per process, at B = 64, H = 16, T = 257, d = 64, packed bf16 q / k / v, device events, median
of --calls after --warmup.  Run the two in separate processes and compare the medians.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_text import PEAK_BF16_TFLOPS, family_rows, time_calls  # noqa: E402

NAME = "openai/clip-vit-large-patch14"
T_TEXT = 77
FAMILIES = [(0, "GEMM (patch embedding, packed q/k/v, out_proj, fc1, fc2, the two projections; uwu_gemm)"),
            (5, "attention (uwu_attention_bidir_fwd, image tower; uwu_attention_causal_fwd, text tower)"),
            (7, "LayerNorm + residual (uwu_add_ln_modulate_fwd, affine)"),
            (10, "patches, embedding, activation, score (uwu_clip_patches, uwu_vit_embed, uwu_bias_act_fwd, uwu_clip_score_accum)")]


def counts(vcfg, tcfg):
    """(image tower GEMM FLOP, image tower attention FLOP, text tower GEMM FLOP, text tower attention FLOP) of one pair, 2 per
    multiply-add; the text tower's attention is the causal half that is computed"""
    D, F, Ly, H, p = vcfg["hidden_size"], vcfg["intermediate_size"], vcfg["num_hidden_layers"], vcfg["num_attention_heads"], vcfg["patch_size"]
    Np = (vcfg["image_size"] // p) ** 2
    Tv = Np + 1
    vg = 2.0 * Np * 3 * p * p * D + Ly * Tv * 2.0 * (4 * D * D + 2 * D * F) + 2.0 * D * vcfg["projection_dim"]
    va = Ly * H * 4.0 * 64 * Tv * Tv
    D, F, Ly, H = tcfg["hidden_size"], tcfg["intermediate_size"], tcfg["num_hidden_layers"], tcfg["num_attention_heads"]
    tg = Ly * T_TEXT * 2.0 * (4 * D * D + 2 * D * F) + 2.0 * D * tcfg["projection_dim"]
    ta = Ly * H * 2.0 * 64 * T_TEXT * (T_TEXT + 1)
    return vg, va, tg, ta


def _on_device(cls, cfg, seed):
    import torch

    model = cls(cfg, init_weights=False, device="cuda")
    model.flat.normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(seed))
    for k, v in model.named_tensors():
        if "norm" in k and k.endswith(".weight"):
            v.fill_(1.0)
    model.refresh_shadow()
    return model


def bench_attention(args):
    import torch

    from uwudiff_amd import ops

    B, H, d, Tn = 64, 16, 64, 257
    qkv = torch.randn(B * Tn, 3 * H * d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)).bfloat16()
    q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:]
    if args.attention == "bidir":
        run = lambda: ops.attention_bidir_fwd(q, k, v, B, Tn, H, d, d ** -0.5)  # noqa: E731
    else:
        run = lambda: ops.attention_fwd(q, k, v, B, Tn, Tn, H, d, d ** -0.5)  # noqa: E731
    times = time_calls(run, args.warmup, args.calls)
    flop = 4.0 * B * H * d * Tn * Tn
    ms = statistics.median(times)
    return dict(kernel="uwu_attention_bidir_fwd" if args.attention == "bidir" else "uwu_attention_fwd", B=B, H=H, T=Tn, d=d, ms=ms,
                ms_min=min(times), tflops=flop / ms / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attention", choices=("bidir", "generic"))
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-calls", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--counts", action="store_true")
    args = ap.parse_args()
    from uwudiff_amd.vision_model import CLIP_CONFIGS

    vcfg, tcfg = CLIP_CONFIGS[NAME]
    vg, va, tg, ta = counts(vcfg, tcfg)
    if args.counts:
        print(f"{NAME}: image tower GEMMs {vg / 1e9:.2f} GFLOP + attention {va / 1e9:.2f} GFLOP per image of 257 tokens; text tower GEMMs "
              f"{tg / 1e9:.2f} GFLOP + causal attention {ta / 1e9:.2f} GFLOP per caption of {T_TEXT} tokens")
        return
    if args.calls < 20:
        raise SystemExit("--calls must be at least 20")
    if args.attention:
        r = bench_attention(args)
        print(json.dumps(r) if args.json else f"B = {r['B']}, H = {r['H']}, T = {r['T']}: {r['kernel']} {r['ms']:.3f} ms (min {r['ms_min']:.3f}), "
              f"{r['tflops']:.1f} TFLOP/s")
        return
    import torch

    from uwudiff_amd import ops
    from uwudiff_amd.text_model import CLIPTextModelWithProjection
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection

    text, vision = _on_device(CLIPTextModelWithProjection, tcfg, 1), _on_device(CLIPVisionModelWithProjection, vcfg, 2)
    S = vcfg["image_size"]
    rows = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        images = torch.randint(0, 256, (B, 3, S, S), generator=g).float().cuda()
        ids = torch.randint(300, 49000, (B, T_TEXT), generator=g)
        mask = torch.zeros(B, T_TEXT, dtype=torch.long)
        for b in range(B):  # caption lengths 8 .. 77
            n = 8 + (b * 23) % 70
            ids[b, 0], ids[b, n - 1:] = 49406, 49407
            mask[b, :n] = 1
        ids, mask = ids.cuda(), mask.cuda()
        acc = torch.zeros(2, dtype=torch.float64, device="cuda")
        run = lambda: ops.clip_score_accum(vision.embed_images(images), text(ids, attention_mask=mask)[0], acc)  # noqa: E731
        times = time_calls(run, args.warmup, args.calls)
        ms = statistics.median(times)
        total = (vg + va + tg + ta) * B
        row = dict(case=f"{NAME} B={B}", call_ms=ms, call_ms_min=min(times), images_per_s=B / ms * 1e3, gflop_per_call=total / 1e9,
                   tflops=total / ms / 1e9, mfma_peak_fraction=total / ms / 1e9 / PEAK_BF16_TFLOPS)
        row["families"] = family_rows(run, args.prof_calls, FAMILIES, ms, "everything else (text embedding and pooling, the class-token "
                                      "gather, launch gaps; not instrumented: call time minus the rows above)")
        rows.append(row)
    if args.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['case']}: {r['call_ms']:.2f} ms per batch (min {r['call_ms_min']:.2f}), {r['images_per_s']:.0f} images/s, "
              f"{r['gflop_per_call']:.1f} GFLOP per batch -> {r['tflops']:.1f} TFLOP/s algorithmic = "
              f"{100 * r['mfma_peak_fraction']:.1f} % of the {PEAK_BF16_TFLOPS:.0f} TFLOP/s bf16 MFMA peak")
        for f in r["families"]:
            extra = (f", {f['launches_per_call']} launches, {f['tflops']:.1f} TFLOP/s, {f['gbytes_per_s']:.0f} GB/s" if "tflops" in f else "")
            print(f"    {f['ms_per_call']:8.3f} ms  {f['kernel']}{extra}")


if __name__ == "__main__":
    main()
