"""Time the AutoencoderKL (uwudiff_amd/vae.py) in bf16 on one GPU.

    python tools/bench_vae.py [--calls 20] [--warmup 3] [--json]

Cases: encode of [16, 3, 256, 256] (the batch of configs/demo_training_pixels.yaml), encode of [1, 3, 1024, 1024], decode of
[4, 4, 32, 32].  Per case: call time from device events around each call (median of --calls, after --warmup), images/s,
algorithmic FLOP/s from the shape-derived counts below (and that rate over the dense bf16 MFMA peak), and the time per kernel
family from the library's live profiler (uwu_prof_*), taken in separate calls.  `--counts` prints the FLOP counts alone (no GPU).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak of the MI355X (bench.py)
FAMILIES = [(9, "conv3x3 implicit GEMM (uwu_conv3x3_fwd, uwu_conv3x3_s2br_fwd)"),
            (0, "GEMM (conv_in / conv_out column GEMMs, 1x1 shortcuts, attention Linears, quant convs)"),
            (5, "attention (uwu_attention_d512_fwd)")]


def flops(cfg, H, W, part):
    """(convolutions + Linears, attention) FLOP of one image, 2 per multiply-add, true channel counts; H x W are the PIXEL
    sides for both parts (the decoder starts at H/8 x W/8)."""
    boc, nl, lat = list(cfg["block_out_channels"]), cfg["layers_per_block"], cfg["latent_channels"]
    conv = lambda cin, cout, hw, taps=9: 2.0 * taps * cin * cout * hw  # noqa: E731

    def resnet(cin, cout, hw):
        return conv(cin, cout, hw) + conv(cout, cout, hw) + (conv(cin, cout, hw, 1) if cin != cout else 0.0)

    def mid(c, hw):
        lin = 4 * conv(c, c, hw, 1) if cfg["mid_block_add_attention"] else 0.0
        return 2 * resnet(c, c, hw) + lin, (4.0 * hw * hw * c if cfg["mid_block_add_attention"] else 0.0)

    total, down = 0.0, len(boc) - 1
    if part == "encode":
        h, w = H, W
        total += conv(cfg["in_channels"], boc[0], h * w)
        ch = boc[0]
        for i, c in enumerate(boc):
            for j in range(nl):
                total += resnet(ch if j == 0 else c, c, h * w)
            ch = c
            if i < down:
                h, w = h // 2, w // 2
                total += conv(c, c, h * w)
        m, attn = mid(ch, h * w)
        total += m + conv(ch, 2 * lat, h * w) + conv(2 * lat, 2 * lat, h * w, 1)
        return total, attn
    h, w = H >> down, W >> down
    rev = boc[::-1]
    total += conv(lat, lat, h * w, 1) + conv(lat, rev[0], h * w)
    m, attn = mid(rev[0], h * w)
    total += m
    ch = rev[0]
    for i, c in enumerate(rev):
        for j in range(nl + 1):
            total += resnet(ch if j == 0 else c, c, h * w)
        ch = c
        if i < down:
            h, w = 2 * h, 2 * w
            total += conv(c, c, h * w)
    return total + conv(ch, cfg["out_channels"], h * w), attn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-calls", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--counts", action="store_true")
    args = ap.parse_args()
    from uwudiff_amd.vae import SDXL_VAE_CONFIG

    if args.counts:
        for part in ("encode", "decode"):
            c, a = flops(SDXL_VAE_CONFIG, 256, 256, part)
            print(f"{part} of one 3x256x256 image: convolutions + Linears {c / 1e9:.1f} GFLOP, attention {a / 1e9:.1f} GFLOP")
        return
    import torch

    from uwudiff_amd import lib as L
    from uwudiff_amd.vae import AutoencoderKL

    if args.calls < 20:
        raise SystemExit("--calls must be at least 20")
    lib = L.load()
    torch.manual_seed(0)
    vae = AutoencoderKL.from_pretrained("sdxl-vae", device="cuda")
    cases = [("encode", (16, 3, 256, 256)), ("encode", (1, 3, 1024, 1024)), ("decode", (4, 4, 32, 32))]
    rows = []
    for part, shape in cases:
        x = torch.randn(shape, device="cuda")
        H, W = (shape[2], shape[3]) if part == "encode" else (8 * shape[2], 8 * shape[3])
        run = (lambda: vae.encode(x).latent_dist.sample()) if part == "encode" else (lambda: vae.decode(x).sample)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        c, a = flops(SDXL_VAE_CONFIG, H, W, part)
        total = (c + a) * shape[0]
        row = dict(case=f"{part} {list(shape)}", call_ms=ms, call_ms_min=min(times), images_per_s=shape[0] / ms * 1e3,
                   gflop_per_call=total / 1e9, tflops=total / ms / 1e9, mfma_peak_fraction=total / ms / 1e9 / PEAK_BF16_TFLOPS,
                   families=[])
        L.check(lib.uwu_prof_enable(1), "prof_enable")
        for _ in range(args.prof_calls):
            run()
        torch.cuda.synchronize()
        L.check(lib.uwu_prof_enable(0), "prof_disable")
        seen = 0.0
        for tag, name in FAMILIES:
            t, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
            L.check(lib.uwu_prof_collect(tag, -1, ctypes.byref(t), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)), "prof_collect")
            if n.value:
                per = t.value / args.prof_calls
                seen += per
                row["families"].append(dict(kernel=name, ms_per_call=per, launches_per_call=n.value // args.prof_calls,
                                            tflops=fl.value / (t.value * 1e-3) / 1e12))
        row["families"].append(dict(kernel="everything else (GroupNorm + SiLU, add, upsample, layout, column gather, draw; not "
                                           "instrumented: call time minus the rows above)", ms_per_call=max(ms - seen, 0.0)))
        rows.append(row)
    if args.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['case']}: {r['call_ms']:.2f} ms per call (min {r['call_ms_min']:.2f}), {r['images_per_s']:.1f} images/s, "
              f"{r['gflop_per_call']:.1f} GFLOP per call -> {r['tflops']:.1f} TFLOP/s algorithmic = "
              f"{100 * r['mfma_peak_fraction']:.1f} % of the {PEAK_BF16_TFLOPS:.0f} TFLOP/s bf16 MFMA peak")
        for f in r["families"]:
            extra = f", {f['launches_per_call']} launches, {f['tflops']:.1f} TFLOP/s" if "tflops" in f else ""
            print(f"    {f['ms_per_call']:8.3f} ms  {f['kernel']}{extra}")


if __name__ == "__main__":
    main()
