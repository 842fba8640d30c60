"""Time the two SDXL text encoders (uwudiff_amd/text_model.py) in bf16 on one GPU.

    python tools/bench_text.py [--calls 20] [--warmup 3] [--json]

Cases: CLIP-L (`text_encoder`) and OpenCLIP-bigG (`text_encoder_2`) at the built-in configurations, T = 77, batches of 12 and 48
captions with right-padded attention masks.  Per case: call time from device events around each forward (median of --calls, after
--warmup), captions/s, algorithmic FLOP/s from the shape-derived counts below (and that rate over the dense bf16 MFMA peak), and
the time per kernel family from the library's live profiler (uwu_prof_*), taken in separate calls.  `--counts` prints the FLOP
and weight-byte counts alone (no GPU).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak of the MI355X (bench.py)
T = 77
FAMILIES = [(0, "GEMM (packed q/k/v, out_proj, fc1, fc2; uwu_gemm with the bias epilogue)"),
            (5, "causal attention (uwu_attention_causal_fwd)"),
            (7, "LayerNorm + residual (uwu_add_ln_modulate_fwd, affine)"),
            (10, "bias-free activation (uwu_bias_act_fwd)")]


def counts(cfg):
    """(GEMM FLOP, causal-attention FLOP) of one caption of T tokens, 2 per multiply-add; (layer weights, embedding tables) in
    parameters.  The attention count is the causal half that is computed: 4 d T (T + 1) / 2 per head."""
    D, F, Lyr, H = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"]
    gemm = Lyr * T * 2.0 * (4 * D * D + 2 * D * F)
    attn = Lyr * H * 2.0 * (D // H) * T * (T + 1)
    weights = Lyr * (4 * (D * D + D) + 2 * D * F + F + D + 4 * D) + 2 * D
    tables = (cfg["vocab_size"] + cfg["max_position_embeddings"]) * D
    return gemm, attn, weights, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-calls", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--counts", action="store_true")
    args = ap.parse_args()
    from uwudiff_amd.text_model import SDXL_TEXT_CONFIGS

    if args.counts:
        for name, cfg in SDXL_TEXT_CONFIGS.items():
            g, a, w, t = counts(cfg)
            print(f"{name}: GEMMs {g / 1e9:.2f} GFLOP + causal attention {a / 1e9:.2f} GFLOP per caption of {T} tokens; "
                  f"{w / 1e6:.1f} M layer parameters ({2 * w / 1e6:.0f} MB in bf16) + {t / 1e6:.1f} M in the embedding tables")
        return
    import torch

    from uwudiff_amd import lib as L
    from uwudiff_amd.text_model import CLIPTextModel

    if args.calls < 20:
        raise SystemExit("--calls must be at least 20")
    lib = L.load()
    rows = []
    for name, cfg in SDXL_TEXT_CONFIGS.items():
        model = CLIPTextModel.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder=name).cuda()
        for B in (12, 48):
            g = torch.Generator().manual_seed(B)
            ids = torch.randint(300, 49000, (B, T), generator=g)
            mask = torch.zeros(B, T, dtype=torch.long)
            for b in range(B):  # caption lengths 8 .. 77
                n = 8 + (b * 23) % 70
                ids[b, 0], ids[b, n - 1:] = 49406, 49407
                mask[b, :n] = 1
            ids, mask = ids.cuda(), mask.cuda()
            run = lambda: model(ids, attention_mask=mask, output_hidden_states=True)  # noqa: E731
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
            gf, af, _, _ = counts(cfg)
            total = (gf + af) * B
            row = dict(case=f"{name} B={B}", call_ms=ms, call_ms_min=min(times), captions_per_s=B / ms * 1e3, gflop_per_call=total / 1e9,
                       tflops=total / ms / 1e9, mfma_peak_fraction=total / ms / 1e9 / PEAK_BF16_TFLOPS, families=[])
            L.check(lib.uwu_prof_enable(1), "prof_enable")
            for _ in range(args.prof_calls):
                run()
            torch.cuda.synchronize()
            L.check(lib.uwu_prof_enable(0), "prof_disable")
            seen = 0.0
            for tag, fam in FAMILIES:
                t, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
                L.check(lib.uwu_prof_collect(tag, -1, ctypes.byref(t), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)), "prof_collect")
                if n.value:
                    per = t.value / args.prof_calls
                    seen += per
                    row["families"].append(dict(kernel=fam, ms_per_call=per, launches_per_call=n.value // args.prof_calls,
                                                tflops=fl.value / (t.value * 1e-3) / 1e12, gbytes_per_s=by.value / (t.value * 1e-3) / 1e9))
            row["families"].append(dict(kernel="everything else (embedding, pooling, launch gaps; not instrumented: call time minus the "
                                               "rows above)", ms_per_call=max(ms - seen, 0.0)))
            rows.append(row)
        del model
        torch.cuda.empty_cache()
    if args.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['case']}: {r['call_ms']:.2f} ms per batch (min {r['call_ms_min']:.2f}), {r['captions_per_s']:.0f} captions/s, "
              f"{r['gflop_per_call']:.1f} GFLOP per batch -> {r['tflops']:.1f} TFLOP/s algorithmic = "
              f"{100 * r['mfma_peak_fraction']:.1f} % of the {PEAK_BF16_TFLOPS:.0f} TFLOP/s bf16 MFMA peak")
        for f in r["families"]:
            extra = (f", {f['launches_per_call']} launches, {f['tflops']:.1f} TFLOP/s, {f['gbytes_per_s']:.0f} GB/s" if "tflops" in f else "")
            print(f"    {f['ms_per_call']:8.3f} ms  {f['kernel']}{extra}")


if __name__ == "__main__":
    main()
