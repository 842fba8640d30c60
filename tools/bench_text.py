"""Time the text encoders (uwudiff_amd/text_model.py, DESIGN.md sections 4.23 and 4.25) in bf16 on one GPU.

    python tools/bench_text.py [--model clip|t5] [--calls 20] [--warmup 3] [--json]
    python tools/bench_text.py --attention      # uwu_attention_relbias_fwd against uwu_attention_bias_fwd

Cases: CLIP-L (`text_encoder`) and OpenCLIP-bigG (`text_encoder_2`) at the built-in configurations, T = 77, batches of 12 and 48
captions with right-padded attention masks.  Per case: call time from device events around each forward (median of --calls, after
--warmup), captions/s, algorithmic FLOP/s from the shape-derived counts below (and that rate over the dense bf16 MFMA peak), and
the time per kernel family from the library's live profiler (uwu_prof_*), taken in separate calls.  `--counts` prints the FLOP
and weight-byte counts alone (no GPU).

`--model t5`: google/t5-v1_1-xxl at B in {12, 48} and T in {77, 256}, the same method and columns.  The 4.76 G weights are drawn on
the device (N(0, 0.02), norms 1: the time of a call does not depend on their values; from_pretrained's own draw goes tensor by
tensor through the host and takes minutes).  `--attention`: both attention kernels at B H = 768, T in {77, 256, 512}, a zero
relative bias against a zero key bias, device events, median of 20 after 3.
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


T5_FAMILIES = [(0, "GEMM (packed q/k/v, o, wi_0 | wi_1, wo; uwu_gemm)"),
               (5, "attention with relative bias (uwu_attention_relbias_fwd)"),
               (7, "RMS norm + residual (uwu_add_rmsnorm_fwd)"),
               (10, "gate and embedding (uwu_gated_act_fwd, uwu_token_embed)")]


def t5_counts(cfg, Tn):
    """(GEMM FLOP, attention FLOP) of one caption of Tn tokens, 2 per multiply-add; (layer weights, embedding table) in parameters"""
    D, F, Lyr, H = cfg["d_model"], cfg["d_ff"], cfg["num_layers"], cfg["num_heads"]
    HD = 64 * H
    gemm = Lyr * Tn * 2.0 * (4 * D * HD + 3 * D * F)
    attn = Lyr * H * 4.0 * 64 * Tn * Tn
    weights = Lyr * (4 * D * HD + 3 * D * F + 2 * D) + D + cfg["relative_attention_num_buckets"] * H
    return gemm, attn, weights, cfg["vocab_size"] * D


def time_calls(run, warmup, calls):
    import torch

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def family_rows(run, prof_calls, families, ms, rest):
    import torch

    from uwudiff_amd import lib as L

    lib = L.load()
    L.check(lib.uwu_prof_enable(1), "prof_enable")
    for _ in range(prof_calls):
        run()
    torch.cuda.synchronize()
    L.check(lib.uwu_prof_enable(0), "prof_disable")
    seen, out = 0.0, []
    for tag, fam in families:
        t, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        L.check(lib.uwu_prof_collect(tag, -1, ctypes.byref(t), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)), "prof_collect")
        if n.value:
            per = t.value / prof_calls
            seen += per
            out.append(dict(kernel=fam, ms_per_call=per, launches_per_call=n.value // prof_calls,
                            tflops=fl.value / (t.value * 1e-3) / 1e12, gbytes_per_s=by.value / (t.value * 1e-3) / 1e9))
    out.append(dict(kernel=rest, ms_per_call=max(ms - seen, 0.0)))
    return out


def bench_t5(args):
    import torch

    from uwudiff_amd.text_model import T5_CONFIGS, T5EncoderModel

    name = "google/t5-v1_1-xxl"
    cfg = T5_CONFIGS[name]
    model = T5EncoderModel(cfg, init_weights=False, device="cuda")
    model.flat.normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(0))
    for k, v in model.named_tensors():
        if "layer_norm" in k:
            v.fill_(1.0)
    model.refresh_shadow()
    rows = []
    for Tn in (77, 256):
        for B in (12, 48):
            g = torch.Generator().manual_seed(B)
            ids = torch.randint(3, 32100, (B, Tn), generator=g)
            mask = torch.zeros(B, Tn, dtype=torch.long)
            for b in range(B):  # caption lengths 8 .. Tn, right-padded
                n = 8 + (b * 23) % (Tn - 7)
                ids[b, n - 1], ids[b, n:] = 1, 0
                mask[b, :n] = 1
            ids, mask = ids.cuda(), mask.cuda()
            run = lambda: model(ids, attention_mask=mask, output_hidden_states=True)  # noqa: E731
            times = time_calls(run, args.warmup, args.calls)
            ms = statistics.median(times)
            gf, af, _, _ = t5_counts(cfg, Tn)
            total = (gf + af) * B
            row = dict(case=f"t5-v1_1-xxl B={B} T={Tn}", call_ms=ms, call_ms_min=min(times), captions_per_s=B / ms * 1e3, gflop_per_call=total / 1e9,
                       tflops=total / ms / 1e9, mfma_peak_fraction=total / ms / 1e9 / PEAK_BF16_TFLOPS)
            row["families"] = family_rows(run, args.prof_calls, T5_FAMILIES, ms, "everything else (bias gather on the first call, launch gaps: "
                                          "call time minus the rows above)")
            rows.append(row)
    return rows


def bench_attention(args):
    """uwu_attention_relbias_fwd (zero relative bias) against uwu_attention_bias_fwd (zero key bias): the kernel that exists and could
    have been stretched instead.  B = 12, H = 64 (B H = 768), packed bf16 q / k / v, device events, median of --calls after --warmup (20 after 3)."""
    import torch

    from uwudiff_amd import ops

    B, H, d = 12, 64, 64
    rows = []
    for Tn in (77, 256, 512):
        qkv = torch.randn(B * Tn, 3 * H * d, device="cuda").bfloat16()
        q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:]
        rel = torch.zeros(H, 2 * Tn - 1, device="cuda")
        kb = torch.zeros(B, Tn, device="cuda")
        new = statistics.median(time_calls(lambda: ops.attention_relbias_fwd(q, k, v, rel, B, Tn, H, d, d ** -0.5), args.warmup, args.calls))
        old = statistics.median(time_calls(lambda: ops.attention_fwd(q, k, v, B, Tn, Tn, H, d, key_bias=kb), args.warmup, args.calls))
        a, b = ops.attention_relbias_fwd(q, k, v, rel, B, Tn, H, d, d ** -0.5), ops.attention_fwd(q, k, v, B, Tn, Tn, H, d, key_bias=kb)[0]
        flop = 4.0 * B * H * d * Tn * Tn
        rows.append(dict(T=Tn, relbias_ms=new, bias_fwd_ms=old, relbias_tflops=flop / new / 1e9, bias_fwd_tflops=flop / old / 1e9,
                         max_abs_diff=float((a.float() - b.float()).abs().max())))
    return rows


def print_rows(rows):
    for r in rows:
        print(f"{r['case']}: {r['call_ms']:.2f} ms per batch (min {r['call_ms_min']:.2f}), {r['captions_per_s']:.0f} captions/s, "
              f"{r['gflop_per_call']:.1f} GFLOP per batch -> {r['tflops']:.1f} TFLOP/s algorithmic = "
              f"{100 * r['mfma_peak_fraction']:.1f} % of the {PEAK_BF16_TFLOPS:.0f} TFLOP/s bf16 MFMA peak")
        for f in r["families"]:
            extra = (f", {f['launches_per_call']} launches, {f['tflops']:.1f} TFLOP/s, {f['gbytes_per_s']:.0f} GB/s" if "tflops" in f else "")
            print(f"    {f['ms_per_call']:8.3f} ms  {f['kernel']}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("clip", "t5"), default="clip")
    ap.add_argument("--attention", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-calls", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--counts", action="store_true")
    args = ap.parse_args()
    from uwudiff_amd.text_model import SDXL_TEXT_CONFIGS

    if args.counts and args.model == "t5":
        from uwudiff_amd.text_model import T5_CONFIGS

        for name, cfg in T5_CONFIGS.items():
            for Tn in (77, 256):
                g, a, w, t = t5_counts(cfg, Tn)
                print(f"{name}: GEMMs {g / 1e9:.2f} GFLOP + attention {a / 1e9:.2f} GFLOP per caption of {Tn} tokens; "
                      f"{w / 1e6:.1f} M layer parameters ({2 * w / 1e6:.0f} MB in bf16, {4 * w / 1e6:.0f} MB fp32 master) + {t / 1e6:.1f} M in "
                      f"the embedding table")
        return
    if args.attention:
        rows = bench_attention(args)
        if args.json:
            print(json.dumps(rows))
            return
        for r in rows:
            print(f"B H = 768, T = {r['T']}: uwu_attention_relbias_fwd {r['relbias_ms']:.3f} ms ({r['relbias_tflops']:.1f} TFLOP/s), "
                  f"uwu_attention_bias_fwd {r['bias_fwd_ms']:.3f} ms ({r['bias_fwd_tflops']:.1f} TFLOP/s); max |difference| {r['max_abs_diff']:.2e}")
        return
    if args.model == "t5":
        if args.calls < 20:
            raise SystemExit("--calls must be at least 20")
        rows = bench_t5(args)
        print(json.dumps(rows)) if args.json else print_rows(rows)
        return
    if args.counts:
        for name, cfg in SDXL_TEXT_CONFIGS.items():
            g, a, w, t = counts(cfg)
            print(f"{name}: GEMMs {g / 1e9:.2f} GFLOP + causal attention {a / 1e9:.2f} GFLOP per caption of {T} tokens; "
                  f"{w / 1e6:.1f} M layer parameters ({2 * w / 1e6:.0f} MB in bf16) + {t / 1e6:.1f} M in the embedding tables")
        return
    import torch

    from uwudiff_amd.text_model import CLIPTextModel

    if args.calls < 20:
        raise SystemExit("--calls must be at least 20")
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
            times = time_calls(run, args.warmup, args.calls)
            ms = statistics.median(times)
            gf, af, _, _ = counts(cfg)
            total = (gf + af) * B
            row = dict(case=f"{name} B={B}", call_ms=ms, call_ms_min=min(times), captions_per_s=B / ms * 1e3, gflop_per_call=total / 1e9,
                       tflops=total / ms / 1e9, mfma_peak_fraction=total / ms / 1e9 / PEAK_BF16_TFLOPS)
            row["families"] = family_rows(run, args.prof_calls, FAMILIES, ms, "everything else (embedding, pooling, launch gaps; not "
                                          "instrumented: call time minus the rows above)")
            rows.append(row)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(rows)) if args.json else print_rows(rows)


if __name__ == "__main__":
    main()
