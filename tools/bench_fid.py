"""Time the FID extractor and a whole ``FrechetInceptionDistance.update`` (uwudiff_amd/inception.py, uwudiff_amd/metrics.py; DESIGN.md
section 4.37) in bf16 on one GPU, and every convolution family against a yardstick that is not the code under test.

    python tools/bench_fid.py [--batches 64 256] [--calls 10] [--warmup 2] [--out profiles/fid_mi355x.txt]
    python tools/bench_fid.py --counts         # the FLOP counts alone, no GPU

1. Extractor and update.  Pictures/s at each batch from device events around each call (median of --calls after --warmup), and the
   algorithmic FLOP/s from the shape-derived count below (11.42 GFLOP per picture): a whole-program rate, pools, operand kernels and
   launch gaps included, not a kernel's share of peak.  Time per family from one extra pass with a device-event pair around every
   operator call (taken apart from the timed calls: the events cost host time).
2. Per convolution family, at the net's own shape with B = 64: ``uwu_conv2d_fwd`` against, for the 3x3 / stride 1 / padding 1
   layers, ``uwu_conv3x3_fwd`` (the implicit kernel the UNet runs) on the same shape with ReLU off, run twice to show the spread of
   a repeat; for 1x1, whose column matrix is the activation itself, also the explicit route as the extractor runs it (``uwu_gemm`` +
   ``uwu_relu_rows``) against the kernel with ReLU on; for every other family ``uwu_gemm`` on a column matrix of the same M, N, K that is already gathered -- the floor of an
   explicit route, the gather excluded -- and, with the gather priced at one write and one read of that matrix at 4 TB/s, what the
   explicit route could not beat.  The two sides alternate in one process.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_text import PEAK_BF16_TFLOPS, time_calls  # noqa: E402


def family(kernel, stride, padding):
    kh, kw = kernel
    if (kh, kw) == (3, 3):
        return "3x3 s2 p0" if stride == 2 else ("3x3 s1 p1" if padding[0] == 1 else "3x3 s1 p0")
    return f"{kh}x{kw}"


def sizes():
    """name -> (H, W) of every convolution's INPUT, from the layer table"""
    from uwudiff_amd.inception import BLOCKS, layer_table

    hw = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 73}
    side = {"A": 35, "B": 35, "C": 17, "D": 17, "E": 8}
    out = {}
    for name, cin, cout, k, s, p in layer_table():
        out[name] = hw[name] if name in hw else side[BLOCKS[name.split(".")[0]][0]]
    return out


def counts():
    """(FLOP per picture, {family: (layers, FLOP)}): 2 per multiply-add, from the layer table"""
    from uwudiff_amd.inception import layer_table
    from uwudiff_amd.ops import conv2d_out_hw

    hw, fam, total = sizes(), {}, 0.0
    for name, cin, cout, k, s, p in layer_table():
        Ho, Wo = conv2d_out_hw(hw[name], hw[name], k, s, p)
        fl = 2.0 * Ho * Wo * cout * k[0] * k[1] * cin
        key = family(k, s, p)
        n, f = fam.get(key, (0, 0.0))
        fam[key] = (n + 1, f + fl)
        total += fl
    return total, fam


def print_counts(log):
    total, fam = counts()
    log(f"InceptionV3 (FID variant, 2048-d): {total / 1e9:.2f} GFLOP per picture in {sum(n for n, _ in fam.values())} convolutions")
    for key, (n, f) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        log(f"  {key:10s} {n:3d} layers  {f / 1e9:6.3f} GFLOP  {100 * f / total:5.1f} %")
    return total


def bench_model(args, log, total):
    import torch

    from uwudiff_amd import ops
    from uwudiff_amd.metrics import FrechetInceptionDistance

    metric = FrechetInceptionDistance(compute_dtype="bf16").to("cuda")
    model = metric.inception
    for B in args.batches:
        images = torch.randint(0, 256, (B, 3, 299, 299), dtype=torch.uint8, device="cuda")
        for what, run in (("extractor", lambda: model(images)), ("update", lambda: metric.update(images, real=True))):
            ms = statistics.median(time_calls(run, args.warmup, args.calls))
            log(f"B = {B:4d} {what:9s}: {ms:9.2f} ms  {B / ms * 1e3:8.0f} pictures/s  {total * B / ms / 1e9:7.1f} TFLOP/s algorithmic, whole program "
                f"({100 * total * B / ms / 1e9 / PEAK_BF16_TFLOPS:.1f} % of the dense bf16 peak)")
        # one pass with an event pair around every operator call
        spans, real = [], {n: getattr(ops, n) for n in ("conv2d_fwd", "conv1x1_gemm_fwd", "pool2d_fwd", "inception_stem", "global_avgpool",
                                                            "fid_stats_accum")}

        def wrap(name, fn):
            def inner(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*a, **k)
                e1.record()
                key = "conv 1x1 (uwu_gemm + ReLU)" if name == "conv1x1_gemm_fwd" else name
                if name == "conv2d_fwd":
                    kern, stride, pad = a[8], (a[9] if len(a) > 9 else k.get("stride", 1)), (a[10] if len(a) > 10 else k.get("padding", 0))
                    key = "conv " + ("stem GEMM" if a[6] == 32 and a[5] == 149 and tuple(kern) == (1, 1) else family(tuple(kern), stride, ops._pair(pad)))
                spans.append((key, e0, e1))
                return r
            return inner

        try:
            for n, fn in real.items():
                setattr(ops, n, wrap(n, fn))
            metric.update(images, real=True)
            torch.cuda.synchronize()
        finally:
            for n, fn in real.items():
                setattr(ops, n, fn)
        by = {}
        for key, e0, e1 in spans:
            by[key] = by.get(key, 0.0) + e0.elapsed_time(e1)
        whole = sum(by.values())
        log(f"B = {B:4d} time per family inside one update (event pairs around each call, {len(spans)} calls, {whole:.2f} ms in all):")
        for key, t in sorted(by.items(), key=lambda kv: -kv[1]):
            log(f"    {key:27s} {t:9.3f} ms  {100 * t / whole:5.1f} %")
        metric.reset()


# family -> one layer of it at the net's own shape: (H, W, C, Cout, kernel, stride, padding)
YARDSTICK_SHAPES = [("3x3 s1 p1", 35, 35, 64, 96, (3, 3), 1, (1, 1)), ("3x3 s1 p1", 35, 35, 96, 96, (3, 3), 1, (1, 1)),
                    ("3x3 s1 p1", 8, 8, 448, 384, (3, 3), 1, (1, 1)), ("1x1", 35, 35, 288, 64, (1, 1), 1, (0, 0)),
                    ("1x1", 17, 17, 768, 192, (1, 1), 1, (0, 0)), ("1x1", 8, 8, 2048, 320, (1, 1), 1, (0, 0)),
                    ("3x3 s1 p0", 149, 149, 32, 32, (3, 3), 1, (0, 0)), ("3x3 s1 p0", 73, 73, 80, 192, (3, 3), 1, (0, 0)),
                    ("1x7", 17, 17, 160, 160, (1, 7), 1, (0, 3)), ("7x1", 17, 17, 192, 192, (7, 1), 1, (3, 0)),
                    ("3x3 s2 p0", 35, 35, 288, 384, (3, 3), 2, (0, 0)), ("3x3 s2 p0", 17, 17, 192, 320, (3, 3), 2, (0, 0)),
                    ("5x5", 35, 35, 48, 64, (5, 5), 1, (2, 2)), ("1x3", 8, 8, 384, 384, (1, 3), 1, (0, 1)), ("3x1", 8, 8, 384, 384, (3, 1), 1, (1, 0))]


def bench_families(args, log):
    import torch

    from uwudiff_amd import ops

    B, dt = 64, torch.bfloat16
    log(f"per family at the net's own shape, B = {B}, bf16, ReLU off; median of {args.calls} after {args.warmup}, the sides alternating")
    for fam, H, W, C, Cout, k, s, p in YARDSTICK_SHAPES:
        Ho, Wo = ops.conv2d_out_hw(H, W, k, s, p)
        M, K = B * Ho * Wo, k[0] * k[1] * C
        x = torch.randn(B * H * W, C, device="cuda").to(dt)
        w = (torch.randn(Cout, K, device="cuda") * K ** -0.5).to(dt)
        bias = torch.zeros(Cout, device="cuda")
        y = torch.empty(M, Cout, device="cuda", dtype=dt)
        new = lambda: ops.conv2d_fwd(x, w, bias, B, H, W, C, Cout, k, s, p, out=y)  # noqa: E731
        if fam == "3x3 s1 p1" and ops.conv3x3_implicit_ok(x, B, H, W, C, Cout, 1):
            old, what = (lambda: ops.conv3x3_fwd(x, w, bias, B, H, W, C, Cout, 1)), "uwu_conv3x3_fwd"
        else:
            col = torch.randn(M, K, device="cuda").to(dt)
            old, what = (lambda: ops.gemm(col, w, bias=bias, epilogue=1, out=y)), "uwu_gemm on a gathered matrix"
        rounds = [(statistics.median(time_calls(new, args.warmup, args.calls)), statistics.median(time_calls(old, args.warmup, args.calls)))
                  for _ in range(2)]
        routed = ""
        if fam == "1x1":  # the explicit route as the extractor runs it: no gather, uwu_gemm + uwu_relu_rows, against the kernel WITH ReLU
            t_r = statistics.median(time_calls(lambda: ops.conv1x1_gemm_fwd(x, w, bias, C, Cout, relu=True, out=y), args.warmup, args.calls))
            t_k = statistics.median(time_calls(lambda: ops.conv2d_fwd(x, w, bias, B, H, W, C, Cout, k, s, p, relu=True, out=y), args.warmup,
                                               args.calls))
            routed = f"; with ReLU: uwu_gemm + uwu_relu_rows {t_r:.3f} ms against uwu_conv2d_fwd {t_k:.3f} ms"
        flop = 2.0 * M * Cout * K
        t_new, t_old = min(r[0] for r in rounds), min(r[1] for r in rounds)
        gather = 2.0 * M * K * 2 / 4e12 * 1e3  # one write and one read of the column matrix at 4 TB/s, in ms
        extra = "" if what == "uwu_conv3x3_fwd" else routed if fam == "1x1" else f"; explicit route at best {t_old + gather:.3f} ms"
        log(f"  {fam:10s} {H:3d}x{W:<3d} {C:4d}->{Cout:<4d} M={M:7d} K={K:5d}: uwu_conv2d_fwd {t_new:.3f} ms ({flop / t_new / 1e9:6.1f} TFLOP/s), repeats "
            f"{[round(r[0], 3) for r in rounds]}; {what} {t_old:.3f} ms, repeats {[round(r[1], 3) for r in rounds]}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--only", choices=["model", "families"], default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    total = print_counts(log)
    if not args.counts:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_fid: no GPU (a timing needs one; --counts prints the FLOP counts)")
        if args.only in (None, "model"):
            bench_model(args, log, total)
        if args.only in (None, "families"):
            bench_families(args, log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
