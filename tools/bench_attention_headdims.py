"""Time self-attention at the Stable Diffusion 1.x head widths next to head width 64 at the same total width.

    python tools/bench_attention_headdims.py [--batch 8] [--rounds 5] [--iters 20]

Rows: d = 40 / H = 8 against d = 64 / H = 5 at T = 4096 (320 channels), d = 80 / H = 8 against d = 64 / H = 10 at T = 1024 (640
channels); bf16, packed q|k|v, forward and backward.  Device events around `iters` launches after a warm-up of every shape; the
rows of one pair alternate inside a round, and the figure is the median over the rounds with the spread (min .. max) beside it.
The TFLOP/s column is the algorithm's work (4 T^2 d per head forward, 10 T^2 d backward) over that time, not a share of peak.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uwudiff_amd import ops  # noqa: E402

PAIRS = [((4096, 8, 40), (4096, 5, 64)), ((1024, 8, 80), (1024, 10, 64))]


def _case(B, T, H, d):
    D = H * d
    qkv = torch.randn(B * T, 3 * D, device="cuda").to(torch.bfloat16)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    o, lse = ops.attention_fwd(q, k, v, B, T, T, H, d)
    do = torch.randn(B * T, D, device="cuda").to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    fwd = lambda: ops.attention_fwd(q, k, v, B, T, T, H, d)  # noqa: E731
    bwd = lambda: ops.attention_bwd(q, k, v, o, do, lse, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B, T, T, H, d)  # noqa: E731
    return fwd, bwd


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention_headdims: needs the GPU (nothing is measured without one)")
    torch.manual_seed(0)
    B = args.batch
    for pair in PAIRS:
        fns = {shape: _case(B, *shape) for shape in pair}
        times = {(shape, i): [] for shape in pair for i in range(2)}
        for shape in pair:  # warm-up of every shape
            for f in fns[shape]:
                _time(f, 3)
        for _ in range(args.rounds):
            for shape in pair:
                for i, f in enumerate(fns[shape]):
                    times[(shape, i)].append(_time(f, args.iters))
        for shape in pair:
            T, H, d = shape
            for i, (name, work) in enumerate((("fwd", 4.0), ("bwd", 10.0))):
                ts = times[(shape, i)]
                med = statistics.median(ts)
                print(f"T={T:5d} H={H:2d} d={d:3d} {name}  {med:9.1f} us  ({min(ts):.1f} .. {max(ts):.1f})  "
                      f"{work * B * H * T * T * d / med / 1e6:7.1f} TFLOP/s")


if __name__ == "__main__":
    main()
