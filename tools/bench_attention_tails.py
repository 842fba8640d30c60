"""Time attention at query counts that are no multiple of 64 -- the token counts of the aspect-ratio buckets -- next to
the next multiple of 64, and next to another build of the library on the same shapes.

    python tools/bench_attention_tails.py [--batch 8] [--rounds 5] [--iters 10] [--lib PATH/libuwu_hip.so]
    python tools/bench_attention_tails.py --against PATH/libuwu_hip.so [--passes 2]

Rows: bf16, packed q|k|v, self-attention, forward and backward, at T = 3952 and 988 with H x d = 10 x 64 and 20 x 64 (the SDXL UNet at
832 x 1216 pixels) and T = 4032 and 1008 with 8 x 40 and 8 x 80 (Stable Diffusion 1.x at 448 x 576), each beside the next multiple
of 64 (4032 / 1024 / 4096 / 1024).  Device events around `iters` launches after a warm-up of every shape; the two rows of a pair
alternate inside a round; the figure is the median over the rounds with the spread (min .. max) beside it.  The TFLOP/s column is
the algorithm's work (4 T^2 d per head forward, 10 T^2 d backward) over that time, not a share of peak.  `route` is what
`uwu_attention_route` says where the library has it ("mfma" / "generic"), "?" where it has not.

--lib: time another build of the library (the parent commit's, say) with this tree's Python.  --against: run this build and that
library in processes of their own, `passes` times in turn, and print both sets of rows.
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uwudiff_amd import lib as L  # noqa: E402

# (ragged T, the next multiple of 64, heads, head width)
PAIRS = [(3952, 4032, 10, 64), (988, 1024, 20, 64), (4032, 4096, 8, 40), (1008, 1024, 8, 80)]


def use_library(path):
    """bind `path` instead of the tree's library; entry points it does not export (an older build) are left out of the table"""
    L.LIB_PATH = os.path.abspath(path)
    have = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L._SIGS if not hasattr(have, n)]:
        del L._SIGS[name]


def _route(T, H, d, backward):
    if "uwu_attention_route" not in L._SIGS:
        return "?"
    D = H * d
    return "mfma" if L.load().uwu_attention_route(int(backward), T, T, d, 3 * D, 3 * D, 3 * D, D, L.BF16) else "generic"


def _case(B, T, H, d):
    from uwudiff_amd import ops

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


def measure(args):
    torch.manual_seed(0)
    B = args.batch
    print(f"library {L.LIB_PATH}", flush=True)
    for ragged, whole, H, d in PAIRS:
        shapes = [(ragged, H, d), (whole, H, d)]
        fns = {s: _case(B, *s) for s in shapes}
        times = {(s, i): [] for s in shapes for i in range(2)}
        for s in shapes:  # warm-up of every shape
            for f in fns[s]:
                _time(f, 2)
        for _ in range(args.rounds):
            for s in shapes:
                for i, f in enumerate(fns[s]):
                    times[(s, i)].append(_time(f, args.iters))
        for s in shapes:
            T = s[0]
            for i, (name, work) in enumerate((("fwd", 4.0), ("bwd", 10.0))):
                ts = times[(s, i)]
                med = statistics.median(ts)
                print(f"T={T:5d} H={H:2d} d={d:3d} {name} {_route(T, H, d, i):8s} {med:10.1f} us  ({min(ts):.1f} .. {max(ts):.1f})  "
                      f"{work * B * H * T * T * d / med / 1e6:7.1f} TFLOP/s", flush=True)
        del fns
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lib", default=None, help="another build of libuwu_hip.so to time instead of the tree's")
    ap.add_argument("--against", default=None, help="another build to time NEXT TO the tree's, each in processes of its own")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds one child process may take (--against)")
    args = ap.parse_args()
    if args.against:
        base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        for p in range(args.passes):
            for extra in ([], ["--lib", args.against]):
                print(f"--- pass {p + 1}: {'this build' if not extra else 'the other library'}", flush=True)
                rc = subprocess.run(base + extra, timeout=args.timeout).returncode
                if rc != 0:  # nothing more is started on a device after a failure
                    sys.exit(f"bench_attention_tails: the child process ended with {rc}")
        return
    if args.lib:
        use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_attention_tails: needs the GPU (nothing is measured without one)")
    measure(args)


if __name__ == "__main__":
    main()
