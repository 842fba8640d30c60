"""The SDXL-shape UNet's forward + backward at a bucket's latent shape next to the square one of the same area.

    python tools/bench_buckets.py [--batch 12] [--warmup 2] [--steps 4] [--rounds 2] [--lib PATH/libuwu_hip.so]

Shapes: 4 x 104 x 152 (832 x 1216 pixels: the UNet attends at T = 3952 and 988, no multiples of 64) and 4 x 128 x 128 (T = 4096 and
1024), batch 12, bf16 -- the setting of `bench.py --model SDXL-UNet --latent 128`: the loss's forward and the backward into the flat
gradient, which is zeroed between steps; no optimizer step.  A host clock around `steps` steps that end in a device synchronise,
after `warmup` steps of that shape; the shapes alternate over `rounds` rounds.  Prints one line per shape and round in images/s.
--lib: time another build of the library (the parent commit's, say) with this tree's Python.
"""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uwudiff_amd import lib as L  # noqa: E402

SHAPES = [(104, 152), (128, 128)]


def use_library(path):
    """bind `path` instead of the tree's library; entry points it does not export (an older build) are left out of the table"""
    L.LIB_PATH = os.path.abspath(path)
    have = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L._SIGS if not hasattr(have, n)]:
        del L._SIGS[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--config", default="sdxl", help="UNet preset (tests: tiny-unet)")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_buckets: needs the GPU (nothing is measured without one)")
    from uwudiff_amd.objective import DiffusionLoss
    from uwudiff_amd.scheduler import EulerDiscreteScheduler
    from uwudiff_amd.unet import UNet2DConditionModel

    dev = torch.device("cuda")
    torch.manual_seed(1215)
    model = UNet2DConditionModel.from_config(args.config, compute_dtype="bf16", device=dev)
    loss_fn = DiffusionLoss(EulerDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder="scheduler"))
    B = args.batch
    cfg = model.cfg_dict
    ctx = torch.randn(B, 77, cfg["cross_attention_dim"]).to(dev)
    n_pool = cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]
    pooled = torch.randn(B, n_pool).to(dev)
    model.flat.grad = torch.empty_like(model.flat.data)
    one = torch.ones((), dtype=torch.float32).to(dev)
    print(f"library {L.LIB_PATH}; {args.config} UNet, batch {B}, bf16, forward + backward", flush=True)

    def step(x, ids):
        L.call("uwu_memset_zero", L.ptr(model.flat.grad), model.flat.grad.numel() * 4, L.stream())
        loss, _ = loss_fn(x, model, encoder_hidden_states=ctx, added_cond_kwargs={"text_embeds": pooled, "time_ids": ids})
        loss.backward(one)
        return loss

    inputs = {}
    for h, w in SHAPES:
        inputs[(h, w)] = (torch.randn(B, 4, h, w).to(dev), torch.tensor([[1024.0, 1024, 0, 0, 8.0 * h, 8.0 * w]] * B).to(dev))
    for r in range(args.rounds):
        for (h, w), (x, ids) in inputs.items():
            for _ in range(args.warmup):
                step(x, ids)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step(x, ids)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            print(f"round {r + 1} latent 4x{h}x{w}: {el / args.steps * 1e3:9.1f} ms / step  {B * args.steps / el:7.2f} images/s  "
                  f"(loss {float(loss.detach()):.4f})", flush=True)


if __name__ == "__main__":
    main()
