"""One batch of 16 training pictures through both paths of ``duwu.data.LocalTextImageTrainDataset``, in one process, on the GPU host:

  CPU path     ``resize_and_crop_image`` per picture (Pillow, one thread), ``torch.stack``, one upload of [16, 3, H, W] fp32
  device path  ``RaggedImages.pack`` (into pinned memory), the upload of the bytes, the coefficient tables (host), the two kernels

PIL decoding is excluded from both (the pictures are made in memory).  The device is synchronised at both ends of every timed
window.  The kernels' rate is given against the bytes they must move: the source rows and columns the windows touch, the uint8
intermediate written and read once, the tables, and the output.

    python tools/bench_preprocess.py [--batch 16] [--reps 5] [--cpu-reps 2] [--filter lanczos]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from duwu.data.utils import plan_resize_and_crop, resize_and_crop_image  # noqa: E402
from uwudiff_amd import lib as L  # noqa: E402
from uwudiff_amd import preprocess as P  # noqa: E402

CASES = [((1024, 1024), 256), ((1024, 1024), 1024), ((3000, 4000), 256), ((3000, 4000), 1024)]  # (source h, w), square target


def wall(fn, reps):
    """median wall time of fn() in ms, the device idle before and after"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def kernel_bytes(meta, tab_off, tables, target, filt):
    """what uwu_image_resize_crop must move for this batch"""
    Wt, Ht = target
    stride = (Wt * 3 + 3) & ~3
    total = tables.size * 4
    for (sh, sw, nh, nw, top, left), toff in zip(meta.tolist(), tab_off.tolist()):
        cols, rows = Wt, Ht
        if nw != sw:
            b = tables[toff[1]:toff[1] + 2 * Wt].reshape(Wt, 2)
            cols = int(b[-1, 0] + b[-1, 1] - b[0, 0])
        if nh != sh:
            b = tables[toff[3]:toff[3] + 2 * Ht].reshape(Ht, 2)
            rows = int(b[-1, 0] + b[-1, 1] - b[0, 0])
        total += rows * cols * 3 + 2 * rows * stride + 3 * Ht * Wt * 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--filter", default="lanczos")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py measures on the GPU host; no GPU found")
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}; Pillow {Image.__version__}; torch threads {torch.get_num_threads()}; "
          f"batch {args.batch}, filter {args.filter}")
    results = []
    for (h, w), t in CASES:
        target = (t, t)
        rng = np.random.default_rng(h + t)
        base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pictures = [Image.fromarray(np.roll(base, 37 * i, axis=1)) for i in range(args.batch)]
        arrays = [torch.from_numpy(np.asarray(p).copy()) for p in pictures]

        def cpu_path():
            np.random.seed(0)
            return torch.stack([resize_and_crop_image(p, target, True, args.filter)[0] for p in pictures]).to(dev)

        state = {}

        def plans():
            np.random.seed(0)
            return [plan_resize_and_crop(w, h, target, True) for _ in pictures]

        def pack():
            state["ragged"] = P.RaggedImages.pack(arrays, plans(), target, args.filter)

        def upload():
            state["data"] = state["ragged"].data.to(dev, non_blocking=True)

        def tables():
            state["tables"] = P.window_tables(state["ragged"].meta.numpy(), target, args.filter)

        def tables_upload():
            state["tab"] = torch.from_numpy(state["tables"][0]).to(dev)

        def kernels():
            r = state["ragged"]
            state["out"] = P.resize_crop(state["data"], r.offsets.numpy(), r.meta.numpy(), target, args.filter,
                                         tables=(state["tab"], state["tables"][1]), ws=state.get("ws"))

        def device_path():
            pack()
            return P.ragged_to_device(state["ragged"], dev)

        # warm-up of every shape, and the two paths must agree before either is timed
        ref, got = cpu_path(), device_path()
        torch.cuda.synchronize()
        assert torch.equal(ref, got), f"the two paths differ at {(h, w)} -> {t}"
        pack(), upload(), tables(), tables_upload()
        meta = state["ragged"].meta.numpy()
        need = int(L.load().uwu_image_resize_crop_ws_bytes(len(pictures), np.ascontiguousarray(meta).ctypes.data, t, t, L.FILTER[args.filter]))
        state["ws"] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        kernels()
        r = {"source": [h, w], "target": t, "batch": args.batch,
             "cpu_path_ms": wall(cpu_path, args.cpu_reps), "device_path_ms": wall(device_path, args.reps),
             "pack_ms": wall(pack, args.reps), "upload_ms": wall(upload, args.reps), "tables_host_ms": wall(tables, args.reps),
             "tables_upload_ms": wall(tables_upload, args.reps), "kernels_ms": wall(kernels, max(args.reps, 20))}
        r["source_mb"] = round(state["ragged"].data.numel() / 1e6, 1)
        r["kernel_mb"] = round(kernel_bytes(meta, state["tables"][1], state["tables"][0], target, args.filter) / 1e6, 2)
        r["kernels_gb_s"] = round(r["kernel_mb"] / r["kernels_ms"], 1)
        r["upload_gb_s"] = round(r["source_mb"] / r["upload_ms"], 1)
        r["speedup"] = round(r["cpu_path_ms"] / r["device_path_ms"], 2)
        results.append(r)
        print(f"{h}x{w} -> {t}x{t}: CPU path {r['cpu_path_ms']:.1f} ms/batch, device path {r['device_path_ms']:.1f} ms/batch "
              f"({r['speedup']}x) = pack {r['pack_ms']:.1f} + upload {r['upload_ms']:.1f} ({r['source_mb']} MB, {r['upload_gb_s']} GB/s) "
              f"+ tables {r['tables_host_ms']:.2f} host, {r['tables_upload_ms']:.2f} upload + kernels {r['kernels_ms']:.3f} "
              f"({r['kernel_mb']} MB to move, {r['kernels_gb_s']} GB/s)", flush=True)
    print(json.dumps({"bench": "preprocess", "results": results}))


if __name__ == "__main__":
    main()
