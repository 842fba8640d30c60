"""Write the folder that configs/demo_training_folder.yaml trains on: seeded synthetic PNGs of mixed sizes and modes, each with its
caption in a ``.txt`` file beside it.

    python tools/make_demo_folder.py [--out data/demo_folder] [--n 50] [--seed 1215]

The pictures are smooth colour fields with a few rectangles and some noise: enough structure that a wrong resize or crop shows.
Landscape, portrait, square and smaller-than-target sizes; modes RGB, L, RGBA and P; some in sub-folders (the dataset searches
recursively).  The same arguments give the same files."""
import argparse
import os

import numpy as np
from PIL import Image

SIZES = [(640, 480), (480, 640), (512, 512), (300, 200), (200, 300), (1024, 768), (333, 517), (96, 128), (257, 255), (800, 260)]  # (w, h)
MODES = ["RGB", "RGB", "RGB", "L", "RGBA", "P"]
COLOURS = ["red", "green", "blue", "amber", "violet", "teal", "grey"]
SHAPES = ["boxes", "bars", "tiles"]


def picture(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.5, 4.0), rng.uniform(0.5, 4.0), rng.uniform(0, 6.28)
        img[:, :, c] = 127.5 + 100.0 * np.sin(fx * xx / w * 6.28 + fy * yy / h * 6.28 + ph)
    for _ in range(int(rng.integers(2, 6))):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = min(w, x0 + int(rng.integers(4, max(5, w // 3)))), min(h, y0 + int(rng.integers(4, max(5, h // 3))))
        img[y0:y1, x0:x1] = rng.integers(0, 256, 3)
    img += rng.normal(0.0, 6.0, img.shape)
    return Image.fromarray(np.clip(img, 0, 255).astype(np.uint8))


def make(out, n=50, seed=1215):
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        mode = MODES[i % len(MODES)]
        img = picture(rng, w, h)
        if mode == "RGBA":
            img.putalpha(Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8)))
        elif mode == "P":
            img = img.quantize(64)
        else:
            img = img.convert(mode)
        folder = os.path.join(out, f"part{i % 3}") if i % 5 == 4 else out
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, f"{i:03d}.png")
        img.save(path)
        caption = f"a {COLOURS[int(rng.integers(len(COLOURS)))]} field with {SHAPES[int(rng.integers(len(SHAPES)))]}, picture {i}"
        with open(os.path.splitext(path)[0] + ".txt", "w") as f:
            f.write(caption + "\n")
        paths.append(path)
    return paths


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "demo_folder"))
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1215)
    args = ap.parse_args()
    print(f"{len(make(args.out, args.n, args.seed))} pictures with captions in {args.out}")
