"""Sampling launcher with the reference's CLI (reference test_scripts/test_sampling.py):

    python test_scripts/test_sampling.py --configs configs/sampling/demo_sampling.yaml [more.yaml ...]

The YAML files are deep-merged in order; ``model_config.{unet, te, vae}`` are loaded with ``load_any``, ``sampling_func`` is
instantiated (a partial of ``duwu.sampling.diffusion_sampling``) and called with them, and the images go to ``save_dir/{i}.png``.

One step the reference's launcher does not have: the models are built under ``seed_everything(sampling_func.seed)``.  A hub name gives
stand-in weights drawn from torch's global seed (nothing is fetched), and a fresh process starts with a random one, so without this the
same command line would give other images in every process.  Weights loaded from a checkpoint or a directory do not depend on it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from duwu.loader import load_any  # noqa: E402
from duwu.utils import instantiate_any  # noqa: E402
from uwudiff_amd.config import load_yaml, merge  # noqa: E402
from uwudiff_amd.engine import seed_everything  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--configs", type=str, nargs="+", default=["configs/sampling/demo_sampling.yaml"])
    args = parser.parse_args(argv)
    config = merge(*[load_yaml(c) for c in args.configs])

    seed_everything(config.sampling_func.get("seed", 42))  # diffusion_sampling's default seed
    models = {name: load_any(config.model_config[name]) for name in ("unet", "te", "vae")}
    images = instantiate_any(config.sampling_func)(**models)

    save_dir = config.get("save_dir", None)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        for i, image in enumerate(images):
            image.save(os.path.join(save_dir, f"{i}.png"))
    return images


if __name__ == "__main__":
    main()
