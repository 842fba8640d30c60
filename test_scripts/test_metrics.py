"""Metrics launcher with the reference's CLI (reference test_scripts/test_metrics.py):

    python test_scripts/test_metrics.py --configs configs/demo_metrics.yaml [more.yaml ...]

The YAML files are deep-merged in order; every entry of ``metrics`` becomes a ``duwu.metrics.MetricConfig``, the images
below ``generated_image_dir`` are listed, and ``compute_metrics`` runs each metric over them.  One line per metric is printed:
``<name>: <value>``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from duwu.metrics import MetricConfig, compute_metrics  # noqa: E402
from duwu.utils import get_images_recursively, instantiate_any  # noqa: E402
from uwudiff_amd.config import load_yaml, merge  # noqa: E402


def metric_config(node):
    """One entry of ``metrics`` -> MetricConfig.  The entry itself has no ``_target_``; its fields that are nodes (``metric_func``,
    ``generated_dataset_func``, ``ref_dataset``) are instantiated one by one, the way hydra's ``instantiate`` walks a plain mapping.
    (The reference hands the whole entry to ``instantiate_any``, which returns a mapping without ``_target_`` as it is.)"""
    return MetricConfig(**{k: instantiate_any(v) if isinstance(v, dict) else v for k, v in node.items()})


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--configs", type=str, nargs="+", default=["configs/demo_metrics.yaml"])
    args = parser.parse_args(argv)
    config = merge(*[load_yaml(c) for c in args.configs])

    generated_images = get_images_recursively(config.generated_image_dir)
    metric_configs = [metric_config(node) for node in config.metrics]
    metrics = compute_metrics(metric_configs, generated_images)
    for name, value in metrics.items():
        print(f"{name}: {float(value):.4f}" if hasattr(value, "item") else f"{name}: {value}")
    return metrics


if __name__ == "__main__":
    main()
