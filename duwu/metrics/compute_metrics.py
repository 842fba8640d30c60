"""``MetricConfig`` / ``compute_metrics`` with the reference's signatures and control flow (reference
src/duwu/metrics/compute_metrics.py:6-29); the bodies are written for this package."""
from collections.abc import Callable, Sequence
from dataclasses import dataclass


@dataclass
class MetricConfig:
    """One metric of a run: its display name, the metric function, the callable that turns the list of generated image paths into
    a dataset, and the reference dataset for metrics that compare against one."""

    name: str
    metric_func: Callable
    generated_dataset_func: Callable
    ref_dataset: Sequence | None = None


def compute_metrics(metric_configs: list[MetricConfig], generated_image_paths: list[str]) -> dict[str, float]:
    """name -> ``metric_func(generated=dataset)``, with ``reference=ref_dataset`` added only where a reference dataset is set"""
    results = {}
    for mc in metric_configs:
        kwargs = {"generated": mc.generated_dataset_func(generated_image_paths)}
        if mc.ref_dataset is not None:
            kwargs["reference"] = mc.ref_dataset
        results[mc.name] = mc.metric_func(**kwargs)
    return results
