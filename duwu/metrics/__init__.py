"""Import surface of the reference's ``duwu.metrics`` (reference src/duwu/metrics/__init__.py)."""
from .clip import compute_clip_score  # noqa: F401
from .compute_metrics import MetricConfig, compute_metrics  # noqa: F401
from .fid import compute_fid  # noqa: F401
