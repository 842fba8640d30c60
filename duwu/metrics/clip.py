"""``compute_clip_score`` with the reference's signature and control flow (reference src/duwu/metrics/clip.py:8-33) on the native
``CLIPScore`` (uwudiff_amd/metrics.py): batches of (image, text) pairs are stacked, scaled to [0, 255] when ``normalize`` says the
dataset yields [0, 1], and fed to ``update``; the result of ``compute`` is returned."""
from collections.abc import Sequence

import torch

from uwudiff_amd.metrics import CLIPScore


def compute_clip_score(
    generated: Sequence[tuple[torch.Tensor, str]],  # (image, text) pairs
    batch_size: int = 256,
    device: str = "cuda",
    disable_tqdm: bool = False,
    normalize: bool = True,
    **clip_kwargs,
):
    metric = CLIPScore(**clip_kwargs).to(device)
    starts = range(0, len(generated), batch_size)
    if not disable_tqdm:
        try:
            from tqdm import tqdm

            starts = tqdm(starts)
        except ModuleNotFoundError:
            pass
    for start in starts:
        pairs = [generated[i] for i in range(start, min(len(generated), start + batch_size))]
        images = torch.stack([image for image, _ in pairs]).to(device)
        if normalize:  # the metric takes [0, 255]
            images = images * 255
        metric.update(images, [text for _, text in pairs])
    return metric.compute()
