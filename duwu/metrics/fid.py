"""``compute_fid`` with the reference's signature and control flow (reference src/duwu/metrics/fid.py:8-41) on the native
``FrechetInceptionDistance`` (uwudiff_amd/metrics.py): the reference set first, then the generated set, in
``batch_size`` slices, then ``compute()``.  Pictures must already be 299 x 299: the extractor's own resize is not built, and a set of
another size is refused before the metric is made, the library loaded or a device touched.  That early check looks at the FIRST
picture of each set only (it is decoded once more when its batch is stacked); a later picture of another size surfaces as the
``torch.stack`` error of its batch, not as the resize message."""
from collections.abc import Sequence

import torch

from uwudiff_amd.inception import check_image_size
from uwudiff_amd.metrics import FrechetInceptionDistance


def _batches(n, batch_size, disable_tqdm, desc):
    starts = range(0, n, batch_size)
    if not disable_tqdm:
        try:
            from tqdm import tqdm

            starts = tqdm(starts, desc=desc)
        except ModuleNotFoundError:
            pass
    return starts


def compute_fid(
    generated: Sequence[torch.Tensor],
    reference: Sequence[torch.Tensor],
    batch_size: int = 256,
    device: str = "cuda",
    disable_tqdm: bool = False,
    **fid_kwargs,
):
    for dataset in (reference, generated):
        if len(dataset):
            check_image_size(tuple(dataset[0].shape), "compute_fid")
    fid = FrechetInceptionDistance(**fid_kwargs).to(device)
    for dataset, real, desc in ((reference, True, "Update FID with reference images"), (generated, False, "Update FID with generated images")):
        for start in _batches(len(dataset), batch_size, disable_tqdm, desc):
            images = torch.stack([dataset[idx] for idx in range(start, min(len(dataset), start + batch_size))]).to(device)
            fid.update(images, real=real)
    return fid.compute()
