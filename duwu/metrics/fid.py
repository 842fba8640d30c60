"""``compute_fid`` with the reference's signature (reference src/duwu/metrics/fid.py:8-15).  The metric itself is not built: FID needs
an InceptionV3 feature extractor."""
from collections.abc import Sequence

import torch


def compute_fid(
    generated: Sequence[torch.Tensor],
    reference: Sequence[torch.Tensor],
    batch_size: int = 256,
    device: str = "cuda",
    disable_tqdm: bool = False,
    **fid_kwargs,
):
    raise NotImplementedError("compute_fid: the InceptionV3 feature extractor FID needs is not built on the HIP kernels (DESIGN.md "
                              "section 7); only the CLIP score is")
