"""reference src/duwu/data/utils.py: the building blocks a dataset of pictures is made from.  ``resize_and_crop_image`` is the
reference's CPU function; ``plan_resize_and_crop`` is the part of it that decides sizes and offsets, shared with the device path
(uwudiff_amd/preprocess.py) so that one numpy seed gives both the same crops.  ``make_buckets`` / ``assign_bucket`` /
``BucketBatchSampler`` (not in the reference, which leaves the training set to its users): aspect-ratio buckets, a set of same-area
target shapes with every batch drawn from one of them."""
import math
from functools import partial

import numpy as np
import torch
from PIL import Image

from uwudiff_amd.transforms import INTERPOLATION, Resize, ToTensor


def vae_image_postprocess(image_tensor: torch.Tensor) -> Image.Image:
    """utils.py:10-19 for one ``[3, H, W]`` image on the device: ``uwudiff_amd.sampling.image_u8`` and one copy to
    the host"""
    from uwudiff_amd.sampling import image_u8

    return Image.fromarray(image_u8(image_tensor[None].contiguous())[0].cpu().numpy())


BicubicResize = partial(Resize, interpolation="bicubic")


def plan_resize_and_crop(width: int, height: int, target_size: tuple[int, int] = (256, 256),
                         random_crop: bool = True) -> tuple[tuple[int, int], tuple[int, int]]:
    """utils.py:31-52 without the pixels: ``(new_size, (left, top))`` for a picture of ``width`` x ``height``.  ``target_size`` is
    (width, height); the aspect-preserving size that covers it is rounded up; a random crop draws ``np.random.randint`` for top
    first, then left."""
    scale_w = target_size[0] / width
    scale_h = target_size[1] / height
    scale = max(scale_w, scale_h)
    new_size = (math.ceil(width * scale), math.ceil(height * scale))
    crop_y = new_size[1] - target_size[1]
    crop_x = new_size[0] - target_size[0]
    if random_crop:
        top = np.random.randint(0, crop_y + 1)
        left = np.random.randint(0, crop_x + 1)
    else:
        top = crop_y // 2
        left = crop_x // 2
    return new_size, (int(left), int(top))


def resize_and_crop_image(
    image: Image.Image,
    target_size: tuple[int, int] = (256, 256),
    random_crop: bool = True,
    filter: str = "lanczos",
) -> tuple[torch.Tensor, tuple[int, int], tuple[int, int]]:
    """utils.py:25-58: aspect-preserving Lanczos resize that covers ``target_size`` = (width, height), a random or centre crop,
    ``ToTensor`` and ``Normalize(0.5, 0.5)``.  Returns ``(tensor [3, height, width], new_size, (left, top))``.  ``filter`` (not in
    the reference, which always takes Lanczos): a name of ``uwudiff_amd.transforms.INTERPOLATION``."""
    new_size, (left, top) = plan_resize_and_crop(image.width, image.height, target_size, random_crop)
    image = image.resize(new_size, INTERPOLATION[filter])
    image = ToTensor()(image)
    cropped_image = image[:, top: top + target_size[1], left: left + target_size[0]]
    half = torch.full((cropped_image.shape[0], 1, 1), 0.5)
    cropped_image = (cropped_image - half) / half  # Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)): sub, then div
    return cropped_image, new_size, (left, top)


def make_buckets(resolution: int = 1024, min_side: int = 512, max_side: int = 2048, step: int = 64) -> list[tuple[int, int]]:
    """The (width, height) targets of aspect-ratio bucketing: for every width that is a multiple of ``step`` in
    ``[min_side, max_side]`` the tallest height on the ``step`` grid whose area stays within ``resolution ** 2`` (capped at
    ``max_side``), and its transpose.  Unique pairs sorted by ``w / h``, then by ``w``.  ``step`` must be a multiple of 64: the VAE
    divides a side by 8 and the UNets halve it up to three times more."""
    resolution, min_side, max_side, step = int(resolution), int(min_side), int(max_side), int(step)
    if step < 64 or step % 64 != 0:
        raise ValueError(f"make_buckets: step must be a positive multiple of 64 (VAE / 8, then up to three halvings), got {step}")
    if not 0 < min_side <= max_side:
        raise ValueError(f"make_buckets: need 0 < min_side <= max_side, got {min_side}, {max_side}")
    pairs = set()
    for w in range(min_side, max_side + 1, step):
        h = min(max_side, (resolution * resolution // w) // step * step)
        if h >= min_side:
            pairs.add((w, h))
            pairs.add((h, w))
    return sorted(pairs, key=lambda p: (p[0] / p[1], p[0]))


def assign_bucket(width: int, height: int, buckets) -> int:
    """The index of the bucket whose aspect ratio is nearest to the picture's: the smallest ``|log(bw / bh) - log(width / height)|``;
    on a tie the lower index."""
    if width <= 0 or height <= 0:
        raise ValueError(f"assign_bucket: bad picture size {width} x {height}")
    if len(buckets) == 0:
        raise ValueError("assign_bucket: no buckets")
    a = math.log(width / height)
    best, best_d = 0, math.inf
    for i, (bw, bh) in enumerate(buckets):
        d = abs(math.log(bw / bh) - a)
        if d < best_d:
            best, best_d = i, d
    return best


class BucketBatchSampler(torch.utils.data.Sampler):
    """A batch sampler whose every batch holds indices of ONE bucket.  ``bucket_of[i]`` is the bucket of dataset index ``i``.

    ``shuffle``: each epoch permutes the indices inside each bucket (buckets in index order), cuts them into batches, then permutes
    the batches -- all with ``torch.randperm`` on torch's global CPU generator, which ``seed_everything`` seeds, as the
    ``DataLoader``'s own shuffling draws from it.  Without: buckets in index order, indices ascending.  The ragged last batch of each
    bucket is kept unless ``drop_last``.  ``len()`` is exact."""

    def __init__(self, bucket_of, batch_size: int, shuffle: bool = False, drop_last: bool = False):
        if isinstance(batch_size, bool) or int(batch_size) < 1:
            raise ValueError(f"BucketBatchSampler: batch_size must be a positive int, got {batch_size!r}")
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.drop_last = bool(drop_last)
        members = {}
        for i, b in enumerate(bucket_of):
            members.setdefault(int(b), []).append(i)
        self.members = [members[b] for b in sorted(members)]

    def __len__(self):
        if self.drop_last:
            return sum(len(m) // self.batch_size for m in self.members)
        return sum((len(m) + self.batch_size - 1) // self.batch_size for m in self.members)

    def __iter__(self):
        batches = []
        for m in self.members:
            order = [m[j] for j in torch.randperm(len(m)).tolist()] if self.shuffle else m
            for at in range(0, len(order), self.batch_size):
                batch = order[at:at + self.batch_size]
                if len(batch) == self.batch_size or not self.drop_last:
                    batches.append(batch)
        if self.shuffle:
            batches = [batches[j] for j in torch.randperm(len(batches)).tolist()]
        return iter(batches)
