"""reference src/duwu/data/utils.py: the building blocks a dataset of pictures is made from.  ``resize_and_crop_image`` is the
reference's CPU function; ``plan_resize_and_crop`` is the part of it that decides sizes and offsets, shared with the device path
(uwudiff_amd/preprocess.py) so that one numpy seed gives both the same crops."""
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
