"""The reference's folder datasets (reference src/duwu/data/text_image_local.py:12-55): images by path, images of a folder, and
(image, caption) pairs whose caption is the ``.txt`` file next to the image.  PIL-based; the default transform is this build's
``ToTensor`` stand-in (uwudiff_amd/transforms.py).  ``LocalTextImageTrainDataset`` (not in the reference, which leaves the training
dataset to its users) is the folder as a training set, built on ``duwu.data.utils.resize_and_crop_image``."""
import warnings
from collections.abc import Callable
from pathlib import Path

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from duwu.data.base import UwUBaseDataset
from duwu.data.utils import BucketBatchSampler, assign_bucket, make_buckets, plan_resize_and_crop, resize_and_crop_image
from duwu.utils import get_images_recursively
from uwudiff_amd.preprocess import RaggedImages
from uwudiff_amd.transforms import ToTensor


class LocalImageDataset(Dataset):
    def __init__(self, image_paths: list[str], image_transform: Callable | None = None):
        self.image_paths = image_paths
        self.image_transform = image_transform or ToTensor()

    def __len__(self):
        return len(self.image_paths)

    def __getitem__(self, idx):
        path = self.image_paths[idx]
        # a decoder warning (a truncated file, an odd profile) is printed with the file it belongs to, once per access
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            with Image.open(path) as raw:
                image = self.image_transform(raw.convert("RGB"))
        for w in caught:
            print(f"{path}: {w.message}")
        return image


class LocalImageDatasetFromFolder(LocalImageDataset):
    def __init__(self, image_dir: str, image_transform: Callable | None = None):
        super().__init__(get_images_recursively(image_dir), image_transform)


class LocalTextImageDataset(LocalImageDataset):
    def __getitem__(self, idx):
        image = super().__getitem__(idx)
        caption = Path(self.image_paths[idx]).with_suffix(".txt").read_text().strip()
        return image, caption


class LocalTextImageTrainDataset(UwUBaseDataset):
    """A folder of pictures with captions as a training set: the items and the collated 5-tuple of ``DummyDataset``, so
    ``TrainDataModule`` and ``DMTrainer`` take it as it is.  The caption of ``x.png`` is the stripped text of ``x.txt`` beside it.
    Every picture goes through ``resize_and_crop_image``: an aspect-preserving resize that covers ``target_size`` = (width, height),
    then a random (``random_crop``) or centre crop, ``ToTensor`` and ``Normalize(0.5, 0.5)``.

    ``resize_on_device=False``: that function itself, on the loader's thread; ``sample`` is its ``[3, height, width]`` tensor.
    ``resize_on_device=True``: ``sample`` is the decoded uint8 ``[h, w, 3]`` picture with its plan; ``collate`` packs the batch into
    a :class:`uwudiff_amd.preprocess.RaggedImages` and ``Fitter._to_device`` resizes it on the GPU (``uwu_image_resize_crop``) to
    the same bits.  Both modes draw the crops from ``np.random`` in the same order: one numpy seed gives both the same batches.

    ``add_time_ids = [orig_h, orig_w, top, left, target_h, target_w]``, SDXL's micro-conditioning: the size of the FILE, the crop's
    offset in the resized picture, and the target.  The file's size rather than the resized one: SDXL conditions on the
    resolution the picture had before any resizing, so that low-resolution sources can be told from sharp ones at sampling time;
    the resized size says nothing the target does not.

    ``buckets`` (aspect-ratio buckets): ``None`` -- every picture takes ``target_size``; a mapping -- the keyword
    arguments of ``duwu.data.utils.make_buckets``; a list of ``[width, height]`` pairs -- taken as given.  The constructor then reads
    every file's size (its header, no decode) and assigns the file to the bucket of the nearest aspect ratio; that bucket is the
    index's target in ``__getitem__`` and in ``add_time_ids``.  A batch must come from one bucket: ``batch_sampler`` gives such
    batches, ``collate`` refuses any other, and ``TrainDataModule`` builds its loader from ``batch_sampler``."""

    def __init__(self, image_dir: str | None = None, image_paths: list[str] | None = None, target_size=(256, 256), random_crop=True,
                 resize_on_device=True, filter="lanczos", tokenizers=(), buckets=None, **kwargs):
        if (image_dir is None) == (image_paths is None):
            raise ValueError("LocalTextImageTrainDataset: give image_dir or image_paths (one of them)")
        if filter not in ("lanczos", "bicubic", "bilinear"):
            raise ValueError(f"LocalTextImageTrainDataset: filter must be lanczos, bicubic or bilinear, got {filter!r}")
        self.image_paths = get_images_recursively(image_dir) if image_paths is None else [str(p) for p in image_paths]
        self.target_size = (int(target_size[0]), int(target_size[1]))
        self.random_crop = bool(random_crop)
        self.resize_on_device = bool(resize_on_device)
        self.filter = filter
        self.tokenizers = list(tokenizers) if isinstance(tokenizers, (list, tuple)) else [tokenizers]
        self.buckets, self.bucket_of = None, None
        if buckets is not None:
            if hasattr(buckets, "keys"):
                self.buckets = make_buckets(**{str(k): buckets[k] for k in buckets.keys()})
            else:
                self.buckets = [(int(b[0]), int(b[1])) for b in buckets]
            if not self.buckets:
                raise ValueError("LocalTextImageTrainDataset: buckets is empty")
            self.bucket_of = []
            for path in self.image_paths:
                with Image.open(path) as raw:  # the header only: no pixel is decoded
                    width, height = raw.size
                self.bucket_of.append(assign_bucket(width, height, self.buckets))

    def set_tokenizers(self, tokenizers):
        self.tokenizers = tokenizers

    def __len__(self):
        return len(self.image_paths)

    def target_of(self, index):
        """(width, height) the picture at ``index`` is resized and cropped to"""
        return self.target_size if self.buckets is None else self.buckets[self.bucket_of[index]]

    def batch_sampler(self, batch_size, shuffle=False, drop_last=False):
        """batches of one bucket each, for ``DataLoader(batch_sampler=...)``"""
        if self.buckets is None:
            raise ValueError("LocalTextImageTrainDataset.batch_sampler: the dataset has no buckets")
        return BucketBatchSampler(self.bucket_of, batch_size, shuffle, drop_last)

    def __getitem__(self, index):
        target = self.target_of(index)
        path = self.image_paths[index]
        txt = Path(path).with_suffix(".txt")
        if not txt.exists():
            raise FileNotFoundError(f"no caption file {txt} for {path}")
        caption = txt.read_text().strip()
        with Image.open(path) as raw:
            image = raw.convert("RGB")
        width, height = image.size
        if self.resize_on_device:
            new_size, (left, top) = plan_resize_and_crop(width, height, target, self.random_crop)
            sample = {"image": torch.from_numpy(np.array(image, dtype=np.uint8)), "plan": (new_size, (left, top))}
        else:
            sample, new_size, (left, top) = resize_and_crop_image(image, target, self.random_crop, self.filter)
        return {
            "sample": sample,
            "caption": caption,
            "tokenizer_out": [t(caption, padding="max_length", truncation=True, return_tensors="pt") for t in self.tokenizers],
            "add_time_ids": torch.tensor([height, width, top, left, target[1], target[0]]),
        }

    def collate(self, batch):
        # the target of the batch: what every item's add_time_ids[4:6] = (height, width) says (one bucket per batch)
        targets = {(int(x["add_time_ids"][5]), int(x["add_time_ids"][4])) for x in batch}
        if len(targets) != 1:
            raise ValueError(f"LocalTextImageTrainDataset.collate: a batch mixes the targets {sorted(targets)}; draw batches of one "
                             f"bucket with batch_sampler()")
        if not self.resize_on_device:
            return UwUBaseDataset.collate(batch)
        ragged = RaggedImages.pack([x["sample"]["image"] for x in batch], [x["sample"]["plan"] for x in batch], targets.pop(),
                                   self.filter)
        # the other four slots as the inherited collate makes them
        _, caption, tokenizer_outputs, added, ca = UwUBaseDataset.collate([{**x, "sample": torch.empty(0)} for x in batch])
        return ragged, caption, tokenizer_outputs, added, ca
