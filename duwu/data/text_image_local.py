"""The reference's folder datasets (reference src/duwu/data/text_image_local.py:12-55): images by path, images of a folder, and
(image, caption) pairs whose caption is the ``.txt`` file next to the image.  PIL-based; the default transform is this build's
``ToTensor`` stand-in (uwudiff_amd/transforms.py)."""
import warnings
from collections.abc import Callable
from pathlib import Path

from PIL import Image
from torch.utils.data import Dataset

from duwu.utils import get_images_recursively
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
