"""``HfImageDataset`` / ``HfPromptDataset`` with the signatures of the reference's Hugging Face wrappers (reference
src/duwu/data/hf_dataset.py:9-51); the bodies are written for this package.  Both work over any sequence of dicts: a
``datasets.Dataset`` where that package is installed, a plain list of ``{"image": PIL image, "caption": [...]}`` otherwise.
``datasets`` is never imported here: nothing is fetched, and the wrappers need nothing of it but ``len``, indexing and iteration."""
from collections.abc import Callable, Sequence

from torch.utils.data import Dataset

from uwudiff_amd.transforms import ToTensor


class HfImageDataset(Dataset):
    """item i: the picture under ``image_key`` of row i, made RGB, through ``image_transform`` (default: ``ToTensor``)"""

    def __init__(self, hf_dataset: Sequence[dict], image_key: str = "image", image_transform: Callable | None = None):
        self.rows, self.key = hf_dataset, image_key
        self.transform = ToTensor() if image_transform is None else image_transform

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, idx):
        picture = self.rows[idx][self.key]
        return self.transform(picture if picture.mode == "RGB" else picture.convert("RGB"))


class HfPromptDataset(Dataset):
    """the captions under ``prompt_key`` (a list per row), read once at construction: the first of every row, or with
    ``all_captions`` every one, row after row"""

    def __init__(self, hf_dataset: Sequence[dict], prompt_key: str = "caption", all_captions: bool = False):
        per_row = (row[prompt_key] for row in hf_dataset)
        self.captions = [c for group in per_row for c in (group if all_captions else group[:1])]

    def __len__(self):
        return len(self.captions)

    def __getitem__(self, idx):
        return self.captions[idx]
