"""PIL-based stand-ins for the four ``torchvision.transforms`` the reference's metric configs name (``configs/demo_metrics.yaml``:
``Compose([Resize(size), ToTensor()])``, and ``CenterCrop`` in the FID block's reference dataset); torchvision is not installable offline, ``uwudiff_amd.config.ALIASES`` points the targets
here.  They work on PIL images only, which is what ``duwu.data.text_image_local`` hands them."""
import numpy as np
import torch
from PIL import Image


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


INTERPOLATION = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


class Resize:
    """Resize of a PIL image to ``size`` = (height, width); an int resizes the SHORTER side to it and keeps the aspect ratio, as
    torchvision does.  ``interpolation``: a name of ``INTERPOLATION`` or a PIL resampling constant; bilinear by default."""

    def __init__(self, size, interpolation="bilinear"):
        if isinstance(interpolation, str) and interpolation.lower() not in INTERPOLATION:
            raise ValueError(f"Resize: interpolation must be one of {sorted(INTERPOLATION)}, got {interpolation!r}")
        self.interpolation = INTERPOLATION[interpolation.lower()] if isinstance(interpolation, str) else interpolation
        self.size = int(size) if isinstance(size, int) else tuple(int(s) for s in size)
        if not isinstance(self.size, int) and len(self.size) not in (1, 2):
            raise ValueError(f"Resize: size must be an int or (height, width), got {size!r}")

    def __call__(self, img):
        if not isinstance(img, Image.Image):
            raise TypeError(f"Resize works on PIL images, got {type(img).__name__}")
        size = self.size if isinstance(self.size, int) or len(self.size) == 2 else self.size[0]
        if isinstance(size, int):
            w, h = img.size
            short = min(w, h)
            wh = (size, max(1, int(size * h / w))) if w == short else (max(1, int(size * w / h)), size)
        else:
            wh = (size[1], size[0])
        return img.resize(wh, self.interpolation)


class ToTensor:
    """PIL image -> float32 [C, H, W] in [0, 1] (``uint8 / 255``)"""

    def __call__(self, img):
        if not isinstance(img, Image.Image):
            raise TypeError(f"ToTensor works on PIL images, got {type(img).__name__}")
        a = np.asarray(img.convert("RGB") if img.mode not in ("RGB", "L") else img, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255)


class CenterCrop:
    """The centre ``size`` = (height, width) (an int: a square) of a PIL image, with torchvision's rounding of the corner
    (``int(round((h - th) / 2))``); a side shorter than the crop is first padded with zeros on both ends, as torchvision does."""

    def __init__(self, size):
        self.size = (int(size), int(size)) if isinstance(size, int) else tuple(int(s) for s in size)
        if len(self.size) == 1:
            self.size = (self.size[0], self.size[0])
        if len(self.size) != 2 or min(self.size) < 1:
            raise ValueError(f"CenterCrop: size must be a positive int or (height, width), got {size!r}")

    def __call__(self, img):
        if not isinstance(img, Image.Image):
            raise TypeError(f"CenterCrop works on PIL images, got {type(img).__name__}")
        th, tw = self.size
        w, h = img.size
        if tw > w or th > h:
            pl, pt = (tw - w) // 2 if tw > w else 0, (th - h) // 2 if th > h else 0
            padded = Image.new(img.mode, (max(w, tw), max(h, th)))
            padded.paste(img, (pl, pt))
            img, (w, h) = padded, padded.size
        top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
        return img.crop((left, top, left + tw, top + th))
