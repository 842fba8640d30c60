"""CLIP score on the native CLIP towers: the part of ``torchmetrics.multimodal.CLIPScore`` that
``duwu.metrics.compute_clip_score`` uses -- ``CLIPScore(model_name_or_path).to(device)``, ``update(images, texts)``, ``compute()``.

    score(image, text) = 100 cos(image_embeds, text_embeds)         metric = max(mean over all pairs, 0)

Both towers run on the HIP kernels (``uwudiff_amd.text_model``, ``uwudiff_amd.vision_model``); the cosine, the sum over a batch and the
running total are ``uwu_clip_score_accum`` on a device-side double accumulator, so an ``update`` never waits for the device and
``compute`` reads two numbers once.  Captions go through the ``SyntheticTokenizer`` the rest of this build uses (no tokenizer files
exist offline).  Images must already have the model's size: the resize belongs to the dataset transform.
"""
import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .conditioning import SyntheticTokenizer
from .vision_model import load_clip_pair


class CLIPScore(nn.Module):
    def __init__(self, model_name_or_path="openai/clip-vit-large-patch14", compute_dtype="bf16", **kw):
        super().__init__()
        if kw:  # torchmetrics' Metric keywords (dist_sync_on_step, ...): nothing is silently ignored
            raise NotImplementedError(f"CLIPScore: {sorted(kw)} not built")
        self.model_name_or_path = str(model_name_or_path)
        self.text_model, self.vision_model = load_clip_pair(model_name_or_path, compute_dtype=compute_dtype)
        if self.text_model.config["projection_dim"] != self.vision_model.config["projection_dim"]:
            raise ValueError("CLIPScore: the two towers project to different widths")
        self.tokenizer = SyntheticTokenizer()  # no name: a path that happens to contain "t5" must not pick the T5-shaped variant
        self.max_length = min(77, int(self.text_model.config["max_position_embeddings"]))
        self.acc = None  # float64 [2] on the device, (sum of scores, pairs): made by the first update, no buffer (a cast must not touch it)

    def reset(self):
        self.acc = None

    @torch.no_grad()
    def update(self, images, texts):
        """images: [B, 3, S, S] (or a list of [3, S, S]) with values in [0, 255], fp32 or uint8, on the device, S the model's
        image_size; texts: B captions (or one).  -> the B scores, fp32 on the device."""
        if isinstance(images, (list, tuple)):
            images = torch.stack(list(images))
        if torch.is_tensor(images) and images.dim() == 3:
            images = images[None]
        texts = [texts] if isinstance(texts, str) else list(texts)
        if not torch.is_tensor(images):
            raise TypeError(f"CLIPScore: images must be a tensor or a list of tensors, got {type(images).__name__}")
        S = int(self.vision_model.config["image_size"])
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, S, S):
            raise ValueError(f"CLIPScore: {self.model_name_or_path} takes images of [3, {S}, {S}], got {tuple(images.shape[1:])}; resize in "
                             f"the dataset transform (torchvision.transforms.Resize with size: [{S}, {S}]) -- an on-device resize is not built")
        if len(texts) != images.shape[0]:
            raise ValueError(f"CLIPScore: {images.shape[0]} images and {len(texts)} texts")
        if not torch.is_tensor(images) or not images.is_cuda or not self.vision_model.flat.is_cuda:
            raise L.UwuError("CLIPScore.update runs on the HIP device only (no CPU fallback): move the metric and the images there")
        tok = self.tokenizer(texts, padding="max_length", truncation=True, return_tensors="pt")
        ids = tok["input_ids"][:, :self.max_length].to(images.device)
        mask = tok["attention_mask"][:, :self.max_length].to(images.device)
        text_embeds = self.text_model(ids, attention_mask=mask)[0]
        image_embeds = self.vision_model.embed_images(images)
        if self.acc is None or self.acc.device != images.device:
            self.acc = torch.zeros(2, dtype=torch.float64, device=images.device)
        return ops.clip_score_accum(image_embeds, text_embeds, self.acc)

    def compute(self):
        """max(mean score, 0) as a scalar tensor on the metric's device; the one place the host waits for the device"""
        if self.acc is None:
            raise RuntimeError("CLIPScore.compute() before any update()")
        total, n = self.acc.tolist()
        return torch.tensor(max(total / n, 0.0), dtype=torch.float32, device=self.acc.device)
