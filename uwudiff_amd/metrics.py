"""The two metrics of ``duwu.metrics`` on native models: the CLIP score (below) and, further down, ``FrechetInceptionDistance`` on the
native InceptionV3.

CLIP score on the native CLIP towers: the part of ``torchmetrics.multimodal.CLIPScore`` that
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


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eigvals(S1 S2)).real, in float64 on the host (torchmetrics' ``_compute_fid``).

    With fewer samples than features most eigenvalues of S1 S2 are zero, and the solver returns each of them as noise of the order
    of eps |S1 S2|; a square root turns 1e-16 into 1e-8, and two thousand of those made the FID of two identical sets of twelve
    pictures -3.6e-6 tr S.  Eigenvalues below D eps max|lambda| -- what the solver cannot tell from zero, the rule of
    ``matrix_rank`` -- therefore count as zero; a true eigenvalue that small adds less than 1e-6 sqrt(max|lambda|)."""
    mu1, sigma1, mu2, sigma2 = (torch.as_tensor(t, dtype=torch.float64, device="cpu") for t in (mu1, sigma1, mu2, sigma2))
    a = (mu1 - mu2).square().sum()
    ev = torch.linalg.eigvals(sigma1 @ sigma2)
    ev = ev[ev.abs() > sigma1.shape[0] * torch.finfo(torch.float64).eps * ev.abs().max()]
    return a + sigma1.trace() + sigma2.trace() - 2 * ev.sqrt().real.sum()


def moments_from_sums(n, total, outer):
    """(mean, covariance) of n samples from their sum [D] and their sum of outer products [D, D]: mean = sum / n, cov = (outer - n mean
    mean^T) / (n - 1), float64"""
    mean = total / n
    return mean, (outer - n * torch.outer(mean, mean)) / (n - 1)


class FrechetInceptionDistance(nn.Module):
    """The part of ``torchmetrics.image.fid.FrechetInceptionDistance`` that ``duwu.metrics.compute_fid`` uses, on the native
    ``FIDInceptionV3``: ``update(imgs, real)`` extracts the 2048-d features in chunks and adds n, the sum and
    the sum of outer products to a float64 block on the device (``uwu_fid_stats_accum``) without waiting for it; ``compute()`` is the one
    place the host waits.  The extractor's weights are seeded unless ``feature_extractor_weights_path`` names a local ``.pth`` holding
    torch-fidelity's ``pt_inception-2015-12-05`` state dict; nothing is fetched.

    One departure from torchmetrics: ``compute()`` counts the eigenvalues of S1 S2 that the solver cannot tell from zero as zero (see
    ``frechet_distance``).  With fewer samples than features -- rank-deficient statistics -- the result therefore differs from what
    torchmetrics prints by the solver noise torchmetrics keeps, a few 1e-6 tr S."""

    def __init__(self, feature=2048, reset_real_features=True, normalize=False, input_img_size=(3, 299, 299),
                 feature_extractor_weights_path=None, compute_dtype="bf16", **kw):
        super().__init__()
        from .inception import FEATURES, FIDInceptionV3, check_image_size

        if kw:  # torchmetrics' Metric keywords (dist_sync_on_step, sync_on_compute, ...): nothing is silently ignored
            raise NotImplementedError(f"FrechetInceptionDistance: {sorted(kw)} not built")
        if isinstance(feature, nn.Module):
            raise NotImplementedError("FrechetInceptionDistance: a module as `feature` (a custom extractor) is not built")
        if not isinstance(feature, int) or isinstance(feature, bool) or feature != FEATURES:
            raise NotImplementedError(f"FrechetInceptionDistance: feature={feature!r} is not built, only the {FEATURES}-d pool feature "
                                      "(64, 192 and 768 tap earlier layers)")
        if not isinstance(reset_real_features, bool) or not isinstance(normalize, bool):
            raise ValueError("FrechetInceptionDistance: reset_real_features and normalize must be bools")
        check_image_size(tuple(input_img_size), "FrechetInceptionDistance")
        self.reset_real_features, self.normalize, self.num_features = reset_real_features, normalize, FEATURES
        self.inception = FIDInceptionV3(compute_dtype=compute_dtype, init_weights=feature_extractor_weights_path is None)
        if feature_extractor_weights_path is not None:
            self.inception.load_state_dict(torch.load(feature_extractor_weights_path, map_location="cpu", weights_only=True))
        self.acc = {True: None, False: None}  # real / generated: float64 [1 + D + D D] on the device, made by the first update

    def reset(self):
        self.acc[False] = None
        if self.reset_real_features:
            self.acc[True] = None

    @torch.no_grad()
    def update(self, imgs, real):
        """imgs: uint8 [B, 3, 299, 299], or floats in [0, 1] under normalize=True, on the device; real: which side they belong to"""
        self.inception.check_images(imgs, self.normalize)
        features = self.inception(imgs, normalize=self.normalize)
        self.update_features(features, real)

    def update_features(self, features, real):
        """the statistics step alone: features fp32 [B, 2048] on the device"""
        real, D = bool(real), self.num_features
        if self.acc[real] is None:
            self.acc[real] = torch.zeros(1 + D + D * D, dtype=torch.float64, device=features.device)
        elif self.acc[real].device != features.device:  # the metric was moved since: the statistics follow, nothing is dropped
            self.acc[real] = self.acc[real].to(features.device)
        chunk = 1024
        for i in range(0, features.shape[0], chunk):
            ops.fid_stats_accum(features[i:i + chunk].contiguous(), self.acc[real])

    def _moments(self, real):
        D, acc = self.num_features, self.acc[real]
        n = 0 if acc is None else int(acc[0].item())
        if n < 2:
            raise RuntimeError("FrechetInceptionDistance.compute(): more than one sample is required for both the real and the generated "
                               f"distribution ({n} {'real' if real else 'generated'})")
        host = acc.cpu()
        return moments_from_sums(n, host[1:1 + D], host[1 + D:].view(D, D))

    def compute(self):
        """the FID as a float32 scalar on the metric's device"""
        (mu1, s1), (mu2, s2) = self._moments(True), self._moments(False)
        return frechet_distance(mu1, s1, mu2, s2).to(torch.float32).to(self.acc[True].device)
