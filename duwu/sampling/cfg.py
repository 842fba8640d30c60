"""reference src/duwu/sampling/cfg.py: bind a prompt batch to the k-diffusion denoiser.  The reference returns closures; here the
same two functions return a ``uwudiff_amd.sampling.GuidedModel``, which is callable the same way (``model(x, sigma,
sigma_cond=None)`` -> ``(cfg_denoised, uncond_denoised)``) and which the fused sampling loops recognise."""
import torch
import torch.nn.functional as F

from uwudiff_amd.sampling import GuidedModel


def _time_ids(time_ids, height, width, rows, like):
    if time_ids is None:
        time_ids = torch.tensor([height, width, 0, 0, height, width]).repeat(rows, 1)
    return time_ids.to(like)


def cond_text_wrapper(prompt, width, height, unet, te, time_ids=None):
    """cfg.py:9-51: one conditional branch, no guidance."""
    emb, normed, pool, mask = te.encode(prompt, padding=True, truncation=True)
    if te.use_normed_ctx:
        emb = normed
    added = None
    if pool is not None:  # sdxl
        added = {"time_ids": _time_ids(time_ids, height, width, emb.size(0), emb), "text_embeds": pool}
    return GuidedModel(unet, emb, mask, added, guided=False)


def cfg_wrapper(prompt, neg_prompt, width, height, unet, te, cfg=5.0, time_ids=None):
    """cfg.py:54-127: the batch is [prompt rows, negative rows]; the shorter context (and its mask) is zero-padded."""
    emb, normed, pool, mask = te.encode(prompt, padding=True, truncation=True)
    neg, neg_normed, neg_pool, neg_mask = te.encode(neg_prompt, padding=True, truncation=True)
    if te.use_normed_ctx:
        emb, neg = normed, neg_normed
    added = None
    if pool is not None:  # sdxl
        ids = _time_ids(time_ids if time_ids is None else time_ids.repeat(2, 1), height, width, 2 * emb.size(0), emb)
        added = {"time_ids": ids, "text_embeds": torch.cat([pool, neg_pool])}
    gap = emb.size(1) - neg.size(1)
    if gap > 0:
        neg = F.pad(neg, (0, 0, 0, gap))
        neg_mask = F.pad(neg_mask, (0, gap)) if neg_mask is not None else None
    elif gap < 0:
        emb = F.pad(emb, (0, 0, 0, -gap))
        mask = F.pad(mask, (0, -gap)) if mask is not None else None
    both = torch.cat([mask, neg_mask]) if mask is not None and neg_mask is not None else None
    return GuidedModel(unet, torch.cat([emb, neg]), both, added, cfg=cfg, guided=True)
