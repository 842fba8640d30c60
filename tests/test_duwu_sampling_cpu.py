"""CPU: the host side of duwu.sampling -- sigma grids against the reference's recorded values, the shipped sampling config, the
sigma grid `diffusion_sampling` builds, `cfg_wrapper`'s assembly (ConcatTextEncoders' host path) and the argument errors."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, ROOT

YAML = os.path.join(ROOT, "configs", "sampling", "demo_sampling.yaml")


# ---------------------------------------------------------------------------------------------- sigma grids
def test_get_sigmas_for_rf_matches_the_reference_values():
    """tests/golden/get_sigmas_rf.npz (tests/make_golden_get_sigmas.py): the same float64 arithmetic on both sides -> 1e-12"""
    from duwu.sampling import get_sigmas as GS

    d = np.load(os.path.join(GOLDEN, "get_sigmas_rf.npz"))
    cases = d["cases"]
    assert len(cases) >= 5 and (cases[:, 2] == 0).any() and (cases[:, 3] == 10).any()
    for i, (steps, smax, smin, rho) in enumerate(cases):
        for disc in ("uniform_time", "sigmoid_time", "sigmoid_time_scale"):
            f = getattr(GS, disc)
            f = f if disc == "uniform_time" else functools.partial(f, rho=rho)
            got = GS.get_sigmas_for_rf(int(steps), smax, smin, f)
            assert got.dtype == np.float64 and got.shape == (int(steps) + 1,)
            np.testing.assert_allclose(got, d[f"{disc}_{i}"], rtol=1e-12, atol=0, err_msg=f"{disc} case {i}")
    # the reference's values as printed to eight decimals: half a unit of the last digit
    np.testing.assert_allclose(GS.get_sigmas_for_rf(4, 14.6146), [14.6146, 2.35534473, 0.87962395, 0.30546487, 0], rtol=0, atol=5e-9)
    np.testing.assert_allclose(GS.get_sigmas_for_rf(4, 14.6146, time_disc_func=GS.sigmoid_time_scale),
                               [14.6146, 6.71267407, 0.87962395, 0.07022162, 0], rtol=0, atol=5e-9)
    # the default discretisation is uniform_time
    assert np.array_equal(GS.get_sigmas_for_rf(7, 3.0, 0.1), GS.get_sigmas_for_rf(7, 3.0, 0.1, GS.uniform_time))


@pytest.mark.parametrize("num_steps", [1, 4, 24])
def test_diffusion_sampling_sigma_grid(num_steps):
    from duwu.sampling.sampling import sampling_sigmas
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    sched = EulerDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder="scheduler")
    s = sampling_sigmas(sched, num_steps)
    assert s.dtype == torch.float32 and s.shape == (num_steps + 1,)
    assert abs(float(s[0]) - 14.6146) < 5e-5 and float(s[-1]) == 0.0
    assert bool((s[1:] < s[:-1]).all())
    # a sample_scheduler replaces the table, a get_sigma_func replaces both
    other = EulerDiscreteScheduler(beta_start=0.001, beta_end=0.03)
    assert float(sampling_sigmas(sched, num_steps, other)[0]) == float(other.sigmas[0])
    from duwu.sampling.get_sigmas import get_sigmas_for_rf

    g = sampling_sigmas(sched, num_steps, other, functools.partial(get_sigmas_for_rf, max_sigma=14.6146))
    assert g.dtype == torch.float32 and g.shape == (num_steps + 1,) and abs(float(g[0]) - 14.6146) < 1e-5 and float(g[-1]) == 0.0


# ---------------------------------------------------------------------------------------------- the shipped config
def test_shipped_sampling_config_resolves():
    import duwu.sampling as DS
    from uwudiff_amd.config import get_obj_from_str, instantiate_any, load_yaml
    from uwudiff_amd.conditioning import ConcatTextEncoders
    from uwudiff_amd.unet import UNet2DConditionModel
    from uwudiff_amd.vae import AutoencoderKL

    cfg = load_yaml(YAML)
    fn = instantiate_any(cfg.sampling_func)
    assert isinstance(fn, functools.partial) and fn.func is DS.diffusion_sampling
    inner = fn.keywords["internal_sampling_func"]
    assert isinstance(inner, functools.partial) and inner.func is DS.sample_euler_ancestral and inner.keywords == {"eta": 0.0}
    assert fn.keywords["num_samples"] == 8 and fn.keywords["num_steps"] == 24 and fn.keywords["cfg_scale"] == 4
    assert (fn.keywords["width"], fn.keywords["height"], fn.keywords["seed"]) == (1024, 1024, 1215)
    assert len(fn.keywords["prompt"]) == len(fn.keywords["neg_prompt"]) == 4
    assert abs(float(fn.keywords["train_scheduler"].sigmas[0]) - 14.6146) < 5e-5
    mc = cfg.model_config
    # the targets resolve (nothing of SDXL size is constructed)
    assert mc.unet["_target_"] == "diffusers.UNet2DConditionModel.from_pretrained"
    unet_target = get_obj_from_str(mc.unet["_target_"])
    assert unet_target.__self__ is UNet2DConditionModel and unet_target.__func__ is UNet2DConditionModel.from_pretrained.__func__
    assert get_obj_from_str(mc.te["_target_"]) is ConcatTextEncoders
    assert get_obj_from_str(mc.vae["_target_"]).__self__ is AutoencoderKL
    for pair in mc.te.text_model_and_configs:
        assert callable(get_obj_from_str(pair[0]["_target_"]))
    for node in (mc.unet, mc.te, mc.vae):
        assert node["_load_config_"] == {"device": "cuda", "precision": "torch.float16", "to_freeze": True}
    assert sorted(DS.__all__ if hasattr(DS, "__all__") else [n for n in dir(DS) if n.startswith(("sample_", "diffusion_"))]) == [
        "diffusion_sampling", "sample_dpm2", "sample_dpm2_cfgpp", "sample_euler_ancestral", "sample_euler_ancestral_cfgpp"]


def test_unet_from_pretrained_takes_a_config_override():
    from uwudiff_amd.unet import TINY_UNET_CONFIG, UNet2DConditionModel

    with pytest.raises(ValueError):
        UNet2DConditionModel.from_pretrained("no/such-model", subfolder="unet")
    small = dict(TINY_UNET_CONFIG, in_channels=4, out_channels=4)
    torch.manual_seed(3)
    m = UNet2DConditionModel.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", subfolder="unet", config=small,
                                             torch_dtype=torch.float16)
    torch.manual_seed(3)
    ref = UNet2DConditionModel.from_config(small)
    assert m.cfg_dict == ref.cfg_dict and m.config.in_channels == 4 and list(m.registry) == list(ref.registry)
    assert torch.equal(m.flat, ref.flat) and bool(m.flat.any())  # seeded initialisation, as from_config
    sd = {k: torch.full_like(v, 0.25) for k, v in ref.state_dict().items()}
    m.load_state_dict({k[len("unet."):]: v for k, v in {"unet." + k: v for k, v in sd.items()}.items()})
    assert all(bool((v == 0.25).all()) for v in m.state_dict().values())


# ---------------------------------------------------------------------------------------------- cfg_wrapper
class _LongestTokenizer:
    """the synthetic tokenizer with `padding=True` honoured as transformers does (pad to the longest row of the call)"""

    def __init__(self, name):
        from uwudiff_amd.conditioning import SyntheticTokenizer

        self.inner = SyntheticTokenizer(name)
        self.model_max_length = self.inner.model_max_length

    def __call__(self, text, padding="max_length", **kw):
        out = self.inner(text, **kw)
        if padding is True:
            n = int(out["attention_mask"].sum(1).max())
            out = {k: v[:, :n] for k, v in out.items()}
        return out


def _encoders(pooled=True, use_normed_ctx=False):
    from uwudiff_amd.conditioning import ConcatTextEncoders, SyntheticCLIPTextModel

    pairs = [(SyntheticCLIPTextModel(hidden=32, seed=1), dict(layer_idx=-2, need_mask=True)),
             (SyntheticCLIPTextModel(hidden=48, seed=2), dict(layer_idx=-2, use_pooled=pooled))]
    te = ConcatTextEncoders(["a", "b"], pairs, zero_for_padding=True, use_normed_ctx=use_normed_ctx)
    te.tokenizers = [_LongestTokenizer("a"), _LongestTokenizer("b")]
    return te


PROMPTS = ["a cat", "a photograph of an astronaut riding a horse", "dogs with pumpkins and a few more words after them"]


@pytest.mark.parametrize("use_normed_ctx", [False, True])
def test_cfg_wrapper_assembles_the_guidance_batch(use_normed_ctx):
    from duwu.sampling.cfg import cfg_wrapper
    from uwudiff_amd.sampling import GuidedModel

    te = _encoders(use_normed_ctx=use_normed_ctx)
    emb, normed, pool, mask = te.encode(PROMPTS, padding=True, truncation=True)
    nemb, nnormed, npool, nmask = te.encode([""] * 3, padding=True, truncation=True)
    assert emb.shape[1] == 12 and nemb.shape[1] == 2  # bos + 10 words + eos against bos + eos
    m = cfg_wrapper(PROMPTS, [""] * 3, width=48, height=64, unet=None, te=te, cfg=4)
    assert isinstance(m, GuidedModel) and m.guided and m.cfg == 4.0
    ids = m.added_cond["time_ids"]
    assert tuple(ids.shape) == (6, 6) and ids.dtype == emb.dtype
    assert torch.equal(ids, torch.tensor([[64.0, 48, 0, 0, 64, 48]] * 6))
    assert torch.equal(m.added_cond["text_embeds"], torch.cat([pool, npool]))
    want, nwant = (normed, nnormed) if use_normed_ctx else (emb, nemb)
    assert tuple(m.context.shape) == (6, 12, 80) and tuple(m.mask.shape) == (6, 12)
    assert torch.equal(m.context[:3], want) and torch.equal(m.context[3:, :2], nwant)
    assert not bool(m.context[3:, 2:].any()) and not bool(m.mask[3:, 2:].any())
    assert torch.equal(m.mask[:3], mask) and torch.equal(m.mask[3:, :2], nmask)
    assert not torch.equal(emb, normed)
    # the other way round: the prompt side is the shorter one
    r = cfg_wrapper([""] * 3, PROMPTS, width=48, height=64, unet=None, te=te)
    assert r.cfg == 5.0 and torch.equal(r.context[3:], want) and not bool(r.context[:3, 2:].any()) and not bool(r.mask[:3, 2:].any())
    # caller-supplied time_ids are repeated for both halves
    mine = torch.tensor([[1.0, 2, 3, 4, 5, 6]] * 3)
    assert torch.equal(cfg_wrapper(PROMPTS, [""] * 3, 48, 64, None, te, time_ids=mine).added_cond["time_ids"], mine.repeat(2, 1))


def test_wrappers_without_a_pooled_output():
    from duwu.sampling.cfg import cfg_wrapper, cond_text_wrapper

    te = _encoders(pooled=False)
    assert cfg_wrapper(PROMPTS, [""] * 3, 64, 64, None, te).added_cond is None
    single = cond_text_wrapper(PROMPTS, 64, 64, None, te)
    assert single.added_cond is None and not single.guided and tuple(single.context.shape) == (3, 12, 80)
    with_pool = cond_text_wrapper(PROMPTS, 48, 64, None, _encoders())
    assert tuple(with_pool.added_cond["time_ids"].shape) == (3, 6) and tuple(with_pool.added_cond["text_embeds"].shape) == (3, 48)


# ---------------------------------------------------------------------------------------------- argument errors
def test_samplers_refuse_what_is_not_built():
    import duwu.sampling as DS
    from duwu.sampling.cfg import cfg_wrapper

    x, sigmas = torch.zeros(1, 4, 8, 8), torch.tensor([2.0, 1.0, 0.0])
    for fn in (DS.sample_euler_ancestral, DS.sample_euler_ancestral_cfgpp, DS.sample_dpm2, DS.sample_dpm2_cfgpp):
        with pytest.raises(TypeError, match="cfg_wrapper.*cond_text_wrapper"):
            fn(lambda x, sigma, **kw: (x, x), x, sigmas)
        model = cfg_wrapper(PROMPTS, [""] * 3, 64, 64, None, _encoders())
        with pytest.raises(NotImplementedError):
            fn(model, x, sigmas, image_to_noise=True)
    from duwu.sampling.k_diffusion_wrapper import DiscreteEpsDDPMDenoiser
    from uwudiff_amd import sampling

    assert DiscreteEpsDDPMDenoiser is sampling.DiscreteEpsDDPMDenoiser
