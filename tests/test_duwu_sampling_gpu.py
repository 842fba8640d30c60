"""GPU: the prompt-to-image path -- the four glue kernels against exact / fp64 references, `diffusion_sampling`
end to end against the CPU oracles (oracle/unet.py, tests/clip_oracle.py, tests/vae_oracle.py, oracle/sampling.py), and the
train -> checkpoint -> `test_scripts/test_sampling.py` round trip."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import clip_oracle, vae_oracle
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _lib():
    from uwudiff_amd import lib as L

    return L


def _philox_normal(n, seed, offset):
    L = _lib()
    out = torch.empty(n, device="cuda")
    L.call("uwu_philox_normal", L.ptr(out), n, seed, offset, L.stream())
    return out


# ---------------------------------------------------------------------------------------------- uwu_cfg_input
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (1, 4, 3, 3)])
def test_cfg_input_is_both_halves_of_the_scaled_input(shape):
    L = _lib()
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g) * 14.6
    c_in = 1.0 / math.sqrt(14.6146 ** 2 + 1.0)
    xd = x.cuda()
    y = torch.full((2 * shape[0],) + shape[1:], float("nan"), device="cuda")
    L.call("uwu_cfg_input", L.ptr(xd), L.ptr(y), shape[0], x[0].numel(), c_in, L.stream())
    want = (x.numpy() * np.float32(c_in)).astype(np.float32)
    got = y.cpu().numpy()
    assert np.array_equal(got[: shape[0]].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[shape[0]:].view(np.uint32), want.view(np.uint32))
    assert torch.equal(xd.cpu(), x)
    with pytest.raises(L.UwuError):  # B * n must be a multiple of 4
        L.call("uwu_cfg_input", L.ptr(xd), L.ptr(y), 1, 35, c_in, L.stream())


# ---------------------------------------------------------------------------------------------- uwu_sampler_combine_draw
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
@pytest.mark.parametrize("offset", [0, 12, 2 ** 32 - 8])
def test_combine_draw_is_philox_normal_then_combine(offset, guided):
    """bit-equal to the two entries it fuses; 192 counters from 2^32 - 8 cross the carry into the counter's high word"""
    L = _lib()
    shape, seed = (3, 4, 8, 8), 1215
    g = torch.Generator().manual_seed(offset % 97 + guided)
    base, ec, eu = [torch.randn(shape, generator=g).cuda() for _ in range(3)]
    eu = eu if guided else None
    n = base.numel()
    cfg, a, b, c = 4.0, -3.2, 1.7, 0.6
    noise = _philox_normal(n, seed, offset)
    want, got = torch.empty_like(base), torch.full_like(base, float("nan"))
    L.call("uwu_sampler_combine", L.ptr(base), L.ptr(ec), L.ptr(eu), L.ptr(noise), L.ptr(want), n, cfg, a, b, c, L.stream())
    L.call("uwu_sampler_combine_draw", L.ptr(base), L.ptr(ec), L.ptr(eu), L.ptr(got), n, cfg, a, b, c, seed, offset, L.stream())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, base)


def test_combine_draw_refuses_odd_sizes_and_reservations_do_not_overlap():
    from uwudiff_amd.sampling import reserve_noise

    L = _lib()
    x = torch.randn(144, device="cuda")
    out = torch.empty_like(x)
    with pytest.raises(L.UwuError):
        L.call("uwu_sampler_combine_draw", L.ptr(x), L.ptr(x), None, L.ptr(out), 142, 1.0, 1.0, 0.0, 1.0, 1, 0, L.stream())
    with pytest.raises(L.UwuError):
        reserve_noise(x.device, 142)
    torch.manual_seed(5)
    n = 3 * 4 * 8 * 8
    (s0, o0), (s1, o1) = reserve_noise(x.device, n), reserve_noise(x.device, n)
    assert s0 == s1 == 5 and o1 >= o0 + n // 4  # one counter per four elements
    both = _philox_normal(2 * n, s0, o0)
    assert torch.equal(_philox_normal(n, s0, o0), both[:n])
    if o1 == o0 + n // 4:  # back to back: the second draw continues the first one's stream
        assert torch.equal(_philox_normal(n, s1, o1), both[n:])
    torch.manual_seed(5)
    assert reserve_noise(x.device, n) == (s0, o0)


# ---------------------------------------------------------------------------------------------- uwu_latent_finish
@pytest.mark.parametrize("rescale", [True, False], ids=["rescale", "plain"])
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 4, 16, 16)])
def test_latent_finish_matches_fp64_and_is_batch_invariant(shape, rescale):
    from uwudiff_amd.sampling import latent_finish

    g = torch.Generator().manual_seed(shape[-1])
    # positive values: y = x / std * 13.3 + 1.125 then has no cancellation, so a relative bound with no absolute term is well posed,
    # and the mean (about 1.7 deviations) is one that an E[x^2] - E[x]^2 reduction would lose digits to
    x = torch.randn(shape, generator=g).abs() * 3.0 + 0.7
    xd = x.cuda()
    y = latent_finish(xd, rescale, 13.3, 1.125)
    x64 = x.double()
    want = (x64 / x64.std([1, 2, 3], keepdim=True) if rescale else x64) * 13.3 + 1.125
    assert y.dtype == torch.float32 and y.shape == x.shape and torch.equal(xd.cpu(), x)
    err = ((y.cpu().double() - want).abs() / want.abs()).max().item()
    print(f"[latent_finish {shape} rescale={rescale}] max relative error {err:.3e}")
    torch.testing.assert_close(y.cpu().double(), want, rtol=1e-5, atol=0)
    if shape[0] == 3:  # sample 1 alone: the same bits as inside the batch
        alone = latent_finish(xd[1:2].contiguous(), rescale, 13.3, 1.125)
        assert torch.equal(alone[0].view(torch.int32), y[1].view(torch.int32))


def test_latent_finish_spans_several_workgroups():
    """n = 4 * 40 * 40 = 6400 > one 4096-element chunk, the last chunk partial"""
    from uwudiff_amd.sampling import latent_finish

    L = _lib()
    x = torch.randn(3, 4, 40, 40, generator=torch.Generator().manual_seed(3)).abs() * 2.0 + 0.5  # positive, as above
    y = latent_finish(x.cuda(), True, 13.3, 1.125)
    x64 = x.double()
    torch.testing.assert_close(y.cpu().double(), x64 / x64.std([1, 2, 3], keepdim=True) * 13.3 + 1.125, rtol=1e-5, atol=0)
    assert torch.equal(latent_finish(x[1:2].cuda(), True, 13.3, 1.125)[0], y[1])
    xd = x.cuda()
    with pytest.raises(L.UwuError):  # rescale without its workspace
        L.call("uwu_latent_finish", L.ptr(xd), L.ptr(y), 3, 6400, 1, 1.0, 0.0, None, 0, L.stream())
    with pytest.raises(L.UwuError):
        L.call("uwu_latent_finish", L.ptr(xd), L.ptr(y), 3, 6398, 0, 1.0, 0.0, None, 0, L.stream())


# ---------------------------------------------------------------------------------------------- uwu_image_u8
def _image_values(dtype):
    """a linspace over [-1.5, 1.5], every level boundary k / 127.5 - 1 and its two fp32 neighbours (865 values, shuffled)"""
    k = np.arange(256, dtype=np.float64)
    edges = (k / 127.5 - 1.0).astype(np.float32)
    vals = np.concatenate([np.linspace(-1.5, 1.5, 97, dtype=np.float32), edges, np.nextafter(edges, np.float32(-2)),
                           np.nextafter(edges, np.float32(2))])
    return torch.from_numpy(np.random.default_rng(0).permutation(vals)).to(dtype)


def _postprocess_numpy(x):
    """vae_image_postprocess (data/utils.py:10-19) in fp32, in its order: [B, 3, H, W] -> uint8 [B, H, W, 3]"""
    v = x.float().cpu().numpy().astype(np.float32)
    v = (v * np.float32(0.5) + np.float32(0.5)) * np.float32(255)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)


def test_postprocess_formula_truncates():
    x = torch.tensor([-1.0, 1.0, 0.0, 0.999, 1 / 127.5 - 1, -7.0, 7.0]).float().view(1, 1, 1, 7).expand(1, 3, 1, 7)
    assert _postprocess_numpy(x)[0, 0, :, 0].tolist() == [0, 255, 127, 254, 0, 0, 255]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 8, 12), (1, 3, 64, 20)])
def test_image_u8_is_the_reference_formula(shape, dtype):
    """(2, 3, 5, 7): H * W = 35 is odd, groups of four pixels straddle the two images and the stream ends on a partial group;
    (1, 3, 8, 12): the vector-load path; (1, 3, 64, 20): the vector path over more than one workgroup"""
    from uwudiff_amd.sampling import image_u8

    vals, numel = _image_values(dtype), int(np.prod(shape))
    for start in range(0, len(vals), numel):  # as many tensors of this shape as hold every value once (the last one wraps around)
        x = vals[torch.arange(start, start + numel) % len(vals)].view(shape)
        got = image_u8(x.cuda())
        assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[2], shape[3], 3)
        assert np.array_equal(got.cpu().numpy(), _postprocess_numpy(x)), start


# ---------------------------------------------------------------------------------------------- end to end
UNET = dict(in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=1,
            down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"),
            transformer_layers_per_block=(1, 2), attention_head_dim=(1, 1), cross_attention_dim=256,
            addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=128 + 6 * 8,
            norm_num_groups=8)  # tests/test_unet_gpu.py TINY at the width of the two text encoders below
# tests/test_text_model_gpu.py's tiny pair at the vocabulary of the tokenizer (ids up to 49407, eos = pad = 49407)
CLIPS = [dict(clip_oracle.TINY_QUICK, vocab_size=49408), dict(clip_oracle.TINY_GELU, vocab_size=49408, eos_token_id=49407)]
VAE = dict(block_out_channels=(32, 32, 64, 64), layers_per_block=1, mid_block_add_attention=False)  # tests/test_vae_cpu.py's, 8x
PROMPTS, NEGATIVES = ["a cat sitting on a table", "a photograph of an astronaut riding a horse"], ["", "blurry"]
RUN = dict(num_steps=4, num_samples=3, padding_mode="cycling", cfg_scale=4.0, width=64, height=64)


class _Stack:
    """the CPU oracles and, per compute dtype, the native models holding the same weights"""

    def __init__(self):
        from oracle.unet import UNetOracle

        torch.manual_seed(1215)
        self.unet = UNetOracle(**UNET)
        with torch.no_grad():  # tests/test_unet_gpu.py run_pair: away from the near-zero init so every branch carries signal
            for n, p in self.unet.named_parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn_like(p) * (0.5 / p[0].numel() ** 0.5))
                elif n.endswith("bias"):
                    p.copy_(torch.randn_like(p) * 0.05)
                else:
                    p.copy_(1 + torch.randn_like(p) * 0.1)
        self.clip_sd = [clip_oracle.random_state_dict(c, seed=31 + i) for i, c in enumerate(CLIPS)]
        self.vae = vae_oracle.AutoencoderKL(**VAE).eval()
        self._native = {}

    def native(self, dtype):
        if dtype not in self._native:
            from uwudiff_amd.conditioning import ConcatTextEncoders
            from uwudiff_amd.text_model import CLIPTextModel
            from uwudiff_amd.unet import UNet2DConditionModel
            from uwudiff_amd.vae import AutoencoderKL

            unet = UNet2DConditionModel(UNET, compute_dtype=dtype, init_weights=False)
            unet.load_state_dict(self.unet.state_dict())
            pairs = []
            for i, (cfg, sd) in enumerate(zip(CLIPS, self.clip_sd)):
                m = CLIPTextModel.from_config(cfg, compute_dtype=dtype, init_weights=False)
                m.load_state_dict(sd)
                pairs.append((m, dict(concat_bucket=0, layer_idx=-2, use_pooled=i == 1, need_mask=False)))
            te = ConcatTextEncoders(tokenizers=["a", "b"], text_model_and_configs=pairs, zero_for_padding=False)
            vae = AutoencoderKL.from_pretrained(dict(VAE), compute_dtype=dtype, init_weights=False)
            vae.load_state_dict(self.vae.state_dict())
            self._native[dtype] = (unet.cuda().eval(), te.cuda().eval(), vae.cuda().eval())
        return self._native[dtype]

    def sample(self, dtype, seed=1215, eta=1.0, **kw):
        from functools import partial

        from duwu.sampling import diffusion_sampling, sample_euler_ancestral
        from uwudiff_amd.scheduler import EulerDiscreteScheduler

        unet, te, vae = self.native(dtype)
        trace = {}
        images = diffusion_sampling(unet=unet, te=te, vae=vae, train_scheduler=EulerDiscreteScheduler.from_pretrained("sdxl"),
                                    prompt=PROMPTS, neg_prompt=NEGATIVES, seed=seed, trace=trace,
                                    internal_sampling_func=partial(sample_euler_ancestral, eta=eta), **dict(RUN, **kw))
        return images, trace

    def context(self, prompts):
        """ConcatTextEncoders' rule (text_encoders.py:139-264) on the CLIP oracle: hidden_states[-2] of both models side by side,
        the pooled vector of the second; no mask and no zeroing (need_mask = zero_for_padding = False)"""
        from uwudiff_amd.conditioning import SyntheticTokenizer

        embs, pooled = [], None
        for i, (cfg, sd) in enumerate(zip(CLIPS, self.clip_sd)):
            tok = SyntheticTokenizer("ab"[i])(prompts)
            out = clip_oracle.forward(sd, cfg, tok["input_ids"], tok["attention_mask"])
            embs.append(out["hidden_states"][-2])
            pooled = out["pooled"] if i == 1 else pooled
        return torch.cat(embs, -1).float(), pooled.float()


@pytest.fixture(scope="module")
def stack():
    return _Stack()


@pytest.fixture(scope="module")
def fp32_run(stack):
    return stack.sample("fp32")


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


def test_sampling_fp32_matches_the_cpu_oracles(stack, fp32_run):
    from duwu.utils import truncate_or_pad_to_length
    from oracle import sampling as OS
    from uwudiff_amd.sampling import DiscreteEpsDDPMDenoiser
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    images, trace = fp32_run
    B, n = RUN["num_samples"], RUN["num_samples"] * 4 * 8 * 8
    sigmas = trace["sigmas"]
    assert len(sigmas) == 5 and float(sigmas[-1]) == 0.0
    draws = trace["noise_draws"]
    assert [d[0] for d in draws] == [0, 1, 2] and len({d[1] for d in draws}) == 1  # the last step (sigma_next = 0) draws nothing
    assert all(b[2] >= a[2] + n // 4 for a, b in zip(draws, draws[1:]))
    noises = [_philox_normal(n, seed, off).cpu().view(B, 4, 8, 8) for _, seed, off in draws] + [None]
    ctx, pool = stack.context(truncate_or_pad_to_length(PROMPTS, B, "cycling"))
    nctx, npool = stack.context(truncate_or_pad_to_length(NEGATIVES, B, "cycling"))
    ids = torch.tensor([[64.0, 64, 0, 0, 64, 64]] * B)
    kw = lambda c, p: {"encoder_hidden_states": c, "added_cond_kwargs": {"text_embeds": p, "time_ids": ids}}  # noqa: E731
    log_sigmas = DiscreteEpsDDPMDenoiser(None, EulerDiscreteScheduler.from_pretrained("sdxl").alphas_cumprod).log_sigmas
    ref = OS.sample_euler_ancestral_cfg(stack.unet, trace["init_x"], sigmas, log_sigmas, kw(ctx, pool), kw(nctx, npool), 4.0, noises,
                                        eta=1.0)
    l2, mx = _rel(trace["latents"], ref)
    print(f"[sampling fp32] final latents: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
    with torch.no_grad():
        img = stack.vae.double().decode(ref.double() / stack.vae.scaling_factor)
    stack.vae.float()
    d2, dm = _rel(trace["decoded"], img)
    print(f"[sampling fp32] decoded images: rel L2 {d2:.3e}, max-abs / max-abs {dm:.3e}")
    assert l2 < 1e-3, (l2, mx)
    assert d2 <= 1e-3 and dm <= 1e-3, (d2, dm)
    # the PIL images are the reference's post-processing of the decoded tensor, byte for byte
    assert len(images) == 3 and all(im.mode == "RGB" and im.size == (64, 64) for im in images)
    want = _postprocess_numpy(trace["decoded"])
    assert all(np.array_equal(np.asarray(im), w) for im, w in zip(images, want))


def test_sampling_follows_the_seed(stack, fp32_run):
    images, trace = fp32_run
    again, trace2 = stack.sample("fp32")
    assert torch.equal(trace["latents"], trace2["latents"])
    assert [im.tobytes() for im in again] == [im.tobytes() for im in images]
    other, _ = stack.sample("fp32", seed=7)
    assert [im.tobytes() for im in other] != [im.tobytes() for im in images]


def test_sampling_rescale_and_the_other_samplers_run(stack):
    from functools import partial

    import duwu.sampling as DS

    images, trace = stack.sample("fp32", rescale=True, vae_std=13.3, vae_mean=1.125)
    assert len(images) == 3 and bool(torch.isfinite(trace["decoded"]).all())
    unet, te, vae = stack.native("fp32")
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    sched = EulerDiscreteScheduler.from_pretrained("sdxl")
    for fn in (DS.sample_euler_ancestral_cfgpp, DS.sample_dpm2, partial(DS.sample_dpm2, s_churn=2.0), DS.sample_dpm2_cfgpp):
        t = {}
        out = DS.diffusion_sampling(unet=unet, te=te, vae=vae, train_scheduler=sched, prompt=PROMPTS, neg_prompt=NEGATIVES,
                                    internal_sampling_func=fn, trace=t, **dict(RUN, num_steps=2))
        assert len(out) == 3 and bool(torch.isfinite(t["latents"]).all()), fn


def test_guided_model_call_returns_the_denoised_pair(stack):
    """the object of cfg_wrapper called as the reference's closure: (cfg_denoised, uncond_denoised) = x - sigma eps, and the
    unguided object of cond_text_wrapper returns (denoised, None)"""
    from duwu.sampling.cfg import cfg_wrapper, cond_text_wrapper
    from uwudiff_amd.sampling import DiscreteEpsDDPMDenoiser
    from uwudiff_amd.scheduler import EulerDiscreteScheduler

    unet, te, _ = stack.native("fp32")
    den = DiscreteEpsDDPMDenoiser(unet, EulerDiscreteScheduler.from_pretrained("sdxl").alphas_cumprod)
    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(2)).cuda() * 3
    sigma = torch.full((2,), 2.5)
    model = cfg_wrapper(PROMPTS, NEGATIVES, 64, 64, den, te, cfg=4.0)
    cfg_den, unc_den = model(x, sigma)
    eps_c, eps_u = model.eps(x, 2.5)
    torch.testing.assert_close(unc_den, x - 2.5 * eps_u, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cfg_den, x - 2.5 * (eps_u + (eps_c - eps_u) * 4.0), rtol=1e-5, atol=1e-4)
    single = cond_text_wrapper(PROMPTS, 64, 64, den, te)
    den1, none = single(x, sigma)
    assert none is None
    torch.testing.assert_close(den1, x - 2.5 * eps_c, rtol=1e-4, atol=1e-4)  # the same branch evaluated in a batch of 2, not 4


def test_sampling_bf16_runs(stack):
    """shape and finiteness only: there is no bf16 bar for a multi-step run"""
    images, trace = stack.sample("bf16")
    assert len(images) == 3 and all(im.mode == "RGB" and im.size == (64, 64) for im in images)
    assert tuple(trace["latents"].shape) == (3, 4, 8, 8) and bool(torch.isfinite(trace["latents"]).all())
    assert tuple(trace["decoded"].shape) == (3, 3, 64, 64) and bool(torch.isfinite(trace["decoded"]).all())


# ---------------------------------------------------------------------------------------------- train, checkpoint, sample
def test_train_checkpoint_then_sample_through_the_launcher(tmp_path):
    from PIL import Image

    from duwu.loader import load_all, load_any
    from duwu.utils import instantiate_any
    from uwudiff_amd.config import load_yaml, merge
    from uwudiff_amd.engine import Fitter, seed_everything
    from uwudiff_amd.unet import TINY_UNET_CONFIG

    unet_cfg = {k: list(v) if isinstance(v, tuple) else v for k, v in dict(TINY_UNET_CONFIG, in_channels=4, out_channels=4,
                                                                           sample_size=8).items()}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml")),
                {"lightning_config": {"fast_dev_run": False, "max_steps": 2, "log_every_n_steps": 1},
                 "data": {"dataset_config": {"sample_size": [4, 8, 8], "n_samples": 8},
                          "dataloader_config": {"batch_size": 4, "num_workers": 0}},
                 "trainer": {"lr": 1e-3, "model_config": {"unet": {"config": unet_cfg, "cond_dim": None}}}})
    del cfg["trainer"]["model_config"]["unet"]["cond_dim"]
    seed_everything(cfg.seed)
    fit = Fitter(**cfg["lightning_config"])
    dm, tr = load_all(cfg)
    fit.fit(tr, dm)
    assert fit.global_step == 2
    ckpt = str(tmp_path / "step2.ckpt")
    fit.save_checkpoint(ckpt)
    trained = {k: v.detach().clone() for k, v in tr.unet.state_dict().items()}

    out_dir = tmp_path / "images"
    override = {"save_dir": str(out_dir),
                "sampling_func": {"num_samples": 2, "num_steps": 2, "width": 64, "height": 64},
                "model_config": {"unet": {"config": unet_cfg,
                                          "_load_config_": {"ckpt_path": ckpt, "state_dict_key": "state_dict", "state_dict_prefix": "unet."}},
                                 "vae": {"pretrained_model_name_or_path": {k: list(v) if isinstance(v, tuple) else v for k, v in VAE.items()}}}}
    opath = tmp_path / "override.yaml"
    opath.write_text(yaml.safe_dump(override))
    shipped = os.path.join(ROOT, "configs", "sampling", "demo_sampling.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test_scripts", "test_sampling.py"), "--configs", shipped, str(opath)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = [out_dir / f"{i}.png" for i in range(2)]
    assert sorted(p.name for p in out_dir.iterdir()) == ["0.png", "1.png"]
    child = [np.asarray(Image.open(p).convert("RGB")) for p in files]
    assert all(c.shape == (64, 64, 3) for c in child)

    # the same sampling in this process: the denoiser holds the checkpoint's weights and gives the child's images, byte for byte;
    # without the checkpoint (seeded initial weights) it gives other images.  The VAE's stand-in weights follow
    # torch.initial_seed(), so the models are built under the seed the launcher builds them under
    merged = merge(load_yaml(shipped), load_yaml(str(opath)))
    seed_everything(merged.sampling_func.seed)
    unet = load_any(merged.model_config.unet)
    loaded = unet.state_dict()
    assert sorted(loaded) == sorted(trained) and all(torch.equal(loaded[k], v) for k, v in trained.items())
    assert not unet.flat.requires_grad
    te, vae = load_any(merged.model_config.te), load_any(merged.model_config.vae)
    here = instantiate_any(merged.sampling_func)(unet=unet, te=te, vae=vae)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(here, child))
    del merged["model_config"]["unet"]["_load_config_"]["ckpt_path"]
    fresh = load_any(merged.model_config.unet)
    assert not all(torch.equal(v, trained[k]) for k, v in fresh.state_dict().items())
    other = instantiate_any(merged.sampling_func)(unet=fresh, te=te, vae=vae)
    assert any(not np.array_equal(np.asarray(a), b) for a, b in zip(other, child))
