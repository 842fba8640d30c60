"""Time prompt-to-image sampling (duwu.sampling.diffusion_sampling) at the SDXL shape on one GPU.

    python tools/bench_sampling.py [--family sdxl] [--sizes 1024 256] [--samples 8] [--steps 24] [--runs 3] [--warmup 1] [--json]
    python tools/bench_sampling.py --family sd15        # the Stable Diffusion 1.x-shape stack at 512 and 256, guidance 7

The models are the nodes of configs/sampling/demo_sampling.yaml (seeded SDXL-shape UNet in bf16, the YAML's text encoders, the
SDXL VAE) or, with --family sd15, of configs/sampling/demo_sampling_sd.yaml; the UNet's initial weights are drawn on the device.  Per size: --warmup runs, then --runs timed runs, the median of each
figure.  A run is the pipeline of diffusion_sampling with device events placed around its stages:

  text encoding        cfg_wrapper (both prompt lists through the text encoders, context assembly)
  sampler step         the loop's wall time / steps (host clock between two device synchronisations), split into
      denoiser forward     device events around every call of the eps model (the batch of 2 x samples)
      glue kernels         device events around every uwu_cfg_input / uwu_sampler_combine[_draw] launch of the loop
      everything else      the step time minus the two rows above: launch gaps and host time
  finish               uwu_latent_finish
  decode               the --samples VAE decodes, one latent each
  post-processing      uwu_image_u8 and the one device-to-host copy
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# per family: the sampling YAML, the default --sizes
FAMILIES = {"sdxl": ("demo_sampling.yaml", [1024, 256]), "sd15": ("demo_sampling_sd.yaml", [512, 256])}
GLUE = ("uwu_cfg_input", "uwu_sampler_combine", "uwu_sampler_combine_draw", "uwu_scale_copy")


class _Spans:
    """pairs of device events, summed after one synchronisation"""

    def __init__(self):
        self.pairs = {}

    def span(self, name):
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.setdefault(name, []).append((e0, e1))
        e0.record()
        return e1

    def total(self, name):
        return sum(a.elapsed_time(b) for a, b in self.pairs.get(name, []))


class _TimedLib:
    """uwudiff_amd.lib with events around the launches of the glue kernels (the module the sampling loops call through)"""

    def __init__(self, lib, spans):
        self._lib, self._spans = lib, spans

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def call(self, name, *args):
        if name not in GLUE:
            return self._lib.call(name, *args)
        end = self._spans.span("glue")
        self._lib.call(name, *args)
        end.record()


def one_run(models, sched, prompts, negatives, size, samples, steps, cfg_scale=4.0, eta=0.0):
    import torch

    from duwu.sampling.cfg import cfg_wrapper
    from duwu.utils import truncate_or_pad_to_length
    from duwu.sampling.sampling import sampling_sigmas
    from uwudiff_amd import lib as L
    from uwudiff_amd import sampling as S

    unet, te, vae = models
    spans = _Spans()
    den = S.DiscreteEpsDDPMDenoiser(unet, sched.alphas_cumprod)
    inner_eps = den.eps

    def timed_eps(*a, **kw):
        end = spans.span("forward")
        out = inner_eps(*a, **kw)
        end.record()
        return out

    den.eps = timed_eps
    torch.manual_seed(1215)
    end = spans.span("text")
    model = cfg_wrapper(truncate_or_pad_to_length(prompts, samples, "cycling"), truncate_or_pad_to_length(negatives, samples, "cycling"),
                        size, size, den, te, cfg=cfg_scale)
    end.record()
    sigmas = sampling_sigmas(sched, steps)
    x = (torch.randn(samples, 4, size // 8, size // 8) * torch.sqrt(1 + sigmas[0] ** 2)).cuda()
    torch.cuda.synchronize()
    S.L = _TimedLib(L, spans)
    try:
        t0 = time.perf_counter()
        latents = S.guided_euler_ancestral(model, x, sigmas, eta=eta)
        torch.cuda.synchronize()
        loop_ms = (time.perf_counter() - t0) * 1e3
    finally:
        S.L = L
    end = spans.span("finish")
    z = S.latent_finish(latents, False, 1 / vae.config.scaling_factor, 0.0)
    end.record()
    end = spans.span("decode")
    img = torch.cat([vae.decode(z[i:i + 1]).sample for i in range(samples)])
    end.record()
    end = spans.span("post")
    pixels = S.image_u8(img).cpu()
    end.record()
    torch.cuda.synchronize()
    assert tuple(pixels.shape) == (samples, size, size, 3)
    fwd, glue = spans.total("forward") / steps, spans.total("glue") / steps
    return dict(text_ms=spans.total("text"), step_ms=loop_ms / steps, forward_ms=fwd, glue_ms=glue, other_ms=loop_ms / steps - fwd - glue,
                finish_ms=spans.total("finish"), decode_ms=spans.total("decode"), post_ms=spans.total("post"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), default="sdxl")
    ap.add_argument("--sizes", type=int, nargs="+", default=None, help="default: 1024 256 (sdxl), 512 256 (sd15)")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--eta", type=float, default=0.0, help="0: the shipped config (no noise); 1: every step but the last draws noise")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch

    from duwu.loader import load_any
    from duwu.utils import instantiate_any
    from uwudiff_amd.config import load_yaml

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_name, sizes = FAMILIES[args.family]
    cfg = load_yaml(os.path.join(root, "configs", "sampling", yaml_name))
    cfg.model_config.unet["device"] = "cuda"  # draw the initial weights (2.6 G at the SDXL shape) on the device
    models = tuple(load_any(cfg.model_config[k]) for k in ("unet", "te", "vae"))
    sched = instantiate_any(cfg.sampling_func.train_scheduler)
    prompts, negatives = list(cfg.sampling_func.prompt), list(cfg.sampling_func.neg_prompt)
    rows = []
    cfg_scale = 4.0 if args.family == "sdxl" else float(cfg.sampling_func.cfg_scale)
    for size in args.sizes or sizes:
        runs = [one_run(models, sched, prompts, negatives, size, args.samples, args.steps, cfg_scale=cfg_scale, eta=args.eta)
                for _ in range(args.warmup + args.runs)][args.warmup:]
        row = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        row.update(size=size, samples=args.samples, steps=args.steps, eta=args.eta, runs=args.runs, warmup=args.warmup)
        rows.append(row)
        torch.cuda.empty_cache()
    if args.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print(f"{r['size']} x {r['size']}, {r['samples']} samples, {r['steps']} steps (eta {r['eta']}; median of {r['runs']} after {r['warmup']}):")
        print(f"    text encoding      {r['text_ms']:10.2f} ms")
        print(f"    sampler step       {r['step_ms']:10.2f} ms = denoiser forward {r['forward_ms']:.2f} + glue kernels {r['glue_ms']:.3f} + "
              f"everything else {r['other_ms']:.2f}")
        print(f"    latent finish      {r['finish_ms']:10.3f} ms")
        print(f"    {r['samples']} decodes          {r['decode_ms']:10.2f} ms")
        print(f"    post-processing    {r['post_ms']:10.2f} ms (uwu_image_u8 + the device-to-host copy)")


if __name__ == "__main__":
    main()
