"""AutoencoderKL (the SDXL VAE) on the HIP kernels: frozen, inference only.

The reference's first shipped config pushes every batch of pixels through ``diffusers.AutoencoderKL.encode(x).latent_dist
.sample()`` (reference src/duwu/trainer/trainer.py:241-244) and decodes with the same class at the end of sampling
(src/duwu/sampling/sampling.py:116-119).  This module restates that model from its public description -- encoder: conv_in,
four DownEncoderBlock2D (two time-embedding-free ResnetBlock2D each, a right/bottom-padded stride-2 convolution after all
but the last), mid block (resnet, one-head attention, resnet), GroupNorm + SiLU + conv_out, 1x1 quant_conv; decoder:
post_quant_conv, conv_in, the same mid block, four UpDecoderBlock2D (three resnets, nearest 2x + convolution after all but the
last), GroupNorm + SiLU + conv_out -- keeps diffusers' parameter names in ``state_dict()`` and runs every operator through
``libuwu_hip.so``:

  * activations stay channels-last ``[B*H*W, C]`` in the compute dtype between kernels; 3x3 convolutions are the implicit
    GEMM of the UNet (``uwu_conv3x3_fwd``), the encoder's downsampler is ``uwu_conv3x3_s2br_fwd``, the mid-block attention
    (one head of width 512) is ``uwu_attention_d512_fwd``, the posterior draw is ``uwu_posterior_draw``;
  * all parameters live in one flat fp32 buffer (+ bf16 shadow), the store every model here shares (``flat.FlatModule``);
    conv weights sit there as ``[Cout][3][3][C]``; ``in_channels`` / ``out_channels`` / ``2 * latent`` are
    padded to 8 with zero weights;
  * there is no backward, no CPU path, no tiling / slicing, no ``kl()``.
"""
import math

import torch

from . import lib as L
from . import ops
from .flat import FlatModule, _Config, pad8

SDXL_VAE_CONFIG = dict(
    in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
    down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4, norm_num_groups=32,
    act_fn="silu", mid_block_add_attention=True, scaling_factor=0.13025, sample_size=1024,
)
# hub names of the reference's YAMLs -> preset (random init: nothing is ever fetched)
# Stable Diffusion 1.x: the same architecture, its own latent scale and training resolution
SD_VAE_CONFIG = dict(SDXL_VAE_CONFIG, scaling_factor=0.18215, sample_size=512)
PRESETS = {
    "madebyollin/sdxl-vae-fp16-fix": SDXL_VAE_CONFIG,
    "stabilityai/stable-diffusion-xl-base-1.0": SDXL_VAE_CONFIG,
    "sdxl-vae": SDXL_VAE_CONFIG,
    "CompVis/stable-diffusion-v1-4": SD_VAE_CONFIG,
    "runwayml/stable-diffusion-v1-5": SD_VAE_CONFIG,
    "bdsqlsz/stable-diffusion-v1-5": SD_VAE_CONFIG,
    "sd-vae": SD_VAE_CONFIG,
}
_EPS = 1e-6
_ATTN_DIM = 512  # the one head width uwu_attention_d512_fwd is built for


class DiagonalGaussianDistribution:
    """``encode(x).latent_dist``: the posterior over latents.  Holds the encoder's channels-last fp32 moments; the NCHW
    tensors are written by ``uwu_posterior_draw`` when first asked for."""

    def __init__(self, moments, B, latent, h, w):
        self._mom, self._shape = moments, (B, latent, h, w)
        self._mean = self._logvar = None

    def _run(self, sample, seed=0, offset=0):
        B, Lc, h, w = self._shape
        need = self._mean is None
        z, mu, lv = ops.posterior_draw(self._mom, B, Lc, h * w, seed, offset, sample=sample, mean=need, logvar=need)
        if need:
            self._mean, self._logvar = mu.view(self._shape), lv.view(self._shape)
        return z.view(self._shape) if sample else None

    @property
    def mean(self):
        if self._mean is None:
            self._run(False)
        return self._mean

    @property
    def logvar(self):
        if self._logvar is None:
            self._run(False)
        return self._logvar

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self):
        return torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        """mean + std * eps; eps from the in-kernel Philox stream at (seed, offset) of ``generator`` (default: the device's
        torch generator), whose offset moves on by the counters used -- the convention of DiffusionLoss._reserve."""
        dev = self._mom.device
        gen = generator
        if gen is None:
            gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        elif gen.device.type != "cuda":
            raise L.UwuError("latent_dist.sample: the generator must live on the HIP device (no CPU path)")
        n = math.prod(self._shape)
        seed, off = gen.initial_seed() & ((1 << 64) - 1), gen.get_offset()
        gen.set_offset(off + (n // 4 + 3) // 4 * 4)
        return self._run(True, seed, off)


class AutoencoderKLOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist

    def __getitem__(self, i):
        return (self.latent_dist,)[i]


class DecoderOutput:
    def __init__(self, sample):
        self.sample = sample

    def __getitem__(self, i):
        return (self.sample,)[i]


class AutoencoderKL(FlatModule):
    def __init__(self, config=None, compute_dtype="bf16", **kw):
        super().__init__()
        init_weights = kw.pop("init_weights", True)
        device = kw.pop("device", None)
        cfg = dict(SDXL_VAE_CONFIG)
        cfg.update({k: v for k, v in (config or {}).items() if not k.startswith("_")})
        cfg.update(kw)
        if compute_dtype not in ("bf16", "fp32"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if cfg["act_fn"] != "silu":
            raise ValueError("AutoencoderKL: only act_fn = silu is built")
        boc = [int(c) for c in cfg["block_out_channels"]]
        cfg["block_out_channels"] = tuple(boc)
        if cfg["mid_block_add_attention"] and boc[-1] != _ATTN_DIM:
            raise ValueError(f"AutoencoderKL: the mid-block attention kernel is built for {_ATTN_DIM} channels, got {boc[-1]}")
        self.config = _Config(cfg)
        self.compute_dtype = compute_dtype
        self.G = int(cfg["norm_num_groups"])
        self.latent = int(cfg["latent_channels"])
        self.cin_pad, self.cout_pad = pad8(cfg["in_channels"]), pad8(cfg["out_channels"])
        self.mom_pad, self.lat_pad = pad8(2 * self.latent), pad8(self.latent)
        P = self.P
        self._conv_meta = {}  # 3x3 convolutions: name -> (cin, cout, stored cin, stored cout)
        self._pw_meta = {}    # 1x1 convolutions, stored as Linear [cout, cin]: the same

        def conv(name, cin, cout, ci=None, co=None):
            ci, co = ci or cin, co or cout
            self._conv_meta[name] = (cin, cout, ci, co)
            P.add(name + ".weight", (co, 9 * ci))
            P.add(name + ".bias", (co,))

        def pw(name, cin, cout, ci=None, co=None):
            ci, co = ci or cin, co or cout
            self._pw_meta[name] = (cin, cout, ci, co)
            P.add(name + ".weight", (co, ci))
            P.add(name + ".bias", (co,))

        def lin(name, cin, cout):
            P.add(name + ".weight", (cout, cin))
            P.add(name + ".bias", (cout,))

        def norm(name, c):
            P.add(name + ".weight", (c,))
            P.add(name + ".bias", (c,))

        def resnet(name, cin, cout):
            norm(name + ".norm1", cin)
            conv(name + ".conv1", cin, cout)
            norm(name + ".norm2", cout)
            conv(name + ".conv2", cout, cout)
            if cin != cout:
                pw(name + ".conv_shortcut", cin, cout)
            return (name, cin, cout)

        def mid(prefix, c):
            plan = dict(res=[resnet(prefix + ".resnets.0", c, c)], attn=None)
            if cfg["mid_block_add_attention"]:
                a = prefix + ".attentions.0"
                norm(a + ".group_norm", c)
                for p in ("to_q", "to_k", "to_v", "to_out.0"):
                    lin(f"{a}.{p}", c, c)
                plan["attn"] = a
            plan["res"].append(resnet(prefix + ".resnets.1", c, c))
            return plan

        nl = int(cfg["layers_per_block"])
        # ---- encoder
        conv("encoder.conv_in", cfg["in_channels"], boc[0], ci=self.cin_pad)
        self.enc_blocks, ch = [], boc[0]
        for i in range(len(boc)):
            cin, ch = ch, boc[i]
            blk = dict(res=[resnet(f"encoder.down_blocks.{i}.resnets.{j}", cin if j == 0 else ch, ch) for j in range(nl)],
                       down=None, ch=ch)
            if i < len(boc) - 1:
                blk["down"] = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                conv(blk["down"], ch, ch)
            self.enc_blocks.append(blk)
        self.enc_mid = mid("encoder.mid_block", boc[-1])
        norm("encoder.conv_norm_out", boc[-1])
        conv("encoder.conv_out", boc[-1], 2 * self.latent, co=self.mom_pad)
        # ---- decoder
        rev = boc[::-1]
        conv("decoder.conv_in", self.latent, rev[0], ci=self.lat_pad)
        self.dec_mid = mid("decoder.mid_block", rev[0])
        self.dec_blocks, ch = [], rev[0]
        for i in range(len(rev)):
            cin, ch = ch, rev[i]
            blk = dict(res=[resnet(f"decoder.up_blocks.{i}.resnets.{j}", cin if j == 0 else ch, ch) for j in range(nl + 1)],
                       up=None, ch=ch)
            if i < len(rev) - 1:
                blk["up"] = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                conv(blk["up"], ch, ch)
            self.dec_blocks.append(blk)
        norm("decoder.conv_norm_out", rev[-1])
        conv("decoder.conv_out", rev[-1], cfg["out_channels"], co=self.cout_pad)
        pw("quant_conv", 2 * self.latent, 2 * self.latent, ci=self.mom_pad, co=self.mom_pad)
        pw("post_quant_conv", self.latent, self.latent, ci=self.lat_pad, co=self.lat_pad)

        self._alloc(compute_dtype == "bf16", device, trainable=False)
        if init_weights:
            self.reset_parameters()
        self.eval()

    # ------------------------------------------------------------------ parameters
    def _public_view(self, v, name):
        """diffusers' layout of a 3x3 / 1x1 convolution: [Cout, Cin, k, k] without the padded channels"""
        base, _, leaf = name.rpartition(".")
        for taps, meta in ((9, self._conv_meta), (1, self._pw_meta)):
            if base in meta:
                return self._conv_public(v, meta[base], taps, leaf == "bias")
        return v

    @torch.no_grad()
    def reset_parameters(self):
        """torch's default initialisers per layer type (Conv2d / Linear: U(+-1/sqrt(fan_in)) for weight and bias, norms 1 / 0),
        seeded from torch.initial_seed() as UNet2DConditionModel.reset_parameters does"""
        g = torch.Generator(device=self.flat.device).manual_seed(torch.initial_seed() % (2 ** 31))
        fan = {}
        for name, (off, shape) in self.P.registry.items():
            v = self._public_view(self.P.base32(name), name)
            if name.endswith(".weight") and len(shape) == 1:
                v.fill_(1.0)
            elif name.endswith(".weight"):
                fan[name[:-7]] = fan_in = math.prod(v.shape[1:])
                v.copy_((torch.rand(v.shape, generator=g, device=v.device) * 2 - 1) / math.sqrt(fan_in))
            elif name[:-5] in fan:
                v.copy_((torch.rand(v.shape, generator=g, device=v.device) * 2 - 1) / math.sqrt(fan[name[:-5]]))
            else:
                v.zero_()
        self.refresh_shadow()

    # ------------------------------------------------------------------ blocks (forward only, channels-last tokens)
    def _gn(self, x, name, B, HW, C, silu):
        # the fixed-order statistics: encode / decode of a sample give the same bits whatever batch it sits in
        return ops.groupnorm_fwd_det(x, self.P.w32(name + ".weight"), self.P.w32(name + ".bias"), B, HW, C, self.G, _EPS, silu)[0]

    def _lin(self, x, name, out_dtype=None):
        return ops.gemm(x, self.P.w(name + ".weight"), bias=self.P.w32(name + ".bias"), epilogue=L.EPI_BIAS, c_dtype=out_dtype)

    def _conv(self, x, name, B, H, W, C):
        Wt, b = self.P.w(name + ".weight"), self.P.w32(name + ".bias")
        if ops.conv3x3_implicit_ok(x, B, H, W, C, Wt.shape[0], 1):
            return ops.conv3x3_fwd(x, Wt, b, B, H, W, C, Wt.shape[0], 1)
        return ops.gemm(ops.im2col3x3(x, B, H, W, C, 1), Wt, bias=b, epilogue=L.EPI_BIAS)

    def _resnet(self, x, r, B, H, W):
        name, cin, cout = r
        h = self._gn(x, name + ".norm1", B, H * W, cin, True)
        h = self._conv(h, name + ".conv1", B, H, W, cin)
        h = self._gn(h, name + ".norm2", B, H * W, cout, True)
        h = self._conv(h, name + ".conv2", B, H, W, cout)
        if cin != cout:
            x = self._lin(x, name + ".conv_shortcut")
        return ops.add(x, h)

    def _mid(self, x, plan, B, H, W):
        C = x.shape[1]
        x = self._resnet(x, plan["res"][0], B, H, W)
        a = plan["attn"]
        if a is not None:  # one head of width C over the H*W tokens, residual added (rescale_output_factor 1)
            h = self._gn(x, a + ".group_norm", B, H * W, C, False)
            q, k, v = (self._lin(h, f"{a}.to_{c}") for c in "qkv")
            o = ops.attention_d512_fwd(q, k, v, B, H * W)
            x = ops.add(x, self._lin(o, a + ".to_out.0"))
        return self._resnet(x, plan["res"][1], B, H, W)

    def _to_cl(self, x, C, cpad, what):
        if not torch.is_tensor(x) or not x.is_cuda or not self.flat.is_cuda:
            raise L.UwuError(f"AutoencoderKL.{what} runs on the HIP device only (no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError(f"AutoencoderKL.{what}: expected [B, {C}, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        x = x.float()
        if cpad != C:
            x = torch.cat([x, x.new_zeros(B, cpad - C, H, W)], dim=1)
        if self.P.bf16 and self.shadow.numel() != self.P.n:
            self.refresh_shadow()
        return ops.nchw_to_cl(x.contiguous(), self.P.dtype)

    # ------------------------------------------------------------------ public calls
    @torch.no_grad()
    def encode(self, x, return_dict=True):
        if torch.is_tensor(x) and x.dim() == 4 and (x.shape[2] % 8 or x.shape[3] % 8):
            raise ValueError(f"AutoencoderKL.encode: H and W must be multiples of 8, got {tuple(x.shape[2:])}")
        h = self._to_cl(x, self.config["in_channels"], self.cin_pad, "encode")
        B, _, H, W = x.shape
        h = self._conv(h, "encoder.conv_in", B, H, W, self.cin_pad)
        for blk in self.enc_blocks:
            for r in blk["res"]:
                h = self._resnet(h, r, B, H, W)
            if blk["down"]:
                Wt = self.P.w(blk["down"] + ".weight")
                h = ops.conv3x3_s2br_fwd(h, Wt, self.P.w32(blk["down"] + ".bias"), B, H, W, blk["ch"], blk["ch"])
                H, W = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        h = self._mid(h, self.enc_mid, B, H, W)
        h = self._gn(h, "encoder.conv_norm_out", B, H * W, h.shape[1], True)
        h = self._conv(h, "encoder.conv_out", B, H, W, h.shape[1])
        mom = self._lin(h, "quant_conv", out_dtype=torch.float32)  # fp32 moments [B*H*W, mom_pad]
        out = AutoencoderKLOutput(DiagonalGaussianDistribution(mom, B, self.latent, H, W))
        return out if return_dict else (out.latent_dist,)

    @torch.no_grad()
    def decode(self, z, return_dict=True, generator=None):
        h = self._to_cl(z, self.latent, self.lat_pad, "decode")
        B, _, H, W = z.shape
        h = self._lin(h, "post_quant_conv")
        h = self._conv(h, "decoder.conv_in", B, H, W, self.lat_pad)
        h = self._mid(h, self.dec_mid, B, H, W)
        for blk in self.dec_blocks:
            for r in blk["res"]:
                h = self._resnet(h, r, B, H, W)
            if blk["up"]:
                h = ops.upsample2x(h, B, H, W, blk["ch"])
                H, W = 2 * H, 2 * W
                h = self._conv(h, blk["up"], B, H, W, blk["ch"])
        h = self._gn(h, "decoder.conv_norm_out", B, H * W, h.shape[1], True)
        h = self._conv(h, "decoder.conv_out", B, H, W, h.shape[1])
        C = self.config["out_channels"]
        img = ops.cl_to_nchw(h, B, self.cout_pad, H * W).view(B, self.cout_pad, H, W)[:, :C].contiguous()
        return DecoderOutput(img) if return_dict else (img,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        post = self.encode(sample).latent_dist
        return self.decode(post.sample(generator) if sample_posterior else post.mode(), return_dict=return_dict)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_config(cls, config, **kw):
        return cls.from_pretrained(config, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, subfolder=None, **kw):
        """Hub names of the reference's YAMLs -> the SDXL preset with seeded default initialisation (nothing is fetched, as
        UNet2DFromScratch.from_config treats hub names); a dict is a configuration; a local directory with ``config.json`` and
        ``diffusion_pytorch_model.safetensors`` is loaded."""
        kw = cls._drop_hub_keywords(kw)
        src = "sdxl-vae" if pretrained_model_name_or_path is None else pretrained_model_name_or_path
        if isinstance(src, dict):
            return cls(dict(src), **kw)
        src = str(src)
        model = cls._from_local_dir(src, subfolder, SDXL_VAE_CONFIG, "diffusion_pytorch_model.safetensors", **kw)  # (force_upcast etc.: not built)
        if model is not None:
            return model
        if src in PRESETS:
            return cls(dict(PRESETS[src]), **kw)
        raise ValueError(f"unknown AutoencoderKL {src!r}: not a local directory with config.json; known names: {sorted(PRESETS)}")
